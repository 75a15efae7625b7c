"""Host side (no GPU): the census of mr_conv2d_f32 instantiations (tests/direct_conv_census.py) that tests/test_gpu_direct_conv_sweeps.py
runs - what it must contain, and its size pinned so that a table or dispatch change shows up as a diff here."""
import collections

import direct_conv_census as census
from monorec_amd import engine

# instantiation keys per arithmetic mode (0 fp32, 1 bf16, 2 bf16x3), measured when the census was written
KEY_COUNTS = {0: 160, 1: 17, 2: 63}

# fp32 table keys no census plan launches.  All of one kind: layers.Upconv as ONE single-phase 2x2 launch over the x2-upsampled input
# (IN_UPSAMPLE2) - the form of the first rounds.  Plan.upconv has issued these layers as the four parity phases of one launch (keys
# ..._p4u) or on the 4-multiply kernel ever since, and no Plan option brings the single-phase form back: the entries are dead.
UNREACHED = """
co64_ci64_k2x2_s1x1_o256x512_b1_p1 co64_ci64_k2x2_s1x1_o256x512_b2_p1 co64_ci64_k2x2_s1x1_o256x512_b4_p1 co64_ci64_k2x2_s1x1_o256x512_b8_p1
co64_ci64_k2x2_s1x1_o512x1024_b1_p1 co96_ci96+256_k2x2_s1x1_o32x64_b1_p1 co96_ci96+256_k2x2_s1x1_o32x64_b2_p1 co96_ci96+256_k2x2_s1x1_o32x64_b4_p1
co96_ci96+256_k2x2_s1x1_o32x64_b8_p1 co96_ci96+256_k2x2_s1x1_o64x128_b1_p1 co96_ci96_k2x2_s1x1_o128x256_b1_p1 co96_ci96_k2x2_s1x1_o128x256_b2_p1
co96_ci96_k2x2_s1x1_o128x256_b4_p1 co96_ci96_k2x2_s1x1_o128x256_b8_p1 co96_ci96_k2x2_s1x1_o256x512_b1_p1 co96_ci96_k2x2_s1x1_o64x128_b1_p1
co96_ci96_k2x2_s1x1_o64x128_b2_p1 co96_ci96_k2x2_s1x1_o64x128_b4_p1 co96_ci96_k2x2_s1x1_o64x128_b8_p1
""".split()

# Order identity (check c of the GPU file): single-chain fp32 keys whose layer has NO second single-chain schedule at all (a 64-channel
# 3x3 stride-2 chunk next to its 5 x 68 tile fills the LDS: only the 1 x 1 register tile, with its two partial sums, also fits) ...
NO_ANCHOR = {"f32-mb2nb1wv4-x4-pl0-pipe-k3x3s2x2-p1"}
# ... and those whose every launchable tile lands on a menu pitch (rows of >= 32 outputs, 3-tap-high tiles of 2 / 4 / 8 / 16 rows have the
# pitches 176 / 240 / 400 / 720, and 32- or 64-channel chunks at 720 do not fit the LDS): anchored on ANOTHER menu pitch
MENU_ANCHORED = {"f32-mb2nb1wv8-x4-pl240-pipe-k3x3s1x1-p1", "f32-mb3nb1wv4-x4-pl176-pipe-k3x3s1x1-p1", "f32-mb1nb2wv8-x4-pl400-pipe-k3x3s1x1-p1",
                 "f32-mb2nb1wv4-x4-pl176-pipe-k3x1s2x1-p1", "f32-mb2nb2wv8-x4-pl400-pipe-k3x3s1x1-p1"}
# ... of which this one has a single launchable tile shape (64-channel chunks of a 3 x 1 stride-(2,1) layer): same pitch, another MB only
SAME_PITCH_ANCHORED = {"f32-mb2nb1wv4-x4-pl176-pipe-k3x1s2x1-p1"}


def test_census_is_not_empty_and_its_size_is_pinned(hip_lib):
    cases = census.census()
    assert cases
    counts = collections.Counter(k.mode for k in cases)
    assert dict(counts) == KEY_COUNTS, dict(counts)
    ids = [census.key_id(k) for k in cases]
    assert len(set(ids)) == len(ids)                      # the readable ids the GPU file is parametrised with name the keys one to one


def test_every_menu_pitch_is_reached_by_a_pipelined_sweep(hip_lib):
    """A pitch of MR_PLANE_MENU (read from csrc/conv_mfma.hip) that no tabled launch takes into sweep_chunk_pipe is a dead instantiation."""
    menu = census.plane_menu()
    assert len(menu) >= 1 and len(set(menu)) == len(menu)
    reached = collections.Counter(k.plane for k in census.census() if "pipe" in k.sweeps and k.mode == 0 and not k.kws)
    dead = [p for p in menu if not reached[p]]
    assert not dead, f"MR_PLANE_MENU pitches no tabled pipelined launch has: {dead}"


def test_every_fp32_table_key_is_launched_by_a_census_plan(hip_lib):
    fp32 = [k for k in engine.TUNED if not k.endswith(("_bf16", "_bf16x3"))]
    sigs = {sig for _, _, _, _, sig, _ in census.launches()}
    missing = sorted(k for k in fp32 if k not in sigs)
    assert missing == sorted(UNREACHED), (sorted(set(missing) - set(UNREACHED)), sorted(set(UNREACHED) - set(missing)))
    assert len(UNREACHED) <= 0.05 * len(fp32), (len(UNREACHED), len(fp32))


def test_representatives_keep_their_key_and_everything_but_the_image_size(hip_lib):
    """Shrinking changes the output grid, the source size that follows from it and the batch - nothing else of the launch; the key is
    re-derived through the library (mr_conv2d_lds_bytes) for the shrunken layer.  No key had to stay at its original size."""
    origin = {}
    for spec, sched, mode, name, sig, where in census.launches():
        origin.setdefault((name, where, mode), (spec, sched))
    for key, case in census.census().items():
        spec, sched = origin[(case.name, case.origin, case.mode)]
        small = case.spec
        assert case.shrunk and tuple(sched) == tuple(case.sched)
        assert census.launch_key(spec, sched, case.mode) == key == census.launch_key(small, case.sched, case.mode)
        for field in ("w_shape", "stride", "pad", "in_mode", "tf", "act", "p0", "p1", "residual", "out_step", "out_off", "phases"):
            assert small[field] == spec[field], (census.key_id(key), field)
        assert [s[1] for s in small["src_shapes"]] == [s[1] for s in spec["src_shapes"]] and small["out_shape"][1] == spec["out_shape"][1]
        assert small["src_shapes"][0][3] % 4 == spec["src_shapes"][0][3] % 4
        assert (small["grid"][1] >= 32) == (spec["grid"][1] >= 32)
        th, tw = census.geometry(small, case.sched, case.mode)["tile"]
        assert small["grid"][1] % tw and (th == 1 or small["grid"][0] % th), (census.key_id(key), small["grid"], (th, tw))     # ragged in both directions
        assert census._macs(small) <= 2 * census.MAX_GMAC * 1e9, (census.key_id(key), census._macs(small))


def test_anchor_schedules_of_the_order_identity(hip_lib):
    """Check (c): every single-chain fp32 key but NO_ANCHOR has an anchor schedule - same chunking and sweep functions, another register
    tile / workgroup size, one partial sum per accumulator - and but for MENU_ANCHORED its pitch is outside the menu."""
    menu, none, on_menu, n = census.plane_menu(), set(), set(), 0
    for key, case in census.census().items():
        if key.mode or key.splitk or key.kws or key.dual:
            assert not census.order_check_applies(case)
            continue
        anchor = census.anchor_schedule(case)
        if anchor is None:
            none.add(census.key_id(key))
            continue
        n += 1
        sched, plane = anchor
        mb, nb, split_k, ck, wv, kws = census.unpack_schedule(sched)
        assert (mb, nb, wv) != (key.mb, key.nb, key.wv) and mb * nb > 1 and split_k == 1 and not kws and ck == case.sched[3]
        akey = census.launch_key(case.spec, sched, 0)
        assert akey.sweeps == key.sweeps and plane == census.library_plane(case.spec, sched, 0)
        if plane in menu:
            assert (plane == key.plane) == (census.key_id(key) in SAME_PITCH_ANCHORED)
            on_menu.add(census.key_id(key))
        else:
            assert akey.plane == 0
    assert none == NO_ANCHOR and on_menu == MENU_ANCHORED, (none, on_menu)
    assert n == 97
