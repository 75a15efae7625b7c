"""Census of the mr_conv2d_b8 forms the bf16 plans launch (host side, no GPU).

mr_conv2d_b8 (csrc/conv_b8.hip) carries every convolution of the bf16 configuration that reads or writes a channel-blocked bf16 ("B8")
activation.  Every bf16 plan shape the tuned_b8.json table was measured for - and one shape without table entries, which follows the rule of
Plan.b8_schedule - is built on the CPU device; every conv_log entry with `b8` is reduced to a KEY - what the compiled code and the run-time
branches of that launch depend on - and one spatially shrunken representative per key is kept.  tests/test_b8_conv_census.py pins the
census, tests/test_gpu_b8_conv_forms.py runs every representative alone against an exact reference.

The key (`Key`):
    mb, nb, wv, wres, f32src   template parameters of conv_b8_kernel (wres: the cout group's whole weight stream is resident in LDS;
                               f32src: some source is dense fp32 - the register-staged path is compiled in)
    srcs                       layout of every source, "b" (B8, LDS-DMA) or "f" (fp32 NCHW, register-staged)
    dst                        "b" or "f": B8 (results wait in `pend`, flushed during the next tile's first chunk) or fp32 (stored at once)
    k, stride                  (KH, KW) maximum over the phases and (SH, SW): the size of the input tile, the lane pitch of the B reads
    phases                     1, or 4 with `taps` the per-phase filter sizes: "2x2" (layers.Refine) or "1-2-2-4" (layers.Upconv: the
                               resident-weight offsets use the per-phase tap count, the tile the maximum)
    walk                       tiles_per_wg > 1: the load cursor crosses tile (and tile-row) boundaries, a B8 destination's results are
                               flushed one tile late, the last workgroup's walk is clipped
    multi_chunk                nchunks > 1 (a one-chunk layer issues the next tile's load in the iteration that flushes)
    two_positions              PLANE > 64 wv: the second staged tile position per thread is live
    act                        MR_ACT_NONE / RELU / LEAKY_RELU
`wres`, PLANE, nchunks, tiles_per_wg and the LDS bytes come from `derive`, a restatement of derive8(); the LDS bytes are cross-checked
against mr_conv2d_b8_lds_bytes for every launch (`library_lds`).  The workgroup target of the tile walk and B8_MAX_PPT are read from the
kernel source.

REFERENCE COST.  A walk representative needs more than 1024 (tile, cout group, batch, phase) jobs, so its grid cannot be two tiles: it is
the smallest grid with tiles_per_wg >= 2, a clipped last walk, a walk across a tile-row boundary and ragged last tile row / column.
Its cost is jobs x tile pixels x the cout group's channels x Cin x taps: what the resident weights allow at most.  The heaviest, measured
on 8 CPU threads when the census was written (HEAVIEST in tests/test_b8_conv_census.py pins which it is):
    bb-b-mb3nb4wv8-wres-k3x3s1x1-p1-walk-q2-pp2-leaky (mask.dec3.1: 3x3 over 32 + 64 channels, 48 out, grid 2729 x 81 x batch 2)
    18.3 GMAC: fp64 conv2d 3.3 s, fp32 0.35 s
MAX_GMAC_WALK = 20 keeps the one fp64 reference of a case (check b of the GPU file; check a takes the fp32 one) at that."""
import collections
import ctypes
import functools
import math
import os
import re

import torch

from monorec_amd import _lib, engine, synth
from monorec_amd._lib import ACT_LEAKY_RELU, ACT_NONE, ACT_RELU, LAYOUT_BF16_B8, LAYOUT_F32_NCHW, B8ConvDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W, F, D) of the bf16 plans: the two shapes of the direct census, the batch shapes the _b4_ / _b8_ / _b32_ keys of tuned_b8.json
# come from (the mask encoder runs on B * F frames), and one shape no table entry was measured for (Plan.b8_schedule's rule).
PLAN_SHAPES = [(1, 256, 512, 2, 32), (1, 512, 1024, 4, 48), (8, 256, 512, 4, 64), (8, 256, 512, 2, 32), (4, 256, 512, 2, 32),
               (2, 256, 512, 2, 32), (1, 320, 640, 2, 32)]
RULE_SHAPE = (1, 320, 640, 2, 32)   # none of its launches has a tuned_b8.json entry: all follow Plan.b8_schedule
MAX_GMAC = 0.3                      # multiply-adds of an ordinary shrunken representative (fp64 CPU reference per case)
MAX_GMAC_WALK = 20.0                # ... of a walk representative (> 1024 jobs): see the module docstring
LDS_LIMIT, WRES_LIMIT = 160 * 1024, 112 * 1024

Key = collections.namedtuple("Key", "mb nb wv wres f32src srcs dst k stride phases taps walk multi_chunk two_positions act")
# kind: "conv" (one phase), "refine" (layers.Refine: 4 phases of 2x2), "upconv" (layers.Upconv: 4 phases of 1, 2, 2 and 4 taps)
Case = collections.namedtuple("Case", "key spec sched name sig origin")
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LEAKY_RELU: "leaky"}
PHASE_TAPS = {"conv": None, "refine": ((2, 2),) * 4, "upconv": ((1, 1), (1, 2), (2, 1), (2, 2))}


def key_id(key):
    """Readable pytest id of a key."""
    return (f"{key.srcs}-{key.dst}-mb{key.mb}nb{key.nb}wv{key.wv}{'-wres' if key.wres else ''}-k{key.k[0]}x{key.k[1]}s{key.stride[0]}x{key.stride[1]}"
            f"-p{key.phases}{'' if key.phases == 1 else 'r' if key.taps == '2x2' else 'u'}{'-walk' if key.walk else ''}"
            f"-{'q2' if key.multi_chunk else 'q1'}-{'pp2' if key.two_positions else 'pp1'}-{ACT_NAMES[key.act]}")


@functools.lru_cache(None)
def kernel_constants():
    """(workgroup target of the tile walk, B8_MAX_PPT, cap of tiles_per_wg), read from csrc/conv_b8.hip."""
    with open(os.path.join(ROOT, "monorec_amd", "csrc", "conv_b8.hip")) as f:
        src = f.read()
    return (int(re.search(r"long long wgs_target = (\d+);", src).group(1)), int(re.search(r"#define B8_MAX_PPT (\d+)", src).group(1)),
            int(re.search(r"if \(tpw > (\d+)\) tpw = \1;", src).group(1)))


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):           # like the hip_lib fixture: hipcc cross-compiles without a GPU
        from monorec_amd import build
        build.build()
    return _lib.load()


def src_channels_of(spec):
    return [int(s[1]) for s in spec["src_shapes"]]


def phase_list(spec):
    """[(kh, kw, pad_top, pad_left, out_off_h, out_off_w)] of the launch's phases, as Plan.conv_b8 / refine / upconv build them."""
    kh, kw = spec["w_shape"][2:]
    if spec["kind"] == "conv":
        return [(kh, kw, spec["pad"][0], spec["pad"][1], 0, 0)]
    if spec["kind"] == "refine":        # engine.transposed_phase_weights: parity 0 reads one row / column above / left of the output
        return [(2, 2, 1 - py, 1 - px, py, px) for py in (0, 1) for px in (0, 1)]
    return [(1 + py, 1 + px, 0, 0, py, px) for py in (0, 1) for px in (0, 1)]          # engine.upconv_phase_weights


def derive(spec, sched):
    """Restatement of derive8() (csrc/conv_b8.hip) for one launch, or None where derive8 rejects it."""
    mb, nb, wv = (int(v) for v in sched[:3])
    wgs_target, max_ppt, tpw_cap = kernel_constants()
    cout, cin, kh, kw = spec["w_shape"]
    (sh, sw), (out_h, out_w) = spec["stride"], spec["grid"]
    batch = spec["src_shapes"][0][0]
    nphase = len(phase_list(spec))
    nchunks = sum(((c + 7) // 8 + 3) // 4 for c in src_channels_of(spec))
    if not (1 <= mb <= 4 and nb in (1, 2, 4) and wv in (4, 8)):
        return None
    th = wv * nb // 2
    tiles_x, tiles_y = (out_w + 31) // 32, (out_h + th - 1) // th
    ih, iw = (th - 1) * sh + kh, 31 * sw + kw
    plane = ih * iw
    if (plane + 64 * wv - 1) // (64 * wv) > max_ppt:
        return None
    ntiles = tiles_x * tiles_y
    ngroups = ((cout + 15) // 16 + mb - 1) // mb
    wall, tile2 = nchunks * kh * kw * mb * 1024, 2 * 64 * plane
    wres = wall + tile2 <= LDS_LIMIT and wall <= WRES_LIMIT
    jobs = ntiles * ngroups * batch * nphase
    if wres:
        lds, tpw = wall + tile2, min(max((jobs + wgs_target - 1) // wgs_target, 1), tpw_cap)
    else:
        lds, tpw = 2 * (64 * plane + 1024 * kh * kw * mb), 1
    if lds > LDS_LIMIT:
        return None
    return dict(mb=mb, nb=nb, wv=wv, th=th, tiles_x=tiles_x, tiles_y=tiles_y, ntiles=ntiles, ngroups=ngroups, ih=ih, iw=iw, plane=plane,
                nchunks=nchunks, wres=wres, lds=lds, tiles_per_wg=tpw, jobs=jobs, nphase=nphase,
                wgs=(ntiles + tpw - 1) // tpw * ngroups * batch * nphase)


def descriptor(spec, sched):
    """The mr_b8_conv_desc Plan.conv_b8 builds for `spec` under `sched`, with placeholder pointers: enough for mr_conv2d_b8_lds_bytes."""
    mb, nb, wv = (int(v) for v in sched[:3])
    cout, cin, kh, kw = spec["w_shape"]
    d = B8ConvDesc()
    n, _, hs, ws = spec["src_shapes"][0]
    for i, (c, lay) in enumerate(zip(src_channels_of(spec), spec["src_layouts"])):
        d.src[i], d.src_channels[i], d.src_layout[i] = 1, c, lay
    d.num_src, d.batch, d.src_h, d.src_w = len(spec["src_shapes"]), n, hs, ws
    d.kh, d.kw, d.stride_h, d.stride_w = kh, kw, spec["stride"][0], spec["stride"][1]
    d.out_h, d.out_w = spec["grid"]
    d.dst, d.dst_layout, d.out_channels = 1, spec["out_layout"], cout
    d.dst_plane_h, d.dst_plane_w = spec["grid"][0] * spec["out_step"][0], spec["grid"][1] * spec["out_step"][1]
    d.out_step_h, d.out_step_w = spec["out_step"]
    d.activation, d.act_p0 = spec["act"], spec["p0"]
    d.cout_blocks_per_wg, d.pixel_blocks_per_wave, d.waves_per_wg = mb, nb, wv
    phases = phase_list(spec)
    d.num_phases = len(phases)
    for i, (pkh, pkw, pt, pl, oh, ow) in enumerate(phases):
        d.phase_weights[i], d.phase_kh[i], d.phase_kw[i] = 1, pkh, pkw
        d.phase_pad_top[i], d.phase_pad_left[i], d.phase_out_off_h[i], d.phase_out_off_w[i] = pt, pl, oh, ow
    return d


def library_lds(spec, sched):
    """mr_conv2d_b8_lds_bytes of the launch, checked against `derive`; raises ValueError when the library rejects the launch."""
    lds = int(_lib_loaded().mr_conv2d_b8_lds_bytes(ctypes.byref(descriptor(spec, sched))))
    g = derive(spec, sched)
    if lds < 0:
        assert g is None, ("derive8() restated wrongly: the library rejects what derive() accepts", spec, sched, lds)
        raise ValueError(f"mr_conv2d_b8_lds_bytes: {lds}")
    assert g is not None and g["lds"] == lds, ("derive8() restated wrongly", spec, sched, lds, g)
    return lds


def launch_key(spec, sched):
    """Key of one launch (module docstring); ValueError when the library rejects it."""
    library_lds(spec, sched)
    g = derive(spec, sched)
    lays = spec["src_layouts"]
    taps = PHASE_TAPS[spec["kind"]]
    return Key(g["mb"], g["nb"], g["wv"], g["wres"], any(l == LAYOUT_F32_NCHW for l in lays),
               "".join("b" if l == LAYOUT_BF16_B8 else "f" for l in lays), "b" if spec["out_layout"] == LAYOUT_BF16_B8 else "f",
               tuple(spec["w_shape"][2:]), tuple(spec["stride"]), g["nphase"],
               "" if taps is None else ("2x2" if spec["kind"] == "refine" else "1-2-2-4"),
               g["tiles_per_wg"] > 1, g["nchunks"] > 1, g["plane"] > 64 * g["wv"], int(spec["act"]))


def template_tuple(key):
    return key.mb, key.nb, key.wv, key.wres, key.f32src


def macs(spec):
    cout, cin = spec["w_shape"][:2]
    return spec["src_shapes"][0][0] * spec["grid"][0] * spec["grid"][1] * cout * cin * sum(p[0] * p[1] for p in phase_list(spec))


def spec_of(c):
    """The census's `spec` of a conv_log entry with `b8`: the entry's own spec + `kind`, told from the multiply-adds per output of the
    four phases (16: the 2x2 phases of Refine; 9: the 1 + 2 + 2 + 4 taps of Upconv)."""
    spec = dict(c["spec"])
    kind = "conv"
    if c["phases"] == 4:
        per_out = c["macs"] // (c["batch"] * c["out"][0] * c["out"][1] * c["cout"] * c["cin"])
        kind = {16: "refine", 9: "upconv"}[per_out]
    spec.update(kind=kind, src_shapes=[tuple(int(v) for v in s) for s in spec["src_shapes"]], src_layouts=tuple(spec["src_layouts"]))
    return spec


def resized(spec, out_h, out_w, batch):
    """`spec` at another output grid / batch: the source plane follows the grid by the layer's stride (four-phase layers: the grid IS the
    source plane); channels, layouts, filter, stride, pad, activation, phases unchanged."""
    _, _, hs, ws = spec["src_shapes"][0]
    (sh, sw), (gh, gw) = spec["stride"], spec["grid"]
    nh, nw = out_h * sh - (gh * sh - hs), out_w * sw - (gw * sw - ws)
    if nh < 1 or nw < 1:
        return None
    return dict(spec, src_shapes=[(batch, int(s[1]), nh, nw) for s in spec["src_shapes"]], grid=(out_h, out_w))


def is_walk_representative(spec, sched):
    """The conditions a `walk` representative meets: tiles_per_wg >= 2, the last workgroup's walk clipped, a walk across a tile-row
    boundary, ragged last tile row and column."""
    g = derive(spec, sched)
    tpw = g["tiles_per_wg"]
    return (tpw >= 2 and g["ntiles"] % tpw != 0 and g["tiles_x"] >= 2 and g["tiles_x"] % tpw != 0 and spec["grid"][0] % g["th"] != 0 and
            spec["grid"][1] % 32 != 0)


def _ragged(tiles, size):
    """Output rows / columns of `tiles` tiles of `size`, the last one ragged (more than half full where the tile has more than 2)."""
    return (tiles - 1) * size + size // 2 + 1 if size > 2 else (tiles - 1) * size + 1


def shrink(spec, sched, key):
    """A representative of `key`.  Ordinary keys: about two tiles and a ragged remainder in each direction, batch 2 - the first candidate
    whose key, re-derived through the library, is `key` and whose multiply-adds stay below MAX_GMAC (fewer tiles, then batch 1, where two
    tiles are too many).  Walk keys: the cheapest grid of batch 2 (then 1) that is a walk representative and keeps the key.  None when no
    candidate keeps the key."""
    g = derive(spec, sched)
    th = g["th"]

    def keeps(cand):
        try:
            return cand is not None and launch_key(cand, sched) == key
        except ValueError:
            return False
    if key.walk:
        best = None
        for batch in (2, 1):
            for tiles_x in range(2, 8):
                for tiles_y in range(1, 1200):
                    jobs = tiles_x * tiles_y * g["ngroups"] * batch * g["nphase"]
                    if jobs <= kernel_constants()[0]:
                        continue
                    cand = resized(spec, _ragged(tiles_y, th), _ragged(tiles_x, 32), batch)
                    if cand is None or not is_walk_representative(cand, sched):
                        continue
                    if best is None or macs(cand) < macs(best):
                        if keeps(cand):
                            best = cand
                    break               # more tile rows only cost more
            if best is not None:
                return best
        return None
    best = None
    for batch in (2, 1):
        for ty, tx in ((3, 3), (3, 2), (2, 3), (2, 2)):
            cand = resized(spec, _ragged(ty, th), _ragged(tx, 32), batch)
            if not keeps(cand):
                continue
            if macs(cand) <= MAX_GMAC * 1e9:
                return cand
            if best is None or macs(cand) < macs(best):
                best = cand
    return best


@functools.lru_cache(None)
def launches():
    """[(spec, (mb, nb, waves), layer name, table key, origin)] of every mr_conv2d_b8 launch of the census plans."""
    from monorec_amd import MonoRecModel
    _lib_loaded()
    out, states = [], {}
    for b, h, w, f, d in PLAN_SHAPES:
        if d not in states:
            states[d] = synth.seeded_state_dict(MonoRecModel(cv_depth_steps=d).state_dict())
        plan = engine.Plan(states[d], b, h, w, f, d, (0.33, 0.0025), "cpu", bf16=1)
        for c in plan.conv_log:
            if c.get("b8"):
                out.append((spec_of(c), (c["mb"], c["nb"], c["waves"]), c["name"], c["sig"] + f"_f{int(c['f32_source'])}", f"b{b}_{h}x{w}_f{f}_d{d}"))
    return out


@functools.lru_cache(None)
def census():
    """{key: Case}: one shrunken representative per key (the first launch that has it, in the order of `launches`)."""
    first = {}
    for spec, sched, name, sig, origin in launches():
        key = launch_key(spec, sched)
        if key not in first:
            first[key] = (spec, sched, name, sig, origin)
    cases = {}
    for key, (spec, sched, name, sig, origin) in first.items():
        small = shrink(spec, sched, key)
        assert small is not None and launch_key(small, sched) == key, (key, name, origin)
        cases[key] = Case(key, small, tuple(sched), name, sig, origin)
    return cases


def dense_spec(srcs_c, lays, cout, k, stride, hw, batch, act, out_layout, p0=0.0, kind="conv"):
    """`spec` of a layer written by hand: sources of `hw` ("b" / "f" per source), PadSameConv2d padding (four-phase kinds: their own)."""
    (kh, kw), (sh, sw) = k, stride
    grid = hw if kind != "conv" else (math.ceil(hw[0] / sh), math.ceil(hw[1] / sw))
    pad = (engine.same_pad(hw[0], kh, sh)[0], engine.same_pad(hw[1], kw, sw)[0]) if kind == "conv" else (0, 0)
    return dict(src_shapes=[(batch, c, hw[0], hw[1]) for c in srcs_c], src_layouts=tuple(LAYOUT_BF16_B8 if l == "b" else LAYOUT_F32_NCHW for l in lays),
                w_shape=(cout, sum(srcs_c), kh, kw), stride=(sh, sw), pad=pad, grid=grid, act=act, p0=p0,
                out_layout=LAYOUT_BF16_B8 if out_layout == "b" else LAYOUT_F32_NCHW, out_step=(1, 1) if kind == "conv" else (2, 2), kind=kind)


def make_case(name, spec, sched):
    return Case(launch_key(spec, sched), spec, tuple(sched), name, None, "extra")


def _extra():
    """The EXTRA list before the cases whose key the census holds are dropped (`extra`)."""
    L, N, R = ACT_LEAKY_RELU, ACT_NONE, ACT_RELU
    return [
        # both strides 2 (the plans stride one direction at a time)
        make_case("stride_2x2", dense_spec((40,), "b", 32, (3, 3), (2, 2), (26, 90), 2, L, "b", 0.1), (2, 1, 8)),
        # mb does not divide ceil(Cout / 16): the last cout group has a wholly padded 16-channel block
        make_case("mb_ragged_b8_out", dense_spec((32,), "b", 48, (3, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (2, 2, 4)),
        make_case("mb_ragged_f32_out", dense_spec((32,), "b", 48, (3, 3), (1, 1), (11, 49), 2, L, "f", 0.1), (2, 2, 4)),
        make_case("mb4_of_5_blocks_b8_out", dense_spec((32,), "b", 72, (1, 3), (1, 1), (9, 49), 2, L, "b", 0.1), (4, 1, 4)),
        # ragged output channels
        make_case("cout_44_b8_out", dense_spec((32,), "b", 44, (3, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (3, 2, 4)),
        make_case("cout_12_b8_out_nb4", dense_spec((32,), "b", 12, (1, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (1, 4, 4)),
        make_case("cout_35_b8_out_nb1", dense_spec((32,), "b", 35, (3, 1), (1, 1), (11, 49), 2, L, "b", 0.1), (3, 1, 8)),
        make_case("cout_22_f32_out", dense_spec((32,), "b", 22, (3, 3), (1, 1), (11, 49), 2, L, "f", 0.1), (1, 2, 8)),
        # ragged source channels
        make_case("b8_source_c_44", dense_spec((44,), "b", 32, (3, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (2, 2, 4)),       # C % 8, ceil(C/8) % 4
        make_case("b8_source_c_40", dense_spec((40,), "b", 32, (3, 3), (1, 1), (11, 49), 2, L, "f", 0.1), (2, 4, 8)),       # ceil(C/8) % 4 only
        make_case("f32_source_c_27", dense_spec((27,), "f", 32, (3, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (2, 2, 4)),
        # three sources, alternating layouts, every one with a ragged last chunk
        make_case("sources_bfb", dense_spec((24, 13, 40), "bfb", 48, (3, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (3, 2, 8)),
        make_case("sources_fbf", dense_spec((13, 24, 7), "fbf", 48, (3, 3), (1, 1), (11, 49), 2, L, "b", 0.1), (3, 2, 4)),
        # ReLU / no activation on a B8 destination: the 8-byte store path (NB = 1) and the exchange path at NB = 4
        make_case("relu_b8_out_nb1", dense_spec((32,), "b", 40, (3, 3), (1, 1), (11, 49), 2, R, "b"), (3, 1, 8)),
        make_case("none_b8_out_nb1", dense_spec((32,), "b", 40, (3, 3), (1, 1), (11, 49), 2, N, "b"), (3, 1, 8)),
        make_case("relu_b8_out_nb4", dense_spec((32,), "b", 40, (3, 3), (1, 1), (37, 49), 2, R, "b"), (3, 4, 8)),
        make_case("none_b8_out_nb4", dense_spec((32,), "b", 40, (3, 3), (1, 1), (37, 49), 2, N, "b"), (3, 4, 8)),
        # a tile walk over four phases of unequal filter sizes (the resident-weight offsets use the per-phase tap count)
        make_case("walk_upconv_phases", dense_spec((24,), "b", 24, (2, 2), (1, 1), (101, 81), 2, N, "b", kind="upconv"), (2, 1, 4)),
        make_case("walk_upconv_phases_f32_out", dense_spec((24, 8), "bf", 20, (2, 2), (1, 1), (105, 81), 2, N, "f", kind="upconv"), (1, 2, 4)),
        # a long walk: tiles_per_wg = 5, one-chunk layer, NB = 1
        make_case("walk_5_tiles", dense_spec((8,), "b", 16, (3, 3), (1, 1), (1365, 81), 2, L, "b", 0.1), (1, 1, 4)),
        # the longest walk a census plan launches, 16 tiles (3 x 2561 tiles x batch 2 = 15366 jobs), over a source with C % 8 != 0
        make_case("walk_16_tiles", dense_spec((4,), "b", 8, (3, 3), (1, 1), (5121, 81), 2, R, "b"), (1, 1, 4)),
        # rows of fewer than 32 outputs: the second pixel-block column of every tile is partly / wholly outside
        make_case("out_w_20", dense_spec((32,), "b", 32, (3, 3), (1, 1), (11, 20), 2, L, "b", 0.1), (2, 4, 4)),
        make_case("out_w_9_f32_out", dense_spec((32,), "f", 32, (3, 3), (1, 1), (11, 9), 2, L, "f", 0.1), (2, 1, 4)),
    ]


@functools.lru_cache(None)
def extra():
    """Hand-written cases for what derive8() accepts but no census plan launches; those whose key the census holds are dropped."""
    have, out = set(census()), []
    for case in _extra():
        if case.key not in have:
            have.add(case.key)
            out.append(case)
    return out


def all_cases():
    return list(census().values()) + extra()


def case_id(case):
    return key_id(case.key) if case.origin != "extra" else case.name


# ---- operands and the CPU reference (shared by the host proof and the GPU file) -----------------------------------------------------------
def bf(x):
    return x.to(torch.bfloat16).float()


def operands(case, integers, seed):
    """(sources, weight, bias) of the case's layer.  integers: sources and weights from {-1, 0, 1}, an integer bias in [-8, 8] - every sum
    is then a small integer; else Gaussian data with bf16-representable sources (so that a source can be handed over in either layout).
    The weight is what the layer's builder takes: (Cout, Cin, kh, kw), or ConvTranspose2d's (Cin, Cout, 4, 4) for "refine"."""
    spec = case.spec
    g = torch.Generator().manual_seed(seed)
    cout, cin, kh, kw = spec["w_shape"]
    wshape = (cin, cout, 4, 4) if spec["kind"] == "refine" else (cout, cin, kh, kw)
    if integers:
        rnd = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        return [rnd(-1, 1, *s) for s in spec["src_shapes"]], rnd(-1, 1, *wshape), rnd(-8, 8, cout)
    taps = 4 if spec["kind"] != "conv" else kh * kw
    return ([bf(torch.randn(*s, generator=g)) for s in spec["src_shapes"]], torch.randn(*wshape, generator=g) / math.sqrt(cin * taps),
            torch.randn(cout, generator=g) * 0.1)


def phase_weights(spec, weight):
    """[(phase weight (Cout, Cin, kh, kw) fp32, pad_top, pad_left, out_off_h, out_off_w)] as the Plan builders hand them to conv_b8."""
    if spec["kind"] == "conv":
        return [(weight, spec["pad"][0], spec["pad"][1], 0, 0)]
    if spec["kind"] == "refine":
        return [(wp, pt, pl, py, px) for (py, px), (wp, pt, pl) in engine.transposed_phase_weights(weight).items()]
    return [(wp, 0, 0, py, px) for (py, px), wp in engine.upconv_phase_weights(weight).items()]


def activate(x, act, p0):
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_LEAKY_RELU:
        return torch.where(x > 0, x, x * p0)
    return x


def reference(case, srcs, weight, bias, act, p0, dtype=torch.float64):
    """(pre-activation, activated) reference of the launch on the destination's written grid, (N, Cout, grid * step): every phase as a
    plain conv2d in `dtype` over the bf16-rounded operands, zero padding as far as the output grid asks for it."""
    spec = case.spec
    (sh, sw), (gh, gw), (sth, stw) = spec["stride"], spec["grid"], spec["out_step"]
    x = bf(torch.cat(srcs, 1)).to(dtype)
    phases = phase_weights(spec, weight)
    pre = torch.zeros(x.shape[0], phases[0][0].shape[0], gh * sth, gw * stw, dtype=dtype)       # (`weight` may hold a slice of the output channels)
    for w, pt, pl, ooh, oow in phases:
        kh, kw = w.shape[2:]
        pb, pr = max(0, (gh - 1) * sh + kh - pt - x.shape[2]), max(0, (gw - 1) * sw + kw - pl - x.shape[3])
        y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, [pl, pr, pt, pb]), bf(w).to(dtype), bias.to(dtype), stride=(sh, sw))
        pre[:, :, ooh::sth, oow::stw] = y[:, :, :gh, :gw]
    return pre, activate(pre, act, p0)


def exact_slope(seed):
    return (0.5, 0.25)[seed & 1]


def case_seed(case):
    return sum(case.spec["w_shape"]) + 31 * case.spec["grid"][1] + 7 * len(case.spec["src_shapes"])


# ---- check (c): anchor schedule and the owner of an output --------------------------------------------------------------------------------
def anchor_schedule(case):
    """Another schedule of the same layer that the library accepts: another mb, nb AND wv; preferred where it flips `wres` or walks one tile
    per workgroup.  None where the layer has none."""
    g0 = derive(case.spec, case.sched)
    found = []
    for wv in (4, 8):
        for nb in (2, 1, 4):
            for mb in (2, 1, 3, 4):
                if mb == g0["mb"] or nb == g0["nb"] or wv == g0["wv"]:
                    continue
                try:
                    library_lds(case.spec, (mb, nb, wv))
                except ValueError:
                    continue
                g = derive(case.spec, (mb, nb, wv))
                rank = 0 if g["wres"] != g0["wres"] else (1 if g0["tiles_per_wg"] > 1 and g["tiles_per_wg"] == 1 else 2)
                found.append((rank, len(found), (mb, nb, wv)))
    return min(found)[2] if found else None


def flipped_layouts(layouts):
    """Check (c): every B8 source as fp32 and every fp32 source as B8."""
    return tuple(LAYOUT_F32_NCHW if l == LAYOUT_BF16_B8 else LAYOUT_BF16_B8 for l in layouts)


def identity_templates(case):
    """The (mb, nb, wv, wres, f32src) instantiations check (c) runs next to the case's own: its anchor schedule, its flipped sources."""
    out = {template_tuple(launch_key(dict(case.spec, src_layouts=flipped_layouts(case.spec["src_layouts"])), case.sched))}
    anchor = anchor_schedule(case)
    if anchor is not None:
        out.add(template_tuple(launch_key(case.spec, anchor)))
    return out


def output_owner(spec, sched, n, co, oy, ox, ph):
    """Where the kernel computes output (n, co, oy, ox) of phase `ph` of the convolution grid under `sched`: tile, workgroup and the
    tile's position in its walk, cout group and block, wave, pixel block, lane of the D fragment."""
    g = derive(spec, sched)
    ty, tx = oy // g["th"], ox // 32
    tile = ty * g["tiles_x"] + tx
    pb = (oy % g["th"]) * 2 + (ox % 32) // 16
    return dict(tile=(ty, tx), workgroup=(tile // g["tiles_per_wg"], (co // 16) // g["mb"], n * g["nphase"] + ph), walk_pos=tile % g["tiles_per_wg"],
                tiles_per_wg=g["tiles_per_wg"], cout_group=(co // 16) // g["mb"], cout_block=(co // 16) % g["mb"], wave=pb // g["nb"],
                pixel_block=pb % g["nb"], lane=(ox % 16) + 16 * ((co % 16) // 4))
