"""Host side (no GPU): the census of mr_conv2d_b8 forms (tests/b8_conv_census.py) that tests/test_gpu_b8_conv_forms.py runs - what it must
contain, its size pinned so that a table, rule or dispatch change shows up as a diff here, and the proof that the exact check of the GPU
file loses nothing to the bf16 rounding of a B8 destination."""
import collections
import itertools

import torch

import b8_conv_census as census
from monorec_amd import engine, synth
from monorec_amd._lib import ACT_RELU, LAYOUT_BF16_B8

# keys of the census plans / of which `walk` / hand-written cases whose key no plan has, counted when the census was written
KEY_COUNT, WALK_KEY_COUNT, EXTRA_COUNT = 131, 28, 22
MAX_TILES_PER_WG = 16                  # the longest walk of a census plan launch (the representatives walk 2 tiles, "walk_5_tiles" 5, "walk_16_tiles" 16)
HEAVIEST = "bb-b-mb3nb4wv8-wres-k3x3s1x1-p1-walk-q2-pp2-leaky"         # the representative with the dearest CPU reference (18.3 GMAC)
TEMPLATES_COVERED = 43                 # of the 96 (mb, nb, wv, wres, f32src) instantiations
IDENTITY_RUNS = (152, 24)                # cases with an anchor schedule, further instantiations that check (c) of the GPU file runs

# tuned_b8.json entries no census plan reaches.  All of one kind: the `_f1` variants of decoder layers whose only fp32 sources are image
# features.  Plans hand the decoders B8 copies of the features (Plan.b8_feature_copies, csrc: mr_f32_nchw_to_b8), which makes these
# launches `_f0`; the `_f1` entries were measured with MR_B8_FEATS=0 - the A/B aid that lets the decoders read the fp32 features - and are
# live only under it (test_unreached_table_entries_are_the_fp32_feature_variants builds that plan).
UNREACHED = ["b8_co96_ci64+64+96_k3x3_s1x1_o128x256_b1_p1_f1", "b8_co96_ci96+128+96_k3x3_s1x1_o64x128_b1_p1_f1",
             "b8_co96_ci96+256_k2x2_s1x1_o32x64_b1_p4_f1"]


def test_census_size_is_pinned_and_every_launch_restates_the_library(hip_lib):
    """The key set is stable, and derive() - the restatement of derive8() that wres, PLANE, nchunks and tiles_per_wg come from - answers
    the library's LDS bytes for every launch of every census plan (library_lds asserts it)."""
    cases = census.census()
    tpw = 0
    for spec, sched, name, sig, origin in census.launches():
        assert census.library_lds(spec, sched) == census.derive(spec, sched)["lds"]
        tpw = max(tpw, census.derive(spec, sched)["tiles_per_wg"])
    walk = sum(k.walk for k in cases)
    extra = census.extra()
    print(f"B8 census: {len(census.launches())} launches of {len(census.PLAN_SHAPES)} plans, {len(cases)} keys, {walk} of them walk keys, "
          f"{len(extra)} extra cases; longest walk of a plan launch: {tpw} tiles")
    assert (len(cases), walk, len(extra), tpw) == (KEY_COUNT, WALK_KEY_COUNT, EXTRA_COUNT, MAX_TILES_PER_WG)
    ids = [census.case_id(c) for c in census.all_cases()]
    assert len(set(ids)) == len(ids)                      # the readable ids the GPU file is parametrised with name the cases one to one
    assert len({c.key for c in census.all_cases()}) == len(ids)
    assert census.kernel_constants() == (1024, 2, 64)     # read from csrc/conv_b8.hip: a change there re-derives every walk representative


def test_representatives_keep_their_key_and_everything_but_the_image_size(hip_lib):
    origin = {}
    for spec, sched, name, sig, where in census.launches():
        origin.setdefault((name, where), (spec, sched))
    heaviest = max(census.all_cases(), key=lambda c: census.macs(c.spec))
    assert census.case_id(heaviest) == HEAVIEST and census.macs(heaviest.spec) <= census.MAX_GMAC_WALK * 1e9
    for key, case in census.census().items():
        spec, sched = origin[(case.name, case.origin)]
        small = case.spec
        assert tuple(sched) == case.sched and census.launch_key(spec, sched) == key == census.launch_key(small, case.sched)
        for field in ("src_layouts", "w_shape", "stride", "pad", "act", "p0", "out_layout", "out_step", "kind"):
            assert small[field] == spec[field], (census.key_id(key), field)
        assert census.src_channels_of(small) == census.src_channels_of(spec)
        g = census.derive(small, case.sched)
        assert small["grid"][0] % g["th"] and small["grid"][1] % 32 and g["tiles_x"] >= 2 and g["tiles_y"] >= 2, (census.key_id(key), small["grid"])
        if key.walk:
            assert census.is_walk_representative(small, case.sched) and g["jobs"] > census.kernel_constants()[0]
            assert census.macs(small) <= census.MAX_GMAC_WALK * 1e9, (census.key_id(key), census.macs(small))
        else:
            # (the four-phase layers over 256 - 576 channels are above MAX_GMAC at two tiles in each direction and batch 1: the least there is)
            least = small["src_shapes"][0][0] == 1 and g["tiles_x"] == g["tiles_y"] == 2
            assert g["tiles_per_wg"] == 1 and (census.macs(small) <= census.MAX_GMAC * 1e9 or least), (census.key_id(key), census.macs(small))
    for case in census.extra():
        assert census.launch_key(case.spec, case.sched) == case.key and census.macs(case.spec) <= census.MAX_GMAC * 1e9
        assert not case.key.walk or census.is_walk_representative(case.spec, case.sched), case.name


def test_every_table_entry_is_launched_by_a_census_plan_or_pinned_as_unreached(hip_lib):
    sigs = collections.defaultdict(set)
    for _, _, _, sig, origin in census.launches():
        sigs[sig].add(origin)
    missing = sorted(k for k in engine.B8_SCHEDULES if k not in sigs)
    print(f"tuned_b8.json: {len(engine.B8_SCHEDULES) - len(missing)} of {len(engine.B8_SCHEDULES)} entries reached; unreached: {missing}")
    assert missing == sorted(UNREACHED), (sorted(set(missing) - set(UNREACHED)), sorted(set(UNREACHED) - set(missing)))
    # Plan.b8_schedule's rule is covered: no launch of RULE_SHAPE has a table entry
    b, h, w, f, d = census.RULE_SHAPE
    rule = [s for s, origins in sigs.items() if f"b{b}_{h}x{w}_f{f}_d{d}" in origins]
    assert rule and not any(s in engine.B8_SCHEDULES for s in rule)


def test_unreached_table_entries_are_the_fp32_feature_variants(hip_lib, monkeypatch):
    """With MR_B8_FEATS=0 (the decoders read the fp32 image features) the 512 x 1024 plan launches exactly the UNREACHED entries."""
    from monorec_amd import MonoRecModel
    monkeypatch.setenv("MR_B8_FEATS", "0")
    b, h, w, f, d = 1, 512, 1024, 4, 48
    plan = engine.Plan(synth.seeded_state_dict(MonoRecModel(cv_depth_steps=d).state_dict()), b, h, w, f, d, (0.33, 0.0025), "cpu", bf16=1)
    got = {c["sig"] + f"_f{int(c['f32_source'])}" for c in plan.conv_log if c.get("b8")}
    assert set(UNREACHED) <= got


def test_template_coverage_is_listed(hip_lib):
    """The (mb, nb, wv, wres, f32src) instantiations that neither the census nor the extra cases run, for the reader; the count is pinned."""
    ran = {census.template_tuple(c.key) for c in census.all_cases()}
    every = set(itertools.product((1, 2, 3, 4), (1, 2, 4), (4, 8), (False, True), (False, True)))
    assert ran <= every
    uncovered = sorted(every - ran)
    print(f"conv_b8_kernel<MB, NB, WV, WRES, F32SRC>: {len(ran)} of {len(every)} instantiations run; not run: " +
          " ".join(f"<{mb},{nb},{wv},{int(wres)},{int(f32)}>" for mb, nb, wv, wres, f32 in uncovered))
    assert len(ran) == TEMPLATES_COVERED
    also = set().union(*(census.identity_templates(c) for c in census.all_cases())) - ran
    anchored = sum(census.anchor_schedule(c) is not None for c in census.all_cases())
    print(f"check (c) - {anchored} of {len(census.all_cases())} cases have an anchor schedule - runs {len(also)} more for bit identity with a case's own: " +
          " ".join(f"<{mb},{nb},{wv},{int(wres)},{int(f32)}>" for mb, nb, wv, wres, f32 in sorted(also)))
    assert (anchored, len(also)) == IDENTITY_RUNS
    wide = {(mb, nb, wv) for mb, nb, wv, _, _ in ran}
    assert any(nb == 4 and wv == 4 for _, nb, wv in wide) and sum(mb == 4 for mb, _, _ in wide) >= 4      # what test_gpu_b8.py never / barely runs


def test_exact_operands_are_lossless_on_a_b8_destination(hip_lib):
    """Check (a) of the GPU file compares a B8 destination - rounded to 8 significant bits - with the reference for EQUALITY.  That
    proves something only if the rounding cannot hide an error: for every case with a B8 destination, every reference value of the exact
    operands, before and after the activation, survives the round trip through bf16; and with ONE weight changed by +-1 at one
    (cout, cin, tap) the ROUNDED references differ at every output that the changed weight reaches with a non-zero source value
    (after ReLU: at every such output that is positive on either side)."""
    n = 0
    for case in census.all_cases():
        spec = case.spec
        if spec["out_layout"] != LAYOUT_BF16_B8:
            continue
        n += 1
        seed = census.case_seed(case)
        srcs, weight, bias = census.operands(case, True, seed)
        p0 = census.exact_slope(seed)
        pre, ref = census.reference(case, srcs, weight, bias, spec["act"], p0, dtype=torch.float32)
        tag = census.case_id(case)
        assert pre.abs().max().item() < 2 ** 24 and torch.equal(pre, pre.round()), tag
        assert torch.equal(census.bf(pre), pre) and torch.equal(census.bf(ref), ref), (tag, float(pre.abs().max()))
        # one weight of the builder's weight tensor, one step up or down (for a four-phase layer it lands in one or more phase filters)
        g = torch.Generator().manual_seed(seed)
        idx = tuple(int(torch.randint(0, s, (1,), generator=g)) for s in weight.shape)
        co = idx[1] if spec["kind"] == "refine" else idx[0]
        delta = 1.0 if (seed >> 1) & 1 else -1.0
        w2 = weight.clone()
        w2[idx] += delta
        one = (lambda w: w[:, co:co + 1]) if spec["kind"] == "refine" else (lambda w: w[co:co + 1])
        pre1, ref1 = census.reference(case, srcs, one(weight), bias[co:co + 1], spec["act"], p0, dtype=torch.float32)
        pre2, ref2 = census.reference(case, srcs, one(w2), bias[co:co + 1], spec["act"], p0, dtype=torch.float32)
        assert torch.equal(pre1[:, 0], pre[:, co]) and torch.equal(ref1[:, 0], ref[:, co]), tag
        reached = pre1 != pre2
        assert reached.any() and float((pre2 - pre1).abs().max()) == 1.0, tag
        assert torch.equal(census.bf(pre2) != census.bf(pre1), reached), tag
        seen = reached & ((pre1 > 0) | (pre2 > 0)) if spec["act"] == ACT_RELU else reached
        assert torch.equal(census.bf(ref2) != census.bf(ref1), seen), tag
    assert n >= 100
