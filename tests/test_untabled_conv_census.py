"""Host side (no GPU): the census of rule-chosen convolution launches (tests/untabled_conv_census.py) that
tests/test_gpu_untabled_conv_forms.py runs - its size pinned, what its shapes must contain, its representatives, and the CLOSURE SWEEP:
over a declared domain of input shapes every plan builds, builds the same twice, and launches no extended key outside (family censuses +
this census).  A change of a rule (engine.nearest_schedules, nearest_form, choose_winograd*, choose_schedule, Plan.b8_schedule), of a
table or of a kernel's validation that sends a layer of the domain to compiled code no exact test runs fails here, naming shape, layer
and key."""
import collections
import os

import b8_conv_census as b8c
import direct_conv_census as dcc
import pointwise_paths
import untabled_conv_census as census

# new extended keys per family and arithmetic mode (direct) / kernel family (reduced), as measured when written
KEY_COUNTS = {"direct": {0: 234, 1: 42, 2: 40}, "reduced": {"w22": 13, "w44": 5, "w44s": 5, "t22": 8, "f23": 6, "ct": 12, "up": 2}, "b8": {"b8": 80}}
SUB_TILE_KEYS, BOTH_SUB_TILE_KEYS = 267, 73          # of them: sub-tile in some direction / in rows and columns
WALK_KEYS = 22                                       # B8 keys with a tile walk: > 1024 jobs, the cost b8_conv_census.MAX_GMAC_WALK allows
# Representatives above MAX_GMAC that are no B8 walk: the 3x3 over 512 channels of ResNet layer4 (2.4 million multiply-adds per output:
# MAX_GMAC is 127 outputs) and the four-phase Refine head over 16 x 16 taps, at batch 1 on one tile plus a ragged remainder or on the
# launch's own sub-tile extent (sub-tile in both directions: the layer as it is, batch 2) - the least there is.  Bounded by 2.5 x
# MAX_GMAC, the allowance tests/test_reduced_conv_census.py gives its representatives; the dearest is 0.71 GMAC.
HEAVY = 13
EXISTING_SUB_TILE = {"reduced": 14, "direct": 5, "b8": 3}        # cases of the three family censuses that are sub-tile in some direction
# Refusals: (family, schedule / form, geometry) the library's validation had to learn to refuse because a representative failed on the
# device.  None: every representative passed as the rules chose it.
REFUSED = []


def test_shapes_hold_every_condition_the_census_is_declared_for(hip_lib):
    shapes = census.UNTABLED_SHAPES
    assert shapes[:10] == census.SURVEYED_SHAPES and len(set(shapes)) == len(shapes) and len(census.SURVEYED_SHAPES) == 10
    assert all(h % 32 == 0 and w % 32 == 0 for _, h, w, _, _ in shapes)
    tabled = {(h, w) for _, h, w, _, _ in dcc.FP32_SHAPES + b8c.PLAN_SHAPES}
    assert any(h // 32 == 1 or w // 32 == 1 for _, h, w, _, _ in shapes)
    assert any((h // 32) % 2 or (w // 32) % 2 for _, h, w, _, _ in shapes)
    assert any((w // 32) % 4 for _, h, w, _, _ in shapes)
    assert any(b not in (1, 2, 4, 8) and (h, w) in tabled for b, h, w, _, _ in shapes)
    assert {1, 3} <= {f for _, _, _, f, _ in shapes}
    assert any(h * w > max(th * tw for th, tw in tabled) for _, h, w, _, _ in shapes)
    by_size = sorted(census.SURVEYED_SHAPES, key=lambda s: s[1] * s[2])
    assert len(census.BF16X3_SHAPES) >= 3 and {by_size[0], by_size[-1]} <= set(census.BF16X3_SHAPES) <= set(shapes)
    assert set(census.sweep_shapes()) >= set(census.CLOSURE_SHAPES)          # nothing rides along that the sweep did not force in


def test_census_size_is_pinned(hip_lib):
    reps = census.census()
    counts = collections.defaultdict(collections.Counter)
    for ext in reps:
        counts[ext[0]][census.mode_of(ext)] += 1
    got = {f: dict(c) for f, c in counts.items()}
    print(f"untabled census: {len(census.launches())} launches of {len(census.UNTABLED_SHAPES)} shapes, {len(reps)} new extended keys: {got}")
    # the keys by name (tests/golden/untabled_conv_keys.txt, one id per line): a rule, table or validation change that moves a launch of these
    # shapes to another key is named here - shape and build, layer, key - before the counts below report it as a number
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "untabled_conv_keys.txt")) as f:
        pinned = set(f.read().split())
    added = [f"{r.launch.origin} {r.launch.name}: {census.ext_id(e)}" for e, r in reps.items() if census.ext_id(e) not in pinned]
    gone = sorted(pinned - {census.ext_id(e) for e in reps})
    assert not added and not gone, (f"{len(added)} extended keys are new to the census, e.g. " + "; ".join(added[:5]) +
                                    f" - {len(gone)} are no longer launched, e.g. " + "; ".join(gone[:5]))
    assert got == KEY_COUNTS, got
    assert (sum(any(e[2:]) for e in reps), sum(e[2] and e[3] for e in reps)) == (SUB_TILE_KEYS, BOTH_SUB_TILE_KEYS)
    ids = [census.ext_id(e) for e in reps]
    assert len(set(ids)) == len(ids)                      # the readable ids the GPU file is parametrised with name the keys one to one
    assert not (set(reps) & census.existing_ext())


def test_every_surveyed_shape_runs_on_the_rules(hip_lib):
    per = collections.defaultdict(lambda: [0, 0])
    for l in census.launches():
        per[l.origin.split("_f32_")[0].split("_bf16")[0]][0 if l.rule else 1] += 1
    for b, h, w, f, d in census.SURVEYED_SHAPES:
        rule, tabled = per[f"b{b}_{h}x{w}_f{f}_d{d}"]
        assert rule > 0, (b, h, w, f, d)
        if (h, w) in ((192, 448), (32, 32)):
            assert tabled == 0, (b, h, w, f, d, tabled)
    # every family takes part, and the new keys come from rule-chosen launches
    assert {l.family for l in census.launches() if l.rule} == {"direct", "reduced", "b8"}
    assert all(r.launch.rule for r in census.census().values())


def test_representatives_keep_their_extended_key_and_everything_but_the_image_size(hip_lib):
    """The extended key of every representative is re-derived through the library (mr_conv2d_lds_bytes, mr_conv2d_b8_lds_bytes) for the
    shrunken layer; a sub-tile direction keeps the launch's own extent; nothing but grid and batch changes."""
    heavy, walk = [], 0
    for ext, rep in census.census().items():
        tag = census.ext_id(ext)
        args, full = census.rep_args(rep), rep.launch.args
        assert census.ext_of(rep.launch) == ext == census.ext_of(rep.launch._replace(args=args)), tag
        if rep.family == "reduced":
            small, orig = args[0], full[0]
            assert small == orig._replace(hw=small.hw, batch=small.batch), tag
            (gh, gw), (oh, ow), batch, obatch = small.hw, orig.hw, small.batch, orig.batch
            assert small.hw[1] % 4 == 0
        else:
            small, orig = args[0], full[0]
            fields = (("w_shape", "stride", "pad", "in_mode", "tf", "act", "p0", "p1", "residual", "out_step", "out_off", "phases") if rep.family == "direct"
                      else ("src_layouts", "w_shape", "stride", "pad", "act", "p0", "out_layout", "out_step", "kind"))
            for field in fields:
                assert small[field] == orig[field], (tag, field)
            assert [s[1] for s in small["src_shapes"]] == [s[1] for s in orig["src_shapes"]] and tuple(args[1:]) == tuple(full[1:]), tag
            (gh, gw), (oh, ow), batch, obatch = small["grid"], orig["grid"], small["src_shapes"][0][0], orig["src_shapes"][0][0]
        assert batch <= max(2, obatch)
        if ext[2]:
            assert gh == oh, tag
        if ext[3]:
            assert gw == ow, tag
        if ext[2] and ext[3]:
            assert batch == min(obatch, 2), tag
        macs = census.macs_of(rep.family, args)
        if rep.family == "b8" and ext[1].walk:
            walk += 1
            assert b8c.is_walk_representative(*args) and macs <= b8c.MAX_GMAC_WALK * 1e9, (tag, macs)
            continue
        assert census.device_bytes(rep) <= pointwise_paths.MAX_DEVICE_BYTES, (tag, census.device_bytes(rep))
        if macs > census.MAX_GMAC * 1e9:
            heavy.append(tag)
            assert (batch == 1 or (ext[2] and ext[3])) and macs <= 2.5 * census.MAX_GMAC * 1e9, (tag, macs)
    assert walk == WALK_KEYS and len(heavy) == HEAVY, (walk, heavy)


def test_existing_cases_have_their_sub_tile_flags_computed(hip_lib):
    """The family censuses' own cases are sub-tile only where the reduced shrink capped at the layer, in the `below_one_tile` extras of the
    reduced forms, in the `out_w_20` / `out_w_9` extras of the B8 kernel and where the direct shrink went below one tile of columns for rows of
    fewer than 32 outputs: the flags are computed for every case, and how many carry one is pinned."""
    have = census.existing_ext()
    sub = collections.Counter(e[0] for e in have if any(e[2:]))
    print(f"sub-tile extended keys among the {len(have)} of the family censuses: {dict(sub)}")
    assert dict(sub) == EXISTING_SUB_TILE, dict(sub)
    assert REFUSED == []


def test_closure_sweep(hip_lib):
    """Over sweep_shapes() - every (H, W) of SWEEP_H x SWEEP_W with W >= H / 2; batch {1, 3, 5}, frames {1, 2, 3}, D {4, 8, 32} in rotation -
    for fp32 "table" and bf16: the plan builds (no ValueError("no launchable schedule")), builds the same conv_log twice, and every
    launch's extended key is in (family censuses + untabled census).  A key outside means: its shape goes into CLOSURE_SHAPES."""
    known = census.existing_ext() | set(census.census())
    shapes = census.sweep_shapes()
    assert len(shapes) == 89 and {(s[0], s[3], s[4]) for s in shapes} == {(b, f, d) for b in (1, 3, 5) for f in (1, 2, 3) for d in (4, 8, 32)}
    thirds = [shapes[:30], shapes[30:60], shapes[60:]]                 # small, middle and large planes meet every value
    for part in thirds:
        assert {s[0] for s in part} == {1, 3, 5} and {s[3] for s in part} == {1, 2, 3} and {s[4] for s in part} == {4, 8, 32}
    outside, launches = [], 0
    for shape in shapes:
        for mode, forms, heads in census.SWEEP_BUILDS:
            origin = census.origin_of(shape, mode, forms, heads)
            try:
                first, second = census.build_plan(shape, mode, forms, heads).conv_log, census.build_plan(shape, mode, forms, heads).conv_log
            except (ValueError, RuntimeError, AssertionError) as e:        # no launchable schedule / refused by the library / by a builder
                raise AssertionError(f"{origin}: the plan does not build - {type(e).__name__}: {e}")
            assert first == second, f"{origin}: two builds of the plan give different conv_logs"
            for c in first:
                l = census.reduce_launch(c, origin)
                launches += 1
                if l.ext not in known:
                    outside.append(f"{origin} {l.name}: {census.ext_id(l.ext)}")
    print(f"closure sweep: {len(shapes)} shapes x {len(census.SWEEP_BUILDS)} builds, {launches} launches, {len(outside)} outside the censuses")
    assert not outside, f"{len(outside)} launches run compiled code / geometry no exact test runs, e.g. " + "; ".join(outside[:5])
