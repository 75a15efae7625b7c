"""CPU: the helpers of tests/plan_poison.py - bit patterns, the classes of plan.buf (on stand-ins and on plans built on the CPU for
every option variant the GPU tests run), the poison fill, the snapshot report and the legal stage orders."""
import collections
import itertools
import types

import pytest
import torch

import plan_poison as pp
from monorec_amd import engine, synth
from monorec_amd.model import MonoRecModel

F32_MAX_BITS = 0x7F7FFFFF


# ---------------------------------------------------------------------------------------------------------------- patterns
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pattern", pp.FILLS)
def test_fill_round_trips_bit_for_bit(dtype, pattern):
    t = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).to(dtype)
    assert pp.fill(t, pattern) is t
    want = pp.PATTERNS[pattern][0 if dtype == torch.float32 else 1]
    b = pp.bits(t)
    assert b.dtype == (torch.int32 if dtype == torch.float32 else torch.int16) and b.data_ptr() == t.data_ptr()
    assert bool((b == want).all()) and pp.pattern_bits(pattern, dtype) == want == pp.pattern_bits(pattern, b.dtype)
    # through a copy, a clone and a device-style bit snapshot the payload is still there
    assert bool((pp.bits(t.clone()) == want).all()) and bool((pp.bits(t).to("cpu", copy=True) == want).all())
    if pattern in pp.POISONS:
        assert bool(pp.is_poison(t, pattern).all()) and bool(pp.is_poison(t).all())
        other = [p for p in pp.POISONS if p != pattern][0]
        assert not bool(pp.is_poison(t, other).any())


def test_patterns_are_what_they_claim_to_be():
    for dtype in (torch.float32, torch.bfloat16):
        nan, huge = pp.fill(torch.empty(4, dtype=dtype), "nan"), pp.fill(torch.empty(4, dtype=dtype), "huge")
        assert bool(torch.isnan(nan).all())
        assert bool(torch.isfinite(huge).all()) and float(huge.float().min()) > 3e38
        assert bool((torch.relu(huge) == huge).all())                      # survives a ReLU; the NaN need not
    # the fp32 NaN rounded or truncated to bf16 is not the bf16 pattern, and the bf16 pattern widened is not the fp32 one
    assert pp.pattern_bits("nan", torch.float32) >> 16 != pp.pattern_bits("nan", torch.bfloat16)
    assert int(pp.bits(pp.fill(torch.empty(1), "nan").to(torch.bfloat16))[0]) & 0xFFFF != pp.pattern_bits("nan", torch.bfloat16)
    assert pp.pattern_bits("huge", torch.float32) >> 16 == pp.pattern_bits("huge", torch.bfloat16)     # (the same value up to bf16 rounding)
    assert len({pp.PATTERNS[p][i] for p in pp.FILLS for i in (0,)}) == 3 and len({pp.PATTERNS[p][1] for p in pp.FILLS}) == 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_is_poison_ignores_ordinary_special_values(dtype):
    t = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1.0, 3.0e38], dtype=dtype)
    assert not bool(pp.is_poison(t).any())
    if dtype == torch.float32:
        fmax = torch.tensor([F32_MAX_BITS, 0x7FC00000, 0x7FC0DEAC, 0x7F7FBEEE, -(0x80000000 - 0x7FC0DEAD)], dtype=torch.int32).view(torch.float32)
        assert float(fmax[0]) == torch.finfo(torch.float32).max and not bool(pp.is_poison(fmax).any())
    else:
        near = torch.tensor([0x7F7E, 0x7FC0, 0x7FDC, 0x7FDE, 0x7F80], dtype=torch.int16).view(torch.bfloat16)
        assert not bool(pp.is_poison(near).any())
    t[2:4] = pp.fill(torch.empty(2, dtype=dtype), "nan")
    t[5] = pp.fill(torch.empty(1, dtype=dtype), "huge")[0]
    assert pp.is_poison(t).tolist() == [False, False, True, True, False, True, False]
    assert pp.is_poison(t, "huge").tolist() == [False] * 5 + [True, False]
    with pytest.raises(ValueError):
        pp.is_poison(t, "zero")
    with pytest.raises(TypeError):
        pp.bits(torch.zeros(2, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------- report
def _snap(**tensors):
    return collections.OrderedDict((k.replace("__", "."), pp.bits(v).clone()) for k, v in tensors.items())


def test_report_on_hand_made_snapshots():
    a32, b16 = torch.arange(8, dtype=torch.float32), torch.arange(8, dtype=torch.float32).to(torch.bfloat16)
    base = _snap(first=a32, mask__enc0__a=b16, last=a32 * 2)
    assert pp.report(base, _snap(first=a32, mask__enc0__a=b16, last=a32 * 2)) == []
    # a never-written tail: pattern on one side, on both sides, or two different patterns - all ignored
    x, y, z = a32.clone(), a32.clone(), a32.clone()
    pp.fill(x[5:], "nan"), pp.fill(y[5:], "huge")
    xb = b16.clone()
    pp.fill(xb[:2], "nan")
    for left, right in itertools.permutations([x, y, z], 2):
        assert pp.report(_snap(first=left, mask__enc0__a=xb, last=a32 * 2), _snap(first=right, mask__enc0__a=b16, last=a32 * 2)) == []
    # a real difference: named, counted, with the first flat index and both bit patterns; allocation order kept
    w = x.clone()
    w[1], w[4] = 7.0, float("nan")                                         # an ordinary NaN (a poison that went through arithmetic) is a difference
    wb = b16.clone()
    wb[3] = 0.5
    lines = pp.report(_snap(first=w, mask__enc0__a=wb, last=a32 * 2), _snap(first=z, mask__enc0__a=b16, last=a32 * 2))
    assert len(lines) == 2 and lines[0].startswith("first: 2 of 8 elements differ, first at flat index 1: 0x40e00000 vs 0x3f800000")
    assert lines[1].startswith("mask.enc0.a: 1 of 8 elements differ, first at flat index 3: 0x3f00 vs 0x4040")
    # only the listed patterns are ignored
    assert pp.report(_snap(first=x), _snap(first=z), patterns=("huge",))[0].startswith("first: 3 of 8")
    assert pp.report(_snap(first=x), _snap(first=z), patterns="nan") == []
    # NaNs with equal bits are equal; a missing or reshaped buffer is reported on either side
    n1 = torch.tensor([float("nan"), 1.0])
    assert pp.report(_snap(first=n1), _snap(first=n1.clone())) == []
    assert len(pp.report(base, _snap(first=a32, last=a32 * 2))) == 1 and len(pp.report(_snap(first=a32), base)) == 2
    assert len(pp.report(_snap(first=a32), _snap(first=a32.reshape(2, 4)))) == 1
    assert pp.poisoned_elements(_snap(first=x, last=z, mid=y), ["first", "last", "mid"]) == {"first": 3, "mid": 3}


def test_unwritten_sets_must_not_depend_on_the_fill():
    clean = torch.arange(8, dtype=torch.float32)
    x, y = clean.clone(), clean.clone()
    pp.fill(x[6:], "nan"), pp.fill(y[6:], "huge")                          # the same never-written tail in both runs
    assert pp.unwritten_sets_differ(_snap(ws=x, o=clean), _snap(ws=y, o=clean)) == []
    z = x.clone()
    pp.fill(z[2:3], "nan")                                                 # a stale NaN that went through an fma chain with its payload intact
    assert pp.report(_snap(ws=z), _snap(ws=y)) == []                       # ... is "not written" to the report
    lines = pp.unwritten_sets_differ(_snap(ws=z, o=clean), _snap(ws=y, o=clean))
    assert len(lines) == 1 and lines[0].startswith("ws: 3 elements still hold the NaN pattern") and "1 positions differ" in lines[0]
    b16 = clean.to(torch.bfloat16)
    xb, yb = b16.clone(), b16.clone()
    pp.fill(xb[:1], "nan"), pp.fill(yb[1:2], "huge")
    assert "2 positions differ" in pp.unwritten_sets_differ(_snap(b=xb), _snap(b=yb))[0]


# ---------------------------------------------------------------------------------------------------------------- stage orders
def test_legal_orders_are_exactly_the_linear_extensions():
    """encoder < encoder_tail, encoder < main, cv < main: `main` follows both `encoder` and `cv` (2 orders of those three), and `encoder_tail` goes
    anywhere behind `encoder` - 3 + 2 = 5 linear extensions, counted here from the pairs and not from the helper's own filter."""
    got = pp.legal_orders()
    assert len(got) == len(set(got)) == 5 and all(sorted(o) == sorted(pp.STAGES) for o in got)
    want = set()
    for o in itertools.permutations(pp.STAGES):                           # the partial order, spelled out pair by pair
        before = {(o[i], o[j]) for i in range(4) for j in range(i + 1, 4)}
        if {("encoder", "encoder_tail"), ("encoder", "main"), ("cv", "main")} <= before:
            want.add(o)
    assert set(got) == want
    assert set(pp.REQUIRED_ORDERS) <= want and len(set(pp.REQUIRED_ORDERS)) == 4
    assert pp.REQUIRED_ORDERS[0] == ("encoder", "encoder_tail", "cv", "main")
    for tail_at in range(1, 4):                                           # encoder_tail is free against cv and main: every position occurs
        assert any(o.index("encoder_tail") == tail_at for o in got)
    assert ("main", "encoder", "cv", "encoder_tail") not in want and ("encoder_tail", "encoder", "cv", "main") not in want


def test_run_stages_wants_each_stage_once_and_resident_outputs():
    calls = []
    plan = types.SimpleNamespace(rebind_outputs=lambda bases=None: calls.append(("rebind", bases)),
                                 run_stage=lambda stage, stream: calls.append((stage, stream)))
    stream = types.SimpleNamespace(cuda_stream=1234)
    pp.run_stages(plan, pp.REQUIRED_ORDERS[2], stream)
    assert calls == [("rebind", None)] + [(s, 1234) for s in pp.REQUIRED_ORDERS[2]]
    for bad in (("encoder", "cv", "main"), ("encoder", "encoder", "cv", "main"), pp.STAGES + ("main",)):
        with pytest.raises(ValueError):
            pp.run_stages(plan, bad, stream)


# ---------------------------------------------------------------------------------------------------------------- classes
def _stand_in(names, **attrs):
    geom = torch.zeros(9 + 24)
    buf = collections.OrderedDict()
    for n in names:
        buf[n] = {"geom": geom, "kinv": geom[:9].view(1, 9), "proj": geom[9:].view(1, 2, 12)}.get(n)
        if buf[n] is None:
            buf[n] = torch.zeros(2, 8, dtype=torch.bfloat16 if n.endswith("_b8") else torch.float32)
    return types.SimpleNamespace(buf=buf, **attrs)


FULL_NAMES = ["keyframe", "frames", "geom", "kinv", "proj", "depths", "feat0", "keyframe_norm", "resnet.pool", "resnet.l1b0.t", "resnet.l1b0.o",
              "feat1", "resnet.l2b0.idt", "feat4", "sfcv", "cost_volume", "mask.enc0.a", "mask.enc1.pool", "mask.cvf4", "mask.dec3.x",
              "cv_mask", "depth.enc4.1.out", "depth.dec0", "pred3", "depth.dec1.t", "depth.dec1.mid", "depth.dec1", "depth.dec4", "pred0",
              "splitk_workspace.encoder", "splitk_workspace.main", "pix_depths"]


def test_classify_on_a_stand_in():
    got = pp.classify(_stand_in(FULL_NAMES))
    assert list(got) == FULL_NAMES                                         # allocation order
    assert [n for n, c in got.items() if c == pp.INPUT] == ["keyframe", "frames", "geom", "kinv", "proj", "depths", "pix_depths"]
    assert [n for n, c in got.items() if c == pp.OUTPUT] == ["feat0", "feat1", "feat4", "sfcv", "cost_volume", "cv_mask", "pred3", "pred0"]
    assert pp.CONSTANT not in got.values() and pp.class_counts(_stand_in(FULL_NAMES)) == {pp.INPUT: 7, pp.OUTPUT: 8, pp.SCRATCH: 17}
    # the option variants move names between the classes
    assert pp.classify(_stand_in(FULL_NAMES, lean_active=True))["sfcv"] == pp.SCRATCH
    for pm in (1, 3):
        assert pp.members(_stand_in(FULL_NAMES, pretrain_mode=pm), pp.CONSTANT) == ["cv_mask"]
    assert pp.classify(_stand_in(FULL_NAMES, pretrain_mode=2))["cv_mask"] == pp.OUTPUT
    assert pp.members(_stand_in(FULL_NAMES, no_cv=True), pp.CONSTANT) == ["sfcv", "cost_volume"]
    extra = pp.classify(_stand_in(FULL_NAMES + ["mask.zero_input", "mask.zero_feat3", "prev_depth", "mask.sfcv_mean", "sfcv_b8", "feat2_b8"]))
    assert [extra[n] for n in ("mask.zero_input", "mask.zero_feat3", "prev_depth", "mask.sfcv_mean", "sfcv_b8", "feat2_b8")] == \
        [pp.CONSTANT, pp.CONSTANT, pp.INPUT, pp.SCRATCH, pp.SCRATCH, pp.SCRATCH]


@pytest.mark.parametrize("name", ["depth.dec5", "mask.enc0.pool", "mask.zero_feat4", "feat4_b8", "splitk_workspace.tail", "scratch", "resnet.l5b0.t",
                                  "depth.dec3.t", "cost_volume_b16"])
def test_classify_rejects_a_name_it_cannot_place(name):
    with pytest.raises(KeyError, match="in no class"):
        pp.classify(_stand_in(FULL_NAMES + [name]))


def test_poison_on_a_stand_in_follows_views():
    plan = _stand_in(FULL_NAMES)
    for t in plan.buf.values():
        t.fill_(1.0)
    plan.buf["feat1.view"] = plan.buf["feat1"][1]                          # (not a name of the engine: placed by hand below)
    plan.buf["resnet.l1b0.t"] = plan.buf["resnet.l1b0.o"].view(16)         # two scratch names on one storage: filled once
    real = pp.classify

    def with_view(p):
        c = real(types.SimpleNamespace(buf={n: t for n, t in p.buf.items() if n != "feat1.view"}))
        c["feat1.view"] = pp.OUTPUT
        return c
    pp.classify = with_view
    try:
        filled = pp.poison(plan, "nan")
    finally:
        pp.classify = real
    assert "feat1" in filled and "feat1.view" not in filled and ("resnet.l1b0.t" in filled) != ("resnet.l1b0.o" in filled)
    assert bool(pp.is_poison(plan.buf["feat1"], "nan").all()) and bool(pp.is_poison(plan.buf["resnet.l1b0.o"], "nan").all())
    for n in ("keyframe", "frames", "geom", "kinv", "proj", "depths", "pix_depths"):
        assert bool((plan.buf[n] == 1.0).all()), n
    # a scratch buffer laid over an input is refused, not filled
    bad = _stand_in(FULL_NAMES)
    bad.buf["depth.dec3"] = bad.buf["geom"][4:12]
    with pytest.raises(ValueError, match="shares memory"):
        pp.poison(bad, "huge")
    assert not bool(pp.is_poison(bad.buf["geom"]).any())


# real plans, built on the CPU (the launches are never run): every configuration family of tests/test_gpu_plan_poison.py
def test_option_cases_cover_those_of_the_model_tests():
    import test_gpu_model
    assert {k: pp.OPTION_CASES.get(k) for k in test_gpu_model.OPTION_CASES} == test_gpu_model.OPTION_CASES and len(test_gpu_model.OPTION_CASES) == 7
    assert sorted(pp.EXPECTED_CONSTANTS) == sorted(pp.OPTION_CASES)


def cpu_plan(depths=8, batch=1, bf16=0, lean=False, skip_layer4=False, **kw):
    m = MonoRecModel(cv_depth_steps=depths, **kw)
    sd = synth.seeded_state_dict(m.state_dict(), seed=0)
    return engine.Plan(sd, batch, 64, 96, 2, depths, m.inv_depth_min_max, "cpu", bf16=bf16, sfcv_mult_mask=m.sfcv_mult_mask,
                       pretrain_mode=m.pretrain_mode, no_cv=m.no_cv, mask_use_cv=m.mask_use_cv or m.simple_mask,
                       mask_use_feats=m.mask_use_feats or m.simple_mask, simple_mask=m.simple_mask, cv_patch_size=m.cv_patch_size,
                       lean_outputs=lean, skip_layer4=skip_layer4)


@pytest.mark.parametrize("case", sorted(pp.OPTION_CASES))
def test_classify_places_every_buffer_of_each_option_variant(hip_lib, case):
    plan = cpu_plan(**pp.OPTION_CASES[case])
    cls = pp.classify(plan)
    assert list(cls) == list(plan.buf)
    assert [n for n, c in cls.items() if c == pp.CONSTANT] == pp.EXPECTED_CONSTANTS[case]
    assert [n for n, c in cls.items() if c == pp.INPUT] == [n for n in plan.buf if n in ("keyframe", "frames", "geom", "kinv", "proj", "depths", "prev_depth")]
    assert ("prev_depth" in plan.buf) == (case == "simple")
    outs = [n for n in engine.OUTPUT_BUFFERS if n in plan.buf and n not in pp.EXPECTED_CONSTANTS[case]]
    assert sorted(n for n, c in cls.items() if c == pp.OUTPUT) == sorted(outs)
    for n in pp.EXPECTED_CONSTANTS[case]:                                     # zeroed when the plan was built
        assert not bool(plan.buf[n].any()), n


def test_classify_and_poison_on_the_full_model_in_fp32_and_bf16(hip_lib):
    full = cpu_plan()
    counts = pp.class_counts(full)
    assert pp.CONSTANT not in counts and counts[pp.INPUT] == 6 and counts[pp.OUTPUT] == 12 and counts[pp.SCRATCH] > 20
    assert any(n.startswith("splitk_workspace.") for n in pp.members(full, pp.SCRATCH))
    skip = cpu_plan(skip_layer4=True)
    assert "feat4" not in skip.buf and pp.class_counts(skip)[pp.OUTPUT] == 11 and not skip.stages["encoder_tail"]
    b8 = cpu_plan(depths=32, bf16=1)
    lean = cpu_plan(depths=32, bf16=1, lean=True)
    off = cpu_plan(depths=8, bf16=1, lean=True)                            # no fusion kernel that writes B8 copies at D = 8: the option falls back
    assert lean.lean_active and not b8.lean_active and not off.lean_active
    assert pp.classify(b8)["sfcv"] == pp.OUTPUT == pp.classify(off)["sfcv"] and pp.classify(lean)["sfcv"] == pp.SCRATCH
    for plan in (b8, lean):
        assert {"sfcv_b8", "cost_volume_b8", "feat0_b8"} <= set(pp.members(plan, pp.SCRATCH))
        assert any(plan.buf[n].dtype == torch.bfloat16 for n in pp.members(plan, pp.SCRATCH))
    assert "sfcv_b8" not in off.buf and "cost_volume_b8" not in off.buf
    # the real fill: scratch and outputs hold the pattern in their own number format, inputs and tables keep their bits
    before = {n: full.buf[n].clone() for n in pp.members(full, pp.INPUT)}
    for plan, pattern in ((full, "nan"), (lean, "huge")):
        filled = pp.poison(plan, pattern)
        assert sorted(filled) == sorted(pp.members(plan, pp.SCRATCH) + pp.members(plan, pp.OUTPUT))
        assert all(bool(pp.is_poison(plan.buf[n], pattern).all()) for n in filled)
        assert not any(bool(pp.is_poison(plan.buf[n]).any()) for n in pp.members(plan, pp.INPUT))
    assert all(torch.equal(pp.bits(full.buf[n]), pp.bits(t)) for n, t in before.items())
    snap = pp.snapshot(full)
    assert list(snap) == list(full.buf) and all(t.device.type == "cpu" and t.dtype == torch.int32 for t in snap.values())
    assert snap["feat0"].data_ptr() != full.buf["feat0"].data_ptr()
    assert pp.poisoned_elements(snap, ["feat0", "depths"]) == {"feat0": full.buf["feat0"].numel()}
    pp.poison(full, "zero")
    assert pp.report(snap, pp.snapshot(full)) == []                        # (pattern against zeros: nothing either side computed)
