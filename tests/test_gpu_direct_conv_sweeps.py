"""GPU (MI355X): mr_conv2d_f32 (csrc/conv_mfma.hip) instantiation by instantiation.

tests/direct_conv_census.py reduces every direct-kernel launch of the measured tables to the key its compiled code depends on (register
tile, workgroup size, arithmetic, staging form, specialised plane pitch, sweep functions, filter, stride, phases, split-K) and keeps one
shrunken layer per key.  Each runs here ALONE, through engine.Plan.bare(...).conv(...) under its own schedule:

  a. exact     small-integer operands: every partial sum is an integer below 2^24, fp32 accumulation is exact in any order (fp32, bf16 -
               the operands are bf16-representable - and bf16x3 alike), so the output must EQUAL the fp64 reference: no tolerance.
  b. gaussian  the bound the kernel tests use, 2e-4 * max(1, |ref|max), against fp64 (bf16: against fp64 of the bf16-rounded operands).
  c. order     the k order of an output is chunk order, tap-major, channel quads ascending, whatever the register tile, the workgroup
               size and the form of the sweep (pipelined with a compiled-in pitch / run-time pitch): the same layer under an anchor
               schedule - same chunking, other tile, a pitch outside the menu (census.anchor_schedule; the few layers that have no such
               schedule are pinned by name in tests/test_direct_conv_census.py) - is bit-identical.
  d. footprint the output lies between guard channels in a tensor prefilled with a sentinel: nothing outside the written positions
               changes, no written position keeps the sentinel, repetitions are bit-identical."""
import math

import pytest
import torch
import torch.nn.functional as F

import direct_conv_census as census
from monorec_amd import engine
from monorec_amd._lib import (ACT_ABS_TANH_AFFINE, ACT_LEAKY_RELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, IN_MAXPOOL2, IN_UPSAMPLE2, TF_RESNET_NORM)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3                                   # untouched channels below and above the written slice
SENTINEL_BITS = 0x7A5A5A5A                  # a finite fp32 (2.8e35) no result takes
REPS = 3

# what the tables do not launch but derive() accepts
EXTRA = [
    # ck = 128 with a tail chunk of 4 channels (132 = 128 + 4): 32 channel quads through the pipelined sweep, then one through the generic
    census.make_case("ck128_tail4", census.dense_spec((132,), 40, (1, 3), (1, 1), (0, 1), (11, 28), 2, ACT_LEAKY_RELU, p0=0.1), (1, 1, 1, 128, 4, 0)),
    # the last source leaves a generic-sweep tail behind pipelined chunks - on a menu pitch (ck 16) and with 32-channel chunks
    census.make_case("ck16_pipe_then_generic", census.dense_spec((32, 20), 48, (3, 3), (1, 1), (1, 1), (11, 72), 2, ACT_LEAKY_RELU, p0=0.1),
                     (2, 2, 1, 16, 4, 0)),
    census.make_case("ck32_pipe_then_generic", census.dense_spec((64, 40), 40, (3, 3), (1, 1), (1, 1), (11, 72), 2, ACT_RELU, residual=True),
                     (1, 2, 1, 32, 8, 0)),
    # the staging forms no table shape reaches (every tabled source width is a multiple of 4; max-pool and keyframe normalisation have
    # their own kernels in the plans): dword LDS-DMA for a ragged width and for the x2 upsampling read, register staging for the rest
    census.make_case("dword_dma_width_70", census.dense_spec((48,), 48, (3, 3), (1, 1), (1, 1), (11, 70), 2, ACT_LEAKY_RELU, p0=0.1), (2, 2, 1, 16, 4, 0)),
    census.make_case("dword_dma_upsample2", dict(census.dense_spec((96, 20), 48, (2, 2), (1, 1), (0, 0), (5, 35), 2, ACT_NONE, in_mode=IN_UPSAMPLE2),
                                                 grid=(10, 70), out_shape=(2, 48, 10, 70)), (3, 1, 1, 16, 4, 0)),
    census.make_case("register_staged_maxpool2", census.dense_spec((32,), 48, (3, 3), (1, 1), (1, 1), (22, 140), 2, ACT_LEAKY_RELU, p0=0.1,
                                                                   in_mode=IN_MAXPOOL2), (3, 2, 1, 16, 4, 0)),
    census.make_case("register_staged_resnet_norm", census.dense_spec((3,), 64, (7, 7), (2, 2), (3, 3), (42, 134), 2, ACT_RELU, tf=TF_RESNET_NORM),
                     (2, 2, 1, 8, 4, 0)),
]
CASES = list(census.census().values()) + EXTRA
IDS = [census.key_id(c.key) if c.origin != "extra" else c.name for c in CASES]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _operands(case, integers, seed):
    """(sources, [weight per phase], bias, residual or None) of the case's layer: small integers (check a) or Gaussian data."""
    spec = case.spec
    g = torch.Generator().manual_seed(seed)
    cout, cin, kh, kw = spec["w_shape"]
    shapes = [(kh, kw)] if spec["phases"] is None else [(p[4], p[5]) for p in spec["phases"]]
    full = (spec["out_shape"][0], cout + 2 * GUARD) + tuple(spec["out_shape"][2:])
    if integers:
        rnd = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        srcs = [rnd(-3, 3, *s) for s in spec["src_shapes"]]
        weights = [rnd(-2, 2, cout, cin, *k) for k in shapes]
        bias, res = rnd(-8, 8, cout), (rnd(-8, 8, *full) if spec["residual"] else None)
    else:
        srcs = [torch.randn(*s, generator=g) for s in spec["src_shapes"]]
        weights = [torch.randn(cout, cin, *k, generator=g) / math.sqrt(cin * k[0] * k[1]) for k in shapes]
        bias, res = torch.randn(cout, generator=g), (torch.randn(*full, generator=g) if spec["residual"] else None)
    return srcs, weights, bias, res


def _activate(x, act, p0, p1):
    if act == ACT_RELU:
        return F.relu(x)
    if act == ACT_LEAKY_RELU:
        return F.leaky_relu(x, p0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    if act == ACT_ABS_TANH_AFFINE:
        t = torch.abs(torch.tanh(x))
        return (1 - t) * p0 + t * p1
    return x


def _phases(spec):
    """[(pad_top, pad_left, out_off_h, out_off_w)] of the launch's phases (one for a plain launch)."""
    if spec["phases"] is None:
        return [(spec["pad"][0], spec["pad"][1], spec["out_off"][0], spec["out_off"][1])]
    return [tuple(p[:4]) for p in spec["phases"]]


def _reference(case, srcs, weights, bias, res, act, p0, p1, round_bf16=False):
    """fp64 reference of the launch as (values, written): the whole destination tensor, guard channels included, and the positions the
    launch writes.  Zero padding as far as the output grid asks for it; `round_bf16`: operands rounded to bf16 first (MR_COMPUTE_BF16)."""
    spec = case.spec
    cout = spec["w_shape"][0]
    (sh, sw), (gh, gw), (sth, stw) = spec["stride"], spec["grid"], spec["out_step"]
    x = torch.cat(srcs, 1)
    if spec["tf"] == TF_RESNET_NORM:
        x = ((x + 0.5) - 0.45) / 0.225
    if spec["in_mode"] == IN_UPSAMPLE2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    elif spec["in_mode"] == IN_MAXPOOL2:
        x = F.max_pool2d(x, 2)
    rb = (lambda t: t.to(torch.bfloat16).double()) if round_bf16 else (lambda t: t.double())
    x = rb(x)
    full = (spec["out_shape"][0], cout + 2 * GUARD) + tuple(spec["out_shape"][2:])
    values, written = torch.zeros(full, dtype=torch.float64), torch.zeros(full, dtype=torch.bool)
    for w, (pt, pl, ooh, oow) in zip(weights, _phases(spec)):
        kh, kw = w.shape[2:]
        pb = max(0, (gh - 1) * sh + kh - pt - x.shape[2])
        pr = max(0, (gw - 1) * sw + kw - pl - x.shape[3])
        y = F.conv2d(F.pad(x, [pl, pr, pt, pb]), rb(w), bias.double(), stride=(sh, sw))[:, :, :gh, :gw]
        sl = (slice(None), slice(GUARD, GUARD + cout), slice(ooh, ooh + (gh - 1) * sth + 1, sth), slice(oow, oow + (gw - 1) * stw + 1, stw))
        if res is not None:
            y = y + res[sl].double()
        values[sl] = _activate(y, act, p0, p1)
        assert not written[sl].any()
        written[sl] = True
    return values.float(), written


def _launch(case, sched, srcs, weights, bias, res, act, p0, p1, reps=1):
    """The layer alone through engine.Plan.bare(...).conv(...) under `sched`: [output tensor (CPU) per repetition], each started from the sentinel."""
    spec = case.spec
    cout = spec["w_shape"][0]
    plan = engine.Plan.bare(DEV, schedule_override={"t": tuple(sched)}, bf16=case.mode)
    out = plan.alloc("out", spec["out_shape"][0], cout + 2 * GUARD, *spec["out_shape"][2:])
    phases = None if spec["phases"] is None else [(w, *p) for w, p in zip(weights, _phases(spec))]
    plan.conv("main", "t", [s.to(DEV) for s in srcs], weights[0] if phases is None else None, bias, out, stride=spec["stride"], pad=spec["pad"],
              grid=spec["grid"], act=act, p0=p0, p1=p1, in_mode=spec["in_mode"], tf=spec["tf"], residual=None if res is None else res.to(DEV),
              out_step=spec["out_step"], out_off=spec["out_off"], out_ch_offset=GUARD, phases=phases)
    log = plan.conv_log[0]
    assert (log["mb"], log["nb"], log["split_k"], log["ck"], log["waves"], log["kws"]) == census.unpack_schedule(sched) and int(log["bf16"]) == case.mode
    assert log["lds"] == census.geometry(spec, sched, case.mode)["lds"]
    plan.finalize()
    outs = []
    for _ in range(reps):
        _bits(out).fill_(SENTINEL_BITS)
        plan.run_stage("main", torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(out.cpu().clone())
    return outs


def _where(case, sched, differs):
    """The first differing output as text: (n, co, oy, ox) of the convolution grid and the tile / cout block / wave / pixel block that computes it."""
    spec = case.spec
    n, c, y, x = (int(v) for v in differs.nonzero()[0])
    (sth, stw) = spec["out_step"]
    ph = next((i for i, (_, _, ooh, oow) in enumerate(_phases(spec)) if (y - ooh) % sth == 0 and (x - oow) % stw == 0 and y >= ooh and x >= oow), None)
    if ph is None or not GUARD <= c < GUARD + spec["w_shape"][0]:
        return f"first difference at destination (n={n}, c={c}, y={y}, x={x}): OUTSIDE the positions the launch writes"
    _, _, ooh, oow = _phases(spec)[ph]
    co, oy, ox = c - GUARD, (y - ooh) // sth, (x - oow) // stw
    own = census.output_owner(spec, sched, case.mode, co, oy, ox)
    return (f"first difference at (n={n}, co={co}, oy={oy}, ox={ox}) phase {ph}: tile {own['tile']}, cout group {own['cout_group']} block {own['cout_block']}, "
            f"wave {own['wave']}, pixel block {own['pixel_block']}, lane {own['lane']}; {int(differs.sum())} of {differs.numel()} differ")


def _check_footprint(case, sched, outs, written, what):
    tag = f"{census.key_id(case.key)} [{case.name}, sched {tuple(sched)}] {what}"
    b0 = _bits(outs[0])
    touched = (b0 != SENTINEL_BITS)
    outside = touched & ~written
    assert not outside.any(), f"{tag}: wrote outside its slice - {_where(case, sched, outside)}"
    missed = written & ~touched
    assert not missed.any(), f"{tag}: left the sentinel in its slice - {_where(case, sched, missed)}"
    for i, o in enumerate(outs[1:], 1):
        d = _bits(o) != b0
        assert not d.any(), f"{tag}: repetition {i} differs from the first - {_where(case, sched, d)}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_direct_conv_instantiation(hip_lib, case):
    """Checks a-d of the module docstring for one instantiation key.  Layers that read the keyframe through TF_RESNET_NORM skip check (a):
    (x + 0.5 - 0.45) / 0.225 is not exact on integers, so their operands are never small integers; they keep b, c and d.  The sigmoid /
    |tanh| heads run check (a) with ACT_NONE (the transcendental is not exact either) and keep their activation in check (b)."""
    spec, sched, key = case.spec, case.sched, case.key
    tag = f"{census.key_id(key)} [{case.name} of {case.origin}, sched {tuple(sched)}, grid {spec['grid']}]"
    seed = sum(spec["w_shape"]) + 31 * spec["grid"][1]
    # ---- a. exact
    if spec["tf"] != TF_RESNET_NORM:
        act = spec["act"] if spec["act"] in (ACT_NONE, ACT_RELU, ACT_LEAKY_RELU) else ACT_NONE
        p0 = (0.5, 0.25)[seed & 1] if act == ACT_LEAKY_RELU else 0.0
        ops = _operands(case, True, seed)
        ref, written = _reference(case, *ops, act, p0, 0.0)
        assert ref.abs().max().item() < 2 ** 24
        outs = _launch(case, sched, *ops, act, p0, 0.0)
        _check_footprint(case, sched, outs, written, "exact")
        wrong = written & (outs[0] != ref)
        assert not wrong.any(), f"{tag}: not EQUAL to the fp64 reference on integer data - {_where(case, sched, wrong)}"
    # ---- b. gaussian, d. footprint and determinism
    ops = _operands(case, False, seed + 1)
    act, p0, p1 = spec["act"], spec["p0"], spec["p1"]
    ref, written = _reference(case, *ops, act, p0, p1, round_bf16=case.mode == 1)
    outs = _launch(case, sched, *ops, act, p0, p1, reps=REPS)
    _check_footprint(case, sched, outs, written, "gaussian")
    err = (outs[0] - ref)[written].abs()
    bound = 2e-4 * max(1.0, ref[written].abs().max().item())
    print(f"{tag}: gaussian max|err| = {err.max().item():.3e} (bound {bound:.3e})")
    assert err.max().item() < bound, f"{tag}: {err.max().item():.3e} >= {bound:.3e} - {_where(case, sched, written & ((outs[0] - ref).abs() >= bound))}"
    # ---- c. order identity under the anchor schedule
    if census.order_check_applies(case):
        anchor, _ = census.anchor_schedule(case)
        other = _launch(case, anchor, *ops, act, p0, p1)
        _check_footprint(case, anchor, other, written, "anchor")
        d = _bits(other[0]) != _bits(outs[0])
        assert not d.any(), f"{tag}: differs from the anchor schedule {anchor} - {_where(case, sched, d)} (under the anchor: {_where(case, anchor, d)})"
