"""GPU (MI355X): the reduced-multiply convolution kernels (csrc/conv_wino*.hip, convt_wino.hip, conv1d_wino.hip) key by key.

tests/reduced_conv_census.py reduces every reduced-multiply launch of the measured tables to the key its compiled code and control flow
depend on and keeps one shrunken layer per key, plus EXTRA cases the tables do not reach.  Each runs here ALONE through
engine.Plan.bare(...) and the public builders (conv, refine, upconv) with engine.WINOGRAD patched so that the layer's own signature maps to
the key's code - table lookup, decode_form, weight packing, descriptor, finalize and run_stage (mr_run_launches) are in the path; a stride-2
half, whose builder fixes the pair, goes through Plan._conv_winograd_1d with the view / dst_split Plan._conv_relu2_stride2 builds:

  a. exact     certified integer operands (census.exact_operands): every fp32 intermediate is exact, so the output must EQUAL the fp64
               reference: no tolerance.  All keys but the F(4,7) ones (tests/test_reduced_conv_census.py pins that set).
  b. gaussian  against fp64, the bar of the family's test in tests/test_gpu_kernels.py: F(2x2,3x3) 2e-5, F(4x4,3x3) 4e-5, Refine / Upconv /
               F(2,3) / F(4,3) / F(2,7) / F(4,4) 1e-5, F(4,7) 6e-5, each times max(1, |ref|max).
  c. twins     forms stated to give identical words do: F(2x2,3x3) and Refine variant 1 = variant 0, conv_wino44w = conv_wino44.
  d. footprint the destination lies between 3 guard channels (a column-split destination: both halves between them) in a tensor
               prefilled with a sentinel: nothing outside the written positions changes, no written position keeps the sentinel.
  e. determinism  three repetitions from the sentinel are bit-identical.

F(2,7) is compiled into the diagnostic library only (python -m monorec_amd.build --timeline): the product library must REFUSE its two
EXTRA cases; they run checks a-e when the diagnostic library is loaded.

Measured maximum Gaussian error against fp64 per form, as a fraction of max(1, |ref|max), over all its keys (MI355X; the first such
measurement - the bars of tests/test_gpu_kernels.py were set against an fp32 CPU reference).  Every key is at least 3 x inside its bar:
    F(2x2,3x3)  conv_wino.hip      27 keys  4.1e-7  (bar 2e-5)        F(2,3)   1-D, both axes  13 keys  3.8e-7  (bar 1e-5)
    F(4x4,3x3)  conv_wino44.hip     8 keys  7.7e-6  (bar 4e-5)        F(4,3)   1-D, both axes  21 keys  2.2e-6  (bar 1e-5)
    F(4x4,3x3)  conv_wino44s.hip    8 keys  7.2e-6  (bar 4e-5)        F(4,4)   stride-2 halves  4 keys  1.4e-6  (bar 1e-5)
    F(4x4,3x3)  conv_wino44w.hip    4 keys  4.5e-6  (bar 4e-5)        F(4,7)   no exact check   6 keys  1.8e-5  (bar 6e-5)
    Refine      convt_wino.hip     13 keys  1.0e-6  (bar 1e-5)        Upconv   4 multiplies     5 keys  7.7e-7  (bar 1e-5)"""
import math

import pytest
import torch
import torch.nn.functional as F

import reduced_conv_census as census
from monorec_amd import engine
from monorec_amd._lib import ACT_LEAKY_RELU, ACT_NONE, ACT_RELU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3                                   # untouched channels below and above the written slice
SENTINEL_BITS = 0x7A5A5A5A                  # a finite fp32 (2.8e35) no result takes
REPS = 3

CT_TOL = {(4, 3): 1e-5, (2, 7): 1e-5, (4, 7): 6e-5, (4, 4): 1e-5}          # test_cooktoom_1d_conv_* / test_cooktoom_f44_*
TOL = {"w22": 2e-5, "w44": 4e-5, "w44s": 4e-5, "w44w": 4e-5, "t22": 1e-5, "f23": 1e-5, "up": 1e-5}

CASES = census.all_cases()
IDS = [census.case_id(c) for c in CASES]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _out_shape(launch):
    n, (h, w) = launch.batch, launch.hw
    if launch.family in ("t22", "up"):
        return (n, launch.cout, 2 * h, 2 * w)
    return (2, n, launch.cout, h, w // 2) if launch.split else (n, launch.cout, h, w)


def _operands(case, integers, seed):
    """(sources as the kernel sees them, weight, bias, residual or None): certified integers (check a) or Gaussian data."""
    launch = case.launch
    g = torch.Generator().manual_seed(seed)
    shape = _out_shape(launch)
    if integers:
        ops = census.exact_operands(case, seed)
        rnd = lambda *s: torch.randint(-8, 9, s, generator=g).float()
        return ops.srcs, ops.weight, rnd(launch.cout), (rnd(*shape) if launch.residual else None)
    srcs = [torch.randn(*s, generator=g) for s in census.source_shapes(launch)]
    wshape = census.weight_shape(launch)
    taps = wshape[2] * wshape[3] // (4 if launch.family == "t22" else 1)         # Refine: 4 of the 16 taps meet in one output
    weight = torch.randn(*wshape, generator=g) / math.sqrt(sum(launch.srcs_c) * taps)
    return srcs, weight, torch.randn(launch.cout, generator=g), (torch.randn(*shape, generator=g) if launch.residual else None)


def _reference(launch, srcs, weight, bias, res, act, p0):
    """fp64 reference of the launch in the shape of its destination, rounded once to fp32.  LeakyReLU as the epilogue has it:
    max(x, fp32(slope) * x) (test_relu_epilogue_and_non_finite_values_documented_deviation)."""
    x, w, b = torch.cat(srcs, 1).double(), weight.double(), bias.double()
    if launch.family == "t22":
        y = F.conv_transpose2d(x, w, b, stride=2)[:, :, 1:-1, 1:-1]
    elif launch.family == "up":
        y = F.conv2d(F.pad(F.interpolate(x, scale_factor=2, mode="nearest"), [0, 1, 0, 1]), w, b)
    elif census.dims_of(launch) == 2:
        y = F.conv2d(x, w, b, padding=1)
    else:
        lo = census.pad_low(launch)
        hi = launch.r - 1 - lo
        y = F.conv2d(F.pad(x, [lo, hi, 0, 0] if launch.axis == 0 else [0, 0, lo, hi]), w, b)
    if launch.split:
        y = torch.stack([y[..., 0::2], y[..., 1::2]])
    if res is not None:
        y = y + res.double()
    if act == ACT_RELU:
        y = torch.clamp_min(y, 0.0)
    elif act == ACT_LEAKY_RELU:
        y = torch.maximum(y, y * float(torch.tensor(p0, dtype=torch.float32)))
    else:
        assert act == ACT_NONE
    assert tuple(y.shape) == _out_shape(launch)
    return y.float()


def _launch(monkeypatch, launch, srcs, weight, bias, res, act, p0, reps=1):
    """The layer alone through its builder: [the whole guarded destination (CPU, flat) per repetition], each started from the sentinel, and
    the offset (in floats) and the shape of the written slice in it."""
    shape = _out_shape(launch)
    guard = GUARD * shape[-2] * shape[-1]
    numel = math.prod(shape)
    state = {}
    if launch.family == "t22":
        state = {"x.conv2d_t.weight": weight, "x.conv2d_t.bias": bias}
    elif launch.family == "up":
        state = {"x.weight": weight, "x.bias": bias}
    plan = engine.Plan.bare(DEV, state=state)
    plan.winograd = True
    whole = plan.alloc("guarded", guard + numel + guard)
    out = whole[guard:guard + numel].view(shape)           # the builders take no channel offset: a contiguous, 16-byte aligned view
    dsrcs = [s.to(DEV) for s in srcs]
    dres = None if res is None else res.to(DEV)
    n, (h, w) = launch.batch, launch.hw
    if launch.stride2:
        # the half of a stride-2 ConvReLU2 pair, alone: the 4-tap (7 taps) / 3-tap (5 taps) stride-1 form over [even | odd] sources
        k = 2 * launch.r - 1
        view, keep = None, dsrcs
        if launch.view:                                     # [even rows | odd rows] of ONE tensor, as Plan._conv_relu2_stride2 hands them over
            c = launch.srcs_c[0]
            x = torch.empty(n, c, 2 * h, w, device=DEV)
            x[:, :, 0::2], x[:, :, 1::2] = dsrcs[0], dsrcs[1]
            view = census.stride2_view(launch, x.data_ptr())
            keep = [x]
        plan._conv_winograd_1d("main", "t", keep, weight, bias, out, act, p0, launch.axis, launch.mbw, launch.m, view=view, dst_split=launch.split,
                               ref_k=(k, 1) if launch.axis == 1 else (1, k), sig="stride2_half")
    else:
        monkeypatch.setitem(engine.WINOGRAD, census.signature(launch), census.table_code(launch))
        if launch.family == "t22":
            plan.refine("main", "t", dsrcs, "x", out)
        elif launch.family == "up":
            plan.upconv("main", "t", dsrcs, "x.weight", "x.bias", out)
        else:
            kh, kw = weight.shape[2:]
            plan.conv("main", "t", dsrcs, weight, bias, out, stride=(1, 1), pad=(kh // 2, kw // 2), grid=(h, w), act=act, p0=p0, residual=dres)
    assert len(plan.conv_log) == 1 and "winograd" in plan.conv_log[0], "the layer did not take a reduced-multiply form"
    ran = census.launch_of(plan.conv_log[0])
    assert ran == launch._replace(p0=ran.p0), (ran, launch)             # the intended form, on the intended shape
    plan.finalize()
    outs = []
    for _ in range(reps):
        _bits(whole).fill_(SENTINEL_BITS)
        plan.run_stage("main", torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(whole.cpu().clone())
    return outs, guard, shape


def _where(launch, differs):
    """The first differing output as text: (n, channel, y, x) of the destination and the workgroup tile / channel group that computes it."""
    idx = [int(v) for v in differs.nonzero()[0]]
    if launch.split:
        half, n, c, y, x = idx
        x = 2 * x + half
    else:
        n, c, y, x = idx
    ky, kx = (y // 2, x // 2) if launch.family in ("t22", "up") else (y, x)
    own = census.output_owner(launch, c, ky, kx)
    return (f"first difference at (n={n}, channel={c}, y={y}, x={x}): workgroup tile {own['tile']}, channel group {own['group']} block {own['block']}; "
            f"{int(differs.sum())} of {differs.numel()} differ")


def _check_footprint(tag, launch, outs, guard, shape, what):
    numel = math.prod(shape)
    b0 = _bits(outs[0])
    for name, region, base in (("below", b0[:guard], -guard), ("above", b0[guard + numel:], numel)):
        bad = (region != SENTINEL_BITS).nonzero()
        assert bad.numel() == 0, (f"{tag} {what}: wrote outside its slice, {name} it - first at float {base + int(bad[0])} relative to the slice "
                                  f"of {numel} floats (plane {shape[-2]} x {shape[-1]}); {bad.shape[0]} floats changed")
    missed = (b0[guard:guard + numel] == SENTINEL_BITS).view(shape)
    assert not missed.any(), f"{tag} {what}: left the sentinel in its slice - {_where(launch, missed)}"
    for i, o in enumerate(outs[1:], 1):
        d = _bits(o) != b0
        assert not d[:guard].any() and not d[guard + numel:].any(), f"{tag} {what}: repetition {i} differs in the guard floats"
        d = d[guard:guard + numel].view(shape)
        assert not d.any(), f"{tag} {what}: repetition {i} differs from the first - {_where(launch, d)}"
    return outs[0][guard:guard + numel].view(shape)


def _twin(launch):
    """The form stated to give identical words (check c), or None."""
    if launch.family in ("w22", "t22") and launch.variant in (0, 1):
        return launch._replace(variant=1 - launch.variant)
    if launch.family in ("w44", "w44w"):
        other = "w44w" if launch.family == "w44" else "w44"
        return launch._replace(family=other, variant=census.VARIANT_OF_FAMILY[other])
    return None


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reduced_conv_form(hip_lib, monkeypatch, case):
    """Checks a-e of the module docstring for one key.  F(2,7) is compiled into the diagnostic library only: the standard build must refuse
    the launch (no silent fall-back), the diagnostic build runs every check."""
    launch, key = case.launch, case.key
    tag = f"{census.case_id(case)} [{case.name} of {case.origin}, plane {launch.hw}, batch {launch.batch}]"
    seed = 1000 + sum(launch.srcs_c) + 31 * launch.hw[1] + launch.cout
    fixed_slope = launch.family == "t22"                       # Plan.refine fixes LeakyReLU(0.1); Plan.upconv has no activation
    if key.family == "ct" and (key.m, key.r) == (2, 7) and not hip_lib.has_diagnostic_forms:
        ops = _operands(case, False, seed)
        with pytest.raises((AssertionError, RuntimeError)):              # the packer and the launch refuse the form
            _launch(monkeypatch, launch, *ops, launch.act, launch.p0)
        return
    # ---- a. exact
    if census.certifiable(key):
        act = launch.act
        p0 = launch.p0 if fixed_slope else ((0.5, 0.25)[seed & 1] if act == ACT_LEAKY_RELU else 0.0)
        ops = _operands(case, True, seed)
        ref = _reference(launch, *ops, act, p0)
        assert ref.abs().max().item() < 2 ** 24
        outs, guard, shape = _launch(monkeypatch, launch, *ops, act, p0)
        got = _check_footprint(tag, launch, outs, guard, shape, "exact")
        wrong = got != ref
        assert not wrong.any(), f"{tag}: not EQUAL to the fp64 reference on certified integer data - {_where(launch, wrong)}"
    # ---- b. gaussian, d. footprint, e. determinism
    ops = _operands(case, False, seed + 1)
    act, p0 = launch.act, launch.p0
    ref = _reference(launch, *ops, act, p0)
    outs, guard, shape = _launch(monkeypatch, launch, *ops, act, p0, reps=REPS)
    got = _check_footprint(tag, launch, outs, guard, shape, "gaussian")
    tol = CT_TOL[(key.m, key.r)] if key.family == "ct" else TOL[key.family]
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs()
    print(f"{tag}: gaussian max|err| = {err.max().item() / scale:.3e} x scale (bar {tol:.1e}; scale {scale:.3f})")
    assert err.max().item() <= tol * scale, f"{tag}: {err.max().item():.3e} > {tol * scale:.3e} - {_where(launch, err > tol * scale)}"
    # ---- c. twins
    other = _twin(launch)
    if other is not None:
        touts, tguard, tshape = _launch(monkeypatch, other, *ops, act, p0)
        tgot = _check_footprint(tag, other, touts, tguard, tshape, "twin")
        d = _bits(tgot) != _bits(got)
        assert not d.any(), f"{tag}: differs from its twin {other.family} variant {other.variant} - {_where(launch, d)}"
