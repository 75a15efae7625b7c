"""GPU (MI355X): mr_conv2d_b8 (csrc/conv_b8.hip) form by form.

tests/b8_conv_census.py reduces every B8 launch of the bf16 plans to the key its compiled code and run-time branches depend on (register
tile, workgroup size, resident weights, fp32 staging, source / destination layouts, filter, stride, phases, tile walk, chunk count, staged
positions per thread, activation) and keeps one shrunken layer per key, next to hand-written cases for what no plan launches.  Each runs
here ALONE, through engine.Plan.bare(..., bf16=1) under its own schedule - .conv_b8, or .refine / .upconv where the Plan builder makes
the phases - into a destination that is a view in the middle of a larger allocation, with guard rows below and guard columns right of the
output grid, prefilled with a finite sentinel:

  a. exact     sources and weights from {-1, 0, 1}, integer bias, LeakyReLU slope 0.5 / 0.25: every sum is a small integer and every
               result has at most 8 significant bits (asserted on the reference), so fp32 AND B8 destinations must EQUAL the reference
               bit for bit - the bf16 rounding of a B8 destination cannot hide a dropped or doubled tap.
  b. gaussian  the bounds of test_gpu_b8._check, against fp64 on the bf16-rounded operands.
  c. identity  an output's sum starts at the bias and takes one MFMA per (chunk, tap), chunk-major, whatever mb, nb, wv, wres and
               tiles_per_wg are: the same layer under an anchor schedule (another mb, nb and wv; census.anchor_schedule) is bit-identical,
               and so is the layer with every fp32 source handed over as B8 and every B8 source as fp32 (the sources are
               bf16-representable) - the other staging path.
  d. footprint nothing outside the written positions loses the sentinel (guard rows / columns, the memory before and behind the view),
               no written position keeps it, the padded channels of a B8 destination's last 8-block are zero, three repetitions are
               bit-identical."""
import pytest
import torch

import b8_conv_census as census
from monorec_amd import engine
from monorec_amd._lib import ACT_LEAKY_RELU, ACT_NONE, LAYOUT_BF16_B8
from test_gpu_b8 import _check, to_b8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_ROWS, GUARD_COLS = 2, 3               # destination plane rows below / columns right of the output grid
MARGIN = 256                                # 16-bit words in front of and behind the destination view
SENTINEL = 0x7A5A                           # finite as bf16 (2.8e35) and, doubled, as fp32 (0x7A5A7A5A): no result takes it
REPS = 3
EXTRA = census.extra()                      # what derive8() accepts but no census plan launches
CASES = list(census.census().values()) + EXTRA
IDS = [census.case_id(c) for c in CASES]


def _box(spec):
    """(rows, columns) of the destination plane the launch writes: the output grid times the output step."""
    return spec["grid"][0] * spec["out_step"][0], spec["grid"][1] * spec["out_step"][1]


def _launch(case, sched, layouts, srcs, weight, bias, act, p0, reps=1):
    """The layer alone under `sched`, sources in `layouts`: [whole allocation as 16-bit words (CPU) per repetition], each started from the
    sentinel.  Through Plan.refine / Plan.upconv where the builder's own activation is asked for and an operand is B8 (what routes the
    builder to the B8 kernel); else through Plan.conv_b8 with the phases the builder would make."""
    spec = case.spec
    kind, cout = spec["kind"], spec["w_shape"][0]
    n = spec["src_shapes"][0][0]
    b8_out = spec["out_layout"] == LAYOUT_BF16_B8
    bh, bw = _box(spec)
    ph, pw = bh + GUARD_ROWS, bw + GUARD_COLS
    words = n * ((cout + 7) // 8) * ph * pw * 8 if b8_out else n * cout * ph * pw * 2
    buf = torch.empty(MARGIN + words + MARGIN, dtype=torch.int16, device=DEV)
    body = buf[MARGIN:MARGIN + words]
    if b8_out:
        out = body.view(torch.bfloat16).view(n, (cout + 7) // 8, ph, pw, 8)
        out.b8_channels = cout
    else:
        out = body.view(torch.float32).view(n, cout, ph, pw)
    dsrcs = []
    for x, lay in zip(srcs, layouts):
        t = to_b8(x).to(DEV) if lay == LAYOUT_BF16_B8 else x.to(DEV)
        if lay == LAYOUT_BF16_B8:
            t.b8_channels = x.shape[1]
        dsrcs.append(t)
    builder_act = {"refine": (ACT_LEAKY_RELU, engine.LEAKY_SLOPE), "upconv": (ACT_NONE, 0.0)}.get(kind)
    via_builder = builder_act == (act, p0) and (b8_out or LAYOUT_BF16_B8 in layouts)
    state = {}
    if via_builder:
        state = {"p.conv2d_t.weight": weight, "p.conv2d_t.bias": bias} if kind == "refine" else {"p.weight": weight, "p.bias": bias}
    plan = engine.Plan.bare(DEV, state=state, schedule_override={"t": tuple(sched)}, bf16=1)
    if kind == "conv":
        plan.conv_b8("main", "t", dsrcs, weight, bias, out, stride=spec["stride"], pad=spec["pad"], grid=spec["grid"], act=act, p0=p0)
    elif via_builder and kind == "refine":
        plan.refine("main", "t", dsrcs, "p", out)
    elif via_builder:
        plan.upconv("main", "t", dsrcs, "p.weight", "p.bias", out)
    else:
        plan.conv_b8("main", "t", dsrcs, None, bias, out, grid=spec["grid"], act=act, p0=p0, out_step=spec["out_step"],
                     phases=census.phase_weights(spec, weight))
    log = plan.conv_log[0]
    g = census.derive(dict(spec, src_layouts=tuple(layouts)), sched)
    assert log["b8"] and (log["mb"], log["nb"], log["waves"]) == tuple(sched) and log["lds"] == g["lds"] and log["phases"] == g["nphase"], (log, g)
    plan.finalize()
    outs = []
    for _ in range(reps):
        buf.fill_(SENTINEL)
        plan.run_stage("main", torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append(buf.cpu())
    return outs


def _planes(case, words):
    """The allocation as (16-bit words in front, destination as (N, C8 or C, plane rows, plane columns) int32 bit patterns - a bf16 in
    the low half -, its float values, words behind)."""
    spec = case.spec
    cout, n = spec["w_shape"][0], spec["src_shapes"][0][0]
    bh, bw = _box(spec)
    ph, pw = bh + GUARD_ROWS, bw + GUARD_COLS
    body = words[MARGIN:len(words) - MARGIN]
    if spec["out_layout"] == LAYOUT_BF16_B8:
        cb = (cout + 7) // 8
        t = body.view(n, cb, ph, pw, 8).permute(0, 1, 4, 2, 3).reshape(n, cb * 8, ph, pw).contiguous()
        return words[:MARGIN], t.int() & 0xFFFF, t.view(torch.bfloat16).float(), words[len(words) - MARGIN:]
    f = body.view(torch.float32).view(n, cout, ph, pw)
    return words[:MARGIN], f.contiguous().view(torch.int32), f, words[len(words) - MARGIN:]


def _where(case, sched, differs):
    """The first differing destination element as text: (n, co, oy, ox, phase) of the convolution grid and what computes it - tile, the
    tile's position in its workgroup's walk, cout group and block, wave, pixel block, lane."""
    spec = case.spec
    n, c, y, x = (int(v) for v in differs.nonzero()[0])
    bh, bw = _box(spec)
    count = f"{int(differs.sum())} of {differs.numel()} differ"
    if y >= bh or x >= bw:
        return f"first difference at destination (n={n}, c={c}, y={y}, x={x}): a GUARD row / column outside the output grid; {count}"
    sth, stw = spec["out_step"]
    ph = next(i for i, p in enumerate(census.phase_list(spec)) if (y - p[4]) % sth == 0 and (x - p[5]) % stw == 0)
    oy, ox = y // sth, x // stw
    own = census.output_owner(spec, sched, n, min(c, spec["w_shape"][0] - 1), oy, ox, ph)
    pad = " (a PADDED channel of the last 8-block)" if c >= spec["w_shape"][0] else ""
    return (f"first difference at (n={n}, co={c}{pad}, oy={oy}, ox={ox}, phase {ph}): tile {own['tile']} = tile {own['walk_pos']} of {own['tiles_per_wg']} in the "
            f"walk of workgroup {own['workgroup']}, cout group {own['cout_group']} block {own['cout_block']}, wave {own['wave']}, pixel block "
            f"{own['pixel_block']}, lane {own['lane']}; {count}")


def _footprint(case, sched, outs, tag):
    """Check (d) on the repetitions of one launch; returns the written box of the first as (bit patterns, values), (N, Cout, rows, columns)."""
    spec = case.spec
    cout = spec["w_shape"][0]
    bh, bw = _box(spec)
    front, bits, vals, back = _planes(case, outs[0])
    assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all()), f"{tag}: wrote in front of / behind the destination tensor"
    sent = SENTINEL if spec["out_layout"] == LAYOUT_BF16_B8 else (SENTINEL << 16 | SENTINEL)
    touched = bits != sent
    written = torch.zeros_like(touched)
    written[:, :, :bh, :bw] = True
    outside = touched & ~written
    assert not outside.any(), f"{tag}: wrote outside the output grid - {_where(case, sched, outside)}"
    missed = written & ~touched
    assert not missed.any(), f"{tag}: left the sentinel inside the output grid - {_where(case, sched, missed)}"
    if bits.shape[1] > cout:                # B8 destination: the next layer reads these against zero weights - 0 * NaN would poison it
        padded = torch.zeros_like(touched)
        padded[:, cout:, :bh, :bw] = True
        bad = padded & ~(torch.isfinite(vals) & (vals == 0))
        assert not bad.any(), f"{tag}: padded channels of the last 8-block are not zero - {_where(case, sched, bad)}"
    for i, o in enumerate(outs[1:], 1):
        d = _planes(case, o)[1] != bits
        assert torch.equal(o, outs[0]), f"{tag}: repetition {i} differs from the first - {_where(case, sched, d) if d.any() else 'outside the tensor'}"
    return bits[:, :cout, :bh, :bw], vals[:, :cout, :bh, :bw]


def _float_bits(ref, b8_out):
    """Bit patterns of an fp32 reference as _planes reports the destination's."""
    i = ref.float().contiguous().view(torch.int32)
    return (i >> 16) & 0xFFFF if b8_out else i


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_b8_conv_form(hip_lib, case):
    """Checks a-d of the module docstring for one key."""
    spec, sched, key = case.spec, case.sched, case.key
    g = census.derive(spec, sched)
    tag = (f"{census.key_id(key)} [{case.name} of {case.origin}, sched {tuple(sched)}, grid {spec['grid']} x batch {spec['src_shapes'][0][0]}, "
           f"tiles_per_wg {g['tiles_per_wg']}]")
    seed = census.case_seed(case)
    b8_out = spec["out_layout"] == LAYOUT_BF16_B8
    lays = spec["src_layouts"]
    # ---- a. exact (an fp32 reference: integer sums are exact in any order)
    srcs, weight, bias = census.operands(case, True, seed)
    p0 = census.exact_slope(seed) if spec["act"] == ACT_LEAKY_RELU else 0.0
    pre, ref = census.reference(case, srcs, weight, bias, spec["act"], p0, dtype=torch.float32)
    assert pre.abs().max().item() < 2 ** 24 and torch.equal(census.bf(pre), pre) and torch.equal(census.bf(ref), ref), f"{tag}: operands too dense"
    outs = _launch(case, sched, lays, srcs, weight, bias, spec["act"], p0)
    bits, _ = _footprint(case, sched, outs, tag + " exact")
    wrong = bits != _float_bits(ref, b8_out)
    assert not wrong.any(), f"{tag}: not EQUAL to the reference on integer data - {_where(case, sched, wrong)}"
    # ---- b. gaussian, d. footprint and determinism
    srcs, weight, bias = census.operands(case, False, seed + 1)
    act, p0 = spec["act"], spec["p0"]
    _, ref = census.reference(case, srcs, weight, bias, act, p0)
    ref = ref.float()
    outs = _launch(case, sched, lays, srcs, weight, bias, act, p0, reps=REPS)
    bits, got = _footprint(case, sched, outs, tag + " gaussian")
    scale = max(1.0, float(ref.abs().max()))
    err = (got - ref).abs()
    if b8_out:
        ratio = err / (2.0 ** -8 * ref.abs() + 1e-4 * scale)
        print(f"{tag}: gaussian max err / (2^-8 |ref| + 1e-4 scale) = {float(ratio.max()):.3f} (bound 1), max|err| = {float(err.max()):.3e}, scale {scale:.2f}")
    else:
        print(f"{tag}: gaussian max|err| = {float(err.max()):.3e} (bound {2e-5 * scale * ref.shape[1] ** 0.5:.3e})")
    _check(got, ref, spec["out_layout"], tag)
    # ---- c. identity: anchor schedule, then the sources in the other layout
    anchor = census.anchor_schedule(case)
    if anchor is not None:
        other = _launch(case, anchor, lays, srcs, weight, bias, act, p0)
        obits, _ = _footprint(case, anchor, other, tag + f" anchor {anchor}")
        d = obits != bits
        assert not d.any(), f"{tag}: differs from the anchor schedule {anchor} - {_where(case, sched, d)} (under the anchor: {_where(case, anchor, d)})"
    flipped = census.flipped_layouts(lays)
    other = _launch(case, sched, flipped, srcs, weight, bias, act, p0)
    obits, _ = _footprint(case, sched, other, tag + " sources in the other layout")
    d = obits != bits
    assert not d.any(), f"{tag}: differs with the sources handed over in the other layout - {_where(case, sched, d)}"
