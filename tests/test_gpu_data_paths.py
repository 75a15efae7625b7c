"""GPU (MI355X): every case of tests/data_paths.py - the launch paths of csrc/preprocess.hip, csrc/select.hip and mr_sparse_metric_sums_f32 -
against a reference that is independent of the code under test, one launch per case: the resize bit for bit against the integer restatement
of Pillow (and Pillow), the lidar / D(V)SO targets bit for bit against the numpy oracle, the selection by bit pattern against a CPU sort, the
stage ratios by bit pattern against median_scaling applied k times with CPU torch.median, the metric sums against fp32 terms summed in fp64."""
import ctypes
import math

import numpy as np
import pytest
import torch

import data_paths as dp
from monorec_amd import input_pipeline, metrics
from oracle import monorec_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the resize ------------------------------------------------------------------------------------------------------------------------------------
def _resize_launch(lib, case):
    """The C entry of the case, called as ImagePreprocessor calls it (tables of the library's host part, max_tile_rows of its rule), with the
    case's row stride and plane stride.  Returns (error code, the output with its guard bytes, where the payload starts, plane stride)."""
    a = case.args
    img = dp.resize_image(case)
    h, w = a["src"]
    ch, (oh, ow) = a["channels"], a["out"]
    stride = w * ch + a.get("row_pad", 0)
    rows = np.full((h, stride), dp.PAD_BYTE, np.uint8)
    rows[:, :w * ch] = img.reshape(h, w * ch)
    src = torch.from_numpy(rows).to(DEV)
    x0, y0, x1, y1 = dp.resize_box(case)
    hks, hb, hk = input_pipeline._axis_tables(lib, x1 - x0, ow)
    vks, vb, vk = input_pipeline._axis_tables(lib, y1 - y0, oh)
    max_rows = max(dp.tile_rows(vb, oh))
    assert max_rows == dp.rule_resize(a["kernel"], ch, y1 - y0, x1 - x0, oh, ow)["max_tile_rows"]
    dev = [torch.from_numpy(t).to(DEV) for t in (hb, hk, vb, vk)]
    args = [src.data_ptr(), h, w, ch, stride, (ctypes.c_int32 * 4)(x0, y0, x1, y1), oh, ow, dev[0].data_ptr(), dev[1].data_ptr(), hks,
            dev[2].data_ptr(), dev[3].data_ptr(), vks, max_rows]
    if a["kernel"] == "u8":
        plane = (oh * ow + 15) // 16 * 16 + a.get("plane_pad", 0)
        out = torch.full((16 + ch * plane + 16,), dp.CANARY, dtype=torch.uint8, device=DEV)
        code = lib.mr_preprocess_image_u8_u8(*args, out.data_ptr() + 16, plane, _stream())
        start = 16
    else:
        plane = oh * ow
        out = torch.full((8 + 3 * plane + 8,), float("nan"), device=DEV)
        start = 8
        if a["kernel"] == "lut":
            lut = torch.from_numpy(dp.response_table()).to(DEV)
            code = lib.mr_preprocess_image_u8_lut_f32(*args, lut.data_ptr(), out.data_ptr() + 4 * start, _stream())
        else:
            code = lib.mr_preprocess_image_u8_f32(*args, out.data_ptr() + 4 * start, _stream())
    torch.cuda.synchronize()
    return code, out.cpu(), start, plane, img


@pytest.mark.parametrize("case", dp.cases_of("resize", run_only=True), ids=dp.case_ids("resize", run_only=True))
def test_resize_is_pillow_exact_on_every_path(hip_lib, case):
    a = case.args
    code, out, start, plane, img = _resize_launch(hip_lib, case)
    assert code == 0, code            # (the accepted 64 KiB tile included: a runtime that rejected it would show here as an error code)
    ch, (oh, ow) = a["channels"], a["out"]
    ref8 = dp.resize_reference_u8(case, img)
    pil = dp.resize_reference_pillow(case, img)
    assert pil is None or np.array_equal(ref8, pil)
    if a["kernel"] == "u8":
        got = out[start:start + ch * plane].view(ch, plane).numpy()
        assert np.array_equal(got[:, :oh * ow].reshape(ch, oh, ow), ref8), int((got[:, :oh * ow].reshape(ch, oh, ow) != ref8).sum())
        assert (got[:, oh * ow:] == dp.CANARY).all()                   # the padding behind every plane keeps its canary
        assert (out[:start] == dp.CANARY).all() and (out[start + ch * plane:] == dp.CANARY).all()
    else:
        want = dp.resize_reference_f32(case, img)
        got = out[start:start + 3 * plane].view(3, oh, ow)
        assert torch.equal(_bits(got), _bits(want)), int((got != want).sum())
        assert bool(torch.isnan(out[:start]).all()) and bool(torch.isnan(out[start + 3 * plane:]).all())


@pytest.mark.parametrize("case", [k for k in dp.cases_of("resize") if k.path.startswith("lds_refuse")], ids=lambda k: k.name)
def test_resize_beyond_the_lds_budget_is_refused_and_writes_nothing(hip_lib, case):
    code, out, start, plane, _ = _resize_launch(hip_lib, case)
    assert code == dp.constants()["err_lds_budget"]
    assert bool(torch.isnan(out).all())


# ---- lidar / D(V)SO targets, scatter, unpack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,case", [(e, k) for e in ("lidar", "dso") for k in dp.cases_of(e, run_only=True)], ids=lambda v: v if isinstance(v, str) else v.name)
def test_sparse_target_equals_the_numpy_oracle(hip_lib, entry, case):
    a = case.args
    png = dp.target_png(case)
    want = dp.target_reference(case, png)
    if entry == "lidar":
        got = input_pipeline.lidar_inverse_depth(png, a["box"], a["out"], device=DEV)
    else:
        got = input_pipeline.dso_inverse_depth(png, (*a["orig"], a["focal"]), a["box"], a["out"], device=DEV)
    got = got.cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(a["out"])
    diff = _bits(got) != _bits(want)
    assert not bool(diff.any()), (int(diff.sum()), int((want != 0).sum()))
    assert int((want != 0).sum()) > 0


@pytest.mark.parametrize("case", dp.cases_of("scatter"), ids=dp.case_ids("scatter"))
def test_scatter_equals_numpy(hip_lib, case):
    index, value = dp.scatter_operands(case)
    n, cells = case.args["n"], case.args["cells"]
    raw = np.frombuffer(index.tobytes() + value.tobytes(), dtype=np.uint8)
    got = input_pipeline.scatter_sparse(raw, n, cells, device=DEV).cpu().numpy()
    want = dp.scatter_reference(index, value, cells)
    assert got.shape == (cells,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("case", dp.cases_of("unpack"), ids=dp.case_ids("unpack"))
def test_unpack_equals_the_torch_expression(hip_lib, case):
    a = case.args
    rec = dp.unpack_record(case)
    n = a["h"] * a["w"]
    src = torch.from_numpy(rec).to(DEV)
    lut = torch.from_numpy(dp.response_table()).to(DEV) if a["lut"] else None
    guard = torch.full((8 + 3 * n + 8,), float("nan"), device=DEV)
    code = hip_lib.mr_unpack_frame_u8_f32(src.data_ptr(), a["channels"], rec.shape[1], a["h"], a["w"], None if lut is None else lut.data_ptr(),
                                          guard.data_ptr() + 32, _stream())
    torch.cuda.synchronize()
    assert code == 0
    out = guard.cpu()
    want = dp.unpack_reference(case, rec)
    assert torch.equal(_bits(out[8:8 + 3 * n].view(3, a["h"], a["w"])), _bits(want))
    assert bool(torch.isnan(out[:8]).all()) and bool(torch.isnan(out[-8:]).all())


# ---- median select ------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


SELECT_SIZES = sorted({k.args["n"] for k in dp.cases_of("select")})


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_median_select_by_bit_pattern_against_a_cpu_sort(hip_lib, n):
    """The samples of one launch are the select cases of one size; each is compared with torch.sort of its selection on the CPU."""
    cases = [k for k in dp.cases_of("select") if k.args["n"] == n]
    ops = [dp.select_operands(k) for k in cases]
    pred = torch.from_numpy(np.stack([p for p, _ in ops])).view(len(cases), 1, 1, n)
    gt = torch.from_numpy(np.stack([g for _, g in ops])).view(len(cases), 1, 1, n)
    stats = metrics.median_stats_device(pred.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    st, fl = stats.cpu(), stats.view(torch.float32).cpu()
    for i, case in enumerate(cases):
        p, g = pred[i].view(-1), gt[i].view(-1)
        sel = g > 0
        m = int(sel.sum())
        ps = p[sel]
        what = (case.name, m)
        assert int(st[i, 0]) == m, what
        assert [int(st[i, 4]), int(st[i, 5]), int(st[i, 6])] == [int(torch.isnan(ps).sum()), int((ps == 0).sum()), int(torch.isinf(ps).sum())], what
        if m == 0:
            assert all(math.isnan(float(fl[i, j])) for j in (1, 2, 3)), what
            continue
        t_sorted = torch.sort(g[sel])[0]
        assert _same(fl[i, 1], t_sorted[(m - 1) // 2]) and _same(fl[i, 1], torch.median(g[sel])), what
        if case.args["kind"] in ("nan_sparse", "nan_dense"):           # lo / hi are not defined with a NaN in the selection (monorec_hip.h)
            assert int(st[i, 4]) > 0
            continue
        p_sorted = torch.sort(ps)[0]
        assert _same(fl[i, 2], p_sorted[(m - 1) // 2]), (what, float(fl[i, 2]), float(p_sorted[(m - 1) // 2]))
        assert _same(fl[i, 3], p_sorted[m // 2]), (what, float(fl[i, 3]), float(p_sorted[m // 2]))
        assert _same(fl[i, 2], torch.median(ps)), what


# ---- stage ratios ---------------------------------------------------------------------------------------------------------------------------------------
def _stage_batch(repeat=1):
    cases = dp.cases_of("stage") * repeat
    ops = [dp.stage_operands(k) for k in cases]
    pred = torch.from_numpy(np.stack([p for p, _ in ops]))
    gt = torch.from_numpy(np.stack([g for _, g in ops]))
    return cases, pred, gt


def _assert_ratios(got, want, cases):
    got, want = got.cpu(), want
    for i, case in enumerate(cases):
        for j in range(want.shape[1]):
            assert _same(got[i, j], want[i, j]), (case.name, i, j, float(got[i, j]), float(want[i, j]))


@pytest.mark.parametrize("stages", [1, dp.constants()["max_stages"]])
def test_stage_ratios_equal_median_scaling_applied_k_times(hip_lib, stages):
    cases, pred, gt = _stage_batch()
    b = len(cases)
    stats = metrics.median_stats_device(pred.view(b, 1, 1, 8).to(DEV), gt.view(b, 1, 1, 8).to(DEV))
    scales, after = metrics.median_stage_scales_device(stats, stages)
    nxt, _ = metrics.median_stage_scales_device(after, 1)                # the statistics after the stages give the next ratio
    torch.cuda.synchronize()
    want = dp.median_scaling_chain(pred, gt, stages + 1)
    _assert_ratios(scales, want[:, :stages], cases)
    _assert_ratios(nxt, want[:, stages:], cases)


def test_stage_ratios_of_70_samples_with_stats_out_null_separate_and_aliasing(hip_lib):
    """More than 64 samples: the `b += 64` loop of the single wave; stats_out NULL, separate and aliasing give the same ratios."""
    stages = dp.constants()["max_stages"]
    cases, pred, gt = _stage_batch(7)
    b = len(cases)
    assert b == 70
    stats = metrics.median_stats_device(pred.view(b, 1, 1, 8).to(DEV), gt.view(b, 1, 1, 8).to(DEV))
    before = stats.clone()
    want = dp.median_scaling_chain(pred, gt, stages)
    outs = []
    for mode in ("null", "separate", "alias"):
        src = before.clone()
        dst = None if mode == "null" else torch.full_like(src, -7) if mode == "separate" else src
        scales = torch.full((b, stages), -7.0, dtype=torch.float32, device=DEV)
        code = hip_lib.mr_median_stage_scales_f32(src.data_ptr(), b, stages, scales.data_ptr(), None if dst is None else dst.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert code == 0
        _assert_ratios(scales, want, cases)
        if mode != "alias":
            assert torch.equal(src, before)                            # the input statistics are only read
        outs.append(dst)
    assert torch.equal(outs[1], outs[2])


# ---- metric sums ----------------------------------------------------------------------------------------------------------------------------------------
def _assert_sums(got, want, kinds, n, what):
    """kinds[c]: "count" (equal), "sum" (n * 2^-52 relative: the same correctly rounded fp32 terms, only the order of the fp64 sum differs),
    "log" (the project's 2e-5: logf of two math libraries).  inf and NaN must be the same."""
    assert got.shape == want.shape, what
    for b in range(want.shape[0]):
        for c, kind in enumerate(kinds):
            g, w = float(got[b, c]), float(want[b, c])
            where = (what, b, c, kind, g, w)
            if math.isnan(w) or math.isinf(w):
                assert (math.isnan(g) and math.isnan(w)) or g == w, where
            elif kind == "count":
                assert g == w, where
            elif kind == "sum":
                assert abs(g - w) <= n * 2.0 ** -52 * abs(w), where
            else:
                assert abs(g - w) <= dp.RTOL_LOG * max(1.0, abs(w)), where


def _roi_pixels(a):
    y0, y1, x0, x1 = a["roi"] if a["roi"] is not None else (0, a["shape"][1], 0, a["shape"][2])
    return (y1 - y0) * (x1 - x0)


def _same_nan_pattern(got, pred, gt, a, what):
    want = orc.sparse_metrics(pred, gt, a["roi"], a["max_distance"])
    for name, g in zip(metrics.SPARSE_METRICS, got):
        assert math.isnan(float(g)) == math.isnan(float(want[name])), (what, name, float(g), float(want[name]))


KIND_OF_COLUMN = {1: "sum", 2: "sum", 3: "sum", 4: "log", 5: "count", 6: "count", 7: "count"}


@pytest.mark.parametrize("case", dp.cases_of("sparse_sums"), ids=dp.case_ids("sparse_sums"))
def test_sparse_metric_sums_against_fp32_terms_summed_in_fp64(hip_lib, case):
    """mr_sparse_metric_sums_f32.  The two cases with a NaN prediction at a valid pixel fail on the kernel as it was before relu / clamp_min
    kept NaN (observed on an MI355X with that kernel linked in: it scored the NaN as a prediction of max_distance and returned the finite
    sum 350.72 for sum |dp - dg| / dg with max_distance 80, and inf without a max_distance, where the reference has NaN); the nine cases
    without a NaN at a valid pixel pass on both kernels with the same bounds: for such inputs the fix changes no bit."""
    a = case.args
    pred, gt, _ = dp.metric_operands(case)
    got = metrics.sparse_metric_sums_device({"result": pred.to(DEV), "target": gt.to(DEV)}, a["roi"], a["max_distance"]).cpu()
    want = dp.sparse_sums_reference(pred, gt, a["roi"], a["max_distance"])
    _assert_sums(got, want, ["count"] + [KIND_OF_COLUMN[c] for c in range(1, 8)], _roi_pixels(a), case.name)
    _same_nan_pattern(metrics.metrics_from_sums(got), pred, gt, a, case.name)


@pytest.mark.parametrize("case", dp.cases_of("stage_sums"), ids=dp.case_ids("stage_sums"))
def test_metric_stage_sums_against_fp32_terms_summed_in_fp64(hip_lib, case):
    a = case.args
    pred, gt, scales = dp.metric_operands(case)
    got = metrics.metric_stage_sums_device(pred.to(DEV), gt.to(DEV), tuple(a["columns"]), a["roi"], a["max_distance"],
                                           None if scales is None else scales.to(DEV)).cpu()
    want = dp.stage_sums_reference(pred, gt, a["roi"], a["max_distance"], a["columns"], scales)
    _assert_sums(got, want, ["count", "count"] + [KIND_OF_COLUMN[c & 0xff] for c in a["columns"]], _roi_pixels(a), case.name)
    if not a["scaled"] and list(a["columns"]) == list(range(1, 8)):
        _same_nan_pattern(metrics.metrics_from_stage_sums(got, tuple(a["columns"])), pred, gt, a, case.name)
