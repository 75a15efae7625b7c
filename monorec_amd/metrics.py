"""Sparse depth metrics of the reference (model/metric_functions/sparse_metrics.py:136-252), same function names
and signatures, computed by ONE fused HIP reduction (mr_sparse_metric_sums_f32) and one 64*B byte device->host
copy per batch instead of ~70 full-tensor ATen passes and 7 host syncs (evaluater/evaluater.py:38-50).

`evaluate.py` looks metrics up by name (`getattr(module_metric, met)`, evaluate.py:24): bind this module instead of
`model.metric` to use them.  The seven calls of one batch share a single kernel launch (the sums are cached on the
data dict).  The two options the evaluation configs never set - `pred_all_valid=False` (utils/util.py:105-106: entries whose
prediction is 0 are masked) and `use_cvmask=True` (sparse_metrics.py:86: entries outside `mvobj_mask > .5` are masked) - only add
entries to the mask, and the reduction masks every entry whose target is 0: they run the same launch on a copy of the target that
is zeroed there (two element-wise device ops, no host synchronisation).
"""
import ctypes
import math

import torch

from . import _lib

_CACHE_KEY = "_monorec_amd_metric_sums"


def sparse_metric_sums_device(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    """(B, 8) float64 DEVICE tensor of per-sample sums - one asynchronous launch, no host synchronisation."""
    pred, gt = data_dict["result"], data_dict["target"]
    if not pred.is_cuda:
        raise RuntimeError("monorec_amd.metrics needs result/target on a HIP device; there is no CPU path")
    lib = _lib.load()
    pred = pred.contiguous().float()
    gt = gt.contiguous().float()
    if not pred_all_valid:                                   # utils/util.py:105-106
        gt = torch.where(pred == 0, torch.zeros_like(gt), gt)
    if use_cvmask:                                           # sparse_metrics.py:86 (KeyError without the mask, like the reference)
        if roi is not None:                                  # the reference crops prediction and target but not the mask: its line raises a shape error
            raise RuntimeError("use_cvmask with a roi: the reference compares the cropped target with the uncropped mvobj_mask and fails; not defined")
        gt = torch.where(data_dict["mvobj_mask"].to(gt.device) > .5, gt, torch.zeros_like(gt))
    b, _, h, w = pred.shape
    assert gt.shape == pred.shape
    sums = torch.empty(b, 8, dtype=torch.float64, device=pred.device)
    roi_arr = (ctypes.c_int32 * 4)(*[int(v) for v in roi]) if roi is not None else None
    if _MEDIAN_KEY in data_dict:     # a median_scaling() result: relu / clamp_min keep NaN there, like the reference (a NaN ratio)
        return metric_stage_sums_device(pred, gt, tuple(range(1, 8)), roi, max_distance)[:, [0] + list(range(2, 9))]
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    _lib.check(lib.mr_sparse_metric_sums_f32(pred.data_ptr(), gt.data_ptr(), b, h, w, roi_arr,
                                             float(max_distance) if max_distance else 0.0, sums.data_ptr(), stream),
               "mr_sparse_metric_sums_f32")
    return sums


def sparse_metric_sums(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    """(B, 8) float64 CPU tensor of per-sample sums; cached on `data_dict` for the (result, target, roi, dist, options) at hand."""
    pred, gt = data_dict["result"], data_dict["target"]
    if not pred.is_cuda:
        raise RuntimeError("monorec_amd.metrics needs result/target on a HIP device; there is no CPU path")
    mv = data_dict["mvobj_mask"] if use_cvmask else None
    key = (pred.data_ptr(), pred._version, gt.data_ptr(), gt._version, None if roi is None else tuple(roi), max_distance,
           bool(pred_all_valid), None if mv is None else (mv.data_ptr(), mv._version))
    cached = data_dict.get(_CACHE_KEY)
    if cached is not None and cached[0] == key:
        return cached[1]
    out = sparse_metric_sums_device(data_dict, roi, max_distance, pred_all_valid, use_cvmask).cpu()
    data_dict[_CACHE_KEY] = (key, out)
    return out


def metrics_from_sums(s):
    """The seven metric values of one batch, in SPARSE_METRICS order, from its (B, 8) sums (CPU float64)."""
    return [_batch_ratio(s, 1), _batch_ratio(s, 2), _per_sample_rms(s, 3), _per_sample_rms(s, 4),
            _batch_ratio(s, 5), _batch_ratio(s, 6), _batch_ratio(s, 7)]


def _batch_ratio(s, col):
    """mask_mean over the whole batch (utils/util.py:110-118): sum over all samples / number of unmasked entries."""
    n = s[:, 0].sum()
    return torch.tensor(float("nan")) if n == 0 else (s[:, col].sum() / n).float()


def _per_sample_rms(s, col):
    """rmse_base / rmse_log_base (sparse_metrics.py:228-239): sqrt of the per-sample masked mean, mean over samples."""
    return torch.sqrt(s[:, col] / s[:, 0]).mean().float()


def abs_rel_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _batch_ratio(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 1)


def sq_rel_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _batch_ratio(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 2)


def rmse_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _per_sample_rms(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 3)


def rmse_log_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _per_sample_rms(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 4)


def a1_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _batch_ratio(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 5)


def a2_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _batch_ratio(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 6)


def a3_sparse_metric(data_dict, roi=None, max_distance=None, pred_all_valid=True, use_cvmask=False):
    return _batch_ratio(sparse_metric_sums(data_dict, roi, max_distance, pred_all_valid, use_cvmask), 7)


def _variants():
    """The `*_sparse_onlyvalid_metric` (pred_all_valid=False) and `*_sparse_onlydynamic_metric` (use_cvmask=True) wrappers of the reference
    (sparse_metrics.py:158-212), one pair per base metric."""
    g = globals()
    for base in ("a1", "a2", "a3", "rmse", "rmse_log", "abs_rel", "sq_rel"):
        fn = g[f"{base}_sparse_metric"]
        g[f"{base}_sparse_onlyvalid_metric"] = (lambda f: lambda data_dict, roi=None, max_distance=None: f(data_dict, roi, max_distance, False))(fn)
        g[f"{base}_sparse_onlydynamic_metric"] = (lambda f: lambda data_dict, roi=None, max_distance=None: f(data_dict, roi, max_distance, use_cvmask=True))(fn)


_variants()

SPARSE_METRICS = ("abs_rel_sparse_metric", "sq_rel_sparse_metric", "rmse_sparse_metric", "rmse_log_sparse_metric",
                  "a1_sparse_metric", "a2_sparse_metric", "a3_sparse_metric")     # configs/evaluate/eval_monorec.json:53-61


# ---- median scaling and the dense-target metrics (evaluater/evaluater.py:36-43, utils/util.py:135-142, sparse_metrics.py:6-78) ----

DENSE_METRICS = ("abs_rel_metric", "sq_rel_metric", "rmse_metric", "rmse_log_metric", "a1_metric", "a2_metric", "a3_metric")
MAX_STAGES = 16                 # MR_MAX_METRIC_STAGES
_DENSE = 0x100                  # MR_METRIC_DENSE
_MEDIAN_KEY = "_monorec_amd_median_stats"
_DENSE_KEY = "_monorec_amd_dense_sums"
_STATS_FIELDS = 8               # mr_median_stats: count, target_median, lo, hi, nans, zeros, infs, reserved (4 bytes each)


def stage_column(name):
    """Column of mr_metric_stage_sums_f32 for a metric name: 1..7 (the mr_sparse_metric_sums_f32 layout), | MR_METRIC_DENSE."""
    if name in SPARSE_METRICS:
        return SPARSE_METRICS.index(name) + 1
    if name in DENSE_METRICS:
        return (DENSE_METRICS.index(name) + 1) | _DENSE
    raise NotImplementedError(f"no fused form of {name}")


def _device_pair(data_dict):
    pred, gt = data_dict["result"], data_dict["target"]
    if not pred.is_cuda:
        raise RuntimeError("monorec_amd.metrics needs result/target on a HIP device; there is no CPU path")
    assert gt.shape == pred.shape
    return pred.contiguous().float(), gt.contiguous().float()


def median_stats_device(pred, gt):
    """(B, 8) int32 DEVICE tensor holding one mr_median_stats per sample (view the float fields with .view(torch.float32)):
    exact lower median of target[target > 0], prediction order statistics sorted[(n-1)//2], sorted[n//2] over the same mask,
    NaN / zero / inf counts.  One launch, no host synchronisation."""
    lib = _lib.load()
    b, _, h, w = pred.shape
    ws = torch.empty(int(lib.mr_median_select_workspace_bytes(b, h, w)), dtype=torch.uint8, device=pred.device)
    stats = torch.empty(b, _STATS_FIELDS, dtype=torch.int32, device=pred.device)
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    _lib.check(lib.mr_median_select_f32(pred.data_ptr(), gt.data_ptr(), b, h, w, ws.data_ptr(), stats.data_ptr(), stream),
               "mr_median_select_f32")
    return stats


def median_stage_scales_device(stats, num_stages):
    """(B, num_stages) float32 ratios of num_stages median_scaling calls in a row and the (B, 8) statistics after them."""
    lib = _lib.load()
    b = stats.shape[0]
    scales = torch.empty(b, num_stages, dtype=torch.float32, device=stats.device)
    after = torch.empty_like(stats)
    stream = torch.cuda.current_stream(stats.device).cuda_stream
    _lib.check(lib.mr_median_stage_scales_f32(stats.data_ptr(), b, num_stages, scales.data_ptr(), after.data_ptr(), stream),
               "mr_median_stage_scales_f32")
    return scales, after


def metric_stage_sums_device(pred, gt, columns, roi=None, max_distance=None, scales=None):
    """(B, 2 + k) float64 DEVICE sums of mr_metric_stage_sums_f32: [#valid, #roi pixels, stage 0, ..., stage k-1]."""
    if not 1 <= len(columns) <= MAX_STAGES:
        raise NotImplementedError(f"{len(columns)} metrics in one pass (at most {MAX_STAGES})")
    lib = _lib.load()
    b, _, h, w = pred.shape
    sums = torch.empty(b, 2 + len(columns), dtype=torch.float64, device=pred.device)
    roi_arr = (ctypes.c_int32 * 4)(*[int(v) for v in roi]) if roi is not None else None
    cols = (ctypes.c_int32 * len(columns))(*columns)
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    _lib.check(lib.mr_metric_stage_sums_f32(pred.data_ptr(), gt.data_ptr(), b, h, w, roi_arr,
                                            float(max_distance) if max_distance else 0.0,
                                            None if scales is None else scales.data_ptr(), len(columns), cols, sums.data_ptr(),
                                            stream), "mr_metric_stage_sums_f32")
    return sums


def staged_metric_sums_device(data_dict, columns, roi=None, max_distance=None, median_scaling=False):
    """One Evaluater batch: (B, 2 + k) float64 device sums of the k configured metrics (stage_column codes, config order).
    With median_scaling, metric j sees the prediction rescaled j + 1 times (evaluater.py:40-43): one selection launch, one
    single-wave launch for the ratios, one reduction launch; no host synchronisation."""
    pred, gt = _device_pair(data_dict)
    scales = median_stage_scales_device(median_stats_device(pred, gt), len(columns))[0] if median_scaling else None
    return metric_stage_sums_device(pred, gt, columns, roi, max_distance, scales)


def metrics_from_stage_sums(s, columns):
    """The k metric values of one batch from its (B, 2 + k) CPU float64 stage sums."""
    out = []
    for j, c in enumerate(columns):
        t = torch.stack([s[:, 1] if c & _DENSE else s[:, 0], s[:, 2 + j]], 1)
        out.append(_per_sample_rms(t, 1) if (c & 0xff) in (3, 4) else _batch_ratio(t, 1))
    return out


def stage_ratios_host(count, target_median, lo, hi, nans, zeros, infs, num_stages):
    """Host mirror (numpy float32) of mr_median_stage_scales_f32: the ratios of num_stages median_scaling calls in a row."""
    import numpy as np
    f = np.float32
    tm, lo, hi = f(target_median), f(lo), f(hi)
    nan = bool(nans) or count == 0
    out = []
    with np.errstate(all="ignore"):
        for _ in range(num_stages):
            r = f("nan") if nan else tm / lo
            out.append(r)
            if np.isnan(r) or (r == 0 and infs) or (np.isinf(r) and zeros):
                nan = True
                continue
            a, c = lo * r, hi * r
            lo, hi = (c, a) if np.signbit(r) else (a, c)
            if r == 0:
                zeros, infs = count, 0
            elif np.isinf(r):
                zeros, infs = 0, count
    return out


def _key(t):
    return (t.data_ptr(), t._version)


def median_scaling(data_dict):
    """utils/util.py:135-142: a NEW dict whose "result" is the prediction times median(target[mask]) / median(prediction[mask])
    per sample (mask = target > 0 over the whole image), the same fp32 multiply by the same ratio as the reference.  The
    selected statistics ride along on the returned dict: calling median_scaling on it again (evaluater.py:40-43 does, once per
    metric) derives the next ratio from them on the device instead of selecting again."""
    pred, gt = data_dict["result"], data_dict["target"]
    if not pred.is_cuda:
        raise RuntimeError("monorec_amd.metrics needs result/target on a HIP device; there is no CPU path")
    cached = data_dict.get(_MEDIAN_KEY)
    if cached is not None and cached[0] == (_key(pred), _key(gt)):
        stats = cached[1]
    else:
        stats = median_stats_device(*_device_pair(data_dict))
    scales, after = median_stage_scales_device(stats, 1)
    out = dict(data_dict)
    out["result"] = pred * scales.view(-1, 1, 1, 1)
    out[_MEDIAN_KEY] = ((_key(out["result"]), _key(gt)), after)
    return out


def dense_metric_sums(data_dict, roi=None, max_distance=None):
    """(B, 9) float64 CPU stage sums of the seven dense-target metrics (DENSE_METRICS order), one launch per data dict."""
    pred, gt = data_dict["result"], data_dict["target"]
    if not pred.is_cuda:
        raise RuntimeError("monorec_amd.metrics needs result/target on a HIP device; there is no CPU path")
    key = (_key(pred), _key(gt), None if roi is None else tuple(roi), max_distance)
    cached = data_dict.get(_DENSE_KEY)
    if cached is not None and cached[0] == key:
        return cached[1]
    p, g = _device_pair(data_dict)
    out = metric_stage_sums_device(p, g, tuple(c | _DENSE for c in range(1, 8)), roi, max_distance).cpu()
    data_dict[_DENSE_KEY] = (key, out)
    return out


def _dense_metric(col):
    def metric(data_dict, roi=None, max_distance=None):
        s = dense_metric_sums(data_dict, roi, max_distance)
        t = torch.stack([s[:, 1], s[:, 1 + col]], 1)
        return _per_sample_rms(t, 1) if col in (3, 4) else _batch_ratio(t, 1)
    metric.__name__ = metric.__qualname__ = DENSE_METRICS[col - 1]
    return metric


abs_rel_metric, sq_rel_metric, rmse_metric, rmse_log_metric, a1_metric, a2_metric, a3_metric = (_dense_metric(c) for c in range(1, 8))
