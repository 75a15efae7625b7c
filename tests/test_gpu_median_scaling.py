"""GPU (MI355X): median scaling (mr_median_select_f32 + mr_median_stage_scales_f32) and the stage-scaled metric reduction
(mr_metric_stage_sums_f32) against the reference's outputs (tests/golden/median_scaling.json) and torch.median."""
import json
import math
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from monorec_amd import evaluate, metrics, synth
from oracle import monorec_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 2e-5     # as tests/test_gpu_metrics.py: fp32 per-element terms, fp64 accumulation here vs fp32 torch sums in the reference
FIXTURE = json.load(open(os.path.join(GOLDEN, "median_scaling.json")))


def f32(h):
    return float(np.uint32(int(h, 16)).view(np.float32))


def same(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def close(got, want):
    got, want = float(got), float(want)
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= RTOL * max(1.0, abs(want))


@pytest.mark.parametrize("name", sorted(FIXTURE["selections"]))
def test_selection_and_ratios_match_reference_and_torch_median(hip_lib, name):
    case = FIXTURE["selections"][name]
    pred, gt = synth.make_median_scaling_pair(*case["gen"])
    p, g = pred.to(DEV), gt.to(DEV)
    stats = metrics.median_stats_device(p, g)
    st = stats.cpu()
    fl = stats.view(torch.float32).cpu()
    for i, s in enumerate(case["samples"]):
        assert int(st[i, 0]) == s["count"]
        assert [int(st[i, 4]), int(st[i, 5]), int(st[i, 6])] == [s["nans"], s["zeros"], s["infs"]], name
        assert same(fl[i, 1], f32(s["target_median"])), (name, i)
        m = g[i] > 0
        if s["count"]:
            assert same(fl[i, 1], torch.median(g[i][m]).item())
        if s["count"] and not s["nans"]:
            assert same(fl[i, 2], f32(s["lo"])) and same(fl[i, 3], f32(s["hi"])), (name, i)
            assert same(fl[i, 2], torch.median(p[i][m]).item())
    scales, _ = metrics.median_stage_scales_device(stats, FIXTURE["stages"])
    scales = scales.cpu()
    for i, row in enumerate(case["ratios"]):
        for j, h in enumerate(row):
            assert same(scales[i, j], f32(h)), (name, i, j, float(scales[i, j]), f32(h))
    # median_scaling() called repeatedly (the drop-in path): the same multiplies by the same ratios, bit for bit
    d, want = {"result": p, "target": g}, pred.clone()
    for j in range(FIXTURE["stages"]):
        d = metrics.median_scaling(d)
        want = want * torch.tensor([f32(row[j]) for row in case["ratios"]], dtype=torch.float32).view(-1, 1, 1, 1)
        got = d["result"].cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0)), (name, j)
    assert d["result"] is not p and metrics._MEDIAN_KEY in d


@pytest.mark.parametrize("name", sorted(FIXTURE["evals"]))
def test_eval_metrics_match_reference_fixture(hip_lib, name):
    case = FIXTURE["evals"][name]
    pred, gt = synth.make_median_scaling_pair(*case["gen"])
    data = {"result": pred.to(DEV), "target": gt.to(DEV)}
    roi, maxd, ms, names = case["roi"], case["max_distance"], case["median_scaling"], case["metrics"]
    cols = tuple(metrics.stage_column(n) for n in names)
    # the native Evaluater's path: one selection, one ratio launch, one reduction
    native = metrics.metrics_from_stage_sums(metrics.staged_metric_sums_device(data, cols, roi, maxd, ms).cpu(), cols)
    # the drop-in path: the reference's _eval_metrics loop over the rebound functions
    d, dropin = data, []
    for n in names:
        if ms:
            d = metrics.median_scaling(d)
        dropin.append(getattr(metrics, n)(d, roi, maxd))
    for n, a, b, want in zip(names, native, dropin, case["values"]):
        assert close(a, want), (name, n, float(a), want)
        assert close(b, want), (name, n, float(b), want)


def test_multi_batch_log_matches_reference_fixture(hip_lib):
    case = FIXTURE["log"]
    cols = tuple(metrics.stage_column(n) for n in case["metrics"])
    per_batch, sizes = [], []
    for gen in case["gens"]:
        pred, gt = synth.make_median_scaling_pair(*gen)
        s = metrics.staged_metric_sums_device({"result": pred.to(DEV), "target": gt.to(DEV)}, cols, case["roi"],
                                              case["max_distance"], case["median_scaling"]).cpu()
        per_batch.append([float(v) for v in metrics.metrics_from_stage_sums(s, cols)])
        sizes.append(gen[0])
    log = evaluate.evaluation_log(per_batch, sizes)
    want = case["log"]
    assert log["valid_batches"] == want["valid_batches"] == 3
    for got, w in zip(log["metrics"] + log["metrics_correct"], want["metrics"] + want["metrics_correct"]):
        assert close(got, w), (got, w)


def _median_scaling_cpu(res, gt):
    """utils/util.py:135-142 written out on the host (torch.median on CPU tensors)."""
    mask = gt > 0
    r = torch.tensor([torch.median(gt[i, mask[i]]) / torch.median(res[i, mask[i]]) for i in range(gt.shape[0])], dtype=torch.float32)
    return res * r.view(-1, 1, 1, 1)


def test_evaluater_median_scaling_matches_oracle_chain(hip_lib):
    from monorec_amd import MonoRecModel
    model = MonoRecModel(cv_depth_steps=8)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    batches = []
    for i in range(4):
        data = synth.make_batch(2, 64, 96, 2, seed=40 + i)
        _, target = synth.make_depth_pair(2, 64, 96, seed=60 + i)
        if i == 2:
            target[1] = 0                      # no ground truth: NaN ratio -> NaN metrics -> the batch is invalid
        batches.append((data, target))
    log = evaluate.Evaluater(model, max_distance=80, median_scaling=True).eval(batches)
    per_batch = []
    for data, target in batches:
        with torch.no_grad():
            res = model(synth.clone_batch(data, "cuda:0"))["result"].cpu().clone()
        vals = []
        for name in metrics.SPARSE_METRICS:
            res = _median_scaling_cpu(res, target)
            vals.append(float(orc.sparse_metrics(res, target, None, 80)[name]))
        per_batch.append(vals)
    want = evaluate.evaluation_log(per_batch, [2] * 4)
    assert log["valid_batches"] == want["valid_batches"] == 3
    for got, w in zip(log["metrics"] + log["metrics_correct"], want["metrics"] + want["metrics_correct"]):
        assert math.isclose(got, w, rel_tol=2e-5, abs_tol=1e-7), (got, w)
    # median_scaling=False is today's evaluation, unchanged
    off = evaluate.Evaluater(model, max_distance=80, median_scaling=False).eval(batches)
    today = evaluate.Evaluater(model, max_distance=80).eval(batches)
    assert off["valid_batches"] == today["valid_batches"]
    for key in ("metrics", "metrics_correct"):
        for a, b in zip(off[key], today[key]):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (key, a, b)
