"""Cost of median scaling on the MI355X: the selection (mr_median_select_f32 + the single-wave ratio launch) and the
stage-scaled reduction at c2 batch 2 (sparse and dense targets) and at 512x1024, and Evaluater.eval at c2 batch 2 with
median_scaling True against False over the same batches.  Prints one JSON line.

    python tools/bench_median.py [--reps 50] [--batches 16]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monorec_amd import evaluate, metrics, synth  # noqa: E402

DEV = "cuda:0"


def _time_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def kernels(reps):
    out = {}
    cols = tuple(metrics.stage_column(n) for n in metrics.SPARSE_METRICS)
    for name, (bsz, h, w, variant) in {"c2_b2_sparse": (2, 256, 512, "plain"), "c2_b2_dense": (2, 256, 512, "dense"),
                                       "b1_512x1024_sparse": (1, 512, 1024, "plain")}.items():
        pred, gt = synth.make_median_scaling_pair(bsz, h, w, 1, variant)
        p, g = pred.to(DEV), gt.to(DEV)
        sel = _time_us(lambda: metrics.median_stage_scales_device(metrics.median_stats_device(p, g), len(cols)), reps)
        scales = metrics.median_stage_scales_device(metrics.median_stats_device(p, g), len(cols))[0]
        red = _time_us(lambda: metrics.metric_stage_sums_device(p, g, cols, None, 80, scales), reps)
        fused = _time_us(lambda: metrics.sparse_metric_sums_device({"result": p, "target": g}, None, 80), reps)
        out[name] = {"selection_us": round(sel, 1), "stage_sums_us": round(red, 1), "unscaled_fused_sums_us": round(fused, 1)}
    return out


def evaluation(nb, repeats):
    from monorec_amd import MonoRecModel
    model = MonoRecModel()
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    batches = []
    for i in range(nb):
        data = synth.make_batch(2, 256, 512, 2, seed=100 + i)
        _, target = synth.make_depth_pair(2, 256, 512, seed=200 + i)
        batches.append((synth.clone_batch(data, DEV), target.to(DEV)))
    res = {}
    for ms in (False, True, False, True):          # interleaved: drift of the clock shows as a spread, not as a bias
        ev = evaluate.Evaluater(model, max_distance=80, median_scaling=ms)
        ev.eval(batches[:2])
        torch.cuda.synchronize()
        best = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            ev.eval(batches)
            torch.cuda.synchronize()
            best.append(time.perf_counter() - t0)
        res.setdefault("median_scaling" if ms else "plain", []).append(round(2 * nb / min(best), 2))
    return {"keyframes_per_s": res, "batches": nb, "batch": 2}


def forward_us(reps):
    from monorec_amd import MonoRecModel
    model = MonoRecModel(hip_in_flight=1)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    data = synth.clone_batch(synth.make_batch(2, 256, 512, 2, seed=3), DEV)
    with torch.no_grad():
        return round(_time_us(lambda: model(data), reps), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"kernels": kernels(a.reps), "forward_c2_b2_us": forward_us(max(5, a.reps // 5)), "eval": evaluation(a.batches, a.repeats)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
