"""TEST INFRASTRUCTURE ONLY.  Fixture of the reference's median scaling (utils/util.py:135-142) and of its
`Evaluater._eval_metrics` / `Evaluater.eval` (evaluater/evaluater.py:38-118) with median scaling and the dense-target metrics.
Runs only where the reference checkout exists (imported read-only through oracle.ref_shims):

    python tools/make_golden_median_scaling.py  ->  tests/golden/median_scaling.json

Inputs come from monorec_amd.synth.make_median_scaling_pair (seeded); no tensor is stored.  Floats that must match bit for
bit (medians, order statistics, ratios) are stored as float32 hex ('0x3f800000'); metric values as plain floats.
"""
import json
import logging
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monorec_amd import synth  # noqa: E402
from oracle import ref_shims  # noqa: E402

STAGES = 7
SPARSE = ["abs_rel_sparse_metric", "sq_rel_sparse_metric", "rmse_sparse_metric", "rmse_log_sparse_metric",
          "a1_sparse_metric", "a2_sparse_metric", "a3_sparse_metric"]          # configs/evaluate/eval_monorec.json:53-61
DENSE = ["a1_metric", "a2_metric", "a3_metric", "rmse_metric", "rmse_log_metric", "abs_rel_metric", "sq_rel_metric"]
MIXED = ["a1_sparse_metric", "abs_rel_metric", "rmse_sparse_metric", "sq_rel_metric", "rmse_log_metric"]


def hexf(v):
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]


def selection(pred, gt):
    """Per sample: count, lower median of the target, prediction sorted[(n-1)//2] and sorted[n//2], NaN / zero / inf counts."""
    out = []
    for i in range(gt.shape[0]):
        m = gt[i] > 0
        t, p = gt[i][m], pred[i][m]
        n = int(m.sum())
        ps = torch.sort(p).values
        out.append({"count": n, "target_median": hexf(torch.median(t)),
                    "lo": hexf(ps[(n - 1) // 2]) if n else hexf(float("nan")), "hi": hexf(ps[n // 2]) if n else hexf(float("nan")),
                    "nans": int(torch.isnan(p).sum()), "zeros": int((p == 0).sum()), "infs": int(torch.isinf(p).sum())})
    return out


def stage_ratios(median_scaling, pred, gt):
    """The ratios of STAGES calls of the reference's median_scaling in a row, checked against its own output bit for bit."""
    d = {"result": pred.clone(), "target": gt.clone()}
    rows = [[] for _ in range(gt.shape[0])]
    for _ in range(STAGES):
        prev = d["result"]
        mask = gt > 0
        r = torch.tensor([torch.median(gt[i, mask[i]]) / torch.median(prev[i, mask[i]]) for i in range(gt.shape[0])],
                         dtype=torch.float32)
        d = median_scaling(d)
        want = prev * r.view(-1, 1, 1, 1)
        assert torch.equal(torch.nan_to_num(d["result"], 7.0), torch.nan_to_num(want, 7.0)), "ratio mirror differs from the reference"
        assert torch.equal(torch.isnan(d["result"]), torch.isnan(want))
        for i in range(gt.shape[0]):
            rows[i].append(hexf(r[i]))
    return rows


class _StandIn:
    """The attributes Evaluater._eval_metrics / Evaluater.eval read from `self`."""

    def __init__(self, metrics, roi, max_distance, median_scaling, loader=None):
        self.metrics, self.roi, self.max_distance, self.median_scaling = metrics, roi, max_distance, median_scaling
        self.data_loader, self.len_data = loader, len(loader or [])
        self.device, self.log_step = "cpu", 10 ** 9
        self.logger = logging.getLogger("median_scaling_fixture")

    class _Forward:                                # the forward is stood in for: the batches carry their "result"
        def eval(self):
            pass

        def __call__(self, data):
            return data

    model = _Forward()

    def _progress(self, i):
        return str(i)


def main():
    ref_shims.reference_model_class()                        # installs the import shims
    import evaluater.evaluater as ev                         # noqa: the real reference modules
    import model.metric as ref_metric
    import utils
    out = {"stages": STAGES, "selections": {}, "evals": {}, "log": {}}

    sel_cases = {"c2_sparse": (2, 256, 512, 5, "plain"), "c2_dense": (2, 256, 512, 6, "dense"), "b1_512x1024": (1, 512, 1024, 7, "plain"),
                 "ties": (2, 64, 96, 8, "ties"), "empty": (2, 64, 96, 9, "empty"), "nan_pred": (2, 64, 96, 10, "nan_pred"),
                 "zero_median": (2, 64, 96, 11, "zero_median"), "negative": (2, 64, 96, 12, "negative"),
                 "small_odd_even": (3, 16, 24, 13, "plain")}
    for name, gen in sel_cases.items():
        pred, gt = synth.make_median_scaling_pair(*gen)
        out["selections"][name] = {"gen": list(gen), "samples": selection(pred, gt),
                                   "ratios": stage_ratios(utils.median_scaling, pred, gt)}
    # a compounding case: the first seed whose second or later ratio is not exactly 1.0
    for seed in range(100, 400):
        gen = (2, 64, 96, seed, "plain")
        pred, gt = synth.make_median_scaling_pair(*gen)
        rows = stage_ratios(utils.median_scaling, pred, gt)
        if any(h != hexf(1.0) for row in rows for h in row[1:]):
            out["selections"]["compound"] = {"gen": list(gen), "samples": selection(pred, gt), "ratios": rows}
            break
    else:
        raise SystemExit("no compounding case found")
    counts = [s["count"] for c in out["selections"].values() for s in c["samples"]]
    assert any(n % 2 for n in counts) and any(n and n % 2 == 0 for n in counts) and 0 in counts

    fns = lambda names: [getattr(ref_metric, n) for n in names]     # noqa: E731
    eval_cases = {
        "eval_monorec": ((2, 64, 96, 20, "plain"), SPARSE, None, 80, False),
        "eval_monorec_ms": ((2, 64, 96, 20, "plain"), SPARSE, None, 80, True),
        "eval_monorec_roi": ((2, 64, 96, 21, "plain"), SPARSE, [8, 56, 8, 88], 80, False),
        "eval_monorec_roi_ms": ((2, 64, 96, 21, "plain"), SPARSE, [8, 56, 8, 88], 80, True),
        "dense_80": ((2, 64, 96, 22, "dense"), DENSE, None, 80, False),
        "dense_80_ms": ((2, 64, 96, 22, "dense"), DENSE, None, 80, True),
        "dense_none": ((2, 64, 96, 23, "plain"), DENSE, None, None, False),          # zero targets: inf depths, NaN abs_rel
        "dense_none_ms_roi": ((2, 64, 96, 24, "dense"), DENSE, [4, 60, 8, 80], None, True),
        "mixed_ms": ((2, 64, 96, 25, "plain"), MIXED, None, 80, True),
        "mixed_ties_ms": ((2, 64, 96, 26, "ties"), MIXED, [8, 56, 8, 88], 80, True),
        "negative_ms": ((2, 64, 96, 12, "negative"), SPARSE, None, 80, True),
        "zero_median_ms": ((2, 64, 96, 11, "zero_median"), MIXED, None, 80, True),
        "compound_ms": (tuple(out["selections"]["compound"]["gen"]), SPARSE + DENSE, None, 80, True),
    }
    for name, (gen, names, roi, maxd, ms) in eval_cases.items():
        pred, gt = synth.make_median_scaling_pair(*gen)
        raw = []
        me = _StandIn(fns(names), roi, maxd, ms)
        me.metrics = [lambda d, r, m, f=f: raw.append(float(f(d, r, m))) or raw[-1] for f in fns(names)]
        acc, valid = ev.Evaluater._eval_metrics(me, {"result": pred.clone(), "target": gt.clone()})
        out["evals"][name] = {"gen": list(gen), "metrics": names, "roi": roi, "max_distance": maxd, "median_scaling": ms,
                              "values": raw, "acc": [float(v) for v in acc], "valid": [float(v) for v in valid]}
        print(name, [round(v, 4) for v in raw])

    gens = [(2, 64, 96, 30, "plain"), (2, 64, 96, 31, "empty"), (1, 64, 96, 32, "ties"), (2, 64, 96, 33, "plain")]
    loader = []
    for gen in gens:
        pred, gt = synth.make_median_scaling_pair(*gen)
        loader.append(({"result": pred, "keyframe": torch.zeros(1)}, gt))
    me = _StandIn(fns(SPARSE), None, 80, True, loader)
    me._eval_metrics = lambda d: ev.Evaluater._eval_metrics(me, d)
    log = ev.Evaluater.eval(me, 0)
    out["log"] = {"gens": [list(g) for g in gens], "metrics": SPARSE, "roi": None, "max_distance": 80, "median_scaling": True,
                  "log": {"metrics": [float(v) for v in log["metrics"]], "metrics_correct": [float(v) for v in log["metrics_correct"]],
                          "valid_batches": float(log["valid_batches"])}}
    print("log", out["log"]["log"])
    with open(os.path.join(ROOT, "tests", "golden", "median_scaling.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True, allow_nan=True)


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
