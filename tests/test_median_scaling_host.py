"""Median scaling and the dense-target metrics, host side (no GPU): the ratio recurrence of mr_median_stage_scales_f32
against the reference's ratios (tests/golden/median_scaling.json, tools/make_golden_median_scaling.py), the Evaluater's
accepted metric names, and the drop-in rebinding of the new names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN
from monorec_amd import evaluate, metrics

FIXTURE = json.load(open(os.path.join(GOLDEN, "median_scaling.json")))


def f32(h):
    return np.uint32(int(h, 16)).view(np.float32)


def same_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


@pytest.mark.parametrize("name", sorted(FIXTURE["selections"]))
def test_host_ratio_recurrence_reproduces_the_reference_ratios(name):
    case = FIXTURE["selections"][name]
    for i, (s, row) in enumerate(zip(case["samples"], case["ratios"])):
        got = metrics.stage_ratios_host(s["count"], f32(s["target_median"]), f32(s["lo"]), f32(s["hi"]), s["nans"], s["zeros"],
                                        s["infs"], FIXTURE["stages"])
        assert len(got) == len(row) == FIXTURE["stages"]
        for j, (g, w) in enumerate(zip(got, row)):
            assert same_f32(g, f32(w)), (name, i, j, g, f32(w))


def test_fixture_covers_the_edge_cases():
    sel = FIXTURE["selections"]
    counts = [s["count"] for c in sel.values() for s in c["samples"]]
    assert 0 in counts and any(n % 2 for n in counts) and any(n and n % 2 == 0 for n in counts)
    assert np.isinf(f32(sel["zero_median"]["ratios"][0][0])) and np.isnan(f32(sel["zero_median"]["ratios"][0][1]))
    assert f32(sel["negative"]["ratios"][-1][0]) < 0 and f32(sel["negative"]["ratios"][-1][1]) != 1.0
    assert any(f32(h) != 1.0 for row in sel["compound"]["ratios"] for h in row[1:])
    assert sel["nan_pred"]["samples"][0]["nans"] == 1 and np.isnan(f32(sel["nan_pred"]["ratios"][0][0]))


def test_evaluater_accepts_dense_names_and_median_scaling():
    class _Model:
        hip_in_flight = 2
    names = ("a1_sparse_metric", "abs_rel_metric", "rmse_metric", "sq_rel_sparse_metric")
    ev = evaluate.Evaluater(_Model(), max_distance=80, metric_names=names, median_scaling=True)
    assert ev.median_scaling and ev._staged and len(ev._cols) == 4
    assert ev._columns == (5, 1 | 0x100, 3 | 0x100, 2)
    assert evaluate.Evaluater(_Model(), metric_names=metrics.DENSE_METRICS)._staged
    assert not evaluate.Evaluater(_Model())._staged                      # the default path is the fused sparse reduction
    for bad in ("sc_inv_metric", "l1_rel_metric", "l1_inv_metric", "completeness_metric", "covered_gt_metric", "nope"):
        with pytest.raises(NotImplementedError):
            evaluate.Evaluater(_Model(), metric_names=("a1_metric", bad), median_scaling=True)


def test_metrics_from_stage_sums_rules():
    import torch
    nan = float("nan")
    # two samples; stages: sparse abs_rel, dense rmse, dense abs_rel (inf/inf -> NaN like the reference)
    s = torch.tensor([[4.0, 10.0, 2.0, 40.0, nan], [0.0, 10.0, 0.0, 90.0, 1.0]], dtype=torch.float64)
    vals = metrics.metrics_from_stage_sums(s, (1, 3 | 0x100, 1 | 0x100))
    assert float(vals[0]) == pytest.approx(0.5)
    assert float(vals[1]) == pytest.approx((2.0 + 3.0) / 2)
    assert np.isnan(float(vals[2]))


def test_host_tensors_have_no_cpu_path():
    import torch
    d = {"result": torch.ones(1, 1, 4, 4), "target": torch.ones(1, 1, 4, 4)}
    for fn in (metrics.median_scaling, metrics.abs_rel_metric, metrics.a1_metric):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(d)


def test_dropin_rebinds_median_scaling_and_dense_metrics(tmp_path):
    """A miniature checkout: utils/util.py defines median_scaling, utils/__init__.py star-imports it, evaluater/evaluater.py
    imports it the reference's way (`from utils import median_scaling`), model/metric.py star-imports the metric functions."""
    root = tmp_path
    for d in ("model/monorec", "model/metric_functions", "utils", "evaluater"):
        (root / d).mkdir(parents=True)
    for d in ("model", "model/monorec", "model/metric_functions", "evaluater"):
        (root / d / "__init__.py").write_text("")
    (root / "model" / "monorec" / "monorec_model.py").write_text("class MonoRecModel:\n    origin = 'reference'\n")
    (root / "model" / "model.py").write_text("from .monorec.monorec_model import MonoRecModel\n")
    (root / "model" / "metric_functions" / "sparse_metrics.py").write_text(
        "".join(f"def {n}(*a, **k):\n    return 'reference'\n" for n in metrics.SPARSE_METRICS + metrics.DENSE_METRICS)
        + "def other_metric(*a, **k):\n    return 'reference'\n")
    (root / "model" / "metric.py").write_text("from .metric_functions.sparse_metrics import *\n")
    (root / "utils" / "util.py").write_text("def median_scaling(data_dict):\n    return 'reference'\n")
    (root / "utils" / "ply_utils.py").write_text("class PLYSaver:\n    origin = 'reference'\n")
    (root / "utils" / "__init__.py").write_text("from .util import *\nfrom .ply_utils import *\n")
    (root / "evaluater" / "evaluater.py").write_text("from utils import median_scaling\n")
    (root / "evaluate_like.py").write_text(
        "import model.metric as module_metric\nimport evaluater.evaluater as ev\nimport utils\n"
        "print(ev.median_scaling.__module__, utils.median_scaling.__module__, utils.util.median_scaling.__module__,\n"
        "      *[getattr(module_metric, n).__module__ for n in ('a1_metric', 'sq_rel_metric', 'rmse_log_metric', 'a1_sparse_metric')],\n"
        "      module_metric.other_metric())\n")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "monorec_amd.dropin", "evaluate_like.py"], cwd=root,
                         env=dict(os.environ, PYTHONPATH=repo), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["monorec_amd.metrics"] * 7 + ["reference"]
