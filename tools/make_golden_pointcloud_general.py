"""TEST INFRASTRUCTURE ONLY.  Fixture of the reference's own `PLYSaver.add_depthmap` (utils/ply_utils.py:34-53, with model/layers.py
Backprojection) on two GENERAL-camera cases of tests/pointcloud_paths.py - a skewed K, a rotation about (1, 2, 3), a translation:

    batch.b3_negative_roi   three cameras, one per batch element, under a roi with negative entries (python slicing)
    uniform.null            dropout 0: the reference draws no random numbers and thins nothing

Runs only where the reference checkout exists (imported read-only through oracle.ref_shims):

    python tools/make_golden_pointcloud_general.py  ->  tests/golden/pointcloud_general.npz, tests/golden/pointcloud_general.json

The class runs unmodified.  Only data is stored: the inputs of each case and the records the reference appended.  The three fixtures of
oracle/make_golden.py (pointcloud_*.npz, pointcloud_cases.json) are not touched."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pointcloud_paths as pc  # noqa: E402
from oracle import ref_shims  # noqa: E402


def main():
    ref_shims.install()
    from utils.ply_utils import PLYSaver as RefPLYSaver                  # noqa: the real reference class
    arrays, meta = {}, {"torch": torch.__version__, "numpy": np.__version__, "cases": {}}
    for name in pc.FIXTURE_CASES:
        case = next(c for c in pc.CASES if f"{c.entry}.{c.name}" == name)
        ops = pc.operands(case)
        assert not ops["masks"] and ops["uniform"] is None and ops["dropout"] == 0
        b, h, w = ops["b"], ops["h"], ops["w"]
        t = lambda x, *s: torch.from_numpy(np.array(x, copy=True)).view(*s)                 # noqa: E731
        saver = RefPLYSaver(h, w, min_d=ops["min_d"], max_d=ops["max_d"], batch_size=b, roi=ops["roi"], dropout=0)
        saver.add_depthmap(t(ops["inv_depth"], b, 1, h, w), t(ops["image"], b, 3, h, w), t(ops["intrinsics"], b, 4, 4), t(ops["pose"], b, 4, 4))
        rec = np.array(saver.data, dtype=np.float32).reshape(-1, 6)
        ours = pc.oracle_records(ops).numpy()
        assert ours.shape == rec.shape and np.array_equal(ours[:, 3:], rec[:, 3:]), (name, ours.shape, rec.shape)
        for key in ("inv_depth", "image", "intrinsics", "pose"):
            arrays[f"{name}.{key}"] = np.asarray(ops[key], dtype=np.float32)
        arrays[f"{name}.records"] = rec
        meta["cases"][name] = dict(b=b, h=h, w=w, min_d=ops["min_d"], max_d=ops["max_d"], roi=ops["roi"], dropout=0, points=int(rec.shape[0]),
                                   oracle_bit_equal_on_the_recording_host=bool(np.array_equal(ours, rec)))
        print(name, rec.shape[0], "points; oracle bit-equal:", meta["cases"][name]["oracle_bit_equal_on_the_recording_host"])
    np.savez_compressed(os.path.join(pc.GOLDEN, "pointcloud_general.npz"), **arrays)
    with open(os.path.join(pc.GOLDEN, "pointcloud_general.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
