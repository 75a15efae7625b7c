"""TEST INFRASTRUCTURE ONLY.  Fixture of the reference's TUM-MonoVO dataset class (data_loader/tum_mono_vo_dataset.py) on the
synthetic sequences of monorec_amd.synth.make_tmvo_tree.  Runs only where the reference checkout exists (imported read-only
through oracle.ref_shims) and scipy is installed (the reference's quaternion step):

    python tools/make_golden_tmvo.py  ->  tests/golden/tmvo_tree.npz, tests/golden/tmvo_tree.json

Per case of synth.TMVO_CASES the unmodified `TUMMonoVODataset(..., color_augmentation=False)` gives: length, `_image_index`,
crop box, intrinsics, inverse response table, all poses, and for every sample the `keyframe` / `frames` tensors (float32) plus
`sequence` / `image_id`.  Only data is stored.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monorec_amd import synth  # noqa: E402
from oracle import ref_shims  # noqa: E402


def main():
    ref_shims.install()
    import scipy
    from data_loader.tum_mono_vo_dataset import TUMMonoVODataset      # noqa: the real reference class
    arrays, meta = {}, {"scipy": scipy.__version__, "torch": torch.__version__, "cases": {}}
    for name, (tree_kw, ds_kw) in synth.TMVO_CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            tree = synth.make_tmvo_tree(os.path.join(tmp, "sequence_xx"), **tree_kw)
            ds = TUMMonoVODataset(tree, color_augmentation=False, **ds_kw)
            first = np.asarray(ds.open_image(0))
            samples = []
            for i in range(len(ds)):
                data, target = ds[i]
                assert sorted(data) == ["frames", "image_id", "intrinsics", "keyframe", "keyframe_intrinsics", "keyframe_pose", "poses", "sequence"]
                assert target.dtype == torch.float32 and tuple(target.shape) == (1, *ds_kw["target_image_size"]) and not target.any()
                assert torch.equal(data["keyframe_pose"], ds._poses[int(data["image_id"])])
                assert all(torch.equal(k, ds._intrinsics) for k in [data["keyframe_intrinsics"]] + data["intrinsics"])
                arrays[f"{name}.{i}.keyframe"] = data["keyframe"].numpy()
                arrays[f"{name}.{i}.frames"] = torch.stack(data["frames"]).numpy()
                arrays[f"{name}.{i}.poses"] = torch.stack(data["poses"]).numpy()
                samples.append({"image_id": int(data["image_id"]), "sequence": int(data["sequence"]),
                                "id_dtype": str(data["image_id"].dtype), "sequence_dtype": str(data["sequence"].dtype),
                                "id_shape": list(data["image_id"].shape)})
            arrays[f"{name}.image_index"] = np.asarray(ds._image_index, dtype=np.int64)
            arrays[f"{name}.intrinsics"] = ds._intrinsics.numpy()
            arrays[f"{name}.inv_pcalib"] = ds._pcalib.numpy()
            arrays[f"{name}.all_poses"] = ds._poses.numpy()
            assert ds._poses.dtype == torch.float32 and ds._intrinsics.dtype == torch.float32 and ds._pcalib.dtype == torch.float32
            meta["cases"][name] = {"length": len(ds), "crop_box": [float(v) for v in ds._crop_box], "offset": int(ds._offset),
                                   "first_image_sha1": hashlib.sha1(first.tobytes()).hexdigest(), "first_image_shape": list(first.shape),
                                   "samples": samples}
            print(name, "len", len(ds), "image_index", ds._image_index, "box", ds._crop_box)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "tmvo_tree.npz"), **arrays)
    with open(os.path.join(ROOT, "tests", "golden", "tmvo_tree.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
