"""TUM-MonoVO data source (data_loader/tum_mono_vo_dataset.py), host side: the bookkeeping of monorec_amd.tum_mono_vo against the
values the unmodified reference class produced on the same synthetic sequences (tests/golden/tmvo_tree.*, written by
tools/make_golden_tmvo.py), the refused options, the DS_Wrapper window of kitti.DeviceLoader and the config front of
pointcloud.run.  The device side is tests/test_gpu_tum_mono_vo.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from monorec_amd import kitti, pointcloud, synth, tum_mono_vo

META = json.load(open(os.path.join(GOLDEN, "tmvo_tree.json")))
Z = np.load(os.path.join(GOLDEN, "tmvo_tree.npz"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(synth.TMVO_CASES)


def _dataset(tmp_path, case, **kw):
    tree_kw, ds_kw = synth.TMVO_CASES[case]
    tree = synth.make_tmvo_tree(tmp_path / "sequence_xx", **tree_kw)
    return tum_mono_vo.TUMMonoVODataset(tree, **dict(dict(ds_kw, color_augmentation=False, device="cpu"), **kw))


def _ulps(a, b):
    """Distance in float32 steps between two float32 arrays (same sign or zero crossing handled through the ordered-integer map)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def test_fixture_covers_the_cases_the_code_shares():
    assert sorted(META["cases"]) == CASES
    assert META["cases"]["wide_f4"]["length"] == 5 and list(Z["wide_f4.image_index"]) == [0, 1, 2, 4, 5, 6, 8, 9, 10]
    assert not np.array_equal(Z["wide_f4.inv_pcalib"], np.arange(256, dtype=np.float32))          # the table is not the identity
    assert META["cases"]["wide_f4"]["crop_box"][0] > 0 and META["cases"]["tall_dilated"]["crop_box"][1] > 0      # both crop branches


@pytest.mark.parametrize("case", CASES)
def test_host_bookkeeping_equals_the_reference_fixture(tmp_path, case):
    ds, want = _dataset(tmp_path, case), META["cases"][case]
    assert len(ds) == want["length"] and ds._offset == want["offset"]
    assert np.array_equal(ds._image_index, Z[f"{case}.image_index"])
    assert [float(v) for v in ds._crop_box] == want["crop_box"]
    assert ds._pcalib.dtype == torch.float32 and np.array_equal(ds._pcalib.numpy(), Z[f"{case}.inv_pcalib"])
    k = ds._intrinsics
    assert k.dtype == torch.float32 and not k.is_cuda
    assert np.array_equal(k.numpy().view(np.uint32), Z[f"{case}.intrinsics"].view(np.uint32))     # bit-equal
    poses, ref = ds._poses.numpy(), Z[f"{case}.all_poses"]
    assert ds._poses.dtype == torch.float32 and poses.shape == ref.shape
    assert np.array_equal(poses[:, :3, 3].view(np.uint32), ref[:, :3, 3].view(np.uint32))          # t * scale_factor: bit-equal
    assert np.array_equal(poses[:, 3], ref[:, 3])
    steps = _ulps(poses[:, :3, :3], ref[:, :3, :3])
    print(f"{case}: {int((steps != 0).sum())} of {steps.size} rotation entries differ from scipy's, max {int(steps.max())} ulp")
    assert steps.max() <= 1
    # the source frames of every sample: the TUM class's own order (not KITTI's symmetric one), as rows of result.txt
    for i, sample in enumerate(want["samples"]):
        assert i + ds._offset == sample["image_id"]
        rows = ds._source_rows(i)
        assert len(rows) == ds.frame_count and i + ds._offset not in rows
        assert np.array_equal(ds._poses[rows].numpy()[:, :3, 3].view(np.uint32), Z[f"{case}.{i}.poses"][:, :3, 3].view(np.uint32))
    assert ds._source_rows(0) == {"wide_f4": [0, 1, 3, 4], "tall_dilated": [0, 4], "rgb": [0, 2]}[case]
    with pytest.raises(IndexError):
        ds[len(ds)]


def test_quaternion_matrices_are_rotations_whatever_the_norm():
    rng = np.random.RandomState(2)
    q = rng.randn(50, 4) * rng.uniform(0.1, 7.0, size=(50, 1))
    m = tum_mono_vo.quaternions_to_matrices(q)
    assert np.allclose(m @ m.transpose(0, 2, 1), np.eye(3), atol=1e-14) and np.allclose(np.linalg.det(m), 1.0, atol=1e-14)
    assert np.array_equal(tum_mono_vo.quaternions_to_matrices([0.0, 0.0, 0.0, 2.0])[0], np.eye(3))
    half = np.sqrt(0.5)
    assert np.allclose(tum_mono_vo.quaternions_to_matrices([0.0, 0.0, half, half])[0], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)


def test_camera_file_in_both_first_line_forms(tmp_path):
    (tmp_path / "a.txt").write_text("0.5 0.75 0.25 0.125 0.9\n640 480\ncrop\n640 480\n")
    (tmp_path / "b.txt").write_text("RadTan 0.5 0.75 0.25 0.125 0 0 0 0\n640 480\n")
    for name in ("a.txt", "b.txt"):
        p = tum_mono_vo.load_orig_intrinsics(tmp_path / name)
        assert p.dtype == np.float64 and (p[0, 0], p[1, 1], p[0, 2], p[1, 2]) == (0.5, 0.75, 0.25, 0.125)
        assert p[2, 2] == p[3, 3] == 1.0 and p.sum() == 3.625


def test_real_geometry_takes_the_row_dropping_branch():
    """1024x1280 -> 480x640: box (0, 32, 1280, 992), exactly 2x."""
    p = np.identity(4)
    _, box = tum_mono_vo.input_pipeline.compute_target_intrinsics(p, (1024, 1280), (480, 640))
    assert tuple(box) == (0, 32.0, 1280, 992.0)


def test_unsupported_options_raise_and_there_is_no_cpu_fallback(tmp_path):
    tree_kw, ds_kw = synth.TMVO_CASES["wide_f4"]
    tree = synth.make_tmvo_tree(tmp_path / "seq", **tree_kw)
    with pytest.raises(NotImplementedError, match="pass color_augmentation=False, as configs/test/pointcloud_monorec_tmvo.json does"):
        tum_mono_vo.TUMMonoVODataset(tree, device="cpu", **ds_kw)                     # the reference's default
    with pytest.raises(NotImplementedError, match="only_keyframes"):
        tum_mono_vo.TUMMonoVODataset(tree, device="cpu", color_augmentation=False, only_keyframes=True, **ds_kw)
    ds = tum_mono_vo.TUMMonoVODataset(tree, device="cpu", color_augmentation=False, **ds_kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ds[0]
    os.makedirs(os.path.join(tree, "images_depth"))
    open(os.path.join(tree, "images_depth", "00002_d.exr"), "wb").close()
    with pytest.raises(NotImplementedError, match="EXR"):
        tum_mono_vo.TUMMonoVODataset(tree, device="cpu", color_augmentation=False, **ds_kw)


def test_multi_dataset_concatenates_sequences(tmp_path):
    trees = [synth.make_tmvo_tree(tmp_path / f"seq{i}", **synth.TMVO_CASES[c][0]) for i, c in enumerate(("wide_f4", "tall_dilated"))]
    kw = dict(frame_count=2, target_image_size=(24, 32), color_augmentation=False, device="cpu")
    multi = tum_mono_vo.TUMMonoVOMultiDataset(trees, **kw)
    assert len(multi) == 7 + 7 and multi.target_image_size == (24, 32) and len(multi.datasets) == 2
    assert len(tum_mono_vo.TUMMonoVOMultiDataset(trees[0], **kw)) == 7          # a single folder, as the reference accepts
    with pytest.raises(IndexError):
        multi[14]
    with pytest.raises(NotImplementedError):
        tum_mono_vo.TUMMonoVOMultiDataset(trees, frame_count=2)


class _Fake:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        t = torch.full((1, 2, 2), float(i))
        return {"keyframe": t, "image_id": torch.tensor([i])}, t


@pytest.mark.parametrize("n,start,end,every_nth", [(11, 0, -1, 1), (11, 3, -1, 1), (11, 0, 7, 1), (11, 2, 9, 3), (11, 1, -1, 4),
                                                   (11, 0, 11, 5), (200, 0, 200, 1), (11, 4, 5, 2), (11, 5, 5, 1)])
def test_device_loader_window_is_the_ds_wrapper_arithmetic(n, start, end, every_nth):
    """utils/util.py:148-163 restated: end == -1 -> len(dataset); item i -> dataset[i * every_nth + start];
    length (end - start) // every_nth, plus one when every_nth does not divide the span."""
    stop = n if end == -1 else end
    length = (stop - start) // every_nth + (1 if (stop - start) % every_nth != 0 else 0)
    want = [i * every_nth + start for i in range(length)]
    for batch_size in (1, 2):
        loader = kitti.DeviceLoader(_Fake(n), batch_size=batch_size, start=start, end=end, every_nth=every_nth)
        got = [int(v) for data, _ in loader for v in data["image_id"].flatten()]
        assert got == want and len(loader) == -(-length // batch_size)


def test_device_loader_defaults_are_the_whole_dataset():
    batches = list(kitti.DeviceLoader(_Fake(7), batch_size=2))
    assert [[int(v) for v in d["image_id"].flatten()] for d, _ in batches] == [[0, 1], [2, 3], [4, 5], [6]]
    shards = [[int(d["image_id"][0]) for d, _ in kitti.DeviceLoader(_Fake(7), batch_size=2, rank=r, world_size=2)] for r in range(2)]
    assert shards == [[0, 4], [2, 6]]
    windowed = [[int(d["image_id"][0]) for d, _ in kitti.DeviceLoader(_Fake(9), 1, rank=r, world_size=2, start=1, every_nth=2)] for r in range(2)]
    assert windowed == [[1, 5], [3, 7]]


def test_pointcloud_run_rejects_unknown_data_sources():
    config = {"arch": {"type": "MonoRecModel", "args": {}}, "data_set": {"type": "OxfordRobotCarDataset", "args": {}}}
    with pytest.raises(ValueError) as err:
        pointcloud.run(config)
    assert all(name in str(err.value) for name in ("KittiOdometryDataset", "TUMMonoVODataset", "TUMMonoVOMultiDataset"))
    assert pointcloud._dataset_class("TUMMonoVODataset") is tum_mono_vo.TUMMonoVODataset
    assert pointcloud._dataset_class("TUMMonoVOMultiDataset") is tum_mono_vo.TUMMonoVOMultiDataset
    assert pointcloud._dataset_class("KittiOdometryDataset") is kitti.KittiOdometryDataset


def test_lut_entry_is_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert re.search(r"\bmr_preprocess_image_u8_lut_f32\s*\(", header) and "mr_preprocess_image_u8_lut_f32" in tum_mono_vo.input_pipeline._lib.ABI
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    assert any("`mr_preprocess_image_u8_lut_f32`" in line and "tum_mono_vo_dataset.py" in line for line in table)
    assert hip_lib.mr_abi_version() >= 21
    # bad arguments are reported, not launched: no table, channels other than 1 or 3
    box = (tum_mono_vo.input_pipeline.ctypes.c_int32 * 4)(0, 0, 8, 8)
    args = lambda channels, lut: (16, 8, 8, channels, 8 * channels, box, 4, 4, 16, 16, 3, 16, 16, 3, 8, lut, 16, None)
    assert hip_lib.mr_preprocess_image_u8_lut_f32(*args(1, None)) == -1
    assert hip_lib.mr_preprocess_image_u8_lut_f32(*args(2, 16)) == -1
    assert hip_lib.mr_preprocess_image_u8_lut_f32(*args(4, 16)) == -1
