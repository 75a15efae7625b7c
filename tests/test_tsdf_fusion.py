"""TSDF fusion without a device: the C entries' declarations and argument checks, the host geometry (bounds, volume size), the
directory reader, the runner's config validation, and self-checks of the numpy restatement the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
from monorec_amd import _lib, tsdf_export as tx, tsdf_fusion as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mr_tsdf_volume_reset_f32", "mr_tsdf_integrate_f32", "mr_tsdf_extract_f32")


# ------------------------------------------------------------------------------------------ C entries
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib.ABI and hasattr(hip_lib, name)
        assert any(f"`{name}`" in line for line in table), name
    assert [len(_lib.ABI[n][1]) for n in ENTRIES] == [7, 15, 13]
    assert int(re.search(r"#define MR_TSDF_MAX_FRAMES (\d+)", header).group(1)) == _lib.MR_TSDF_MAX_FRAMES == tf.MAX_FRAMES == 8
    tile = tuple(int(re.search(r"#define MR_TSDF_TILE_%s (\d+)" % a, header).group(1)) for a in "XYZ")
    assert tile == _lib.MR_TSDF_TILE == tf.TILE and tile[0] * tile[1] * tile[2] == 256 * 4
    # the mirror of mr_tsdf_view: 16 floats and two pointers
    assert ctypes.sizeof(_lib.TsdfView) == 16 * 4 + 2 * ctypes.sizeof(ctypes.c_void_p) and _lib.TsdfView.depth_cm.offset == 64


def test_entries_reject_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    tsdf, weight, colour, depth, image, records, cursor = (base + 4096 * i for i in range(7))
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    inf, nan = float("inf"), float("nan")

    def views(n, depth_p=depth, image_p=image):
        array = (_lib.TsdfView * max(n, 1))()
        for v in array:
            v.m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
            v.fx = v.fy = 30.0
            v.cx, v.cy = 19.5, 11.5
            v.depth_cm, v.colour = depth_p, image_p
        return array

    def reset(t=tsdf, w=weight, c=colour, nx=8, ny=4, nz=2):
        return hip_lib.mr_tsdf_volume_reset_f32(t, w, c, nx, ny, nz, None)

    def integrate(t=tsdf, w=weight, c=colour, nx=8, ny=4, nz=2, o=origin, voxel=0.1, trunc=0.5, limit=inf, frames="one", n=1, hh=24, ww=40):
        return hip_lib.mr_tsdf_integrate_f32(t, w, c, nx, ny, nz, o, voxel, trunc, limit, views(n) if frames == "one" else frames, n, hh, ww, None)

    def extract(t=tsdf, w=weight, c=colour, nx=8, ny=4, nz=2, o=origin, voxel=0.1, min_weight=0.0, r=records, cap=16, cur=cursor):
        return hip_lib.mr_tsdf_extract_f32(t, w, c, nx, ny, nz, o, voxel, min_weight, r, cap, cur, None)

    huge = [dict(nx=1 << 20, ny=1 << 20, nz=1), dict(nx=1 << 14, ny=1 << 13, nz=1 << 13), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)]
    volume = [dict(t=None), dict(w=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(t=tsdf + 2), dict(w=weight + 1), dict(c=colour + 2)] + huge
    for kw in volume:
        assert reset(**kw) == -1, ("reset", kw)
        assert integrate(**kw) == -1, ("integrate", kw)
        assert extract(**kw) == -1, ("extract", kw)
    for kw in [dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan),
               dict(limit=nan), dict(frames=None), dict(n=0), dict(n=9), dict(n=-1), dict(hh=0), dict(ww=-2),
               dict(frames=views(1, depth_p=None)), dict(frames=views(1, image_p=None)), dict(frames=views(3, image_p=None), n=3)]:
        assert integrate(**kw) == -1, ("integrate", kw)
    for kw in [dict(o=None), dict(voxel=0.0), dict(voxel=nan), dict(min_weight=nan), dict(cur=None), dict(cap=-1), dict(cur=cursor + 4),
               dict(r=records + 2)]:
        assert extract(**kw) == -1, ("extract", kw)
    assert b"argument" in hip_lib.mr_error_string(-1).lower()


# ------------------------------------------------------------------------------------------ host geometry
def test_bounds_from_frusta_against_hand_computed_boxes():
    k = torch.tensor([[10.0, 0, 4.5], [0, 10.0, 2.5], [0, 0, 1]])            # 6 x 10 image: u in [-.5, 9.5] -> x/z in [-.5, .5]; v: y/z in [-.3, .3]
    eye = torch.eye(4)
    # one camera at the origin looking along z, 2 m deep: corners (+-1, +-.6, 2) and the centre; voxel .25 rounds y outwards to +-.75
    assert tf.bounds_from_frusta([eye], k, 6, 10, 2.0, voxel_size=0.25) == ((-1.0, -0.75, 0.0), (1.0, 0.75, 2.0))
    # a second camera 3.1 m along x looking along -x (z_cam = -x_world, x_cam = z_world): x from 1.1 to 3.1, z in +-1
    turned = torch.tensor([[0.0, 0, -1, 3.1], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
    lo, hi = tf.bounds_from_frusta([eye, turned], k, 6, 10, 2.0, voxel_size=0.25)
    assert lo == (-1.0, -0.75, -1.0) and hi == (3.25, 0.75, 2.0)
    # a 4 x 4 intrinsics matrix and numpy poses are accepted; the box is whole voxels
    k4 = torch.eye(4)
    k4[:3, :3] = k
    lo, hi = tf.bounds_from_frusta([turned.numpy()], k4, 6, 10, 2.0, voxel_size=0.3)
    assert np.allclose(lo, (0.9, -0.6, -1.2)) and np.allclose(hi, (3.3, 0.6, 1.2))
    assert tf.dims_of_bounds((lo, hi), 0.3) == (9, 5, 9)
    # one intrinsics matrix per pose: the second camera with half the focal length sees twice as wide (z in +-2, y in +-1.2)
    wide = k.clone()
    wide[0, 0] = wide[1, 1] = 5.0
    lo, hi = tf.bounds_from_frusta([eye, turned], [k, wide], 6, 10, 2.0, voxel_size=0.25)
    assert lo == (-1.0, -1.25, -2.0) and hi == (3.25, 1.25, 2.0)
    assert tf.bounds_from_frusta([eye, turned], torch.stack([k, wide]), 6, 10, 2.0, voxel_size=0.25) == (lo, hi)
    with pytest.raises(ValueError, match="2 poses but 3 intrinsics"):
        tf.bounds_from_frusta([eye, turned], [k, k, k], 6, 10, 2.0)
    with pytest.raises(ValueError):
        tf.bounds_from_frusta([eye], k, 6, 10, float("inf"))
    with pytest.raises(ValueError):
        tf.bounds_from_frusta([], k, 6, 10, 2.0)


def test_a_volume_above_max_bytes_names_the_voxel_size_that_fits():
    bounds = ((0.0, 0.0, 0.0), (10.0, 10.0, 10.0))
    with pytest.raises(ValueError, match=r"101 x 101 x 101 voxels of 0\.1 m need .* GiB.*a voxel size of (\S+) m would fit") as e:
        tf.TSDFVolume(bounds, 0.1, max_bytes=1 << 20)                          # raised before any device is touched
    fits = float(re.search(r"a voxel size of (\S+) m would fit", str(e.value)).group(1))
    assert tf.volume_bytes(tf.dims_of_bounds(bounds, fits)) <= 1 << 20 < tf.volume_bytes(tf.dims_of_bounds(bounds, fits * 0.9))
    assert tf.volume_bytes((101, 101, 101), colour=False) == 101 ** 3 * 8
    for kw in (dict(voxel_size=0.0), dict(voxel_size=0.1, trunc=0.0), dict(bounds=None), dict(origin=(0, 0, 0), dims=(4, 4, 4))):
        with pytest.raises(ValueError):
            tf.TSDFVolume(**{**dict(bounds=bounds, voxel_size=0.1, max_bytes=1 << 20), **kw})
    with pytest.raises(RuntimeError, match="CPU fallback"):
        tf.TSDFVolume(origin=(0, 0, 0), dims=(4, 4, 4), voxel_size=0.1, device="cpu")


# ------------------------------------------------------------------------------------------ the directory reader
def test_directory_reader_orders_numerically_and_inverts_the_pose_again(tmp_path):
    rng = np.random.default_rng(3)
    poses = ref.arc_poses(4)
    written = {}
    for number in (10, 2, 1000000, 0):                                        # 1000000 has seven digits: a lexical sort would misplace it
        depth = rng.integers(0, 3000, size=(6, 10)).astype(np.int16)
        colour = rng.integers(0, 256, size=(6, 10, 3)).astype(np.uint8)
        pose = torch.from_numpy(poses[len(written)])
        tx.write_frame_files(tmp_path, number, depth, colour, torch.inverse(pose).numpy())
        written[number] = (depth, pose)
    (tmp_path / "frames.json").write_text("{}")                              # other files are ignored
    frames = tf.list_export_directory(tmp_path)
    assert [n for n, _ in frames] == [0, 2, 10, 1000000]
    for number, base in frames:
        depth, colour, cam_to_world = tf.read_export_frame(base)
        assert depth.dtype == np.int16 and np.array_equal(depth, written[number][0])
        assert colour.dtype == np.uint8 and colour.shape == (6, 10, 3)
        text = torch.from_numpy(np.loadtxt(base + ".pose.txt").astype(np.float32))
        assert cam_to_world.dtype == torch.float32 and torch.equal(cam_to_world, torch.inverse(text))
        assert torch.allclose(cam_to_world, written[number][1], atol=1e-5)
    (tmp_path / "nothing").mkdir()
    with pytest.raises(ValueError, match="no frame"):
        tf.fuse_directory(tmp_path / "nothing")


# ------------------------------------------------------------------------------------------ the runner's config
def test_runner_config_validation():
    base = {"arch": {"type": "MonoRecModel", "args": {}}, "data_set": {"type": "KittiOdometryDataset", "args": {}}, "max_d": 30}
    got = tf.fusion_settings(base)
    assert got["voxel_size"] == 0.1 and got["trunc"] == 0.5 and got["fuse_batch"] == 4 and got["file_name"] == "tsdf.ply"
    assert got["bounds"] is None and got["save_volume"] is None and got["max_bytes"] == 8 << 30
    got = tf.fusion_settings(dict(base, voxel_size=0.05, trunc_voxels=3, fuse_batch=8, tsdf_max_bytes=123, file_name="a.ply", save_volume="v.npz",
                                  bounds=[[0, 0, 0], [1, 2, 3]]))
    assert abs(got["trunc"] - 0.15) < 1e-12 and got["fuse_batch"] == 8 and got["max_bytes"] == 123 and got["save_volume"] == "v.npz"
    for bad in (dict(voxel_size=0), dict(trunc_voxels=-1), dict(fuse_batch=0), dict(fuse_batch=9), dict(bounds=[[0, 0, 0], [1, -2, 3]])):
        with pytest.raises(ValueError):
            tf.run(dict(base, **bad))                                          # before a model or a dataset is built
    no_size = {k: v for k, v in base.items() if k != "max_d"}
    with pytest.raises(ValueError, match="bounds.*max_d"):
        tf.run(no_size)
    with pytest.raises(ValueError, match="MonoRecModel"):
        tf.run(dict(base, arch={"type": "Other"}))
    with pytest.raises(ValueError, match="no device data source"):
        tf.run(dict(base, data_set={"type": "Other", "args": {}}))


# ------------------------------------------------------------------------------------------ the restatement itself
@pytest.fixture(scope="module")
def fused():
    """The small volume after the ten frames that see the scene, with the frames."""
    frames = ref.make_frames(ref.INTRINSICS_60)
    vol = ref.new_volume(**ref.SMALL)
    for pose, depth, colour in frames[:10]:
        ref.integrate(vol, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, colour)
    return vol, frames


def test_roundf_rounds_halves_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, -0.49999997, 8388609.0, 2.4999998, -0.0, 1e30, -np.inf], np.float32)
    want = np.array([1.0, 2.0, 3.0, -1.0, -3.0, 0.0, -0.0, 8388609.0, 2.0, -0.0, 1e30, -np.inf], np.float32)
    got = ref.roundf(x)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


def test_a_frame_looking_away_changes_nothing(fused):
    vol, frames = fused
    pose, depth, colour = frames[10]
    after = ref.copy_volume(vol)
    depth = np.full_like(depth, 300)                                        # even with depth everywhere
    stats = ref.integrate(after, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, colour)
    assert stats["behind"].all() and not stats["updated"].any()
    for key in ("tsdf", "weight", "colour"):
        assert np.array_equal(after[key], vol[key])


def test_the_same_frame_twice_keeps_tsdf_and_doubles_the_weight():
    frames = ref.make_frames(ref.INTRINSICS_60)
    pose, depth, colour = frames[4]
    once = ref.new_volume(**ref.SMALL)
    stats = ref.integrate(once, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, colour)
    twice = ref.copy_volume(once)
    ref.integrate(twice, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, colour)
    seen = stats["updated"]
    assert 0.3 < seen.mean() < 0.9
    assert np.array_equal(twice["tsdf"], once["tsdf"])                       # (t * 1 + t) / 2 is exact
    assert np.array_equal(twice["weight"], np.where(seen, 2, 0)) and np.array_equal(once["weight"], np.where(seen, 1, 0))
    assert np.array_equal(twice["colour"], once["colour"])
    assert np.all(once["tsdf"][~seen] == 1) and np.all(once["colour"][~seen] == 0) and np.all(once["colour"][..., 3] == 0)


def test_every_extracted_point_lies_within_a_voxel_of_the_surface(fused):
    vol, _ = fused
    for min_weight in (0, 2):
        records = ref.extract(vol, min_weight)
        assert records.dtype == np.float32 and records.shape[1] == 6 and len(records) > 500
        assert ref.surface_distance(records[:, :3]).max() <= float(vol["voxel"])
        assert records[:, 3:].min() >= 0 and records[:, 3:].max() <= 255 and np.array_equal(records[:, 3:], np.floor(records[:, 3:]))
    assert len(ref.extract(vol, 2)) < len(ref.extract(vol, 0)) and len(ref.extract(ref.new_volume(**ref.SMALL))) == 0
    assert len(ref.extract(vol, 10)) == 0
    shuffled = ref.extract(vol)[np.random.default_rng(0).permutation(len(ref.extract(vol)))]
    assert np.array_equal(ref.sort_records(shuffled), ref.sort_records(ref.extract(vol)))
