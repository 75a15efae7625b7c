"""The TSDF ray-cast without a device: the two C entries' declarations and argument checks, the runner's new config keys, and the numpy
restatement (tests/tsdf_render_ref.py) held against the analytic scene of tests/tsdf_fusion_ref.py - it hits what the scene shows, at
the scene's depth, and the skipping rule spares work without changing a depth."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tsdf_fusion_ref as ref
import tsdf_render_ref as rref
from monorec_amd import _lib, tsdf_fusion as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mr_tsdf_skip_grid_u8", "mr_tsdf_render_f32")
H, W = 24, 40
RANGE = dict(t_min=0.5, t_max=6.0, step=0.06)


# ------------------------------------------------------------------------------------------ C entries
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib.ABI and hasattr(hip_lib, name)
        assert any(f"`{name}`" in line for line in table), name
    assert [len(_lib.ABI[n][1]) for n in ENTRIES] == [8, 18]
    assert int(re.search(r"#define MR_TSDF_BRICK (\d+)", header).group(1)) == _lib.MR_TSDF_BRICK == tf.BRICK == rref.BRICK
    assert _lib.MR_TSDF_BRICK in (4, 8)


def test_ray_view_mirrors_the_header():
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    body = re.search(r"typedef struct mr_tsdf_ray_view \{(.*?)\} mr_tsdf_ray_view;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|uint8_t)\s*(\*?)\s*([^;]+);", body, re.M)
    size, names = 0, []
    for kind, pointer, declared in fields:
        for name in declared.split(","):
            name = name.strip()
            count = int(re.search(r"\[(\d+)\]", name).group(1)) if "[" in name else 1
            each = 8 if pointer else 4
            size = (size + each - 1) // each * each + each * count
            names.append(name.split("[")[0])
    assert names == [f[0] for f in _lib.TsdfRayView._fields_] == ["m", "fx", "fy", "cx", "cy", "depth", "normal", "colour"]
    assert ctypes.sizeof(_lib.TsdfRayView) == size == 88
    assert _lib.TsdfRayView.depth.offset == 64 and _lib.TsdfRayView.colour.offset == 80


def test_entries_reject_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    tsdf, weight, colour, bricks, depth, normal, image = (base + 4096 * i for i in range(7))
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def grid(t=tsdf, w=weight, nx=8, ny=4, nz=2, min_weight=0.0, b=bricks):
        return hip_lib.mr_tsdf_skip_grid_u8(t, w, nx, ny, nz, min_weight, b, None)

    def one_view(fx=30.0, fy=30.0, d=depth, n=normal, c=image):
        view = _lib.TsdfRayView()
        view.m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        view.fx, view.fy, view.cx, view.cy = fx, fy, 3.5, 1.5
        view.depth, view.normal, view.colour = d, n, c
        return view

    def render(t=tsdf, w=weight, c=colour, nx=8, ny=4, nz=2, o=origin, voxel=0.1, min_weight=0.0, b=bricks, views="one", count=None,
               h=4, width=8, t_min=0.5, t_max=2.0, step=0.1, **view):
        if views == "one":
            views = (_lib.TsdfRayView * 1)(one_view(**view))
        elif views == "nine":
            views = (_lib.TsdfRayView * 9)(*[one_view(**view) for _ in range(9)])
        n = count if count is not None else (len(views) if views is not None else 1)
        return hip_lib.mr_tsdf_render_f32(t, w, c, nx, ny, nz, o, voxel, min_weight, b, views, n, h, width, t_min, t_max, step, None)

    huge = [dict(nx=1 << 20, ny=1 << 20, nz=1), dict(nx=1 << 14, ny=1 << 13, nz=1 << 13), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)]
    volume = [dict(t=None), dict(w=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(t=tsdf + 2), dict(w=weight + 1), dict(min_weight=nan)] + huge
    for kw in volume:
        assert grid(**kw) == -1, ("grid", kw)
        assert render(**kw) == -1, ("render", kw)
    assert grid(b=None) == -1
    cases = [dict(c=colour + 2), dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan),
             dict(views=None), dict(count=0), dict(count=-1), dict(views="nine"), dict(d=None), dict(d=depth + 2), dict(n=normal + 1),
             dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=nan), dict(h=0), dict(width=0), dict(h=-3),
             dict(step=0.0), dict(step=-0.1), dict(step=nan), dict(t_min=-0.5), dict(t_min=nan), dict(t_max=0.25), dict(t_max=nan),
             dict(t_max=inf), dict(t_min=inf, t_max=inf), dict(t_min=0.0, t_max=2.0, step=1e-6), dict(t_min=0.0, t_max=1048576.5, step=1.0),
             dict(t_min=1000.0, t_max=1000.0, step=1e-12)]
    for kw in cases:
        assert render(**kw) == -1, ("render", kw)
    assert b"argument" in hip_lib.mr_error_string(-1).lower()


# ------------------------------------------------------------------------------------------ the runner's keys
def test_fusion_settings_accept_the_new_keys_and_reject_other_metrics():
    base = {"max_d": 30}
    plain = tf.fusion_settings(base)
    assert plain["fused_metrics"] == [] and plain["render_dir"] is None
    assert {k: v for k, v in plain.items() if k not in ("fused_metrics", "render_dir")} == dict(
        voxel_size=0.1, trunc=0.5, bounds=None, max_bytes=8 << 30, fuse_batch=4, file_name="tsdf.ply", mesh_file_name=None, save_volume=None)
    names = ["abs_rel_sparse_onlyvalid_metric", "a1_sparse_onlyvalid_metric", "rmse_log_sparse_onlyvalid_metric"]
    got = tf.fusion_settings(dict(base, fused_metrics=names, render_dir="views"))
    assert got["fused_metrics"] == names and got["render_dir"] == "views"
    assert sorted(tf.FUSED_METRICS) == sorted(f"{b}_sparse_onlyvalid_metric" for b in ("a1", "a2", "a3", "rmse", "rmse_log", "abs_rel", "sq_rel"))
    for bad in (["abs_rel_sparse_metric"], ["a1_sparse_onlydynamic_metric"], ["abs_rel_metric"], ["nothing"], "abs_rel_sparse_onlyvalid_metric", [3]):
        with pytest.raises(ValueError, match="onlyvalid"):
            tf.fusion_settings(dict(base, fused_metrics=bad))
    with pytest.raises(ValueError, match="onlyvalid"):                      # before a model or a dataset is built: neither is in this config
        tf.Fusion(dict(base, fused_metrics=["a1_sparse_metric"]))


# ------------------------------------------------------------------------------------------ the restatement on the analytic scene
@functools.lru_cache(maxsize=None)
def _fused(name, focal):
    k = ref.INTRINSICS_30 if focal == 30 else ref.INTRINSICS_60
    frames = ref.make_frames(k)
    vol = ref.new_volume(**(ref.SMALL if name == "small" else ref.WIDE))
    for pose, depth, colour in frames[:10]:
        ref.integrate(vol, ref.world_to_camera(pose), k, depth, colour)
    return vol, frames, k


@functools.lru_cache(maxsize=None)
def _view(name, focal, pose):
    vol, frames, k = _fused(name, focal)
    return rref.render(vol, frames[pose][0], k, H, W, bricks=rref.brick_flags(vol, 0.0), **RANGE)


def test_brick_flags_have_the_halo_on_the_plus_side():
    vol = ref.new_volume((17, 9, 8), (0, 0, 0), 0.1, 0.3, colour=False)
    vol["weight"][...] = 1
    assert not rref.brick_flags(vol, brick=8).any() and rref.brick_flags(vol, brick=8).shape == (1, 2, 3)
    assert rref.brick_flags(vol, brick=4).shape == (2, 3, 5) and rref.brick_flags(vol).shape == rref.brick_flags(vol, brick=rref.BRICK).shape
    vol["tsdf"][0, 8, 16] = -0.5                                           # the first voxel of brick (2, 1, 0) closes bricks 1 and 0 along x, y
    assert rref.brick_flags(vol, brick=8)[0].tolist() == [[0, 1, 1], [0, 1, 1]]
    assert rref.brick_flags(vol, brick=4)[0].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1]] and not rref.brick_flags(vol, brick=4)[1].any()
    assert not rref.brick_flags(vol, min_weight=1.0, brick=8).any()
    vol["tsdf"][0, 8, 16], vol["tsdf"][7, 7, 15] = 1.0, -0.0
    assert not rref.brick_flags(vol, brick=8).any()                        # -0 is not negative
    vol["tsdf"][7, 7, 15] = -1e-3
    assert rref.brick_flags(vol, brick=8)[0].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert rref.brick_flags(vol, brick=4).sum() == 1 and rref.brick_flags(vol, brick=4)[1, 1, 3] == 1


@pytest.mark.parametrize("name,focal,least", [("small", 30, 0.20), ("wide", 30, 0.45), ("small", 60, 0.65)])
def test_the_restatement_sees_the_scene(name, focal, least):
    vol, frames, k = _fused(name, focal)
    for pose in (0, 5, 9):
        got = _view(name, focal, pose)
        share = float(got["hit"].mean())
        scene = rref.scene_depth(frames[pose][0], k, H, W)
        both = got["hit"] & (scene > 0)
        error = np.abs(got["depth"].astype(np.float64) - scene)[both]
        print(f"{name} f={focal} pose {pose}: hit share {share:.3f}, |depth - scene| median {np.median(error) * 1000:.2f} mm max {error.max():.3f} m, "
              f"cells {got['evaluations']} -> {got['brick_evaluations']}")
        assert share >= least and both.sum() > 0.9 * got["hit"].sum()
        assert np.median(error) < 0.01
        assert np.array_equal(got["hit"], got["depth"] > 0)
        # the skipping rule: the same depth bit for bit, nothing skipped that could have mattered, and work spared
        assert np.array_equal(got["depth"], got["brick_depth"]) and got["skipped_negative"] == 0
        assert got["brick_evaluations"] < got["evaluations"]
        # unit normals that face the camera, colours from the fused images
        n = got["normal"][got["hit"]]
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1).max() < 1e-6 and not got["normal"][~got["hit"]].any()
        assert np.median(n @ frames[pose][0][:3, 2]) < -0.5
        assert got["colour"][got["hit"]].max() > 100 and not got["colour"][~got["hit"]].any()
    away = _view(name, focal, 10)
    assert not away["hit"].any() and not away["depth"].any() and away["evaluations"] == 0


def test_a_ray_that_leaves_through_a_back_face_ends():
    vol = rref.slab_volume()
    bricks = rref.brick_flags(vol)
    front = rref.render(vol, rref.slab_pose(0.9), ref.INTRINSICS_60, 23, 37, 0.0, 3.0, 0.06, bricks=bricks)
    inside = rref.render(vol, rref.slab_pose(1.4), ref.INTRINSICS_60, 23, 37, 0.0, 3.0, 0.06, bricks=bricks)
    assert front["hit"].mean() > 0.5 and np.abs(front["depth"][front["hit"]] - (1.21 - 0.9)).max() < 0.06      # the first slab's front face
    assert not inside["hit"].any()                                         # not the second slab
    for got in (front, inside):
        assert np.array_equal(got["depth"], got["brick_depth"]) and got["skipped_negative"] == 0


def test_sample_count_follows_the_rounded_t():
    assert rref.sample_count(0.5, 6.0, 0.06) == 92 and rref.sample_count(0.0, 0.0, 1.0) == 1 and rref.sample_count(1.0, 2.0, 0.25) == 5
