"""The ray-cast of the block-sparse TSDF volume without a device: the C entry's declaration and argument checks, the runner's
`sparse_render` key, the numpy restatement (tests/tsdf_sparse_render_ref.py) held against the dense one, and the preconditions of the
cases of test_gpu_tsdf_sparse_render.py - the views hit the scene, and many of their hits lie in cells that straddle a block face."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tsdf_fusion_ref as ref
import tsdf_render_ref as rref
import tsdf_sparse_ref as sref
import tsdf_sparse_render_ref as srref
from monorec_amd import _lib, tsdf_fusion as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mr_tsdf_sparse_render_f32"
H, W = 24, 40
RANGE = dict(t_min=0.5, t_max=6.0, step=0.06)
SPECS = {"first": sref.FIRST, "second": sref.SECOND}


# ------------------------------------------------------------------------------------------ the C entry
def test_the_entry_is_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    assert re.search(r"\bint %s\s*\(" % ENTRY, header) and ENTRY in _lib.ABI and hasattr(hip_lib, ENTRY)
    assert any(f"`{ENTRY}`" in line for line in table)
    assert len(_lib.ABI[ENTRY][1]) == 19
    params = re.search(r"\bint %s\s*\(([^)]*)\)" % ENTRY, header).group(1)
    assert len(params.split(",")) == 19
    sources = __import__("monorec_amd.build", fromlist=["SOURCES"]).SOURCES
    assert ("tsdf_sparse_render.hip", ["-ffp-contract=off"]) in sources


def test_the_entry_rejects_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    table, tsdf, weight, colour, depth, normal, image = (base + 4096 * i for i in range(7))
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def one_view(fx=30.0, fy=30.0, d=depth, n=normal, c=image):
        view = _lib.TsdfRayView()
        view.m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        view.fx, view.fy, view.cx, view.cy = fx, fy, 3.5, 1.5
        view.depth, view.normal, view.colour = d, n, c
        return view

    def render(tb=table, nbx=2, nby=2, nbz=1, t=tsdf, w=weight, c=colour, used=2, o=origin, voxel=0.1, min_weight=0.0, views="one", count=None,
               h=4, width=8, t_min=0.5, t_max=2.0, step=0.1, **view):
        if views == "one":
            views = (_lib.TsdfRayView * 1)(one_view(**view))
        elif views == "nine":
            views = (_lib.TsdfRayView * 9)(*[one_view(**view) for _ in range(9)])
        n = count if count is not None else (len(views) if views is not None else 1)
        return hip_lib.mr_tsdf_sparse_render_f32(tb, nbx, nby, nbz, t, w, c, used, o, voxel, min_weight, views, n, h, width, t_min, t_max, step, None)

    # the table and the pool, as test_tsdf_sparse.py has them for the other sparse entries
    shared = [dict(tb=None), dict(t=None), dict(w=None), dict(nbx=0), dict(nby=-1), dict(nbz=0), dict(tb=table + 2), dict(t=tsdf + 4), dict(t=tsdf + 8),
              dict(w=weight + 4), dict(c=colour + 4), dict(c=colour + 8), dict(nbx=1 << 16, nby=1 << 15, nbz=1), dict(nbx=1 << 11, nby=1 << 10, nbz=1 << 10),
              dict(nbx=2 ** 31 - 1, nby=2 ** 31 - 1, nbz=2 ** 31 - 1)]
    # more than 2^27 blocks along one axis, whatever the product
    long = [dict(nbx=(1 << 27) + 1, nby=1, nbz=1), dict(nbx=1, nby=(1 << 27) + 1, nbz=1), dict(nbx=1, nby=1, nbz=(1 << 27) + 1), dict(nbx=1 << 30, nby=1, nbz=1)]
    slots = [dict(used=-1), dict(used=5), dict(used=1 << 31, nbx=1 << 10, nby=1 << 10, nbz=1 << 10), dict(used=1 << 40)]
    volume = [dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan), dict(min_weight=nan)]
    # every view, size and range case of mr_tsdf_render_f32 (tests/test_tsdf_render.py)
    views = [dict(views=None), dict(count=0), dict(count=-1), dict(views="nine"), dict(d=None), dict(d=depth + 2), dict(n=normal + 1),
             dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=nan), dict(h=0), dict(width=0), dict(h=-3),
             dict(step=0.0), dict(step=-0.1), dict(step=nan), dict(t_min=-0.5), dict(t_min=nan), dict(t_max=0.25), dict(t_max=nan),
             dict(t_max=inf), dict(t_min=inf, t_max=inf), dict(t_min=0.0, t_max=2.0, step=1e-6), dict(t_min=0.0, t_max=1048576.5, step=1.0),
             dict(t_min=1000.0, t_max=1000.0, step=1e-12)]
    for kw in shared + long + slots + volume + views:
        assert render(**kw) == -1, kw


# ------------------------------------------------------------------------------------------ the runner's key
def test_runner_config_with_sparse_render():
    base = {"arch": {"type": "MonoRecModel", "args": {}}, "data_set": {"type": "KittiOdometryDataset", "args": {}}, "max_d": 30}
    keys = set(tf.fusion_settings(base))
    assert set(tf.fusion_settings(dict(base, sparse_volume=True, sparse_render=True))) == keys and "sparse_render" not in keys
    assert tf.sparse_render_setting(base) is False and tf.sparse_render_setting(dict(base, sparse_volume=True)) is False
    assert tf.sparse_render_setting(dict(base, sparse_volume=True, sparse_render=True)) is True
    for bad in ("yes", 1, 0, None, [True]):
        with pytest.raises(ValueError, match="sparse_render"):
            tf.run(dict(base, sparse_volume=True, sparse_render=bad))
    for config in (dict(base, sparse_render=True), dict(base, sparse_volume=False, sparse_render=True)):
        with pytest.raises(ValueError, match="sparse_render needs sparse_volume"):
            tf.run(config)
    # 200 m x 200 m x 40 m at 0.1 m: renders and score no longer ask for the dense copy, the next check in line speaks
    road = dict(base, sparse_volume=True, sparse_render=True, bounds=[[0, 0, 0], [200, 200, 40]], voxel_size=0.1, arch={"type": "Other"})
    for key, value in (("render_dir", "renders"), ("fused_metrics", ["abs_rel_sparse_onlyvalid_metric"])):
        with pytest.raises(ValueError, match="MonoRecModel"):
            tf.run(dict(road, **{key: value}))
        with pytest.raises(ValueError, match=rf"{key} with sparse_volume.*2008 x 2008 x 408 voxels.*tsdf_max_bytes"):
            tf.run(dict(road, sparse_render=False, **{key: value}))          # as before without the key
    with pytest.raises(ValueError, match=r"^monorec_amd.tsdf_fusion: mesh_file_name with sparse_volume.*2008 x 2008 x 408 voxels.*tsdf_max_bytes"):
        tf.run(dict(road, mesh_file_name="mesh.ply", render_dir="renders", fused_metrics=["abs_rel_sparse_onlyvalid_metric"]))


# ------------------------------------------------------------------------------------------ the restatement and the GPU cases' preconditions
@functools.lru_cache(maxsize=None)
def _restated(name):
    return sref.fuse(SPECS[name], ref.make_frames(sref.K), 3)


@functools.lru_cache(maxsize=None)
def _view(name, pose):
    vol = _restated(name)
    blocks = tuple(d // 8 for d in vol["dims"])
    return srref.render_virtual(vol, (0, 0, 0), vol["origin"], blocks, ref.make_frames(sref.K)[pose][0], sref.K, H, W, *RANGE.values())


@pytest.mark.parametrize("name", ["first", "second"])
def test_render_virtual_at_offset_zero_equals_the_dense_restatement(name):
    vol = _restated(name)
    for pose in (0, 5, 9, 10):
        want = rref.render(vol, ref.make_frames(sref.K)[pose][0], sref.K, H, W, *RANGE.values())
        got = _view(name, pose)
        for key in ("depth", "normal"):
            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), (pose, key)
        assert np.array_equal(got["colour"], want["colour"]) and np.array_equal(got["hit"], want["hit"])
        assert np.array_equal(got["base"][..., 0] >= 0, want["hit"])


@pytest.mark.parametrize("name,blocks,allocated,straddling", [("first", 144, 30, 70), ("second", 384, 47, 130)])
def test_the_views_of_the_gpu_cases_hit_the_scene_across_block_faces(name, blocks, allocated, straddling):
    vol = _restated(name)
    assert vol["allocated"].size == blocks and int(vol["allocated"].sum()) == allocated
    for pose in (0, 5, 9):
        view = _view(name, pose)
        assert view["hit"].mean() > 0.4, (pose, view["hit"].mean())
        base = view["base"][view["hit"]]
        on_face = int(((base % 8) == 7).any(axis=1).sum())                    # the 8 corners lie in more than one block
        assert on_face >= 50 and on_face >= straddling, (pose, on_face)
        # every hit cell has its base in an allocated block (min_weight 0: corner i itself is seen)
        assert vol["allocated"][base[:, 2] >> 3, base[:, 1] >> 3, base[:, 0] >> 3].all()
    assert not _view(name, 10)["hit"].any()                                   # the pose that looks away


def test_the_clip_cases_through_the_table():
    """The volumes test_gpu_tsdf_sparse_render.py makes of rref.CLIP_CASES - whole blocks, storage only where a block holds a seen
    negative voxel: `render_virtual` equals the dense restatement of what the table stands for, the face cases keep their hits
    without the all-positive blocks, and hit cells straddle block faces."""
    dropped = 0
    for case in rref.CLIP_CASES:
        vol, pose, k, march = rref.case_inputs(case)
        stands_for = sref.without_positive_blocks(vol)
        assert all(d % 8 == 0 and d - 8 < n <= d for d, n in zip(stands_for["dims"], vol["dims"])) and stands_for["allocated"].any()
        dropped += int((~stands_for["allocated"]).sum())
        want = rref.render(stands_for, pose, k, rref.CLIP_H, rref.CLIP_W, *march)
        got = srref.render_virtual(stands_for, (0, 0, 0), stands_for["origin"], tuple(d // 8 for d in stands_for["dims"]), pose, k,
                                   rref.CLIP_H, rref.CLIP_W, *march)
        for key in ("depth", "normal"):
            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), (case["id"], key)
        assert np.array_equal(got["colour"], want["colour"]) and np.array_equal(got["hit"], want["hit"]), case["id"]
        if case["group"] in (1, 2):
            whole = rref.render(vol, pose, k, rref.CLIP_H, rref.CLIP_W, *march)
            base = got["base"][got["hit"]]
            assert np.array_equal(want["depth"].view(np.uint32), whole["depth"].view(np.uint32)), case["id"]
            assert int(((base % 8) == 7).any(axis=1).sum()) >= 100, case["id"]
            assert (~stands_for["allocated"]).any() == (case["group"] == 2), case["id"]
    assert dropped > 200
