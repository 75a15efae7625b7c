"""GPU: the TSDF ray-cast - `mr_tsdf_skip_grid_u8` / `mr_tsdf_render_f32` behind `TSDFVolume.skip_grid` / `render` / `render_result`
against the numpy restatement of tests/tsdf_render_ref.py, on the fused volumes of tests/tsdf_fusion_ref.py's scene and on an analytic
pair of slabs: depth, normal, colour and brick bytes are compared bit for bit.  Then the skip-grid cache and the runner's `score()`."""
import functools
import os

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
import tsdf_render_ref as rref
from monorec_amd import metrics, synth, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INTRINSICS = {30: ref.INTRINSICS_30, 60: ref.INTRINSICS_60}
VOLUMES = {"small": ref.SMALL, "wide": ref.WIDE}
VOXEL = 0.06
RANGE = dict(t_min=0.5, t_max=6.0, step=VOXEL)


def _k3(k):
    return torch.tensor([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], dtype=torch.float32)


# ------------------------------------------------------------------------------------------ references, computed once, never modified
@functools.lru_cache(maxsize=None)
def _frames(focal):
    return ref.make_frames(INTRINSICS[focal])


@functools.lru_cache(maxsize=None)
def _fused(name, focal, count=10, colour=True):
    """The volume after the first `count` frames (the ten arc poses that see the scene; the eleventh looks away)."""
    vol = ref.new_volume(colour=colour, **VOLUMES[name])
    for pose, depth, image in _frames(focal)[:count]:
        ref.integrate(vol, ref.world_to_camera(pose), INTRINSICS[focal], depth, image if colour else None)
    return vol


@functools.lru_cache(maxsize=None)
def _slabs(colour=True):
    return rref.slab_volume(colour=colour)


def _volume(kind, focal=60, colour=True):
    return _slabs(colour) if kind == "slabs" else _fused(kind, focal, 10, colour)


POSES = {"inside": rref.inside_pose, "behind": rref.behind_pose, "slab_front": lambda: rref.slab_pose(0.9), "slab_inside": lambda: rref.slab_pose(1.4)}


def _pose(focal, which):
    return POSES[which]() if isinstance(which, str) else _frames(focal)[which][0]


@functools.lru_cache(maxsize=None)
def _want(kind, focal, which, height, width, t_min, t_max, step, min_weight=0.0, colour=True):
    vol = _volume(kind, focal, colour)
    return rref.render(vol, _pose(focal, which), INTRINSICS[focal], height, width, t_min, t_max, step, min_weight)


def _load(vol):
    """A device volume holding the arrays of a restatement's volume dict."""
    volume = tf.TSDFVolume(origin=vol["origin"], dims=vol["dims"], voxel_size=float(vol["voxel"]), trunc=float(vol["trunc"]),
                           colour=vol["colour"] is not None, device=DEV)
    volume.tsdf.copy_(torch.from_numpy(vol["tsdf"].reshape(-1)))
    volume.weight.copy_(torch.from_numpy(vol["weight"].reshape(-1)))
    if vol["colour"] is not None:
        volume.colour.copy_(torch.from_numpy(vol["colour"].reshape(-1, 4)))
    volume.drop_skip_grids()
    return volume


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: {int((_bits(got) != _bits(want)).sum())} of {want.size} elements differ"


def _check(views, index, want, what):
    assert views["depth"].is_cuda and views["depth"].dtype == torch.float32
    _same(views["depth"][index], want["depth"], f"{what} depth")
    if views["normal"] is not None:
        _same(views["normal"][index], want["normal"], f"{what} normal")
    if views["colour"] is not None:
        _same(views["colour"][index], want["colour"], f"{what} colour")


# ------------------------------------------------------------------------------------------ 1. the brick bytes
@pytest.mark.parametrize("kind,focal", [("small", 60), ("small", 30), ("wide", 30), ("slabs", 60)])
def test_skip_grid_equals_the_restatement(hip_lib, kind, focal):
    vol = _volume(kind, focal)
    volume = _load(vol)
    for min_weight in (0, 2):
        want = rref.brick_flags(vol, min_weight)
        got = volume.skip_grid(min_weight)
        assert got.is_cuda and got.dtype == torch.uint8 and volume.skip_grid(min_weight) is got          # cached per min_weight
        _same(got, want, f"{kind} bricks min_weight {min_weight}")
        assert 0 < want.sum() < want.size or kind == "slabs"
    assert volume.skip_grid(0) is not volume.skip_grid(2)


def test_skip_grid_sets_the_bricks_a_voxel_closes(hip_lib):
    """One negative voxel on a brick corner flags the eight bricks whose inclusive ranges hold it; unseen or -0 flags nothing."""
    vol = ref.new_volume((37, 19, 17), (0, 0, 0), 0.1, 0.3, colour=False)
    vol["weight"][...] = 1
    vol["tsdf"][16, 8, 32], vol["tsdf"][3, 3, 3], vol["weight"][3, 3, 3], vol["tsdf"][1, 1, 20] = -0.5, -0.5, 0.0, -0.0
    want = rref.brick_flags(vol)
    assert want.shape == tuple(-(-n // tf.BRICK) for n in (17, 19, 37)) and want.sum() == 8
    _same(_load(vol).skip_grid(), want, "corner voxel")


# ------------------------------------------------------------------------------------------ 2. views of the fused scene
@pytest.mark.parametrize("size", [(24, 40), (23, 37)], ids=["24x40", "23x37"])
@pytest.mark.parametrize("kind,focal", [("small", 30), ("small", 60), ("wide", 30)])
def test_views_of_the_scene_equal_the_restatement(hip_lib, kind, focal, size):
    """Poses 0, 5, 9 and the one that looks away, four views in one launch; 23 x 37 leaves partial pixel tiles."""
    volume = _load(_fused(kind, focal))
    which = [0, 5, 9, 10]
    poses = torch.from_numpy(np.stack([_pose(focal, p) for p in which]))
    views = volume.render(poses, _k3(INTRINSICS[focal]), *size, **RANGE)
    plain = volume.render(poses, _k3(INTRINSICS[focal]), *size, skip=False, **RANGE)
    for j, p in enumerate(which):
        want = _want(kind, focal, p, *size, *RANGE.values())
        _check(views, j, want, f"{kind} pose {p}")
        _check(plain, j, want, f"{kind} pose {p} without bricks")
        assert (want["hit"].mean() > 0.2) if p != 10 else (not want["hit"].any())
    for key in ("depth", "normal", "colour"):
        assert torch.equal(views[key], plain[key])


@pytest.mark.parametrize("which,t_min,t_max", [("inside", 0.0, 3.0), ("behind", 0.0, 3.0), ("inside", 0.13, 0.9)])
def test_cameras_inside_and_behind(hip_lib, which, t_min, t_max):
    """A camera inside the volume (rays that start between seen voxels), and one behind the wall looking back: its rays enter the
    surface from inside, leave through the front and end there - zero depth wherever the restatement says so."""
    volume = _load(_fused("small", 60))
    want = _want("small", 60, which, 23, 37, t_min, t_max, VOXEL / 2)
    for skip in (True, False):
        views = volume.render(torch.from_numpy(_pose(60, which)), _k3(INTRINSICS[60]), 23, 37, t_min=t_min, t_max=t_max, step=VOXEL / 2, skip=skip)
        _check(views, 0, want, f"{which} skip={skip}")
    assert (want["hit"].mean() > 0.3) if which == "inside" else (not want["hit"].any() and want["evaluations"] > 1000)


@pytest.mark.parametrize("which", ["slab_front", "slab_inside"])
def test_a_ray_that_leaves_through_a_back_face_ends(hip_lib, which):
    """Two slabs behind each other: from in front the first is hit; from inside the first the ray ends at its back face and the
    second slab is not reported."""
    volume = _load(_slabs())
    want = _want("slabs", 60, which, 23, 37, 0.0, 3.0, VOXEL)
    for skip in (True, False):
        views = volume.render(torch.from_numpy(_pose(60, which)), _k3(INTRINSICS[60]), 23, 37, t_min=0.0, t_max=3.0, step=VOXEL, skip=skip)
        _check(views, 0, want, f"{which} skip={skip}")
    assert (want["hit"].mean() > 0.5) if which == "slab_front" else (not want["hit"].any())


@pytest.mark.parametrize("min_weight", [0, 2])
@pytest.mark.parametrize("voxels", [0.5, 1.0, 2.5])
def test_steps_and_min_weights(hip_lib, voxels, min_weight):
    volume = _load(_fused("small", 60))
    step = float(np.float32(VOXEL * voxels))
    want = _want("small", 60, 5, 23, 37, 0.5, 6.0, step, float(min_weight))
    for skip in (True, False):
        views = volume.render(torch.from_numpy(_pose(60, 5)), _k3(INTRINSICS[60]), 23, 37, t_min=0.5, t_max=6.0, step=step, min_weight=min_weight,
                              skip=skip)
        _check(views, 0, want, f"step {voxels} min_weight {min_weight} skip={skip}")
    assert want["hit"].mean() > 0.3
    if min_weight:
        assert want["hit"].sum() < _want("small", 60, 5, 23, 37, 0.5, 6.0, step, 0.0)["hit"].sum()


# ------------------------------------------------------------------------------------------ 3. optional outputs, batches
def test_a_volume_without_colour_and_views_without_normal_or_colour(hip_lib):
    want = _want("small", 60, 0, 24, 40, *RANGE.values(), 0.0, False)
    volume = _load(_fused("small", 60, 10, False))
    pose, k = torch.from_numpy(_pose(60, 0)), _k3(INTRINSICS[60])
    views = volume.render(pose, k, 24, 40, **RANGE)
    _check(views, 0, want, "no colour volume")
    assert not bool(views["colour"].any()) and bool(views["normal"].any())
    coloured = _load(_fused("small", 60))
    full = _want("small", 60, 0, 24, 40, *RANGE.values())
    _same(full["depth"], want["depth"], "colour does not move the depth")
    for normals, colour in ((False, True), (True, False), (False, False)):
        views = coloured.render(pose, k, 24, 40, normals=normals, colour=colour, **RANGE)
        assert (views["normal"] is None) == (not normals) and (views["colour"] is None) == (not colour)
        _check(views, 0, full, f"normals={normals} colour={colour}")
    with pytest.raises(ValueError, match="intrinsics"):
        coloured.render(torch.eye(4).repeat(3, 1, 1), torch.eye(3).repeat(2, 1, 1), 24, 40)


def test_eight_views_in_one_launch_equal_eight_launches(hip_lib):
    volume = _load(_fused("wide", 30))
    which = [0, 2, 4, 5, 7, 9, 10, 3]
    poses = torch.from_numpy(np.stack([_pose(30, p) for p in which]))
    ks = torch.stack([_k3(INTRINSICS[30 if j % 2 == 0 else 60]) for j in range(8)])          # one calibration per view
    together = volume.render(poses, ks, 23, 37, **RANGE)
    for j in range(8):
        alone = volume.render(poses[j], ks[j], 23, 37, **RANGE)
        for key in ("depth", "normal", "colour"):
            assert torch.equal(together[key][j], alone[key][0]), (key, j)
    for j in (0, 3, 5):
        _check(together, j, _want("wide", 30, which[j], 23, 37, *RANGE.values()) if j % 2 == 0 else
               rref.render(_fused("wide", 30), _pose(30, which[j]), INTRINSICS[60], 23, 37, *RANGE.values()), f"view {j}")
    many = volume.render(poses.repeat(2, 1, 1)[:11], ks.repeat(2, 1, 1)[:11], 23, 37, **RANGE)           # two launches: 8 + 3
    assert torch.equal(many["depth"][:8], together["depth"]) and torch.equal(many["depth"][8:], together["depth"][:3])


def test_render_result_is_the_inverse_depth(hip_lib):
    volume = _load(_fused("small", 60))
    poses = torch.from_numpy(np.stack([_pose(60, 0), _pose(60, 10)]))
    depth = volume.render(poses, _k3(INTRINSICS[60]), 24, 40, **RANGE)["depth"]
    result = volume.render_result(poses, _k3(INTRINSICS[60]), 24, 40, **RANGE)
    assert tuple(result.shape) == (2, 1, 24, 40) and result.is_cuda and result.dtype == torch.float32
    want = _want("small", 60, 0, 24, 40, *RANGE.values())["depth"]
    with np.errstate(divide="ignore"):
        _same(result[0, 0], np.where(want > 0, np.float32(1.0) / want, np.float32(0.0)).astype(np.float32), "inverse depth")
    assert torch.equal(result[:, 0] != 0, depth > 0) and not bool(result[1].any())
    with pytest.raises(RuntimeError, match="CPU fallback"):
        tf.TSDFVolume(origin=(0, 0, 0), dims=(4, 4, 4), voxel_size=0.1, device="cpu")


# ------------------------------------------------------------------------------------------ 4. the skip-grid cache
def test_integrate_and_reset_drop_the_skip_grid(hip_lib):
    """Nine frames on the device, a render (which builds the grid), the tenth frame, a render again: it equals the restatement of
    the volume after ten.  After reset() nothing is hit."""
    frames, k = _frames(60), _k3(INTRINSICS[60])
    spec = VOLUMES["small"]
    volume = tf.TSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV)

    def integrate(lo, hi):
        volume.integrate(torch.from_numpy(np.stack([f[1] for f in frames[lo:hi]])).to(DEV), torch.from_numpy(np.stack([f[2] for f in frames[lo:hi]])).to(DEV),
                         torch.from_numpy(np.stack([f[0] for f in frames[lo:hi]])), k)

    pose = torch.from_numpy(_pose(60, 9))
    empty = volume.render(pose, k, 24, 40, **RANGE)                        # builds the grid of the empty volume: a stale one skips everything
    grid = volume.skip_grid(0)
    assert not bool(empty["depth"].any()) and not bool(grid.any())
    integrate(0, 3)
    assert volume.skip_grid(0) is not grid
    before = volume.render(pose, k, 24, 40, **RANGE)
    grid = volume.skip_grid(0)
    _same(grid, rref.brick_flags(_fused("small", 60, 3)), "bricks after three frames")
    _check(before, 0, rref.render(_fused("small", 60, 3), _pose(60, 9), INTRINSICS[60], 24, 40, *RANGE.values()), "three frames")
    assert bool(before["depth"].any())
    integrate(3, 10)
    assert volume.skip_grid(0) is not grid
    after = volume.render(pose, k, 24, 40, **RANGE)
    _same(volume.skip_grid(0), rref.brick_flags(_fused("small", 60)), "bricks after ten frames")
    _check(after, 0, _want("small", 60, 9, 24, 40, *RANGE.values()), "ten frames")
    assert not torch.equal(before["depth"], after["depth"])
    volume.reset()
    cleared = volume.render(pose, k, 24, 40, **RANGE)
    assert not bool(cleared["depth"].any()) and not bool(cleared["normal"].any()) and not bool(cleared["colour"].any())
    assert not bool(volume.skip_grid(0).any())


# ------------------------------------------------------------------------------------------ 5. the runner
def test_score_equals_the_metric_functions_by_hand(hip_lib, tmp_path):
    """The synthetic KITTI tree and seeded model of test_gpu_tsdf_fusion.py's runner test: `score()` against the metric functions
    applied to `render_result` of all exported keyframes as one batch, and the files of `render_dir`."""
    from PIL import Image
    from monorec_amd import MonoRecModel
    tree = synth.make_kitti_tree(tmp_path / "kitti", sequences=(("03", 120, 400),), frames=20)
    model = MonoRecModel(cv_depth_steps=16, hip_in_flight=4)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    names = ["abs_rel_sparse_onlyvalid_metric", "rmse_sparse_onlyvalid_metric", "a1_sparse_onlyvalid_metric"]
    config = {"name": "TSDF render", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": 10, "min_d": 3, "max_d": 30, "use_mask": False,
              "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": 3, "output_dir": str(tmp_path / "out"), "render_dir": str(tmp_path / "views"),
              "fused_metrics": names, "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": 16}},
              "data_set": {"type": "KittiOdometryDataset", "args": args}}
    with pytest.raises(ValueError, match="onlyvalid"):
        tf.Fusion(dict(config, fused_metrics=["abs_rel_sparse_metric"]), model=model)
    fusion = tf.Fusion(config, model=model).fuse()
    scored = fusion.score()
    items = fusion.stream.export_items()
    assert len(items) == 10 == scored["samples"] and list(scored["metrics"]) == names                    # two render launches: 8 + 2
    samples = [fusion.stream.dataset[i] for i in items]
    result = fusion.volume.render_result(torch.stack([d["keyframe_pose"] for d, _ in samples]), torch.stack([d["keyframe_intrinsics"] for d, _ in samples]),
                                         64, 96, t_min=0.0, t_max=30.0)
    target = torch.stack([t for _, t in samples]).to(DEV)
    data = dict(result=result, target=target)
    covered = int(((target > 0) & (result != 0)).sum()) / int((target > 0).sum())
    print(f"score: {scored}, by hand coverage {covered:.4f}, {int((result != 0).sum())} rendered pixels")
    assert bool((result != 0).any()) and 0 < covered <= 1 and scored["coverage"] == covered
    for name in names:
        want = float(getattr(metrics, name)(data))
        assert scored["metrics"][name] == want and np.isfinite(want), name
    # the files: one pair per exported keyframe, the export's crop, the depth the render gave
    assert fusion.write() > 0
    files = sorted(os.listdir(tmp_path / "views"))
    assert files == sorted(f"frame-{n:06d}.fused.{kind}" for n in range(10) for kind in ("color.jpg", "depth.png"))
    geometry = [fusion.stream.dataset.keyframe_geometry(i) for i in items]
    views = fusion.volume.render(torch.stack([g[0] for g in geometry]), torch.stack([fusion.shifted(g[1]) for g in geometry]), 56, 84, t_min=0.0,
                                 t_max=30.0, normals=False)
    for n in (0, 9):
        with Image.open(tmp_path / "views" / f"frame-{n:06d}.fused.depth.png") as img:
            png = np.array(img).astype(np.int64)
        want = (views["depth"][n] * 100.0).clamp(0, 65535).to(torch.int32).cpu().numpy()
        assert png.shape == (56, 84) and np.array_equal(png, want) and png.any()
        with Image.open(tmp_path / "views" / f"frame-{n:06d}.fused.color.jpg") as img:
            assert img.size == (84, 56) and img.mode == "RGB"


# ------------------------------------------------------------------------------------------ 6. where the clip to the box decides
H, W = rref.CLIP_H, rref.CLIP_W


@pytest.mark.parametrize("case", rref.CLIP_CASES, ids=[c["id"] for c in rref.CLIP_CASES])
def test_clip_cases_equal_the_restatement(hip_lib, case):
    """rref.CLIP_CASES: samples ON the faces of the box, rays parallel to them, origins on the box, thin volumes, far cameras, a t_max
    that decides, poses that are no rotation (tests/test_tsdf_render.py proves on the CPU that an exact clip has nothing to spare in
    them).  The restatement marches every sample, so equality bit for bit says the kernel's clip dropped none that mattered."""
    vol, pose, k, (t_min, t_max, step) = rref.case_inputs(case)
    want = rref.render(vol, pose, k, H, W, t_min, t_max, step)
    volume = _load(vol)
    for skip in (True, False):
        views = volume.render(torch.from_numpy(pose), _k3(k), H, W, t_min=t_min, t_max=t_max, step=step, skip=skip)
        _check(views, 0, want, f"{case['id']} skip={skip}")


def test_a_pose_that_is_not_finite_in_a_batch(hip_lib):
    """Three views in one launch, the middle pose with a NaN in its rotation and an inf in its translation: every sample of every ray of
    it is outside (a NaN compares false), so it is all zero, as the restatement says; its neighbours are what they are alone."""
    case = next(c for c in rref.CLIP_CASES if c["id"] == "1-enter-zlo")
    vol, pose, k, (t_min, t_max, step) = rref.case_inputs(case)
    other = next(c for c in rref.CLIP_CASES if c["id"] == "3-oblique-zlo")["pose"]
    broken = pose.copy()
    broken[0, 1], broken[1, 3] = np.nan, np.inf
    volume = _load(vol)
    for skip in (True, False):
        march = dict(t_min=t_min, t_max=t_max, step=step, skip=skip)
        views = volume.render(torch.from_numpy(np.stack([pose, broken, other])), _k3(k), H, W, **march)
        for j, p in enumerate((pose, broken, other)):
            want = rref.render(vol, p, k, H, W, t_min, t_max, step)
            assert want["hit"].any() == (j != 1)
            _check(views, j, want, f"view {j} skip={skip}")
            if j != 1:
                alone = volume.render(torch.from_numpy(p), _k3(k), H, W, **march)
                for key in ("depth", "normal", "colour"):
                    assert torch.equal(views[key][j], alone[key][0]), (key, j)
        assert not bool(views["depth"][1].any()) and not bool(views["normal"][1].any()) and not bool(views["colour"][1].any())


@pytest.mark.parametrize("case", [c for c in rref.CLIP_CASES if c["group"] == "noise"], ids=lambda c: c["id"])
def test_bricks_of_a_volume_that_is_no_scene(hip_lib, case):
    """One voxel in 200 negative, independent of its neighbours: the brick bytes equal the restatement's, and the march that skips and
    the one that does not both equal the full march, for min_weight 0 and 1."""
    vol, pose, k, (t_min, t_max, step) = rref.case_inputs(case)
    volume = _load(vol)
    for min_weight in (0, 1):
        _same(volume.skip_grid(min_weight), rref.brick_flags(vol, min_weight), f"bricks min_weight {min_weight}")
        want = rref.render(vol, pose, k, H, W, t_min, t_max, step, min_weight)
        assert want["hit"].any()
        for skip in (True, False):
            views = volume.render(torch.from_numpy(pose), _k3(k), H, W, t_min=t_min, t_max=t_max, step=step, min_weight=min_weight, skip=skip)
            _check(views, 0, want, f"{case['id']} min_weight {min_weight} skip={skip}")
