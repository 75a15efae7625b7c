"""GPU: the ray-cast of the block-sparse TSDF volume - `mr_tsdf_sparse_render_f32` behind `SparseTSDFVolume.render` / `render_result` -
against the numpy restatements (tests/tsdf_render_ref.py on the volume the table stands for, tests/tsdf_sparse_render_ref.py through the
table) and against the dense render of the gathered volume: depth, normal and colour bit for bit, no tolerance anywhere.  Then the
runner's `sparse_render` key.  tests/test_tsdf_sparse_render.py asserts that these views hit the scene across block faces."""
import functools
import os

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
import tsdf_render_ref as rref
import tsdf_sparse_ref as sref
import tsdf_sparse_render_ref as srref
from monorec_amd import synth, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECS = {"first": sref.FIRST, "second": sref.SECOND}
KMAT = torch.tensor([[sref.K[0], 0.0, sref.K[2]], [0.0, sref.K[1], sref.K[3]], [0.0, 0.0, 1.0]])
RANGE = dict(t_min=0.5, t_max=6.0, step=0.06)
OFFSET = (2048, 2048, 232)
BIG = (4096, 4096, 512)


# ------------------------------------------------------------------------------------------ references, computed once, never modified
@functools.lru_cache(maxsize=None)
def _frames():
    return ref.make_frames(sref.K)                      # eleven 24 x 40 frames on the arc; the last one looks away


def _pose(which):
    return _frames()[which][0]


def _poses(which):
    return torch.from_numpy(np.stack([_pose(p) for p in which]))


@functools.lru_cache(maxsize=None)
def _restated(name, colour=True):
    return sref.fuse(SPECS[name], _frames(), 3, colour=colour)


@functools.lru_cache(maxsize=None)
def _want(name, which, height, width, t_min=0.5, t_max=6.0, step=0.06, min_weight=0.0, colour=True):
    return rref.render(_restated(name, colour), _pose(which), sref.K, height, width, t_min, t_max, step, min_weight)


@functools.lru_cache(maxsize=None)
def _fused(name, colour=True):
    """The device volume after the eleven frames in launches of 3.  Shared by the tests, which only read it."""
    spec = SPECS[name]
    volume = tf.SparseTSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], colour=colour,
                                 device=DEV)
    depth = torch.from_numpy(np.stack([f[1] for f in _frames()])).to(DEV)
    image = torch.from_numpy(np.stack([f[2] for f in _frames()])).to(DEV)
    poses = torch.from_numpy(np.stack([f[0] for f in _frames()]))
    for lo in range(0, len(_frames()), 3):
        volume.integrate(depth[lo:lo + 3], image[lo:lo + 3] if colour else None, poses[lo:lo + 3], KMAT)
    assert volume.allocated_blocks() == int(_restated(name, colour)["allocated"].sum()) == dict(first=30, second=47)[name]
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


def _equal(a, b):
    return all((a[key] is None and b[key] is None) or torch.equal(a[key], b[key]) for key in ("depth", "normal", "colour"))


# ------------------------------------------------------------------------------------------ 1. the fused scene
@pytest.mark.parametrize("size", [(24, 40), (23, 37)], ids=["24x40", "23x37"])
@pytest.mark.parametrize("name", ["first", "second"])
def test_views_of_the_fused_scene_equal_the_restatement_and_the_dense_render(hip_lib, name, size):
    """Poses 0, 5, 9 and the one that looks away, four views in one launch; 23 x 37 leaves partial pixel tiles."""
    volume, which = _fused(name), [0, 5, 9, 10]
    views = volume.render(_poses(which), KMAT, *size, **RANGE)
    steps = volume.render(_poses(which), KMAT, *size, skip=False, **RANGE)
    dense = volume.to_dense(volume.bounds)
    gathered = [dense.render(_poses(which), KMAT, *size, skip=skip, **RANGE) for skip in (True, False)]
    for j, p in enumerate(which):
        want = _want(name, p, *size)
        assert (want["hit"].mean() > 0.4) if p != 10 else (not want["hit"].any())
        _check(views, j, want, f"{name} pose {p}")
        _check(steps, j, want, f"{name} pose {p} without the jump")
    for other in [steps] + gathered:
        assert _equal(views, other)


# ------------------------------------------------------------------------------------------ 2. missing neighbours
def _corner_scene():
    """The corner scene of tests/test_gpu_tsdf_sparse.py: a dense restatement volume of 3 x 2 x 2 blocks, four balls, each with a pole
    between voxel 7 and 8 (or 15 and 16) of one axis, so that sign changes sit on faces between blocks; tsdf = clip(distance / 3 voxels,
    -1, 1), weights 3, about one in ten 1, a few 0, random colours."""
    dims = (24, 16, 16)
    vol = ref.new_volume(dims, (-0.3, 0.2, 1.0), 0.06, 0.18)
    rng = np.random.default_rng(5)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims[::-1]), indexing="ij")
    balls = [(3.2, 4.0, 4.0, 4.5), (12.0, 3.3, 4.0, 4.4), (4.0, 12.0, 3.4, 4.3), (12.0, 11.0, 11.5, 3.7)]
    dist = np.min([np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r for cx, cy, cz, r in balls], axis=0)
    vol["tsdf"] = np.clip(dist / 3.0, -1.0, 1.0).astype(np.float32)
    draw = rng.random(dist.shape)
    vol["weight"] = np.where(draw < 0.03, 0.0, np.where(draw < 0.13, 1.0, 3.0)).astype(np.float32)
    vol["colour"][..., :3] = rng.integers(0, 256, size=dist.shape + (3,), dtype=np.uint8)
    return vol


def test_cells_across_block_faces_with_a_neighbour_missing(hip_lib, tmp_path):
    """Three of the twelve blocks have no storage: a cell that reaches into one reads 1 / 0 / 0 there.  With min_weight = -1 those
    corners count as seen, so a kernel that skipped every sample in a missing block would lose hits."""
    full = _corner_scene()
    allocated = np.ones((2, 2, 3), bool)
    allocated[1, 1, 2] = allocated[0, 0, 2] = allocated[1, 0, 0] = False      # (bz, by, bx)
    want_volume = sref.sparsify(full, allocated)
    coords, tsdf, weight, rgb = sref.blocks_of(want_volume)
    order = np.random.default_rng(1).permutation(len(coords))                 # through `load`, in an order that is not the table's
    np.savez(tmp_path / "corner.npz", blocks=coords[order], tsdf=tsdf[order], weight=weight[order], colour=rgb[order],
             origin=np.asarray(want_volume["origin"], np.float32), dims=np.asarray(want_volume["dims"], np.int64), voxel_size=want_volume["voxel"],
             trunc=want_volume["trunc"], frames=np.int64(5))
    volume = tf.SparseTSDFVolume.load(tmp_path / "corner.npz", device=DEV)
    assert volume.allocated_blocks() == 9 and volume.blocks == (3, 2, 2)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.42, 0.68, 0.1)
    k, size, march = (60.0, 60.0, 19.5, 11.5), (24, 40), dict(t_min=0.5, t_max=2.5, step=0.03)
    kmat = torch.tensor([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])
    for min_weight in (0, 2, -1):
        want = rref.render(want_volume, pose, k, *size, *march.values(), min_weight)
        whole = rref.render(full, pose, k, *size, *march.values(), min_weight)
        differ = int((_bits(want["depth"]) != _bits(whole["depth"])).sum())
        assert want["hit"].sum() > 50 and differ > 5, (min_weight, int(want["hit"].sum()), differ)
        through = srref.render_virtual(want_volume, (0, 0, 0), volume.origin, volume.blocks, pose, k, *size, *march.values(), min_weight)
        for key in ("depth", "normal", "colour"):
            _same(through[key], want[key], f"render_virtual {key} min_weight {min_weight}")
        for skip in (True, False):
            views = volume.render(torch.from_numpy(pose), kmat, *size, min_weight=min_weight, skip=skip, **march)
            _check(views, 0, want, f"min_weight {min_weight} skip {skip}")


# ------------------------------------------------------------------------------------------ 3. large block coordinates
def _big_volume(offset):
    """4096 x 4096 x 512 voxels with the FIRST restatement's blocks at voxel `offset`, which is where FIRST's origin lies."""
    spec, sub = sref.FIRST, _restated("first")
    origin = tuple(o - i * spec["voxel_size"] for o, i in zip(spec["origin"], offset))
    volume = tf.SparseTSDFVolume(origin=origin, dims=BIG, voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV, capacity_blocks=256)
    coords, tsdf, weight, colour = sref.blocks_of(sub)
    volume.set_blocks(coords + np.asarray(offset) // 8, tsdf, weight, colour)
    assert volume.blocks == (512, 512, 64) and volume.allocated_blocks() == 30
    return volume, sub


def test_large_block_coordinates(hip_lib):
    with pytest.raises(ValueError, match=r"4096 x 4096 x 512 voxels of 0\.06 m need 96\.00 GiB"):
        tf.TSDFVolume(origin=(0, 0, 0), dims=BIG, voxel_size=0.06, device=DEV)
    volume, sub = _big_volume(OFFSET)
    which = [0, 5, 9]
    views = volume.render(_poses(which), KMAT, 24, 40, **RANGE)
    steps = volume.render(_poses(which), KMAT, 24, 40, skip=False, **RANGE)
    for j, p in enumerate(which):
        want = srref.render_virtual(sub, OFFSET, volume.origin, volume.blocks, _pose(p), sref.K, 24, 40, *RANGE.values())
        assert want["hit"].mean() > 0.3 and (want["base"][want["hit"]] >= np.asarray(OFFSET)).all()
        _check(views, j, want, f"pose {p} at {OFFSET}")
    assert _equal(views, steps)


# ------------------------------------------------------------------------------------------ 4. long empty marches
def test_long_marches_through_blocks_without_storage(hip_lib):
    """t_max = 200 m in steps of 0.06 m: 3 326 samples per ray, nearly all of them in blocks without storage of a 245 m wide table."""
    volume, sub = _big_volume((0, 0, 0))
    march = dict(t_min=0.5, t_max=200.0, step=0.06)
    assert rref.sample_count(*march.values()) == 3326
    which = [0, 10]
    views = volume.render(_poses(which), KMAT, 24, 40, **march)
    steps = volume.render(_poses(which), KMAT, 24, 40, skip=False, **march)
    near = _fused("first").render(_poses(which), KMAT, 24, 40, **RANGE)["depth"].cpu().numpy()
    for j, p in enumerate(which):
        want = srref.render_virtual(sub, (0, 0, 0), volume.origin, volume.blocks, _pose(p), sref.K, 24, 40, *march.values())
        _check(views, j, want, f"pose {p} to 200 m")
        hit = near[j] > 0                                                     # a hit never moves when t_max grows
        assert hit.mean() > 0.4 if p == 0 else not hit.any()
        assert np.array_equal(_bits(want["depth"][hit]), _bits(near[j][hit]))
        assert not ((want["depth"] > 0) & (want["depth"] <= 5.9) & ~hit).any()
    assert _equal(views, steps)


# ------------------------------------------------------------------------------------------ 5. odds and ends
def test_eight_views_in_one_launch_equal_eight_launches(hip_lib):
    volume, which = _fused("second"), list(range(8))
    together = volume.render(_poses(which), KMAT, 23, 37, **RANGE)
    assert tuple(together["depth"].shape) == (8, 23, 37) and (together["depth"] > 0).float().mean() > 0.4
    for j, p in enumerate(which):
        alone = volume.render(torch.from_numpy(_pose(p)), KMAT, 23, 37, **RANGE)
        for key in ("depth", "normal", "colour"):
            assert torch.equal(together[key][j], alone[key][0]), (key, p)
    nine = volume.render(_poses(which + [9]), KMAT, 23, 37, **RANGE)          # two launches: 8 and 1
    assert torch.equal(nine["depth"][:8], together["depth"]) and torch.equal(nine["colour"][:8], together["colour"])
    _check(nine, 8, _want("second", 9, 23, 37), "the ninth view")


def test_a_volume_without_colour_and_views_without_normal_or_colour(hip_lib):
    plain, volume = _fused("first", False), _fused("first")
    assert plain.colour is None
    views = plain.render(_poses([0, 5]), KMAT, 24, 40, **RANGE)
    for j, p in enumerate((0, 5)):
        _check(views, j, _want("first", p, 24, 40, colour=False), f"plain pose {p}")
    assert not views["colour"].any() and (views["depth"] > 0).float().mean() > 0.4
    lean = volume.render(_poses([0, 5]), KMAT, 24, 40, normals=False, colour=False, **RANGE)
    assert lean["normal"] is None and lean["colour"] is None
    for j, p in enumerate((0, 5)):
        _check(lean, j, _want("first", p, 24, 40), f"lean pose {p}")
    only_colour = volume.render(_poses([5]), KMAT, 24, 40, normals=False, **RANGE)
    assert only_colour["normal"] is None
    _check(only_colour, 0, _want("first", 5, 24, 40), "colour without normal")


def test_a_freshly_reset_volume_renders_nothing(hip_lib):
    spec = sref.FIRST
    volume = tf.SparseTSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV)
    assert volume.allocated_blocks() == 0
    for min_weight in (0, -1):
        for skip in (True, False):
            views = volume.render(_poses([0, 5]), KMAT, 23, 37, min_weight=min_weight, skip=skip, **RANGE)
            assert not views["depth"].any() and not views["normal"].any() and not views["colour"].any()
    assert not volume.render_result(_poses([0]), KMAT, 24, 40, **RANGE).any()


def test_render_result_is_the_inverse_depth(hip_lib):
    volume = _fused("first")
    depth = volume.render(_poses([0, 9]), KMAT, 24, 40, **RANGE)["depth"]
    result = volume.render_result(_poses([0, 9]), KMAT, 24, 40, **RANGE)
    assert tuple(result.shape) == (2, 1, 24, 40) and (depth > 0).float().mean() > 0.4
    assert torch.equal(result[:, 0], torch.where(depth > 0, 1.0 / depth, torch.zeros_like(depth)))
    assert torch.equal(result, volume.to_dense(volume.bounds).render_result(_poses([0, 9]), KMAT, 24, 40, **RANGE))


def test_more_than_2_to_the_20_samples_raise_before_the_call(hip_lib):
    volume = _fused("first")
    for march in (dict(t_min=0.0, t_max=2.0, step=1e-6), dict(t_min=0.0, t_max=1048576.5, step=1.0)):
        with pytest.raises(ValueError, match=r"t_max.*step"):
            volume.render(_poses([0]), KMAT, 24, 40, **march)
    views = volume.render(_poses([0]), KMAT, 24, 40, t_min=0.0, t_max=1048575.0, step=1.0)      # exactly 2^20 samples
    assert tuple(views["depth"].shape) == (1, 24, 40)


# ------------------------------------------------------------------------------------------ 6. the runner
STEPS, KEYFRAMES = 16, 6
METRICS = ["abs_rel_sparse_onlyvalid_metric", "a1_sparse_onlyvalid_metric"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return synth.make_kitti_tree(tmp_path_factory.mktemp("kitti"), sequences=(("03", 120, 400),), frames=20)


@pytest.fixture(scope="module")
def model(hip_lib):
    from monorec_amd import MonoRecModel
    m = MonoRecModel(cv_depth_steps=STEPS, hip_in_flight=4)
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=0))
    return m.to(DEV).eval()


def _config(tree, out_dir, **more):
    """The config of test_runner_with_sparse_volume_equals_fusing_by_hand (tests/test_gpu_tsdf_sparse.py) with renders and a score."""
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    return dict({"name": "sparse TSDF fusion", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": KEYFRAMES, "min_d": 3, "max_d": 30,
                 "use_mask": False, "output_dir": str(out_dir), "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": 1, "sparse_volume": True,
                 "file_name": "surface.ply", "render_dir": os.path.join(str(out_dir), "renders"), "fused_metrics": METRICS,
                 "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": STEPS}},
                 "data_set": {"type": "KittiOdometryDataset", "args": args}}, **more)


def _files(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in sorted(os.listdir(directory))}


def test_runner_renders_and_scores_the_sparse_volume_itself(tree, model, tmp_path):
    config_a = _config(tree, tmp_path / "a", sparse_render=True)
    config_b = _config(tree, tmp_path / "b", sparse_render=False)
    a = tf.Fusion(config_a, model=model).fuse()
    b = tf.Fusion(config_b, model=model).fuse()
    count = a.write()
    assert count == b.write() > 100
    score_a, score_b = a.score(), b.score()
    assert a._dense is None and b._dense is not None                          # run A never gathered the volume
    assert score_a == score_b and score_a["samples"] == KEYFRAMES and 0 < score_a["coverage"] <= 1
    assert set(score_a["metrics"]) == set(METRICS) and all(np.isfinite(v) for v in score_a["metrics"].values())
    files_a, files_b = _files(config_a["render_dir"]), _files(config_b["render_dir"])
    assert len(files_a) == 2 * KEYFRAMES and sorted(files_a) == sorted(files_b)
    assert sum(name.endswith(".fused.depth.png") for name in files_a) == sum(name.endswith(".fused.color.jpg") for name in files_a) == KEYFRAMES
    for name in files_a:
        assert files_a[name] == files_b[name], name
    # a budget of the table and the allocated slots alone: no room for the dense copy
    blocks_total, allocated = a.volume.table.numel(), a.volume.allocated_blocks()
    budget = 4 * blocks_total + allocated * (512 * 12 + 4)
    assert 0 < allocated < blocks_total and budget < tf.volume_bytes(a.volume.dims)
    with pytest.raises(ValueError, match="with sparse_volume need the volume gathered"):
        tf.Fusion(dict(config_b, tsdf_max_bytes=budget), model=model).fuse().score()
    tight = tf.Fusion(dict(config_a, tsdf_max_bytes=budget, output_dir=str(tmp_path / "c"), render_dir=str(tmp_path / "c" / "renders")),
                      model=model).fuse()
    assert tight.volume.capacity == allocated and tight.write() == count
    assert tight.score() == score_a and _files(str(tmp_path / "c" / "renders")) == files_a


# ------------------------------------------------------------------------------------------ 7. where the clip to the box decides
@pytest.mark.parametrize("case", rref.CLIP_CASES, ids=[c["id"] for c in rref.CLIP_CASES])
def test_clip_cases_equal_the_restatement_and_the_dense_render(hip_lib, case):
    """rref.CLIP_CASES (tests/test_gpu_tsdf_render.py has them on the dense volume) through the table: the case's volume rounded up to
    whole blocks, with a pool that holds the blocks with a seen negative voxel and no other - the rest read as unseen.  The restatement
    is of that volume.  The faces of the box are faces of blocks, and hits lie in cells that straddle blocks
    (tests/test_tsdf_sparse_render.py counts them)."""
    vol, pose, k, (t_min, t_max, step) = rref.case_inputs(case)
    stands_for = sref.without_positive_blocks(vol)
    coords, tsdf, weight, rgb = sref.blocks_of(stands_for)
    volume = tf.SparseTSDFVolume(origin=stands_for["origin"], dims=stands_for["dims"], voxel_size=float(stands_for["voxel"]),
                                 trunc=float(stands_for["trunc"]), device=DEV, capacity_blocks=len(coords))
    volume.set_blocks(coords, tsdf, weight, rgb)
    assert volume.dims == stands_for["dims"] and volume.allocated_blocks() == volume.capacity == len(coords) > 0
    want = rref.render(stands_for, pose, k, rref.CLIP_H, rref.CLIP_W, t_min, t_max, step)
    kmat = torch.tensor([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])
    march = dict(t_min=t_min, t_max=t_max, step=step)
    views = volume.render(torch.from_numpy(pose), kmat, rref.CLIP_H, rref.CLIP_W, **march)
    _check(views, 0, want, case["id"])
    dense = volume.to_dense(volume.bounds)
    assert dense.dims == volume.dims
    for skip in (True, False):
        assert _equal(views, dense.render(torch.from_numpy(pose), kmat, rref.CLIP_H, rref.CLIP_W, skip=skip, **march)), skip
