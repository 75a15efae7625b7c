"""GPU: the TSDF mesh - `mr_tsdf_mesh_vertices_f32` / `mr_tsdf_mesh_triangles_f32` behind `TSDFVolume.mesh` against the numpy
restatement of tests/tsdf_mesh_ref.py: an analytic sphere (closed, and with a hole in the weights), the fused volumes of
test_gpu_tsdf_fusion.py, degenerate shapes, a capacity below the count, the .ply and the runner.  Every comparison is exact."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
import tsdf_mesh_ref as mref
from monorec_amd import _lib, synth, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = ref.INTRINSICS_60
K3 = torch.tensor([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=torch.float32)
VOLUMES = {"small": ref.SMALL, "wide": ref.WIDE}
ORDER = [0, 10, 1, 2, 3, 4, 5, 6, 7, 8, 9]             # the eleven frames in test_gpu_tsdf_fusion.py's order


# ------------------------------------------------------------------------------------------ references, computed once, never modified
@functools.lru_cache(maxsize=None)
def _analytic(name, colour):
    vol = mref.sphere_volume(colour=colour, **mref.SPHERE_VOLUME)
    return mref.with_hole(vol) if name == "hole" else vol


@functools.lru_cache(maxsize=None)
def _fused(name):
    frames = ref.make_frames(K)
    vol = ref.new_volume(**VOLUMES[name])
    for i in ORDER:
        pose, depth, image = frames[i]
        ref.integrate(vol, ref.world_to_camera(pose), K, depth, image)
    return vol


@functools.lru_cache(maxsize=None)
def _want(kind, name, colour, min_weight):
    vol = _analytic(name, colour) if kind == "analytic" else _fused(name)
    got = mref.mesh(vol, min_weight)
    return got, mref.canonical(got["vertices"], got["triangles"])


def _load(vol):
    """A device volume holding the arrays of a restatement's volume dict."""
    volume = tf.TSDFVolume(origin=vol["origin"], dims=vol["dims"], voxel_size=float(vol["voxel"]), trunc=float(vol["trunc"]),
                           colour=vol["colour"] is not None, device=DEV)
    volume.tsdf.copy_(torch.from_numpy(vol["tsdf"].reshape(-1)))
    volume.weight.copy_(torch.from_numpy(vol["weight"].reshape(-1)))
    if vol["colour"] is not None:
        volume.colour.copy_(torch.from_numpy(vol["colour"].reshape(-1, 4)))
    return volume


def _mesh(volume, min_weight=0):
    vertices, triangles = volume.mesh(min_weight)
    assert vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 6
    assert triangles.is_cuda and triangles.dtype == torch.int32 and triangles.dim() == 2 and triangles.shape[1] == 3
    assert volume.mesh_counts(min_weight) == (vertices.shape[0], triangles.shape[0])
    vertices, triangles = vertices.cpu().numpy(), triangles.cpu().numpy()
    if len(triangles):
        assert triangles.min() >= 0 and triangles.max() < len(vertices)
    return vertices, triangles


# ------------------------------------------------------------------------------------------ 1. the sphere, closed and with a hole
@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("name", ["closed", "hole"])
def test_sphere_equals_the_restatement_and_is_welded(hip_lib, name, colour):
    """41 x 19 x 21: three tiles along y, six along z - vertices and triangles of one surface come from many workgroups.  The sphere spans
    x = 14 .. 29 and does not touch the seam x = 31 | 32; section 7 is about the seams."""
    vol = _analytic(name, colour)
    want, canonical = _want("analytic", name, colour, 0)
    vertices, triangles = _mesh(_load(vol))
    assert vertices.shape == want["vertices"].shape and triangles.shape == want["triangles"].shape and len(triangles) > 2000
    assert np.array_equal(mref.canonical(vertices, triangles), canonical)
    assert (vertices[:, 3:].max() > 100) if colour else (not vertices[:, 3:].any())
    topo, ref_topo = mref.topology(triangles), mref.topology(want["triangles"])          # of the device's own indices
    assert topo["repeated"] == [] and topo["V"] == len(vertices)
    if name == "closed":
        assert topo["open"] == [] and topo["V"] - topo["E"] + topo["F"] == 2
    else:
        assert all(n == 1 for _, _, n in topo["open"]) and len(topo["open"]) == len(ref_topo["open"]) > 0
        assert (topo["V"], topo["E"], topo["F"]) == (ref_topo["V"], ref_topo["E"], ref_topo["F"])


# ------------------------------------------------------------------------------------------ 2. fused volumes
@pytest.mark.parametrize("name", ["small", "wide"])
def test_fused_volumes_equal_the_restatement(hip_lib, name):
    """37 x 21 x 13 (odd nx) and 128 x 24 x 12 (most tiles empty) after the eleven frames, fused on the device."""
    frames = [ref.make_frames(K)[i] for i in ORDER]
    spec = VOLUMES[name]
    volume = tf.TSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV)
    volume.integrate(torch.from_numpy(np.stack([f[1] for f in frames])).to(DEV), torch.from_numpy(np.stack([f[2] for f in frames])).to(DEV),
                     torch.from_numpy(np.stack([f[0] for f in frames])), K3)
    counts = []
    for min_weight in (0, 2):
        want, canonical = _want("fused", name, True, min_weight)
        vertices, triangles = _mesh(volume, min_weight)
        assert np.array_equal(mref.canonical(vertices, triangles), canonical) and len(vertices) == len(want["vertices"])
        topo = mref.topology(triangles)
        assert topo["repeated"] == [] and all(n <= 2 for _, _, n in topo["open"])
        # the vertices are extract()'s records on the axis edges plus the restatement's on the diagonals
        points = volume.extract(min_weight).cpu().numpy()
        diagonal = want["vertices"][want["keys"][:, 3] >= 3]
        assert len(points) == int((want["keys"][:, 3] < 3).sum()) > 500 and len(diagonal) > 500
        assert np.array_equal(ref.sort_records(np.concatenate([points, diagonal])), ref.sort_records(vertices))
        counts.append(len(triangles))
    assert 0 < counts[1] < counts[0]


# ------------------------------------------------------------------------------------------ 3. degenerate shapes
_slab = ref.slab                                   # shared with test_gpu_tsdf_fusion.py


@pytest.mark.parametrize("dims,axis", [((40, 1, 9), 0), ((1, 9, 9), 1), ((9, 9, 1), 0)])
def test_a_volume_one_voxel_thick_has_vertices_but_no_triangle(hip_lib, dims, axis):
    vol = _slab(dims, axis)
    want = mref.mesh(vol)
    vertices, triangles = _mesh(_load(vol))
    assert len(want["vertices"]) > 8 and (want["keys"][:, 3] >= 3).any() and len(want["triangles"]) == 0
    assert triangles.shape == (0, 3) and np.array_equal(ref.sort_records(vertices), ref.sort_records(want["vertices"]))


def test_no_sign_change_means_empty_tensors_and_no_fill_launch(hip_lib):
    volume = tf.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=(40, 12, 9), voxel_size=0.1, device=DEV)
    calls = []
    launches = volume._mesh_launches
    volume._mesh_launches = lambda *a, **kw: (calls.append(len(a) + len(kw)), launches(*a, **kw))[1]
    for fill in (None, 0.5):                                               # untouched (unseen, tsdf 1); all seen in front of any surface
        if fill is not None:
            volume.tsdf.fill_(fill)
            volume.weight.fill_(1.0)
        del calls[:]
        vertices, triangles = volume.mesh()
        assert tuple(vertices.shape) == (0, 6) and tuple(triangles.shape) == (0, 3) and vertices.is_cuda and triangles.dtype == torch.int32
        assert calls == [2]                                                # the count launches (min_weight, cursor) alone
    zero = _load(_slab((40, 12, 9), 0, zero=True))                         # tsdf == 0 counts as outside everywhere
    assert zero.mesh_counts() == (0, 0) and zero.count() == 0
    with pytest.raises(RuntimeError, match="CPU fallback"):
        tf.TSDFVolume(origin=(0, 0, 0), dims=(4, 4, 4), voxel_size=0.1, device="cpu")


# ------------------------------------------------------------------------------------------ 4. capacity
def _fill_with_a_third_of_the_capacity(vol, want):
    """The two entries called directly with sentinel-filled outputs and capacities of a third of the counts."""
    n, m = len(want["vertices"]), len(want["triangles"])
    volume = _load(vol)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    cap_v, cap_t = n // 3, m // 3
    vertices = torch.full((n, 6), -7.0, dtype=torch.float32, device=DEV)
    triangles = torch.full((m, 3), -7, dtype=torch.int32, device=DEV)
    base = torch.full((volume.tsdf.numel(),), -7, dtype=torch.int32, device=DEV)
    cursor = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(lib.mr_tsdf_mesh_vertices_f32(*volume._volume_args(), volume._origin, volume.voxel_size, 0.0, vertices.data_ptr(), cap_v,
                                             base.data_ptr(), cursor.data_ptr(), stream), "vertices")
    _lib.check(lib.mr_tsdf_mesh_triangles_f32(volume.tsdf.data_ptr(), volume.weight.data_ptr(), *volume.dims, 0.0, base.data_ptr(),
                                              triangles.data_ptr(), cap_t, cursor.data_ptr() + 8, stream), "triangles")
    assert cursor.tolist() == [n, m]
    assert bool((vertices[cap_v:] == -7).all()) and bool((triangles[cap_t:] == -7).all())
    assert not bool((vertices[:cap_v, :3] == -7).any()) and not bool((triangles[:cap_t] == -7).any())
    # vertex_base is written for the voxels that own a vertex and for no other
    owners = np.zeros(vol["tsdf"].shape, bool)
    owners[want["keys"][:, 2], want["keys"][:, 1], want["keys"][:, 0]] = True
    assert np.array_equal(base.cpu().numpy().reshape(owners.shape) != -7, owners)
    # the records below the capacity are vertices of the mesh
    records = {r.tobytes() for r in want["vertices"]}
    assert all(r.tobytes() in records for r in vertices[:cap_v].cpu().numpy())


def test_a_capacity_below_the_count_writes_nothing_beyond_it(hip_lib):
    _fill_with_a_third_of_the_capacity(_analytic("closed", True), _want("analytic", "closed", True, 0)[0])


def test_a_capacity_below_the_count_on_a_noise_volume(hip_lib):
    """The same where nearly every voxel owns vertices and every tile's triangles reach into the next: 65 x 17 x 9."""
    vol = mref.noise_volume(ref.SEAM_DIMS[2], seed=1)
    want = mref.mesh(vol)
    assert (want["masks"] != 0).mean() > 0.5 and (want["masks"] == 0).sum() > 100
    _fill_with_a_third_of_the_capacity(vol, want)


# ------------------------------------------------------------------------------------------ 5. the file
def test_save_mesh_ply_parses_back_to_the_same_mesh(hip_lib, tmp_path):
    want, canonical = _want("analytic", "hole", True, 0)
    volume = _load(_analytic("hole", True))
    buffer = io.BytesIO()
    assert volume.save_mesh_ply(buffer) == (len(want["vertices"]), len(want["triangles"]))
    assert volume.save_mesh_ply(tmp_path / "m.ply", min_weight=0) == (len(want["vertices"]), len(want["triangles"]))
    for data in (buffer.getvalue(), open(tmp_path / "m.ply", "rb").read()):
        assert np.array_equal(mref.canonical(*mref.parse_mesh_ply(data)), canonical)


# ------------------------------------------------------------------------------------------ 6. the runner
def test_runner_writes_the_mesh_next_to_unchanged_points(hip_lib, tmp_path):
    """The synthetic KITTI tree and seeded model of test_gpu_tsdf_fusion.py's runner test, once with `mesh_file_name` and once without.
    The points files have the same header and the same records; the ORDER of `extract`'s records is unspecified (one atomicAdd per
    workgroup) and differs between any two runs, so the records are compared sorted, exactly."""
    from monorec_amd import MonoRecModel
    tree = synth.make_kitti_tree(tmp_path / "kitti", sequences=(("03", 120, 400),), frames=20)
    model = MonoRecModel(cv_depth_steps=16, hip_in_flight=4)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    config = {"name": "TSDF mesh", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": 9, "min_d": 3, "max_d": 30, "use_mask": False,
              "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": 3, "file_name": "surface.ply",
              "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": 16}},
              "data_set": {"type": "KittiOdometryDataset", "args": args}}
    plain = tf.run(dict(config, output_dir=str(tmp_path / "plain")), model=model)
    fusion = tf.Fusion(dict(config, output_dir=str(tmp_path / "mesh"), mesh_file_name="mesh.ply"), model=model).fuse()
    assert fusion.write() == plain > 0 and sorted(os.listdir(tmp_path / "mesh")) == ["mesh.ply", "surface.ply"]
    assert os.listdir(tmp_path / "plain") == ["surface.ply"]
    with_mesh, without = (open(tmp_path / d / "surface.ply", "rb").read().partition(b"end_header\n") for d in ("mesh", "plain"))
    assert with_mesh[:2] == without[:2] and len(with_mesh[2]) == len(without[2]) == 24 * plain
    assert np.array_equal(ref.sort_records(np.frombuffer(with_mesh[2], "<f4")), ref.sort_records(np.frombuffer(without[2], "<f4")))
    vertices, triangles = mref.parse_mesh_ply(open(tmp_path / "mesh" / "mesh.ply", "rb").read())
    assert fusion.mesh_counts == (len(vertices), len(triangles)) and len(triangles) > 0
    tsdf, weight, colour = fusion.volume.grids()
    want = mref.mesh(dict(dims=fusion.volume.dims, origin=tuple(np.float32(v) for v in fusion.volume.origin), voxel=np.float32(fusion.volume.voxel_size),
                          tsdf=tsdf, weight=weight, colour=colour))
    assert np.array_equal(mref.canonical(vertices, triangles), mref.canonical(want["vertices"], want["triangles"]))


# ------------------------------------------------------------------------------------------ 7. vertices across tile seams
def _equals_the_restatement(vol, min_weight=0):
    """The device mesh of `vol` against the restatement through `mref.canonical`, exactly, and `extract` against its axis-edge vertices."""
    want = mref.mesh(vol, min_weight)
    volume = _load(vol)
    vertices, triangles = _mesh(volume, min_weight)
    assert vertices.shape == want["vertices"].shape and triangles.shape == want["triangles"].shape
    assert np.array_equal(mref.canonical(vertices, triangles), mref.canonical(want["vertices"], want["triangles"]))
    assert np.array_equal(ref.sort_records(volume.extract(min_weight).cpu().numpy()), ref.sort_records(mref.axis_vertices(want)))
    return want


@pytest.mark.parametrize("background", [1, -1], ids=["positive", "negative"])
@pytest.mark.parametrize("axis,seam", [(axis, seam) for axis, tile in enumerate(mref.TILE) for seam in (tile, tile - 1)])
def test_every_sign_pattern_of_a_cube_on_a_tile_seam(hip_lib, axis, seam, background):
    """mref.pattern_volume: tests/test_tsdf_mesh.py shows that the twelve together put every (owner mask, edge type) pair on a vertex
    whose owner lies in the next tile - 192 per axis, where the fixtures above reach 15 / 53 / 89."""
    want = _equals_the_restatement(mref.pattern_volume(axis, seam, background))
    assert len(want["triangles"]) > 20000


@pytest.mark.parametrize("min_weight", [0, 1])
@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("dims", ref.SEAM_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_noise_volumes_equal_the_restatement(hip_lib, dims, colour, min_weight):
    """Independent random signs, a tenth unseen, zeros of both signs, a tile and a bit along every axis."""
    want = _equals_the_restatement(mref.noise_volume(dims, seed=1, colour=colour), min_weight)
    assert len(want["triangles"]) > (900 if min_weight else 4000)


@pytest.mark.parametrize("dims", ref.SEAM_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_seam_volumes_equal_the_restatement(hip_lib, dims):
    """ref.seam_volume, built for `extract` to cross every tile seam and ragged end, as a mesh."""
    for min_weight in (0, 1):
        assert len(_equals_the_restatement(ref.seam_volume(dims), min_weight)["triangles"]) > 100
