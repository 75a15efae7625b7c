"""GPU: vertex normals and the clustered level of detail of the TSDF mesh - `mesh(min_weight, cell, normals)` of `TSDFVolume` and
`SparseTSDFVolume` (the mr_tsdf_mesh_cluster_* / mr_tsdf_sparse_mesh_cluster_* entries and the two *_vertices_normals_* ones) - against
the numpy restatement of tests/tsdf_mesh_lod_ref.py.  Volumes are filled directly.  Every comparison is bit-exact, on
`tsdf_mesh_lod_ref.canonical` (the order of both arrays is unspecified)."""
import functools
import io

import numpy as np
import pytest
import torch

import tsdf_mesh_lod_ref as lod
import tsdf_mesh_ref as mref
import tsdf_sparse_ref as sref
from monorec_amd import _lib, synth, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = [(2, False), (2, True), (4, False), (4, True), (8, False), (8, True), (1, True)]      # (cell, normals)
KINDS = ("sphere", "plane", "pockets")
TILE = tf.CLUSTER_TILE
SEAM_DIMS = tuple(t + 8 for t in TILE)                  # one cluster of the largest cell beyond one workgroup tile, along each axis


# ------------------------------------------------------------------------------------------ references, computed once, never modified
@functools.lru_cache(maxsize=None)
def _field(dims, kind):
    return lod.field_volume(dims, kind, seed=sum(dims))


@functools.lru_cache(maxsize=None)
def _want(vol_key, min_weight, cell):
    """The restatement with normals (its vertices and triangles are those without), and its canonical forms with and without them."""
    vol = vol_key() if callable(vol_key) else _field(*vol_key)
    want = lod.mesh(vol, float(min_weight), cell=cell, normals=True)
    return want, lod.canonical(want["vertices"], want["triangles"]), lod.canonical(want["vertices"], want["triangles"], want["normals"])


def _load(vol):
    volume = tf.TSDFVolume(origin=vol["origin"], dims=vol["dims"], voxel_size=float(vol["voxel"]), trunc=float(vol["trunc"]),
                           colour=vol["colour"] is not None, device=DEV)
    volume.tsdf.copy_(torch.from_numpy(vol["tsdf"].reshape(-1)))
    volume.weight.copy_(torch.from_numpy(vol["weight"].reshape(-1)))
    if vol["colour"] is not None:
        volume.colour.copy_(torch.from_numpy(vol["colour"].reshape(-1, 4)))
    return volume


def _load_sparse(stands_for, order=None):
    coords, tsdf, weight, colour = sref.blocks_of(stands_for)
    volume = tf.SparseTSDFVolume(origin=stands_for["origin"], dims=stands_for["dims"], voxel_size=float(stands_for["voxel"]),
                                 trunc=float(stands_for["trunc"]), colour=colour is not None, device=DEV, capacity_blocks=max(len(coords), 1))
    if order is not None:
        coords, tsdf, weight, colour = coords[order], tsdf[order], weight[order], colour[order] if colour is not None else None
    volume.set_blocks(coords, tsdf, weight, colour)
    return volume


def _mesh(volume, min_weight, cell, normals):
    """`mesh` on the host, its shapes, types and `mesh_counts` checked."""
    out = volume.mesh(min_weight, cell=cell, normals=normals)
    assert len(out) == (3 if normals else 2)
    vertices, triangles = out[:2]
    assert vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 6
    assert triangles.is_cuda and triangles.dtype == torch.int32 and triangles.dim() == 2 and triangles.shape[1] == 3
    assert volume.mesh_counts(min_weight, cell=cell) == (vertices.shape[0], triangles.shape[0])
    if normals:
        assert out[2].is_cuda and out[2].dtype == torch.float32 and tuple(out[2].shape) == (vertices.shape[0], 3)
    out = [t.cpu().numpy() for t in out]
    if len(out[1]):
        assert out[1].min() >= 0 and out[1].max() < len(out[0])
    if normals:
        lengths = np.linalg.norm(out[2].astype(np.float64), axis=1)
        assert np.all((np.abs(lengths - 1) < 1e-6) | (lengths == 0))
    return out


def _check(volume, vol_key, min_weight, variants=VARIANTS):
    """Every variant of `volume` against the restatement; returns the triangle counts per cell."""
    counts = {}
    for cell, normals in variants:
        want, plain, with_normals = _want(vol_key, min_weight, cell)
        got = _mesh(volume, min_weight, cell, normals)
        assert (len(got[0]), len(got[1])) == (len(want["vertices"]), len(want["triangles"])), (cell, normals)
        assert lod.same(lod.canonical(*got), with_normals if normals else plain), (cell, normals)
        counts[cell] = len(got[1])
    return counts


# ------------------------------------------------------------------------------------------ 1. dense volumes
@pytest.mark.parametrize("min_weight", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims", [(16, 16, 16), (17, 13, 9)], ids=["16x16x16", "17x13x9"])
def test_dense_volumes_equal_the_restatement(hip_lib, dims, kind, min_weight):
    """16^3: whole clusters.  17 x 13 x 9: a partial cluster on every high side for every cell.  The sphere is closed, the plane leaves
    the grid, the pockets are unseen voxels (weight 0, with min_weight 1 also weight 1) next to the surface."""
    vol = _field(dims, kind)
    counts = _check(_load(vol), (dims, kind), min_weight)
    assert counts[1] > counts[2] > counts[4] > 0 and counts[4] >= counts[8]
    if kind == "pockets":
        seen = vol["weight"] > min_weight
        assert 0 < (~seen).sum() and len(_want((dims, kind), min_weight, 1)[0]["triangles"]) < len(_want((dims, "sphere"), min_weight, 1)[0]["triangles"])


# ------------------------------------------------------------------------------------------ 2. tile seams
def test_a_surface_across_the_seams_of_the_cluster_tile(hip_lib):
    """40 x 16 x 16: one cluster of 8 beyond the tile of the clustered vertex kernel along each axis (and several tiles of the triangle
    kernel).  The plane has cubes based in the last voxel before each seam, so triangles there map owners in two workgroups' clusters."""
    assert SEAM_DIMS == (40, 16, 16) and TILE == _lib.MR_TSDF_CLUSTER_TILE
    key = (SEAM_DIMS, "plane")
    cubes = mref.mesh(_field(*key))["cubes"]
    for axis in range(3):
        assert (cubes[:, axis] == TILE[axis] - 1).any() and (cubes[:, axis] == TILE[axis]).any()
    counts = _check(_load(_field(*key)), key, 0)
    assert counts[8] > 0
    _check(_load(_field(SEAM_DIMS, "pockets")), (SEAM_DIMS, "pockets"), 1)


# ------------------------------------------------------------------------------------------ 3. sparse volumes
SPARSE_DIMS = (24, 16, 16)                              # 3 x 2 x 2 blocks


@functools.lru_cache(maxsize=None)
def _sparse(kind):
    """The field on 3 x 2 x 2 blocks without two blocks that hold seen voxels of both signs: missing storage next to the surface."""
    vol = lod.field_volume(SPARSE_DIMS, kind, seed=11)
    seen = vol["weight"] > 0
    both = sref.any_per_block(seen & (vol["tsdf"] < 0)) & sref.any_per_block(seen & ~(vol["tsdf"] < 0))
    crossed = np.argwhere(both)
    assert len(crossed) >= 6
    allocated = np.ones(both.shape, bool)
    for bz, by, bx in (crossed[1], crossed[-2]):
        allocated[bz, by, bx] = False
    return sref.sparsify(vol, allocated)


def _sparse_pockets():
    return _sparse("pockets")


def _sparse_plane():
    return _sparse("plane")


@pytest.mark.parametrize("min_weight", [0, 1])
@pytest.mark.parametrize("key", [_sparse_pockets, _sparse_plane], ids=["pockets", "plane"])
def test_sparse_volumes_equal_the_restatement_and_the_gathered_volume(hip_lib, key, min_weight):
    stands_for = key()
    n = int(stands_for["allocated"].sum())
    assert n == 10
    order = np.random.default_rng(5).permutation(n)
    assert not np.array_equal(order, np.arange(n))
    table_order, permuted = _load_sparse(stands_for), _load_sparse(stands_for, order)
    assert np.array_equal(permuted.block_of_slot[:n].cpu().numpy(), table_order.block_of_slot[:n].cpu().numpy()[order])
    dense = table_order.to_dense(table_order.bounds)
    assert dense.dims == SPARSE_DIMS
    counts = _check(table_order, key, min_weight)
    assert counts[1] > counts[2] > counts[4] > 0
    _check(permuted, key, min_weight)
    _check(dense, key, min_weight)                                            # to_dense(bounds).mesh(cell, normals): the same canonical mesh
    # the missing blocks cut the mesh: fewer triangles than the field with every block
    whole = lod.mesh(lod.field_volume(SPARSE_DIMS, "pockets" if key is _sparse_pockets else "plane", seed=11), float(min_weight))
    assert counts[1] < len(whole["triangles"])


# ------------------------------------------------------------------------------------------ 4. nothing to mesh
def test_empty_volumes_give_empty_arrays(hip_lib):
    dense = tf.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=(17, 13, 9), voxel_size=0.1, device=DEV)
    sparse = tf.SparseTSDFVolume(origin=(0.0, 0.0, 0.0), dims=(24, 16, 16), voxel_size=0.1, device=DEV)
    for volume in (dense, sparse):
        for cell, normals in VARIANTS:
            out = volume.mesh(cell=cell, normals=normals)
            assert [tuple(t.shape) for t in out] == [(0, 6), (0, 3), (0, 3)][:len(out)] and len(out) == (3 if normals else 2)
            assert all(t.is_cuda for t in out) and out[1].dtype == torch.int32
            assert volume.mesh_counts(cell=cell) == (0, 0)
        data = io.BytesIO()
        assert volume.save_mesh_ply(data, cell=4, normals=True) == (0, 0) and lod.parse_mesh_ply(data.getvalue())[2].shape == (0, 3)


# ------------------------------------------------------------------------------------------ 5. the path without cell and normals
def _as_before(volume, min_weight=0.0):
    """`mesh(min_weight)` as the method was before it took `cell` and `normals`: the two entries called directly, count then fill."""
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    _, vertex_entry, triangle_entry = volume._SURFACE_ENTRIES

    def launches(cursor, vertices, triangles, base):
        with_colour, without_colour = volume._surface_args(base)
        out = (None, 0) if vertices is None else (vertices.data_ptr(), vertices.shape[0])
        pointer = base.data_ptr() if base is not None else None
        _lib.check(getattr(lib, vertex_entry)(*with_colour, volume._origin, volume.voxel_size, float(min_weight), out[0], out[1], pointer,
                                              cursor.data_ptr(), stream), vertex_entry)
        out = (None, 0) if triangles is None else (triangles.data_ptr(), triangles.shape[0])
        _lib.check(getattr(lib, triangle_entry)(*without_colour, float(min_weight), pointer, out[0], out[1], cursor.data_ptr() + 8, stream),
                   triangle_entry)
    cursor = torch.zeros(2, dtype=torch.int64, device=DEV)
    launches(cursor, None, None, None)
    n, m = cursor.tolist()
    vertices = torch.empty(n, 6, dtype=torch.float32, device=DEV)
    triangles = torch.empty(m, 3, dtype=torch.int32, device=DEV)
    cursor.zero_()
    launches(cursor, vertices, triangles, torch.empty(volume._mesh_voxels(), dtype=torch.int32, device=DEV))
    assert cursor.tolist() == [n, m]
    return vertices.cpu().numpy(), triangles.cpu().numpy()


def test_the_mesh_without_cell_and_normals_is_the_one_it_was(hip_lib):
    """One workgroup meshes each of these volumes - a dense one of a single tile, a sparse one of a single block -, so the order of both
    arrays is defined and must be the same too; the larger volumes of the other tests are compared as canonical meshes."""
    single = lod.field_volume(tuple(tf.TILE), "plane", seed=2)
    block = sref.sparsify(lod.field_volume((8, 8, 8), "pockets", seed=4), np.ones((1, 1, 1), bool))
    for volume in (_load(single), _load_sparse(block)):
        before = _as_before(volume)
        assert len(before[1]) > 20
        for got in (volume.mesh(), volume.mesh(0), volume.mesh(0, 1, False), volume.mesh(cell=1, normals=False)):
            assert len(got) == 2
            assert np.array_equal(got[0].cpu().numpy().view(np.uint32), before[0].view(np.uint32)) and np.array_equal(got[1].cpu().numpy(), before[1])
        with_normals = volume.mesh(normals=True)
        assert np.array_equal(with_normals[0].cpu().numpy().view(np.uint32), before[0].view(np.uint32))      # the same records in the same order
        assert np.array_equal(with_normals[1].cpu().numpy(), before[1])
    for volume in (_load(_field((17, 13, 9), "pockets")), _load_sparse(_sparse("pockets"))):
        for min_weight in (0, 1):
            got = [t.cpu().numpy() for t in volume.mesh(min_weight)]
            assert lod.same(lod.canonical(*got), lod.canonical(*_as_before(volume, min_weight)))


def test_cells_that_do_not_divide_the_block_raise(hip_lib):
    volume = _load(_field((16, 16, 16), "sphere"))
    for bad in (3, 16, 0):
        with pytest.raises(ValueError, match="must be one of 1, 2, 4, 8"):
            volume.mesh(cell=bad)
    lib, cursor = _lib.load(), torch.zeros(1, dtype=torch.int64, device=DEV)
    for bad in (1, 3, 16, 0, -2):
        assert lib.mr_tsdf_mesh_cluster_vertices_f32(*volume._volume_args(), volume._origin, volume.voxel_size, 0.0, bad, None, 0, None, None,
                                                     cursor.data_ptr(), None) == -1
    assert cursor.item() == 0


# ------------------------------------------------------------------------------------------ 6. the runner
STEPS, KEYFRAMES = 16, 6


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
    """The config of the fusion runner tests (tests/test_gpu_tsdf_sparse_mesh.py) with a dense volume."""
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    return dict({"name": "TSDF fusion", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": KEYFRAMES, "min_d": 3, "max_d": 30,
                 "use_mask": False, "output_dir": str(out_dir), "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": 1,
                 "file_name": "surface.ply", "mesh_file_name": "mesh.ply",
                 "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": STEPS}},
                 "data_set": {"type": "KittiOdometryDataset", "args": args}}, **more)


def test_runner_writes_the_clustered_mesh_with_normals(tree, model, tmp_path):
    fusion = tf.Fusion(_config(tree, tmp_path, mesh_cell=4, mesh_normals=True), model=model).fuse()
    fusion.write()
    volume = fusion.volume
    nx, ny, nz = volume.dims
    vol = dict(dims=volume.dims, origin=tuple(np.float32(o) for o in volume.origin), voxel=np.float32(volume.voxel_size),
               trunc=np.float32(volume.trunc), offset=(0, 0, 0), tsdf=volume.tsdf.cpu().numpy().reshape(nz, ny, nx),
               weight=volume.weight.cpu().numpy().reshape(nz, ny, nx), colour=volume.colour.cpu().numpy().reshape(nz, ny, nx, 4))
    want = lod.mesh(vol, 0.0, cell=4, normals=True)
    text = open(tmp_path / "mesh.ply", "rb").read()
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in text
    vertices, triangles, normals = lod.parse_mesh_ply(text)
    assert fusion.mesh_counts == (len(vertices), len(triangles)) == (len(want["vertices"]), len(want["triangles"])) and len(triangles) > 20
    assert lod.same(lod.canonical(vertices, triangles, normals), lod.canonical(want["vertices"], want["triangles"], want["normals"]))
