"""GPU: the mesh of the block-sparse TSDF volume - `mr_tsdf_sparse_mesh_vertices_f32` / `mr_tsdf_sparse_mesh_triangles_f32` behind
`SparseTSDFVolume.mesh` - against `tsdf_mesh_ref.mesh` of the dense volume the sparse one stands for (a block without storage unseen)
and against the dense class on the gathered volume: cubes and owners across block faces, neighbours without storage, slot order, stale
table entries, fused volumes, closedness, a capacity below the count, a volume the dense class refuses, the runner.  Every mesh
comparison is on `tsdf_mesh_ref.canonical`: bit-exact, order-free, no tolerance."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
import tsdf_mesh_ref as mref
import tsdf_sparse_mesh_ref as smref
import tsdf_sparse_ref as sref
from monorec_amd import _lib, synth, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECS = {"first": sref.FIRST, "second": sref.SECOND}
KMAT = torch.tensor([[sref.K[0], 0.0, sref.K[2]], [0.0, sref.K[1], sref.K[3]], [0.0, 0.0, 1.0]])
OFFSET = (2048, 2048, 232)
BIG = (4096, 4096, 512)


def _load(stands_for, order=None, capacity=None):
    """A device volume holding the allocated blocks of a sparse restatement volume, in table order or in `order`: slot i holds block
    order[i]."""
    coords, tsdf, weight, colour = sref.blocks_of(stands_for)
    volume = tf.SparseTSDFVolume(origin=stands_for["origin"], dims=stands_for["dims"], voxel_size=float(stands_for["voxel"]),
                                 trunc=float(stands_for["trunc"]), colour=colour is not None, device=DEV,
                                 capacity_blocks=capacity or max(len(coords), 1))
    if order is not None:
        coords, tsdf, weight, colour = coords[order], tsdf[order], weight[order], colour[order] if colour is not None else None
    volume.set_blocks(coords, tsdf, weight, colour)
    assert volume.allocated_blocks() == int(stands_for["allocated"].sum()) and volume.dims == tuple(stands_for["dims"])
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


def _same_mesh(got, want, canonical):
    vertices, triangles = got
    assert vertices.shape == want["vertices"].shape and triangles.shape == want["triangles"].shape
    assert np.array_equal(ref.sort_records(vertices), ref.sort_records(want["vertices"]))
    assert np.array_equal(mref.canonical(vertices, triangles), canonical)


def _dense_mesh(volume, min_weight=0):
    vertices, triangles = volume.to_dense(volume.bounds).mesh(min_weight)
    return vertices.cpu().numpy(), triangles.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. cubes and owners across block faces
@pytest.mark.parametrize("axis,seam,background", smref.PATTERNS, ids=[f"axis{a}-seam{s}-{'pos' if b > 0 else 'neg'}" for a, s, b in smref.PATTERNS])
def test_pattern_volumes_equal_the_restatement_and_the_dense_mesh(hip_lib, axis, seam, background):
    """16 x 56 x 56 voxels, 98 blocks, all allocated: every sign pattern of a cube that straddles the block face at voxel 8 of `axis`
    (tests/test_tsdf_sparse_mesh.py proves that together they rank every owner mask and edge type across the face)."""
    stands_for = smref.pattern(axis, seam, background)
    want, canonical = smref.mesh(stands_for)
    volume = _load(stands_for)
    got = _mesh(volume)
    assert len(got[1]) > 2000
    _same_mesh(got, want, canonical)
    dense = _dense_mesh(volume)
    assert np.array_equal(mref.canonical(*dense), canonical) and volume.to_dense(volume.bounds).mesh_counts() == (len(got[0]), len(got[1]))


# ------------------------------------------------------------------------------------------ 2. neighbours without storage
MISSING = [("pattern", 0), ("pattern", 1), ("pattern", 2), ("noise", 3), ("noise", 4)]


def _missing(kind, which, colour):
    return smref.positive_dropped(which, colour) if kind == "pattern" else smref.noise(which, colour)


@pytest.mark.parametrize("min_weight", [0, 1])
@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("kind,which", MISSING, ids=[f"{k}{w}" for k, w in MISSING])
def test_blocks_without_storage_are_unseen(hip_lib, kind, which, colour, min_weight):
    """The pattern volumes without their all-positive blocks (36 of 98 keep storage: cubes lose corners, owners stay), and noise with
    40 % of 3^3 blocks gone.  The pattern volumes' weights are all 1, so min_weight 1 leaves them no mesh at all; the noise volumes'
    are 0 .. 3."""
    stands_for = _missing(kind, which, colour)
    assert not stands_for["allocated"].all() and (stands_for["colour"] is not None) == colour
    want, canonical = smref.mesh(stands_for, min_weight)
    volume = _load(stands_for)
    got = _mesh(volume, min_weight)
    assert (len(got[1]) > 1000) == (kind == "noise" or min_weight == 0) and (len(got[1]) > 0 or kind == "pattern")
    _same_mesh(got, want, canonical)
    assert np.array_equal(mref.canonical(*_dense_mesh(volume, min_weight)), canonical)           # min_weight >= 0: the gathered volume's mesh
    assert (got[0][:, 3:].max() > 100) if colour and len(got[0]) else (not got[0][:, 3:].any())


# ------------------------------------------------------------------------------------------ 3. slot order
@pytest.mark.parametrize("kind,which", [("pattern", 1), ("noise", 3)], ids=["pattern1", "noise3"])
def test_the_order_of_the_slots_does_not_matter(hip_lib, kind, which):
    stands_for = _missing(kind, which, True)
    want, canonical = smref.mesh(stands_for)
    n = int(stands_for["allocated"].sum())
    for seed in (0, 1):
        order = np.random.default_rng(seed).permutation(n)
        assert not np.array_equal(order, np.arange(n))
        _same_mesh(_mesh(_load(stands_for, order)), want, canonical)
    _same_mesh(_mesh(_load(stands_for, np.arange(n)[::-1].copy())), want, canonical)


# ------------------------------------------------------------------------------------------ the entries called directly
def _entries(volume, num_slots, min_weight=0.0, capacity=None, rows=None, canary=-7):
    """The four launches on `num_slots` slots: counts, then fills into buffers of `rows` = (vertices, triangles) rows (default: the
    counts) filled with `canary`, with capacities `capacity` (default: the counts).  Returns counts, fill cursors and the host arrays."""
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    table, slots = volume._table_args(), volume.block_of_slot.data_ptr()
    cursor = torch.zeros(2, dtype=torch.int64, device=DEV)

    def launch(vertices, cap_v, triangles, cap_t, base):
        _lib.check(lib.mr_tsdf_sparse_mesh_vertices_f32(*table, slots, num_slots, volume._origin, volume.voxel_size, float(min_weight), vertices, cap_v,
                                                        base, cursor.data_ptr(), stream), "vertices")
        _lib.check(lib.mr_tsdf_sparse_mesh_triangles_f32(*table[:6], slots, num_slots, float(min_weight), base, triangles, cap_t,
                                                         cursor.data_ptr() + 8, stream), "triangles")
    launch(None, 0, None, 0, None)
    n, m = cursor.tolist()
    cap_v, cap_t = (n, m) if capacity is None else capacity
    rows_v, rows_t = (n, m) if rows is None else rows
    assert cap_v <= rows_v and cap_t <= rows_t                                # nothing is asked to write beyond its buffer
    vertices = torch.full((rows_v, 6), float(canary), dtype=torch.float32, device=DEV)
    triangles = torch.full((rows_t, 3), canary, dtype=torch.int32, device=DEV)
    base = torch.full((max(num_slots, 1) * 512,), canary, dtype=torch.int32, device=DEV)
    cursor.zero_()
    launch(vertices.data_ptr(), cap_v, triangles.data_ptr(), cap_t, base.data_ptr())
    return (n, m), tuple(cursor.tolist()), vertices.cpu().numpy(), triangles.cpu().numpy(), base.cpu().numpy()


# ------------------------------------------------------------------------------------------ 4. stale table entries
@pytest.mark.parametrize("kind,which,k", [("pattern", 2, 9), ("noise", 4, 5)], ids=["pattern2-9", "noise4-5"])
def test_a_table_entry_at_or_above_num_slots_is_no_slot(hip_lib, kind, which, k):
    """n blocks loaded, the entries called with num_slots = n - k: the last k slots' blocks still have their table entries, which read
    as no slot - as neighbours too.  The blocks are shuffled first so that the k lie anywhere in the volume."""
    stands_for = _missing(kind, which, True)
    coords = sref.blocks_of(stands_for)[0]
    n = len(coords)
    order = np.random.default_rng(7).permutation(n)
    volume = _load(stands_for, order)
    want, canonical = smref.mesh(smref.without_blocks(stands_for, coords[order[n - k:]]))
    whole = smref.mesh(stands_for)[0]
    assert 0 < len(want["triangles"]) < len(whole["triangles"])
    counts, filled, vertices, triangles, _ = _entries(volume, n - k)
    assert counts == filled == (len(want["vertices"]), len(want["triangles"]))
    _same_mesh((vertices, triangles), want, canonical)


# ------------------------------------------------------------------------------------------ 5. fused volumes
@functools.lru_cache(maxsize=None)
def _frames():
    return ref.make_frames(sref.K)                      # eleven 24 x 40 frames on the arc; the last one looks away


@functools.lru_cache(maxsize=None)
def _restated(name):
    return sref.fuse(SPECS[name], _frames(), 3)


@pytest.mark.parametrize("name", ["first", "second"])
def test_fused_volumes_equal_the_restatement_the_dense_mesh_and_extract(hip_lib, name):
    """48 x 32 x 48 and 128 x 32 x 48 voxels after the eleven frames in launches of 3, fused on the device: 30 of 144 and 47 of 384
    blocks."""
    spec = SPECS[name]
    volume = tf.SparseTSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV)
    depth = torch.from_numpy(np.stack([f[1] for f in _frames()])).to(DEV)
    image = torch.from_numpy(np.stack([f[2] for f in _frames()])).to(DEV)
    poses = torch.from_numpy(np.stack([f[0] for f in _frames()]))
    for lo in range(0, len(_frames()), 3):
        volume.integrate(depth[lo:lo + 3], image[lo:lo + 3], poses[lo:lo + 3], KMAT)
    assert volume.allocated_blocks() == int(_restated(name)["allocated"].sum()) == dict(first=30, second=47)[name]
    counts = []
    for min_weight in (0, 2):
        want, canonical = smref.mesh(_restated(name), min_weight)
        got = _mesh(volume, min_weight)
        _same_mesh(got, want, canonical)
        assert np.array_equal(mref.canonical(*_dense_mesh(volume, min_weight)), canonical)
        topo = mref.topology(got[1])
        assert topo["repeated"] == [] and all(c <= 2 for _, _, c in topo["open"])
        # the vertices are extract()'s records on the axis edges plus the restatement's on the diagonals
        points = volume.extract(min_weight).cpu().numpy()
        diagonal = want["vertices"][want["keys"][:, 3] >= 3]
        assert len(points) == int((want["keys"][:, 3] < 3).sum()) > 300 and len(diagonal) > 300
        assert np.array_equal(ref.sort_records(points), ref.sort_records(mref.axis_vertices(want)))
        assert np.array_equal(ref.sort_records(np.concatenate([points, diagonal])), ref.sort_records(got[0]))
        counts.append(len(got[1]))
    assert 0 < counts[1] < counts[0]


# ------------------------------------------------------------------------------------------ 6. closedness
def test_the_sphere_is_closed_and_a_removed_block_opens_it_only_round_itself(hip_lib):
    stands_for = smref.sphere()                                               # 48 x 24 x 24 voxels, 54 blocks, all allocated
    want, canonical = smref.mesh(stands_for)
    vertices, triangles = _mesh(_load(stands_for))
    _same_mesh((vertices, triangles), want, canonical)
    topo = mref.topology(triangles)                                           # of the device's own indices
    assert topo["open"] == [] and topo["repeated"] == [] and topo["V"] == len(vertices) and topo["V"] - topo["E"] + topo["F"] == 2
    block = smref.surface_block(stands_for)
    cut = smref.without_blocks(stands_for, [block])
    want, canonical = smref.mesh(cut)
    vertices, triangles = _mesh(_load(cut))
    _same_mesh((vertices, triangles), want, canonical)
    topo = mref.topology(triangles)
    assert topo["repeated"] == [] and len(topo["open"]) > 0 and all(c == 1 for _, _, c in topo["open"])
    # an open edge lies on a cube with a corner in the removed block: both ends within one voxel of it (positions are exact to well
    # under a hundredth of a voxel)
    voxel, origin = np.float64(stands_for["voxel"]), np.asarray(stands_for["origin"], np.float64)
    ends = (vertices[np.asarray([(i, j) for i, j, _ in topo["open"]]), :3].astype(np.float64) - origin) / voxel
    lo = np.asarray(block) * 8
    assert np.all(ends >= lo - 1.01) and np.all(ends <= lo + 8.01)


# ------------------------------------------------------------------------------------------ 7. a capacity below the count
@pytest.mark.parametrize("kind,which", [("pattern", 0), ("noise", 3)], ids=["pattern0", "noise3"])
def test_fills_stop_at_the_capacity_and_the_cursors_count_on(hip_lib, kind, which):
    stands_for = _missing(kind, which, True)
    want, _ = smref.mesh(stands_for)
    n, m = len(want["vertices"]), len(want["triangles"])
    volume = _load(stands_for)
    slots = volume.allocated_blocks()
    cap_v, cap_t = n // 3, m // 3
    counts, filled, vertices, triangles, _ = _entries(volume, slots, capacity=(cap_v, cap_t), rows=(n + 64, m + 64))
    assert counts == filled == (n, m)                                         # the cursors report the full counts
    assert (vertices[cap_v:] == -7.0).all() and (triangles[cap_t:] == -7).all()           # nothing at or beyond the capacity
    records = {r.tobytes() for r in want["vertices"]}
    assert cap_v > 1000 and all(r.tobytes() in records for r in vertices[:cap_v])
    assert not (triangles[:cap_t] == -7).any() and triangles[:cap_t].min() >= 0 and triangles[:cap_t].max() < n
    # a capacity of 0 with an output writes nothing; the full capacity in the larger buffer leaves the canary rows alone
    counts, filled, vertices, triangles, _ = _entries(volume, slots, capacity=(0, 0), rows=(8, 8))
    assert counts == filled == (n, m) and (vertices == -7.0).all() and (triangles == -7).all()
    counts, filled, vertices, triangles, base = _entries(volume, slots, rows=(n + 64, m + 64))
    assert (vertices[n:] == -7.0).all() and (triangles[m:] == -7).all()
    assert np.array_equal(mref.canonical(vertices[:n], triangles[:m]), smref.mesh(stands_for)[1])
    # vertex_base: written exactly for the pool voxels that own a vertex
    coords = sref.blocks_of(stands_for)[0]
    owns = np.stack([want["masks"][z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] for x, y, z in coords]).reshape(-1) != 0
    assert np.array_equal(base != -7, owns) and base[owns].min() >= 0 and base[owns].max() < n


# ------------------------------------------------------------------------------------------ 8. a volume the dense class refuses
def test_a_volume_the_dense_class_refuses(hip_lib):
    """4096 x 4096 x 512 voxels (96 GiB dense, 32 GiB of vertex_base alone) with the FIRST restatement's 30 blocks at voxel OFFSET: the
    workspace is 30 x 512 x 4 bytes."""
    with pytest.raises(ValueError, match=r"4096 x 4096 x 512 voxels of 0\.06 m need 96\.00 GiB"):
        tf.TSDFVolume(origin=(0, 0, 0), dims=BIG, voxel_size=0.06, device=DEV)
    spec, sub = sref.FIRST, _restated("first")
    origin = tuple(o - i * spec["voxel_size"] for o, i in zip(spec["origin"], OFFSET))
    volume = tf.SparseTSDFVolume(origin=origin, dims=BIG, voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV, capacity_blocks=256)
    coords, tsdf, weight, colour = sref.blocks_of(sub)
    volume.set_blocks(coords + np.asarray(OFFSET) // 8, tsdf, weight, colour)
    assert volume.blocks == (512, 512, 64) and volume.allocated_blocks() == 30 and volume._mesh_voxels() == 30 * 512
    want, _ = smref.mesh(sub)
    vertices, triangles = _mesh(volume)
    assert (len(vertices), len(triangles)) == (len(want["vertices"]), len(want["triangles"])) and len(triangles) > 1000
    assert volume.to_dense().mesh_counts() == (len(vertices), len(triangles))                 # of the box of the allocated blocks
    # the same topology as the small volume's mesh, and the same colours; the positions belong to another origin
    assert np.array_equal(vertices[:, 3:].astype(np.float64).sum(axis=0), want["vertices"][:, 3:].astype(np.float64).sum(axis=0))
    topo, small = mref.topology(triangles), mref.topology(want["triangles"])
    assert topo["repeated"] == [] and (topo["V"], topo["E"], topo["F"], len(topo["open"])) == (small["V"], small["E"], small["F"], len(small["open"]))
    # the vertices on the axis edges are extract()'s records, the others as many as the restatement's on the diagonals
    points = volume.extract().cpu().numpy()
    rows = {r.tobytes() for r in vertices}
    assert len(points) == int((want["keys"][:, 3] < 3).sum()) and len({r.tobytes() for r in points}) == len(points)
    assert all(r.tobytes() in rows for r in points)
    lo = np.asarray(origin) + np.asarray(OFFSET) * spec["voxel_size"]
    assert (vertices[:, :3] > lo - 0.1).all() and (vertices[:, :3] < lo + np.asarray(spec["dims"]) * spec["voxel_size"] + 0.1).all()


# ------------------------------------------------------------------------------------------ 9. the runner
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
    """The config of test_runner_with_sparse_volume_equals_fusing_by_hand (tests/test_gpu_tsdf_sparse.py) with a mesh file."""
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    return dict({"name": "sparse TSDF fusion", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": KEYFRAMES, "min_d": 3, "max_d": 30,
                 "use_mask": False, "output_dir": str(out_dir), "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": 1, "sparse_volume": True,
                 "file_name": "surface.ply", "mesh_file_name": "mesh.ply",
                 "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": STEPS}},
                 "data_set": {"type": "KittiOdometryDataset", "args": args}}, **more)


def test_runner_meshes_the_sparse_volume_itself(tree, model, tmp_path):
    a = tf.Fusion(_config(tree, tmp_path / "a", sparse_mesh=True), model=model).fuse()
    b = tf.Fusion(_config(tree, tmp_path / "b"), model=model).fuse()
    count = a.write()
    assert count == b.write() > 100 and a.mesh_counts == b.mesh_counts and a.mesh_counts[1] > 100
    assert a._dense is None and b._dense is not None                          # run A never gathered the volume
    file_a = mref.parse_mesh_ply(open(tmp_path / "a" / "mesh.ply", "rb").read())
    file_b = mref.parse_mesh_ply(open(tmp_path / "b" / "mesh.ply", "rb").read())
    assert a.mesh_counts == (len(file_a[0]), len(file_a[1]))
    assert np.array_equal(mref.canonical(*file_a), mref.canonical(*file_b))
    # a budget of the table and the allocated slots alone: no room for the dense copy
    blocks_total, allocated = a.volume.table.numel(), a.volume.allocated_blocks()
    budget = 4 * blocks_total + allocated * (512 * 12 + 4)
    assert 0 < allocated < blocks_total and budget < tf.volume_bytes(a.volume.dims)
    with pytest.raises(ValueError, match="mesh_file_name with sparse_volume need the volume gathered"):
        tf.Fusion(_config(tree, tmp_path / "d", tsdf_max_bytes=budget), model=model).fuse().write()
    assert not os.path.exists(tmp_path / "d" / "mesh.ply")
    tight = tf.Fusion(_config(tree, tmp_path / "c", sparse_mesh=True, tsdf_max_bytes=budget), model=model).fuse()
    assert tight.volume.capacity == allocated and tight.write() == count and tight._dense is None
    file_c = mref.parse_mesh_ply(open(tmp_path / "c" / "mesh.ply", "rb").read())
    by_hand = tuple(t.cpu().numpy() for t in tight.volume.mesh())
    assert tight.mesh_counts == (len(by_hand[0]), len(by_hand[1])) == a.mesh_counts
    assert np.array_equal(mref.canonical(*file_c), mref.canonical(*by_hand)) and np.array_equal(mref.canonical(*file_c), mref.canonical(*file_a))


# ------------------------------------------------------------------------------------------ 10. nothing to mesh
def test_an_empty_volume_gives_empty_tensors_and_no_fill_launch(hip_lib):
    volume = tf.SparseTSDFVolume(origin=(0.0, 0.0, 0.0), dims=(40, 12, 9), voxel_size=0.1, device=DEV)
    calls = []
    launches = volume._mesh_launches
    volume._mesh_launches = lambda *a, **kw: (calls.append(len(a) + len(kw)), launches(*a, **kw))[1]
    for fill in (None, 0.5):                    # no block allocated; every block allocated, all seen in front of any surface
        if fill is not None:
            n = volume.table.numel()
            volume.set_blocks(volume._block_coords(np.arange(n)), np.full((n, 8, 8, 8), fill, np.float32), np.ones((n, 8, 8, 8), np.float32),
                              np.zeros((n, 8, 8, 8, 4), np.uint8))
            assert volume.allocated_blocks() == n == 20
        del calls[:]
        vertices, triangles = volume.mesh()
        assert tuple(vertices.shape) == (0, 6) and tuple(triangles.shape) == (0, 3) and vertices.is_cuda and triangles.dtype == torch.int32
        assert calls == [2]                                                   # the count launches (min_weight, cursor) alone
        assert volume.mesh_counts() == (0, 0) and volume.count() == 0
    data = io.BytesIO()
    assert volume.save_mesh_ply(data) == (0, 0) and mref.parse_mesh_ply(data.getvalue())[0].shape == (0, 6)
    with pytest.raises(RuntimeError, match="CPU fallback"):
        tf.SparseTSDFVolume(origin=(0, 0, 0), dims=(8, 8, 8), voxel_size=0.1, device="cpu")
