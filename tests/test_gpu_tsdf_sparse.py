"""The block-sparse TSDF volume on the GPU: SparseTSDFVolume's integrate, extract and gather kernels against the numpy restatement
(tests/tsdf_sparse_ref.py), bit for bit; late allocation, a pool that runs out, a volume the dense class refuses, save / load, the runner."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
import tsdf_sparse_ref as sref
from monorec_amd import synth, tsdf_export as tx, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECS = {"first": sref.FIRST, "second": sref.SECOND}
KMAT = torch.tensor([[sref.K[0], 0.0, sref.K[2]], [0.0, sref.K[1], sref.K[3]], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def _frames():
    return ref.make_frames(sref.K)                      # eleven 24 x 40 frames on the arc; the last one looks away


@functools.lru_cache(maxsize=None)
def _restated(name, batch, colour=True):
    """The restatement after the eleven frames in launches of `batch`.  Shared, never modified."""
    return sref.fuse(SPECS[name], _frames(), batch, colour=colour)


def _volume(spec, colour=True, **kw):
    return tf.SparseTSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], colour=colour,
                               device=DEV, **kw)


def _fuse(volume, frames, batch, ks=None, max_depth_m=None):
    """`ks`: one (fx, fy, cx, cy) per frame; None: sref.K for all."""
    depth = torch.from_numpy(np.stack([f[1] for f in frames])).to(DEV)
    image = torch.from_numpy(np.stack([f[2] for f in frames])).to(DEV)
    poses = torch.from_numpy(np.stack([f[0] for f in frames]))
    kmat = None if ks is None else torch.tensor(np.stack([ref.k_matrix(k) for k in ks]), dtype=torch.float32)
    for lo in range(0, len(frames), batch):
        volume.integrate(depth[lo:lo + batch], image[lo:lo + batch] if volume.has_colour else None, poses[lo:lo + batch],
                         KMAT if ks is None else kmat[lo:lo + batch], max_depth_m)
    return volume


@functools.lru_cache(maxsize=None)
def _fused(name, batch=3, colour=True):
    """The device volume after the same launches.  Shared by the tests that only read it."""
    return _fuse(_volume(SPECS[name], colour), _frames(), batch)


def _assert_not_degenerate(want, points=True):
    allocated = want["allocated"]
    assert allocated.any() and not allocated.all(), "some blocks allocated, some not"
    if points:
        assert len(sref.extract(want)) > 100


def _assert_grids_equal(dense, want, box=None, what=""):
    """The dense volume `dense` against the restatement (or its box (offset, dims) in voxels)."""
    tsdf, weight, colour = dense.grids()
    cut = (slice(None),) * 3 if box is None else tuple(slice(o, o + d) for o, d in zip(box[0][::-1], box[1][::-1]))
    assert np.array_equal(weight, want["weight"][cut]), what
    assert np.array_equal(tsdf, want["tsdf"][cut]), what
    if want["colour"] is None:
        assert colour is None
    else:
        assert np.array_equal(colour, want["colour"][cut]), what


def _assert_table_consistent(volume, want):
    nbx, nby, nbz = volume.blocks
    table = volume.table.cpu().numpy().reshape(nbz, nby, nbx)
    assert np.array_equal(table >= 0, want["allocated"])                      # the blocks with storage are the restatement's
    n = volume.allocated_blocks()
    assert n == int(want["allocated"].sum()) and not volume.overflowed()
    assert np.array_equal(np.sort(table[table >= 0]), np.arange(n))           # the slots: a permutation of 0 .. n - 1
    block_of_slot = volume.block_of_slot[:n].cpu().numpy()
    assert np.array_equal(table.reshape(-1)[block_of_slot], np.arange(n))
    assert volume.bytes_in_use() == 4 * table.size + n * 512 * (12 if volume.has_colour else 8)


# ------------------------------------------------------------------------------------------ 1. integrate
@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("name", ["first", "second"])
def test_integrate_equals_the_restatement(hip_lib, name, batch, colour):
    want = _restated(name, batch, colour)
    _assert_not_degenerate(want)
    assert int(want["allocated"].sum()) == dict(first=30, second=47)[name] and want["allocated"].size == dict(first=144, second=384)[name]
    volume = _fused(name, batch, colour)
    assert volume.frames == 11 and volume.dims == SPECS[name]["dims"]
    _assert_table_consistent(volume, want)
    _assert_grids_equal(volume.to_dense(volume.bounds), want, what=(name, batch, colour))


def test_late_allocation_loses_earlier_launches_and_keeps_earlier_frames(hip_lib):
    eye = np.eye(4, dtype=np.float32)
    image = np.full((24, 40, 3), 100, np.uint8)
    frames = [(eye, np.full((24, 40), cm, np.int16), image) for cm in (300, 300, 200)]
    want, volume, counts = sref.new_volume(**sref.FIRST), _volume(sref.FIRST), []
    for frame in frames:                                                      # three launches of one frame
        new = sref.integrate_launch(want, [frame])
        _fuse(volume, [frame], 1)
        counts.append(volume.allocated_blocks())
        _assert_table_consistent(volume, want)
    assert counts == [24, 24, 48] and int(new.sum()) == 24                    # the blocks round z = 2 m come with the third launch
    dense = sref.dense(sref.FIRST, frames)
    late = sref.per_voxel(new)
    got = volume.to_dense(volume.bounds)
    _assert_grids_equal(got, want)
    weight = got.grids()[1]
    assert (dense["weight"][late] == 3).sum() > 1000 and np.all(weight[late][dense["weight"][late] == 3] == 1)
    # the same three frames in one launch: those blocks have the dense weights
    together = _fuse(_volume(sref.FIRST), frames, 3)
    want3 = sref.fuse(sref.FIRST, frames, 3)
    _assert_table_consistent(together, want3)
    got3 = together.to_dense(together.bounds)
    _assert_grids_equal(got3, want3)
    keep = sref.per_voxel(want3["allocated"])
    assert np.array_equal(got3.grids()[1][keep], dense["weight"][keep]) and np.array_equal(got3.grids()[0][keep], dense["tsdf"][keep])


def _assert_records_equal(volume, want, weights=(0, 1)):
    for min_weight in weights:
        expect = ref.sort_records(sref.extract(want, min_weight))
        assert volume.count(min_weight) == len(expect), min_weight
        assert np.array_equal(ref.sort_records(volume.extract(min_weight).cpu().numpy()), expect), min_weight


@pytest.mark.parametrize("case", sref.CULL_CASES, ids=sref.cull_case_id)
def test_culls_that_cut(hip_lib, case):
    """Neither the planes per block nor the launch's box of blocks may change a result: ref.camera_cases' cameras - inside and round
    the volume, turned any way, poses that are no rotations, principal points outside the image, fy = 4 fx, one K per frame - with a
    depth limit that puts the faces of the box inside the table (test_tsdf_sparse.py proves that on the restatement), round the origin
    and 1.5 km from it, in launches of 1, 3 and 8."""
    kind, depth, shift, batch, colour = case
    spec, frames, ks, limit = sref.cull_inputs(kind, depth, shift)
    want = sref.fuse(spec, frames, batch, colour=colour, intrinsics=ks, max_depth_m=limit)
    _assert_not_degenerate(want, points=False)
    volume = _fuse(_volume(spec, colour), frames, batch, ks, depth)
    assert volume.frames == 8
    _assert_table_consistent(volume, want)
    _assert_grids_equal(volume.to_dense(volume.bounds), want, what=case)
    _assert_records_equal(volume, want)


# ------------------------------------------------------------------------------------------ 2. extract
@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("name", ["first", "second"])
def test_extract_equals_the_dense_extract_and_the_restatement(hip_lib, name, colour):
    want = _restated(name, 3, colour)
    _assert_not_degenerate(want)
    volume = _fused(name, 3, colour)
    dense = volume.to_dense(volume.bounds)
    for min_weight, least in ((0, 2000), (2, 2000)):
        expect = ref.sort_records(sref.extract(want, min_weight))
        assert len(expect) > least
        if colour and min_weight == 0:
            assert len(expect) == dict(first=2551, second=3731)[name]
        got = volume.extract(min_weight)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(expect), 6) and volume.count(min_weight) == len(expect)
        assert np.array_equal(ref.sort_records(got.cpu().numpy()), expect)
        assert np.array_equal(ref.sort_records(dense.extract(min_weight).cpu().numpy()), expect)
    assert volume.count(100) == 0 and tuple(volume.extract(100).shape) == (0, 6)
    data = io.BytesIO()
    assert volume.save_ply(data) == len(sref.extract(want))


def test_extract_with_a_capacity_below_the_count_writes_nothing_beyond_it(hip_lib):
    from monorec_amd import _lib
    volume, want = _fused("first"), _restated("first", 3)
    expect = {r.tobytes() for r in sref.extract(want)}
    count, room = len(expect), 1000
    assert count == 2551
    records = torch.full((count, 6), -7.0, dtype=torch.float32, device=DEV)
    cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().mr_tsdf_sparse_extract_f32(*volume._table_args(), volume.block_of_slot.data_ptr(), volume.allocated_blocks(),
                                                      volume._origin, volume.voxel_size, 0.0, records.data_ptr(), room, cursor.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "mr_tsdf_sparse_extract_f32")
    assert int(cursor.item()) == count                                        # counted whatever the capacity
    got = records.cpu().numpy()
    assert np.all(got[room:] == -7.0)
    written = [r for r in got[:room] if not np.all(r == -7.0)]                # the workgroups' ranges tile 0 .. count: every row below `room` has its record
    assert len(written) == room and all(r.tobytes() in expect for r in written)
    assert len({r.tobytes() for r in written}) == len(written)


def _corner_scene():
    """A dense restatement volume of 3 x 2 x 2 blocks `ref.seam_volume` style: four balls, each with a pole between voxel 7 and 8 (or 15
    and 16) of one axis, so that sign changes sit on the faces between blocks (0,0,0) | (1,0,0) along x, (1,0,0) | (1,1,0) along y,
    (0,1,0) | (0,1,1) along z and (1,1,1) | (2,1,1) along x; tsdf = clip(distance / 3 voxels, -1, 1), weights 3, about one in ten 1, a
    few 0, random colours."""
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


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
def test_extract_across_block_faces_with_a_neighbour_missing(hip_lib, colour, tmp_path):
    full = _corner_scene()
    if not colour:
        full["colour"] = None
    allocated = np.ones((2, 2, 3), bool)
    allocated[1, 1, 2] = allocated[0, 0, 2] = allocated[1, 0, 0] = False      # (bz, by, bx): three of the twelve blocks have no storage
    want = sref.sparsify(full, allocated)
    for min_weight in (0, 2):
        for axis, owners in enumerate(ref.crossing_owners(want, min_weight)):
            face = [slice(None)] * 3
            face[2 - axis] = 7                                                # voxel 7 owns the edge 7 | 8 across the block face
            assert owners[tuple(face)].sum() >= 3, (axis, min_weight)
        lost = ref.crossing_owners(full, min_weight)[0][8:, 8:, 15].sum()     # along x into block (2, 1, 1), which is missing
        assert lost >= 3 and not ref.crossing_owners(want, min_weight)[0][8:, 8:, 15].any()
        assert len(ref.extract(want, min_weight)) <= len(ref.extract(full, min_weight)) - lost
    # through `load`, in an order that is not the table's
    coords, tsdf, weight, rgb = sref.blocks_of(want)
    order = np.random.default_rng(1).permutation(len(coords))
    arrays = dict(blocks=coords[order], tsdf=tsdf[order], weight=weight[order], origin=np.asarray(want["origin"], np.float32),
                  dims=np.asarray(want["dims"], np.int64), voxel_size=want["voxel"], trunc=want["trunc"], frames=np.int64(5))
    if colour:
        arrays["colour"] = rgb[order]
    np.savez(tmp_path / "seams.npz", **arrays)
    volume = tf.SparseTSDFVolume.load(tmp_path / "seams.npz", device=DEV)
    assert volume.allocated_blocks() == 9 and volume.frames == 5 and volume.blocks == (3, 2, 2)
    _assert_table_consistent(volume, want)
    _assert_grids_equal(volume.to_dense(volume.bounds), want)
    for min_weight in (0, 2):
        expect = ref.sort_records(ref.extract(want, min_weight))
        assert len(expect) > 200
        assert np.array_equal(ref.sort_records(volume.extract(min_weight).cpu().numpy()), expect)
        assert np.array_equal(ref.sort_records(volume.to_dense(volume.bounds).extract(min_weight).cpu().numpy()), expect)


# ------------------------------------------------------------------------------------------ 3. gather
def test_gather_of_boxes_off_the_block_grid_and_of_unallocated_space(hip_lib):
    volume, want = _fused("second"), _restated("second", 3)
    _assert_not_degenerate(want)
    for box in (((43, 5, 9), (21, 13, 17)), ((57, 0, 1), (30, 32, 47)), ((0, 7, 30), (128, 2, 8)), ((75, 16, 35), (1, 1, 1))):
        dense = volume.to_dense(offset=box[0], dims=box[1])
        assert dense.dims == box[1] and dense.frames == 11
        assert dense.origin == tuple(float(np.float32(o) + np.float32(i) * np.float32(volume.voxel_size)) for o, i in zip(volume.origin, box[0]))
        _assert_grids_equal(dense, want, box, what=box)
        assert (dense.grids()[1] > 0).any()
    # the same by bounds in metres, and the default: the box of the allocated blocks
    lo = tuple(o + i * volume.voxel_size for o, i in zip(volume.origin, (16, 8, 8)))
    hi = tuple(o + i * volume.voxel_size for o, i in zip(volume.origin, (40, 20, 30)))
    _assert_grids_equal(volume.to_dense((lo, hi)), want, ((16, 8, 8), (25, 13, 23)))
    bz, by, bx = np.nonzero(want["allocated"])
    box = (tuple(8 * int(v.min()) for v in (bx, by, bz)), tuple(8 * int(v.max() - v.min() + 1) for v in (bx, by, bz)))
    assert volume.allocated_box() == box
    _assert_grids_equal(volume.to_dense(), want, box)
    # a box wholly inside blocks without storage
    free = np.argwhere(~want["allocated"])
    bz, by, bx = (int(v) for v in free[len(free) // 2])
    empty = volume.to_dense(offset=(bx * 8 + 1, by * 8 + 2, bz * 8), dims=(7, 5, 8))
    tsdf, weight, colour = empty.grids()
    assert np.all(tsdf == 1) and np.all(weight == 0) and np.all(colour == 0) and empty.count() == 0
    with pytest.raises(ValueError, match="leaves the volume"):
        volume.to_dense(offset=(120, 0, 0), dims=(9, 8, 8))
    with pytest.raises(ValueError, match="GiB"):
        volume.to_dense(volume.bounds, max_bytes=1 << 20)


def test_gather_beyond_one_grid_of_workgroups(hip_lib):
    """Above 65536 workgroups of 256 voxels the gather kernel strides: a box of 263 x 256 x 256 = 17 235 968 voxels (an odd dx under
    the 64-bit i / dx), and one of 256^3 = 16 777 216, the last size that does not.  Eight blocks, the table's first and last among
    them; everything else reads as the empty state."""
    dims = (264, 256, 256)
    volume = tf.SparseTSDFVolume(origin=(-0.3, 0.2, 1.0), dims=dims, voxel_size=0.06, trunc=0.18, device=DEV, capacity_blocks=8)
    nbx, nby, nbz = volume.blocks
    assert (nbx, nby, nbz) == (33, 32, 32)
    rng = np.random.default_rng(11)
    index = np.concatenate([[0, nbx * nby * nbz - 1], rng.choice(np.arange(1, nbx * nby * nbz - 1), size=6, replace=False)])
    coords = volume._block_coords(index)
    assert (coords[:, 0] == 0).any() and (coords[:, 0] == 32).any() and len(np.unique(index)) == 8     # blocks that each box cuts or leaves out
    tsdf = rng.uniform(-1, 1, size=(8, 8, 8, 8)).astype(np.float32)
    weight = rng.integers(0, 5, size=(8, 8, 8, 8)).astype(np.float32)
    colour = rng.integers(0, 256, size=(8, 8, 8, 8, 4)).astype(np.uint8)
    colour[..., 3] = 0
    volume.set_blocks(coords, tsdf, weight, colour)
    want_t, want_w = np.ones(dims[::-1], np.float32), np.zeros(dims[::-1], np.float32)
    want_c = np.zeros(dims[::-1] + (4,), np.uint8)
    for (bx, by, bz), t, w, c in zip(coords, tsdf, weight, colour):
        cut = (slice(bz * 8, bz * 8 + 8), slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
        want_t[cut], want_w[cut], want_c[cut] = t, w, c
    for offset, size in (((1, 0, 0), (263, 256, 256)), ((0, 0, 0), (256, 256, 256))):
        assert (size[0] * size[1] * size[2] > 65536 * 256) == (offset[0] == 1)
        dense = volume.to_dense(offset=offset, dims=size)
        got_t, got_w, got_c = dense.grids()
        cut = tuple(slice(o, o + d) for o, d in zip(offset[::-1], size[::-1]))
        assert got_t.shape == size[::-1] and (want_w[cut] > 0).sum() > 1000
        assert np.array_equal(got_w, want_w[cut]) and np.array_equal(got_t, want_t[cut]) and np.array_equal(got_c, want_c[cut])
        del dense, got_t, got_w, got_c


# ------------------------------------------------------------------------------------------ 4. a pool that runs out
def test_a_full_pool_drops_blocks_and_writes_nothing_out_of_bounds(hip_lib):
    want = _restated("first", 3)
    assert int(want["allocated"].sum()) == 30
    volume = _volume(sref.FIRST, capacity_blocks=8)
    n, guard = 8 * 512, 1024
    # the pool arrays inside larger buffers, guard words behind them
    tsdf = torch.full((n + guard,), -123.0, dtype=torch.float32, device=DEV)
    weight = torch.full((n + guard,), -123.0, dtype=torch.float32, device=DEV)
    colour = torch.full((n + guard, 4), 0x5A, dtype=torch.uint8, device=DEV)
    slots = torch.full((8 + guard,), -77, dtype=torch.int32, device=DEV)
    volume.tsdf, volume.weight, volume.colour, volume.block_of_slot = tsdf[:n], weight[:n], colour[:n], slots[:8]
    _fuse(volume, _frames(), 3)
    assert volume.overflowed() and volume.allocated_blocks() == 8 and int(volume.cursor.item()) > 8
    assert torch.all(tsdf[n:] == -123.0) and torch.all(weight[n:] == -123.0) and torch.all(colour[n:] == 0x5A) and torch.all(slots[8:] == -77)
    table = volume.table.cpu().numpy()
    assert (table >= 0).sum() == 8 and np.array_equal(np.sort(table[table >= 0]), np.arange(8)) and table.max() == 7
    assert np.array_equal(table[slots[:8].cpu().numpy()], np.arange(8))
    # every stored block is the restatement's: a block gets its slot in the launch that first bands it, or never
    coords, got_t, got_w, got_c = volume.blocks_host()
    assert len(coords) == 8
    for (bx, by, bz), t, w, c in zip(coords, got_t, got_w, got_c):
        cut = (slice(bz * 8, bz * 8 + 8), slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
        assert want["allocated"][bz, by, bx]
        assert np.array_equal(t, want["tsdf"][cut]) and np.array_equal(w, want["weight"][cut]) and np.array_equal(c, want["colour"][cut])
    points = volume.extract().cpu().numpy()
    have = {r.tobytes() for r in sref.extract(want)}
    # which eight blocks found room is unspecified: read them off the table; the points are those of the restatement cut down to them
    stored = (table >= 0).reshape(want["allocated"].shape)
    assert stored.sum() == 8 and not (stored & ~want["allocated"]).any()
    assert np.array_equal(ref.sort_records(points), ref.sort_records(ref.extract(sref.sparsify(want, stored))))
    assert 0 < len(points) < len(have)


def test_reset_and_reuse(hip_lib):
    """`reset()` clears the table and the cursor alone.  The second content allocates fewer blocks than the first, so the first's
    block_of_slot entries and pool data lie beyond the new count - and must stay out of every result."""
    volume = _fuse(_volume(sref.SECOND), _frames(), 3)
    first = _restated("second", 3)
    _assert_table_consistent(volume, first)
    volume.reset()
    assert volume.allocated_blocks() == 0 and volume.count() == 0 and volume.frames == 0 and not volume.overflowed()
    assert tuple(volume.extract().shape) == (0, 6) and bool((volume.table == -1).all())
    # the rigid case with a 2 m limit: its first two frames alone band 20 blocks, fewer than the arc's 47
    spec, frames, ks, limit = sref.cull_inputs("rigid", 2.0, "origin")
    assert spec == sref.SECOND
    for count, batch in ((2, 1), (8, 3)):                                     # ... and then all eight: 139 blocks, past the stale ones again
        want = sref.fuse(spec, frames[:count], batch, intrinsics=ks[:count], max_depth_m=limit)
        _assert_not_degenerate(want)
        assert int(want["allocated"].sum()) == {2: 20, 8: 139}[count] and int(first["allocated"].sum()) == 47
        _fuse(volume, frames[:count], batch, ks[:count], limit)
        assert volume.frames == count
        _assert_table_consistent(volume, want)
        _assert_grids_equal(volume.to_dense(volume.bounds), want)
        _assert_records_equal(volume, want)
        volume.reset()
    assert volume.allocated_blocks() == 0 and volume.count() == 0 and volume.frames == 0


# ------------------------------------------------------------------------------------------ 5. a volume the dense class refuses
def test_a_volume_the_dense_class_refuses(hip_lib):
    offset = (2048, 2048, 232)
    spec = dict(sref.FIRST, origin=tuple(o - i * sref.FIRST["voxel_size"] for o, i in zip(sref.FIRST["origin"], offset)))
    big = dict(origin=spec["origin"], dims=(4096, 4096, 512), voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV)
    with pytest.raises(ValueError, match=r"4096 x 4096 x 512 voxels of 0\.06 m need 96\.00 GiB"):
        tf.TSDFVolume(**big)
    volume = tf.SparseTSDFVolume(capacity_blocks=256, **big)
    assert volume.blocks == (512, 512, 64) and volume.table.numel() * 4 == 64 << 20
    _fuse(volume, _frames(), 3)
    want = sref.fuse(dict(spec, offset=offset), _frames(), 3)                 # the restatement of the sub-box alone: blocks do not depend on each other
    _assert_not_degenerate(want)
    allocated = volume.allocated_blocks()
    assert not volume.overflowed() and int(want["allocated"].sum()) <= allocated < 256
    # memory: the table, and exactly 512 x 12 bytes per allocated block, against 103 GB dense
    assert volume.bytes_in_use() == (64 << 20) + allocated * 512 * 12 < tf.volume_bytes(volume.dims) // 1000
    assert tf.sparse_bytes(volume.blocks, volume.capacity) == (64 << 20) + 256 * (512 * 12 + 4)
    dense = volume.to_dense(offset=offset, dims=spec["dims"])
    _assert_grids_equal(dense, want)
    table = volume.table.reshape(64, 512, 512)[29:35, 256:260, 256:262].cpu().numpy()
    assert np.array_equal(table >= 0, want["allocated"])
    # the surface points of the sub-box: the sparse extract places them where the restatement does
    expect = sref.extract(want)
    got = volume.extract().cpu().numpy()
    assert len(got) >= len(expect) > 2000
    have = {r.tobytes() for r in got}
    assert all(r.tobytes() in have for r in expect)                           # (the volume has more: the scene goes on beyond the sub-box)


# ------------------------------------------------------------------------------------------ 6. save / load
def test_save_and_load_round_trip(hip_lib, tmp_path):
    volume, want = _fused("first"), _restated("first", 3)
    volume.save(tmp_path / "sparse.npz")
    with np.load(tmp_path / "sparse.npz") as z:
        saved = {k: z[k] for k in z.files}
    coords, tsdf, weight, colour = sref.blocks_of(want)                       # the table's order, whatever the slots were
    assert np.array_equal(saved["blocks"], coords) and saved["blocks"].dtype == np.int32 and saved["tsdf"].shape == (30, 8, 8, 8)
    assert np.array_equal(saved["tsdf"], tsdf) and np.array_equal(saved["weight"], weight) and np.array_equal(saved["colour"], colour)
    assert tuple(saved["dims"]) == (48, 32, 48) and int(saved["frames"]) == 11 and saved["colour"].shape == (30, 8, 8, 8, 4)
    again = tf.SparseTSDFVolume.load(tmp_path / "sparse.npz", device=DEV, capacity_blocks=40)
    assert again.capacity == 40 and again.frames == 11 and again.origin == volume.origin and again.trunc == volume.trunc
    _assert_table_consistent(again, want)
    _assert_grids_equal(again.to_dense(again.bounds), want)
    assert np.array_equal(ref.sort_records(again.extract().cpu().numpy()), ref.sort_records(volume.extract().cpu().numpy()))
    # and it goes on integrating: one more frame into both
    _fuse(again, _frames()[:1], 1)
    more = sref.fuse(sref.FIRST, _frames(), 3)
    sref.integrate_launch(more, _frames()[:1])
    _assert_grids_equal(again.to_dense(again.bounds), more)
    with pytest.raises(ValueError, match="pool of 20"):
        tf.SparseTSDFVolume.load(tmp_path / "sparse.npz", device=DEV, capacity_blocks=20)
    plain = _fused("first", 3, False)
    data = io.BytesIO()
    plain.save(data)
    data.seek(0)
    back = tf.SparseTSDFVolume.load(data, device=DEV)
    assert back.colour is None and not back.has_colour
    _assert_grids_equal(back.to_dense(back.bounds), _restated("first", 3, False))


def test_cpu_tensors_raise(hip_lib):
    volume = _volume(sref.FIRST)
    pose, depth, image = _frames()[0]
    with pytest.raises(RuntimeError):
        volume.integrate(torch.from_numpy(depth), torch.from_numpy(image), pose, KMAT)
    assert volume.allocated_blocks() == 0 and volume.count() == 0 and tuple(volume.extract().shape) == (0, 6)
    with pytest.raises(ValueError, match="no block is allocated"):
        volume.to_dense()


# ------------------------------------------------------------------------------------------ 7. the runner
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
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    return dict({"name": "sparse TSDF fusion", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": KEYFRAMES, "min_d": 3, "max_d": 30,
                 "use_mask": False, "output_dir": str(out_dir), "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": 1, "sparse_volume": True,
                 "file_name": "surface.ply", "save_volume": os.path.join(str(out_dir), "volume.npz"),
                 "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": STEPS}},
                 "data_set": {"type": "KittiOdometryDataset", "args": args}}, **more)


def _by_hand(config, model, origin, dims):
    """model(data) -> pack_frames -> integrate, one keyframe per launch with owned outputs, into a SparseTSDFVolume of the runner's geometry."""
    from monorec_amd import kitti
    dataset = kitti.KittiOdometryDataset(**dict(config["data_set"]["args"], device=DEV))
    loader = kitti.DeviceLoader(dataset, batch_size=1, start=config["start"], end=config["end"])
    volume = tf.SparseTSDFVolume(origin=origin, dims=dims, voxel_size=config["voxel_size"], trunc=config["voxel_size"] * config["trunc_voxels"],
                                 device=DEV)
    crop = config["roi"]
    with torch.no_grad():
        for data, _ in loader:
            out = model(data)
            k = data["keyframe_intrinsics"][0].clone()
            k[0, 2] -= crop[2]
            k[1, 2] -= crop[0]
            depth, colour, _ = tx.pack_frames(out["result"].clone(), data["keyframe"].clone(), crop, config["min_d"], config["max_d"])
            volume.integrate(depth[0], colour[0], data["keyframe_pose"][0], k)
    dataset.close()
    return volume


def test_runner_with_sparse_volume_equals_fusing_by_hand(tree, model, tmp_path):
    config = _config(tree, tmp_path)
    count = tf.run(config, model=model)
    with np.load(config["save_volume"]) as z:
        saved = {k: z[k] for k in z.files}
    assert int(saved["frames"]) == KEYFRAMES and all(int(d) % 8 == 0 for d in saved["dims"])
    blocks_total = int(np.prod(saved["dims"] // 8))
    assert 0 < len(saved["blocks"]) < blocks_total and count > 100            # some blocks allocated, some not, and some points
    volume = _by_hand(config, model, saved["origin"], saved["dims"])
    coords, tsdf, weight, colour = volume.blocks_host()
    assert np.array_equal(saved["blocks"], coords) and np.array_equal(saved["weight"], weight) and np.array_equal(saved["tsdf"], tsdf)
    assert np.array_equal(saved["colour"], colour)
    data = open(tmp_path / "surface.ply", "rb").read()
    head, body = data[:data.index(b"end_header\n")].decode().split("\n"), data[data.index(b"end_header\n") + len(b"end_header\n"):]
    assert head[2] == f"element vertex {count}" and len(body) == 24 * count
    assert np.array_equal(ref.sort_records(np.frombuffer(body, "<f4")), ref.sort_records(volume.extract().cpu().numpy()))
    assert np.array_equal(ref.sort_records(np.frombuffer(body, "<f4")), ref.sort_records(volume.to_dense(volume.bounds).extract().cpu().numpy()))
    # the mesh goes through the whole volume gathered into a dense one: its vertices on the axis edges are these points
    fusion = tf.Fusion(dict(config, mesh_file_name="mesh.ply", save_volume=None), model=model).fuse()
    assert fusion.write() == count and fusion.mesh_counts[0] >= count and fusion.mesh_counts[1] > 0
    assert fusion.dense().dims == tuple(int(d) for d in saved["dims"]) and fusion.volume.allocated_blocks() == len(coords)
    # a pool that runs out raises after the loop and names the key
    with pytest.raises(RuntimeError, match=r"pool of \d+ blocks.*ran out.*tsdf_max_bytes"):
        tf.run(dict(config, tsdf_max_bytes=4 * blocks_total + 3 * (512 * 12 + 4)), model=model)
