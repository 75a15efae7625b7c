"""The block-sparse TSDF volume without a device: the C entries' declarations and argument checks, the block rounding and the budget of
`SparseTSDFVolume`, the runner's `sparse_volume` key, and self-checks of the numpy restatement the GPU tests compare against."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tsdf_fusion_ref as ref
import tsdf_sparse_ref as sref
from monorec_amd import _lib, tsdf_fusion as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mr_tsdf_sparse_integrate_f32", "mr_tsdf_sparse_extract_f32", "mr_tsdf_sparse_gather_f32")


# ------------------------------------------------------------------------------------------ C entries
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib.ABI and hasattr(hip_lib, name)
        assert any(f"`{name}`" in line for line in table), name
    assert [len(_lib.ABI[n][1]) for n in ENTRIES] == [19, 16, 17]
    for name in ENTRIES:                                                      # the header's parameter lists have as many entries
        params = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(params.split(",")) == len(_lib.ABI[name][1]), name
    assert int(re.search(r"#define MR_TSDF_BLOCK (\d+)", header).group(1)) == _lib.MR_TSDF_BLOCK == tf.BLOCK == sref.B == 8
    assert ("tsdf_sparse.hip", ["-ffp-contract=off"]) in __import__("monorec_amd.build", fromlist=["SOURCES"]).SOURCES


def test_entries_reject_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    table, tsdf, weight, colour, slots, cursor, depth, image, records, out_t, out_w, out_c = (base + 4096 * i for i in range(12))
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

    def integrate(tb=table, nbx=2, nby=2, nbz=1, t=tsdf, w=weight, c=colour, bos=slots, cap=4, cur=cursor, o=origin, voxel=0.1, trunc=0.5,
                  limit=inf, frames="one", n=1, hh=24, ww=40):
        return hip_lib.mr_tsdf_sparse_integrate_f32(tb, nbx, nby, nbz, t, w, c, bos, cap, cur, o, voxel, trunc, limit,
                                                    views(n) if frames == "one" else frames, n, hh, ww, None)

    def extract(tb=table, nbx=2, nby=2, nbz=1, t=tsdf, w=weight, c=colour, bos=slots, used=2, o=origin, voxel=0.1, min_weight=0.0, r=records,
                cap=16, cur=cursor):
        return hip_lib.mr_tsdf_sparse_extract_f32(tb, nbx, nby, nbz, t, w, c, bos, used, o, voxel, min_weight, r, cap, cur, None)

    def gather(tb=table, nbx=2, nby=2, nbz=1, t=tsdf, w=weight, c=colour, x0=0, y0=0, z0=0, dx=16, dy=16, dz=8, ot=out_t, ow=out_w, oc=out_c):
        return hip_lib.mr_tsdf_sparse_gather_f32(tb, nbx, nby, nbz, t, w, c, x0, y0, z0, dx, dy, dz, ot, ow, oc, None)

    # the table and the pool: every entry
    shared = [dict(tb=None), dict(t=None), dict(w=None), dict(nbx=0), dict(nby=-1), dict(nbz=0), dict(tb=table + 2), dict(t=tsdf + 4), dict(t=tsdf + 8),
              dict(w=weight + 4), dict(c=colour + 4), dict(c=colour + 8), dict(nbx=1 << 16, nby=1 << 15, nbz=1), dict(nbx=1 << 11, nby=1 << 10, nbz=1 << 10),
              dict(nbx=2 ** 31 - 1, nby=2 ** 31 - 1, nbz=2 ** 31 - 1)]
    for kw in shared:
        assert integrate(**kw) == -1, ("integrate", kw)
        assert extract(**kw) == -1, ("extract", kw)
        assert gather(**kw) == -1, ("gather", kw)
    # integrate: what is new, then every case of the dense entry
    for kw in [dict(bos=None), dict(cur=None), dict(bos=slots + 2), dict(cur=cursor + 4), dict(cap=0), dict(cap=-3), dict(cap=1 << 31), dict(cap=1 << 40),
               dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan),
               dict(limit=nan), dict(frames=None), dict(n=0), dict(n=9), dict(n=-1), dict(hh=0), dict(ww=-2),
               dict(frames=views(1, depth_p=None)), dict(frames=views(1, image_p=None)), dict(frames=views(3, image_p=None), n=3)]:
        assert integrate(**kw) == -1, ("integrate", kw)
    for kw in [dict(bos=None), dict(cur=None), dict(bos=slots + 2), dict(cur=cursor + 4), dict(used=-1), dict(used=5), dict(o=None), dict(voxel=0.0),
               dict(voxel=nan), dict(min_weight=nan), dict(cap=-1), dict(r=records + 2)]:
        assert extract(**kw) == -1, ("extract", kw)
    for kw in [dict(ot=None), dict(ow=None), dict(c=None), dict(ot=out_t + 2), dict(ow=out_w + 1), dict(oc=out_c + 2), dict(x0=-1), dict(z0=-8),
               dict(dx=0), dict(dy=-1), dict(dz=0), dict(dx=17), dict(x0=1), dict(y0=9, dy=8), dict(z0=1, dz=8)]:
        assert gather(**kw) == -1, ("gather", kw)
    # no slot in use: nothing to launch, and not an error
    assert extract(used=0) == 0


# ------------------------------------------------------------------------------------------ the class on the host
def test_bounds_are_rounded_up_to_whole_blocks():
    # the constructor sets dims and blocks before it asks for the device; read them off an instance that stopped there
    def built(**kw):
        volume = tf.SparseTSDFVolume.__new__(tf.SparseTSDFVolume)
        with pytest.raises(RuntimeError, match="CPU fallback"):
            volume.__init__(device="cpu", **kw)
        return volume

    v = built(origin=(-1.3, -0.8, 0.9), dims=(45, 27, 42), voxel_size=0.06)
    assert v.blocks == (6, 4, 6) and v.dims == (48, 32, 48) and v.capacity == 144
    assert v.origin == tuple(float(np.float32(x)) for x in (-1.3, -0.8, 0.9))
    v = built(bounds=((0.0, 0.0, 0.0), (1.0, 0.7, 0.1)), voxel_size=0.1, colour=False)
    assert tf.dims_of_bounds(((0.0, 0.0, 0.0), (1.0, 0.7, 0.1)), 0.1) == (11, 8, 2)
    assert v.blocks == (2, 1, 1) and v.dims == (16, 8, 8) and not v.has_colour
    lo, hi = v.bounds
    assert lo == (0.0, 0.0, 0.0) and np.allclose(hi, (1.5, 0.7, 0.7), atol=1e-6)
    v = built(origin=(0, 0, 0), dims=(8, 16, 24), voxel_size=0.5, trunc=1.0)
    assert v.blocks == (1, 2, 3) and v.dims == (8, 16, 24) and v.trunc == 1.0
    for kw in (dict(voxel_size=0.0), dict(trunc=0.0), dict(dims=(8, 8)), dict(dims=(8, 0, 8)), dict(bounds=((0, 0, 0), (1, 1, 1)))):
        with pytest.raises(ValueError):
            tf.SparseTSDFVolume(**{**dict(origin=(0, 0, 0), dims=(8, 8, 8), voxel_size=0.1, device="cpu"), **kw})
    with pytest.raises(ValueError, match="SparseTSDFVolume: give either bounds"):
        tf.SparseTSDFVolume(voxel_size=0.1)


def test_the_budget_covers_table_and_pool():
    slot = 512 * 12 + 4
    assert tf.sparse_bytes((6, 4, 6), 30) == 144 * 4 + 30 * slot and tf.sparse_bytes((6, 4, 6), 30, colour=False) == 144 * 4 + 30 * (512 * 8 + 4)
    geometry = dict(origin=(0, 0, 0), dims=(48, 32, 48), voxel_size=0.06)

    def capacity(**kw):
        volume = tf.SparseTSDFVolume.__new__(tf.SparseTSDFVolume)
        with pytest.raises(RuntimeError, match="CPU fallback"):
            volume.__init__(device="cpu", **{**geometry, **kw})
        return volume.capacity

    assert capacity() == 144                                                  # never more than every block
    assert capacity(max_bytes=144 * 4 + 10 * slot + slot - 1) == 10          # what fits
    assert capacity(max_bytes=144 * 4 + 10 * slot, capacity_blocks=10) == 10
    assert capacity(colour=False, max_bytes=144 * 4 + 3 * (512 * 8 + 4)) == 3
    with pytest.raises(ValueError, match=r"a pool of 11 blocks.*room for 10 blocks"):
        tf.SparseTSDFVolume(max_bytes=144 * 4 + 10 * slot, capacity_blocks=11, **geometry)
    with pytest.raises(ValueError, match=r"at least 1"):
        tf.SparseTSDFVolume(max_bytes=144 * 4 + slot - 1, **geometry)
    with pytest.raises(ValueError, match=r"at least 1"):
        tf.SparseTSDFVolume(capacity_blocks=0, **geometry)
    # a table that alone exceeds the budget names its size: 512 x 512 x 64 blocks are 64 MiB of table
    with pytest.raises(ValueError, match=r"512 x 512 x 64 blocks.*the table alone needs 64\.0 MiB, more than max_bytes = 32\.0 MiB"):
        tf.SparseTSDFVolume(origin=(0, 0, 0), dims=(4096, 4096, 512), voxel_size=0.06, max_bytes=32 << 20)
    with pytest.raises(ValueError, match=r"fewer than 2\^31"):
        tf.SparseTSDFVolume(origin=(0, 0, 0), dims=(1 << 15, 1 << 15, 1 << 13), voxel_size=0.06, max_bytes=1 << 50)
    # the volume of the GPU test: the dense class refuses it, the sparse one is table plus pool
    with pytest.raises(ValueError, match=r"4096 x 4096 x 512 voxels of 0\.06 m need 96\.00 GiB"):
        tf.TSDFVolume(origin=(0, 0, 0), dims=(4096, 4096, 512), voxel_size=0.06)
    assert tf.volume_bytes((4096, 4096, 512)) == 103079215104 and tf.sparse_bytes((512, 512, 64), 256) == (64 << 20) + 256 * slot
    assert capacity(origin=(0, 0, 0), dims=(4096, 4096, 512), capacity_blocks=256) == 256


# ------------------------------------------------------------------------------------------ the runner's config
def test_runner_config_with_sparse_volume():
    base = {"arch": {"type": "MonoRecModel", "args": {}}, "data_set": {"type": "KittiOdometryDataset", "args": {}}, "max_d": 30}
    keys = {"voxel_size", "trunc", "bounds", "max_bytes", "fuse_batch", "file_name", "mesh_file_name", "save_volume", "fused_metrics", "render_dir"}
    assert set(tf.fusion_settings(base)) == keys and set(tf.fusion_settings(dict(base, sparse_volume=True))) == keys
    assert tf.fusion_settings(dict(base, sparse_volume=True)) == tf.fusion_settings(base)
    assert tf.sparse_setting(base) is False and tf.sparse_setting(dict(base, sparse_volume=True)) is True
    with pytest.raises(ValueError, match="sparse_volume"):
        tf.run(dict(base, sparse_volume="yes"))
    # 200 m x 200 m x 40 m at 0.1 m: the dense volume that the mesh, the renders and the score would need does not fit 8 GiB
    road = dict(base, sparse_volume=True, bounds=[[0, 0, 0], [200, 200, 40]], voxel_size=0.1)
    for key, value in (("mesh_file_name", "mesh.ply"), ("render_dir", "renders"), ("fused_metrics", ["abs_rel_sparse_onlyvalid_metric"])):
        with pytest.raises(ValueError, match=rf"{key} with sparse_volume.*2008 x 2008 x 408 voxels.*tsdf_max_bytes"):
            tf.run(dict(road, **{key: value}))                                # before a model or a dataset is built
    # without them, and without sparse_volume, the next check in line speaks: the config gets as far as the model
    with pytest.raises(ValueError, match="MonoRecModel"):
        tf.run(dict(road, arch={"type": "Other"}))
    with pytest.raises(ValueError, match="MonoRecModel"):
        tf.run(dict(road, sparse_volume=False, mesh_file_name="mesh.ply", arch={"type": "Other"}))
    with pytest.raises(ValueError, match="MonoRecModel"):                     # a dense copy that fits is no obstacle
        tf.run(dict(road, bounds=[[0, 0, 0], [20, 20, 4]], mesh_file_name="mesh.ply", arch={"type": "Other"}))


# ------------------------------------------------------------------------------------------ the restatement itself
@functools.lru_cache(maxsize=None)
def _fused(name, batch):
    spec = dict(first=sref.FIRST, second=sref.SECOND, ragged=dict(sref.FIRST, dims=(45, 27, 42)))[name]
    frames = ref.make_frames(sref.K)
    dense = sref.dense(spec, frames)
    rounded = dict(spec, dims=tuple((d + 7) // 8 * 8 for d in spec["dims"]))
    return sref.fuse(rounded, frames, batch), dense


@pytest.mark.parametrize("name,blocks,allocated", [("first", 144, 30), ("second", 384, 47), ("ragged", 144, 30)])
def test_the_allocated_set_is_a_strict_non_empty_subset(name, blocks, allocated):
    for batch in (1, 3, 8):
        sparse, _ = _fused(name, batch)
        assert sparse["allocated"].size == blocks and int(sparse["allocated"].sum()) == allocated
        keep = sref.per_voxel(sparse["allocated"])
        assert np.all(sparse["weight"][~keep] == 0) and np.all(sparse["tsdf"][~keep] == 1) and np.all(sparse["colour"][~keep] == 0)
        assert np.array_equal(sref.any_per_block(sparse["weight"] > 0) | sparse["allocated"], sparse["allocated"])
    assert np.array_equal(_fused(name, 1)[0]["allocated"], _fused(name, 8)[0]["allocated"])   # whatever the launches, the same blocks


def test_every_allocated_voxel_of_the_arc_scene_equals_the_dense_restatement():
    """The arc's frames all see the surface from the start: every block is banded by the first launch that sees it at all, so nothing
    is lost and the allocated blocks equal the dense volume's."""
    for name in ("first", "second"):
        for batch in (1, 3, 8):
            sparse, dense = _fused(name, batch)
            keep = sref.per_voxel(sparse["allocated"])
            assert keep.any() and not keep.all()
            for key in ("tsdf", "weight", "colour"):
                assert np.array_equal(sparse[key][keep], dense[key][keep]), (name, batch, key)
            assert (dense["weight"][~keep] > 0).any()                         # free space the sparse volume does not store


def test_the_sparse_points_are_a_subset_of_the_dense_points():
    for name, points, dense_points in (("first", 2551, 2551), ("second", 3731, 3732)):
        sparse, dense = _fused(name, 3)
        got, want = sref.extract(sparse), ref.extract(dense)
        assert len(got) == points and len(want) == dense_points
        have = {r.tobytes() for r in want}
        assert all(r.tobytes() in have for r in got)                          # (the one missing crosses into a block of free space only)
        assert 0 < len(sref.extract(sparse, 2)) < len(got)


def test_a_block_banded_late_loses_the_free_space_of_earlier_launches():
    eye = np.eye(4, dtype=np.float32)
    image = np.full((24, 40, 3), 100, np.uint8)
    frames = [(eye, np.full((24, 40), cm, np.int16), image) for cm in (300, 300, 200)]
    one_by_one, counts = sref.new_volume(**sref.FIRST), []
    for frame in frames:
        new = sref.integrate_launch(one_by_one, [frame])
        counts.append(int(one_by_one["allocated"].sum()))
    assert counts == [24, 24, 48] and int(new.sum()) == 24
    late = sref.per_voxel(new)
    dense = sref.dense(sref.FIRST, frames)
    got, want = one_by_one["weight"][late], dense["weight"][late]              # behind the 2 m surface only the first two frames see a voxel
    assert set(np.unique(want)) == {0.0, 2.0, 3.0} and (want == 3).sum() > 1000
    assert np.all(got[want == 3] == 1) and np.all(got[want < 3] == 0)         # weight 1 where a dense volume has 3
    together = sref.fuse(sref.FIRST, frames, 3)                               # one launch: the frames before the banding one count
    assert np.array_equal(together["allocated"], one_by_one["allocated"])
    keep = sref.per_voxel(together["allocated"])
    assert np.array_equal(together["weight"][keep], dense["weight"][keep]) and np.array_equal(together["tsdf"][keep], dense["tsdf"][keep])


def test_blocks_of_and_sparsify_round_trip():
    sparse, dense = _fused("first", 3)
    coords, tsdf, weight, colour = sref.blocks_of(sparse)
    assert coords.shape == (30, 3) and tsdf.shape == weight.shape == (30, 8, 8, 8) and colour.shape == (30, 8, 8, 8, 4)
    index = (coords[:, 2].astype(np.int64) * 4 + coords[:, 1]) * 6 + coords[:, 0]
    assert np.all(np.diff(index) > 0)
    x, y, z = coords[7]
    assert np.array_equal(tsdf[7], sparse["tsdf"][z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8])
    again = sref.sparsify(dense, sparse["allocated"])
    for key in ("tsdf", "weight", "colour"):
        assert np.array_equal(again[key], sparse[key])


# ------------------------------------------------------------------------------------------ the inputs of the culling tests
@functools.lru_cache(maxsize=None)
def _cull_measures(kind, depth, shift):
    """What the restatement and `bounds_from_frusta` say about one set of inputs of test_culls_that_cut, in launches of one frame (a
    larger launch changes these voxels and more: a block allocated at its end keeps every frame's update).  The geometric box of a
    frame is the box of its pyramid out to min(max_depth_m, 327.67) + trunc: no slack, no code under test.  In voxel indices:
    interior  frames whose box has a face strictly inside the table
    faces     (axis, side) where some frame has that face strictly inside the table AND changes a voxel of the face's own layer of
              blocks - a launch box that is one block short there loses that voxel
    outside   how far, in voxels, a changed voxel lies outside its frame's box, at most
    changed   voxels some launch changed; allocated, blocks: the blocks with storage at the end, and all"""
    spec, frames, ks, limit = sref.cull_inputs(kind, depth, shift)
    changed = []
    vol = sref.fuse(spec, frames, 1, colour=False, intrinsics=ks, max_depth_m=limit, changed=changed)
    dims, origin, voxel = np.array(spec["dims"]), np.array(spec["origin"], dtype=np.float64), spec["voxel_size"]
    interior, faces, outside = 0, set(), 0.0
    for (pose, _, _), k, mask in zip(frames, ks, changed):
        lo, hi = tf.bounds_from_frusta([pose], ref.k_matrix(k), ref.CASE_H, ref.CASE_W, min(limit, 327.67) + spec["trunc"], voxel)
        box = ((np.array(lo) - origin) / voxel, (np.array(hi) - origin) / voxel)
        index = np.nonzero(mask)[::-1]                                        # x, y, z of the changed voxels
        inside = False
        for axis in range(3):
            if len(index[axis]):
                outside = max(outside, box[0][axis] - index[axis].min(), index[axis].max() - box[1][axis])
            for side in range(2):
                face = box[side][axis]
                if 0 < face < dims[axis] - 1:
                    inside = True
                    if np.any(index[axis] // sref.B == int(np.floor(face / sref.B))):
                        faces.add((axis, side))
        interior += inside
    return dict(interior=interior, faces=faces, outside=float(outside), changed=int(np.any(changed, axis=0).sum()),
                allocated=int(vol["allocated"].sum()), blocks=vol["allocated"].size)


def test_the_cases_of_the_culling_test_are_sharp():
    """Before a GPU sees them: the inputs of test_culls_that_cut put the faces of the launch box inside the table, with voxels the
    restatement changes right behind them, on every side and under every depth limit."""
    cases = sref.CULL_CASES
    assert len(cases) == 40
    for depth in sref.CULL_DEPTHS:                                            # every value of every axis meets every depth limit
        mine = [c for c in cases if c[1] == depth]
        assert {c[0] for c in mine} == set(ref.CAMERA_KINDS) and {c[2] for c in mine} == set(sref.SHIFTS)
        assert {c[3] for c in mine} == {1, 3, 8} and {c[4] for c in mine} == {True, False}
    for depth in sref.CULL_DEPTHS:
        for shift in sref.SHIFTS:
            group = set()
            for kind in ref.CAMERA_KINDS:
                m = _cull_measures(kind, depth, shift)
                what = (kind, depth, shift, m)
                assert m["outside"] <= sref.B, what                           # the helper itself: nothing changes beyond its frame's pyramid
                assert m["changed"] >= 500 and 0 < m["allocated"] < m["blocks"], what
                if depth is not None:
                    assert m["interior"] >= 7, what
                if kind != "wild":                                            # (wild's launch box is the whole table: its faces prove nothing)
                    group |= m["faces"]
            if depth is not None:
                assert group == {(axis, side) for axis in range(3) for side in range(2)}, (depth, shift, group)
