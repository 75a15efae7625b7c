"""The mesh of the block-sparse TSDF volume without a device: the two C entries' declarations and argument checks, the runner's
`sparse_mesh` key, and the preconditions of the cases of test_gpu_tsdf_sparse_mesh.py, proven on the numpy restatement - the pattern
volumes put every (owner mask, edge type) pair on a vertex whose owner lies in the next BLOCK, and the noise volumes with blocks missing
still give a large mesh."""
import ctypes
import os
import re

import numpy as np
import pytest

import tsdf_mesh_ref as mref
import tsdf_sparse_mesh_ref as smref
import tsdf_sparse_ref as sref
from monorec_amd import _lib, tsdf_fusion as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mr_tsdf_sparse_mesh_vertices_f32", "mr_tsdf_sparse_mesh_triangles_f32"]


# ------------------------------------------------------------------------------------------ the C entries
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib.ABI and hasattr(hip_lib, name)
        assert any(f"`{name}`" in line for line in table), name
    assert [len(_lib.ABI[n][1]) for n in ENTRIES] == [17, 14]
    for name in ENTRIES:                                                      # the header's parameter lists have as many entries
        params = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(params.split(",")) == len(_lib.ABI[name][1]), name
    # the tetrahedron tables are stated once, in the header both mesh sources include
    csrc = os.path.join(ROOT, "monorec_amd", "csrc")
    stated = [name for name in sorted(os.listdir(csrc)) if re.search(r"TET_CASES\[16\]\s*=", open(os.path.join(csrc, name)).read())]
    assert stated == ["tsdf_mesh.h"]
    for source in ("tsdf_fusion.hip", "tsdf_sparse.hip"):
        assert '#include "tsdf_mesh.h"' in open(os.path.join(csrc, source)).read()


def test_entries_reject_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    table, tsdf, weight, colour, slots, cursor, out, vbase = (base + 4096 * i for i in range(8))
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan = float("nan")

    def vertices(tb=table, nbx=2, nby=2, nbz=1, t=tsdf, w=weight, c=colour, bos=slots, used=2, o=origin, voxel=0.1, min_weight=0.0, r=out, cap=16,
                 vb=vbase, cur=cursor):
        return hip_lib.mr_tsdf_sparse_mesh_vertices_f32(tb, nbx, nby, nbz, t, w, c, bos, used, o, voxel, min_weight, r, cap, vb, cur, None)

    def triangles(tb=table, nbx=2, nby=2, nbz=1, t=tsdf, w=weight, bos=slots, used=2, min_weight=0.0, vb=vbase, r=out, cap=16, cur=cursor):
        return hip_lib.mr_tsdf_sparse_mesh_triangles_f32(tb, nbx, nby, nbz, t, w, bos, used, min_weight, vb, r, cap, cur, None)

    # the table, pool and alignment cases of mr_tsdf_sparse_extract_f32 (tests/test_tsdf_sparse.py)
    shared = [dict(tb=None), dict(t=None), dict(w=None), dict(nbx=0), dict(nby=-1), dict(nbz=0), dict(tb=table + 2), dict(t=tsdf + 4), dict(t=tsdf + 8),
              dict(w=weight + 4), dict(w=weight + 8), dict(nbx=1 << 16, nby=1 << 15, nbz=1), dict(nbx=1 << 11, nby=1 << 10, nbz=1 << 10),
              dict(nbx=2 ** 31 - 1, nby=2 ** 31 - 1, nbz=2 ** 31 - 1), dict(bos=None), dict(bos=slots + 2), dict(cur=None), dict(cur=cursor + 4)]
    used = [dict(used=-1), dict(used=5), dict(used=1 << 31, nbx=1 << 10, nby=1 << 10, nbz=1 << 10), dict(used=1 << 40)]
    mesh = [dict(min_weight=nan), dict(vb=vbase + 2), dict(vb=vbase + 1), dict(vb=None), dict(cap=-1), dict(r=out + 2), dict(r=None, vb=vbase + 1)]
    for kw in shared + used + mesh:
        assert vertices(**kw) == -1, kw
        assert triangles(**kw) == -1, kw
    for kw in (dict(c=colour + 4), dict(c=colour + 8), dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan)):
        assert vertices(**kw) == -1, kw
    # no slot in use: nothing to launch, and no error - with outputs or counting, with or without vertex_base
    assert vertices(used=0) == 0 and triangles(used=0) == 0
    assert vertices(used=0, r=None, vb=None) == 0 and triangles(used=0, r=None, vb=None) == 0


# ------------------------------------------------------------------------------------------ the runner's key
def test_runner_config_with_sparse_mesh():
    base = {"arch": {"type": "MonoRecModel", "args": {}}, "data_set": {"type": "KittiOdometryDataset", "args": {}}, "max_d": 30}
    keys = set(tf.fusion_settings(base))
    assert set(tf.fusion_settings(dict(base, sparse_volume=True, sparse_mesh=True))) == keys and "sparse_mesh" not in keys
    assert tf.sparse_mesh_setting(base) is False and tf.sparse_mesh_setting(dict(base, sparse_volume=True)) is False
    assert tf.sparse_mesh_setting(dict(base, sparse_volume=True, sparse_mesh=True)) is True
    for bad in ("yes", 1, 0, None, [True]):
        with pytest.raises(ValueError, match="sparse_mesh"):
            tf.run(dict(base, sparse_volume=True, sparse_mesh=bad))
    for config in (dict(base, sparse_mesh=True), dict(base, sparse_volume=False, sparse_mesh=True)):
        with pytest.raises(ValueError, match="sparse_mesh needs sparse_volume"):
            tf.run(config)
    # 200 m x 200 m x 40 m at 0.1 m: the mesh no longer asks for the dense copy, the next check in line speaks
    road = dict(base, sparse_volume=True, bounds=[[0, 0, 0], [200, 200, 40]], voxel_size=0.1, arch={"type": "Other"}, mesh_file_name="mesh.ply")
    with pytest.raises(ValueError, match="MonoRecModel"):
        tf.run(dict(road, sparse_mesh=True))
    for config in (road, dict(road, sparse_mesh=False), dict(road, sparse_render=True)):                 # as before without the key
        with pytest.raises(ValueError, match=r"^monorec_amd.tsdf_fusion: mesh_file_name with sparse_volume.*2008 x 2008 x 408 voxels.*tsdf_max_bytes"):
            tf.run(config)
    # each key lifts its own outputs only
    more = dict(road, render_dir="renders", fused_metrics=["abs_rel_sparse_onlyvalid_metric"])
    with pytest.raises(ValueError, match=r"^monorec_amd.tsdf_fusion: render_dir, fused_metrics with sparse_volume need"):
        tf.run(dict(more, sparse_mesh=True))
    with pytest.raises(ValueError, match="MonoRecModel"):
        tf.run(dict(more, sparse_mesh=True, sparse_render=True))


# ------------------------------------------------------------------------------------------ the GPU cases' preconditions
@pytest.mark.parametrize("axis", smref.AXES)
def test_the_pattern_volumes_put_every_owner_mask_across_a_block_face(axis):
    """The four volumes of an axis together: all 3 x 64 (owner mask, edge type) pairs on vertices whose owner lies in the next block
    along it than the base voxel of the triangle's cube - ranked with a mask from the second halo layer and a vertex_base from another
    slot."""
    pairs = set()
    for seam in smref.SEAMS:
        for background in smref.BACKGROUNDS:
            vol = smref.pattern(axis, seam, background)
            assert sorted(vol["dims"]) == [16, 56, 56] and vol["dims"][axis] == 16 and vol["allocated"].all() and vol["allocated"].size == 98
            result, _ = smref.mesh(vol)
            pairs |= {p for p in mref.seam_pairs(vol, result, tile=(8, 8, 8)) if p[0] == axis}
    assert len(pairs) == mref.SEAM_PAIRS == 192


def test_dropping_the_positive_blocks_cuts_the_pattern_mesh():
    vol = smref.positive_dropped(0)
    whole, _ = smref.mesh(smref.pattern(0, 8, 1))
    cut, _ = smref.mesh(vol)
    assert (int(vol["allocated"].sum()), vol["allocated"].size) == (36, 98)
    assert (len(cut["triangles"]), len(whole["triangles"])) == (16264, 22088)


@pytest.mark.parametrize("seed", sorted(smref.NOISE_SEEDS))
def test_the_noise_volumes_keep_a_large_mesh_with_blocks_missing(seed):
    vol = smref.noise(seed)
    full, _ = smref.mesh(smref.all_blocks(mref.noise_volume(smref.NOISE_DIMS, seed)))
    got, _ = smref.mesh(vol)
    kept = int(vol["allocated"].sum())
    assert 10 <= kept <= 20 and vol["allocated"].size == 27
    assert 10000 < len(got["triangles"]) < len(full["triangles"]) and len(got["vertices"]) > 10000
    assert mref.topology(got["triangles"])["repeated"] == []
    if seed == 3:
        assert (kept, len(got["vertices"]), len(got["triangles"]), len(full["triangles"])) == (16, 20049, 31155, 59185)
    low, _ = smref.mesh(vol, 1.0)                                             # weights are 0 .. 3: min_weight 1 leaves a smaller mesh
    assert 1000 < len(low["triangles"]) < len(got["triangles"])


def test_a_removed_block_opens_the_sphere_only_round_itself():
    vol = smref.sphere()
    closed, _ = smref.mesh(vol)
    topo = mref.topology(closed["triangles"])
    assert topo["open"] == [] and topo["repeated"] == [] and topo["V"] - topo["E"] + topo["F"] == 2
    block = smref.surface_block(vol)
    cut, _ = smref.mesh(smref.without_blocks(vol, [block]))
    topo = mref.topology(cut["triangles"])
    assert topo["repeated"] == [] and 0 < len(topo["open"]) and 0 < len(cut["triangles"]) < len(closed["triangles"])
    # every triangle the cut removed belonged to a cube with a corner in the block
    assert _triangle_ids(cut) <= _triangle_ids(closed)
    gone = np.asarray(sorted(_triangle_ids(closed) - _triangle_ids(cut)))
    assert len(gone) == len(closed["triangles"]) - len(cut["triangles"])
    assert smref.cube_touches_block(gone[:, :3], block).all()


def _triangle_ids(result):
    """The set of (cube x y z, tetrahedron, the three vertex keys) over the triangles: a triangle's identity across two meshes."""
    ids = np.concatenate([result["cubes"], result["tets"][:, None], result["keys"][result["triangles"]].reshape(-1, 12)], axis=1)
    return set(map(tuple, ids.tolist()))
