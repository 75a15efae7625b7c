"""The TSDF mesh without a device: the two C entries' declarations and argument checks, the mesh .ply writer, and the numpy
restatement of the marching-tetrahedra rules (tests/tsdf_mesh_ref.py) held against what they promise - a closed, outward-wound
2-manifold on a closed surface, open only where voxels are unseen, with `extract`'s points on the axis edges."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import tsdf_fusion_ref as ref
import tsdf_mesh_ref as mref
from monorec_amd import _lib, pointcloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mr_tsdf_mesh_vertices_f32", "mr_tsdf_mesh_triangles_f32")


# ------------------------------------------------------------------------------------------ C entries
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib.ABI and hasattr(hip_lib, name)
        assert any(f"`{name}`" in line for line in table), name
    assert [len(_lib.ABI[n][1]) for n in ENTRIES] == [14, 11]
    assert "within ABI 24" in header


def test_entries_reject_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    tsdf, weight, colour, out, vbase, cursor = (base + 4096 * i for i in range(6))
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan = float("nan")

    def vertices(t=tsdf, w=weight, c=colour, nx=8, ny=4, nz=2, o=origin, voxel=0.1, min_weight=0.0, r=out, cap=16, vb=vbase, cur=cursor):
        return hip_lib.mr_tsdf_mesh_vertices_f32(t, w, c, nx, ny, nz, o, voxel, min_weight, r, cap, vb, cur, None)

    def triangles(t=tsdf, w=weight, nx=8, ny=4, nz=2, min_weight=0.0, vb=vbase, r=out, cap=16, cur=cursor):
        return hip_lib.mr_tsdf_mesh_triangles_f32(t, w, nx, ny, nz, min_weight, vb, r, cap, cur, None)

    huge = [dict(nx=1 << 20, ny=1 << 20, nz=1), dict(nx=1 << 14, ny=1 << 13, nz=1 << 13), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)]
    int32 = [dict(nx=2048, ny=1024, nz=1024), dict(nx=1 << 16, ny=1 << 15, nz=1), dict(nx=2048, ny=1024, nz=1028)]    # 2^31 voxels and beyond
    volume = [dict(t=None), dict(w=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(t=tsdf + 2), dict(w=weight + 1)] + huge + int32
    shared = [dict(min_weight=nan), dict(cur=None), dict(cur=cursor + 4), dict(cap=-1), dict(r=out + 2), dict(vb=vbase + 2), dict(vb=None),
              dict(r=None, vb=vbase + 1)]
    for kw in volume + shared:
        assert vertices(**kw) == -1, ("vertices", kw)
        assert triangles(**kw) == -1, ("triangles", kw)
    for kw in [dict(c=colour + 2), dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan)]:
        assert vertices(**kw) == -1, ("vertices", kw)
    assert b"argument" in hip_lib.mr_error_string(-1).lower()


# ------------------------------------------------------------------------------------------ the file
def test_write_mesh_ply_round_trips():
    rng = np.random.default_rng(5)
    vertices = rng.normal(size=(7, 6)).astype(np.float32)
    triangles = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    for tri in (triangles, triangles.astype(np.int64), np.zeros((0, 3), np.int32)):
        buffer = io.BytesIO()
        pointcloud.write_mesh_ply(buffer, vertices, tri)
        got_v, got_t = mref.parse_mesh_ply(buffer.getvalue())
        assert np.array_equal(got_v, vertices) and np.array_equal(got_t, tri) and got_t.dtype == np.int32
    buffer = io.BytesIO()
    pointcloud.write_mesh_ply(buffer, np.zeros((0, 6), np.float32), np.zeros((0, 3), np.int32))
    assert mref.parse_mesh_ply(buffer.getvalue())[0].shape == (0, 6)
    with pytest.raises(ValueError, match="outside"):
        pointcloud.write_mesh_ply(io.BytesIO(), vertices, np.array([[0, 1, 7]]))


# ------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def sphere():
    vol = mref.sphere_volume(**mref.SPHERE_VOLUME)
    return vol, mref.mesh(vol)


def test_the_case_table_is_complete_and_complementary():
    """Every case uses exactly the edges between an inside and an outside corner, and the complement of a case is its mirror image."""
    for case, tris in mref.CASES.items():
        inside = [i for i in range(4) if case >> i & 1]
        crossing = {e for e, (p, q) in enumerate(mref.TET_EDGES) if (p in inside) != (q in inside)}
        assert {e for tri in tris for e in tri} == crossing and len(tris) == (0, 1, 2, 1, 0)[len(inside)]
        assert len(mref.CASES[15 - case]) == len(tris)
        directed = {(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)}
        mirrored = {(t[(k + 1) % 3], t[k]) for t in mref.CASES[15 - case] for k in range(3)}
        if len(tris) == 1:
            assert directed == mirrored
        elif tris:                                             # the outlines of the two quads are opposite; the diagonals may differ
            outline = lambda d: {e for e in d if (e[1], e[0]) not in d}
            assert outline(directed) == outline(mirrored) and len(outline(directed)) == 4


def test_the_closed_sphere_is_a_closed_outward_manifold(sphere):
    vol, got = sphere
    nx, ny, nz = vol["dims"]
    assert nx > 32 and ny > 8 and nz > 4                                   # more than one workgroup tile along every axis
    centre, radius, voxel = np.array(ref.SPHERE[:3]), ref.SPHERE[3], float(vol["voxel"])
    lo = np.array([float(v) for v in vol["origin"]])
    hi = lo + (np.array(vol["dims"]) - 1) * voxel
    assert np.all(centre - radius - voxel >= lo) and np.all(centre + radius + voxel <= hi)
    assert not (vol["tsdf"] == 0).any()
    vertices, triangles, keys = got["vertices"], got["triangles"], got["keys"]
    print(f"sphere: {len(vertices)} vertices ({int((keys[:, 3] < 3).sum())} on axis edges), {len(triangles)} triangles")
    assert len(vertices) > 1000 and len(triangles) > 2000
    topo = mref.topology(triangles)
    assert topo["open"] == [] and topo["repeated"] == [] and topo["V"] == len(vertices)
    assert topo["V"] - topo["E"] + topo["F"] == 2
    p = vertices[:, :3].astype(np.float64)
    a, b, c = (p[triangles[:, k]] for k in range(3))
    normal = np.cross(b - a, c - a)
    assert np.all(np.einsum("ij,ij->i", normal, (a + b + c) / 3 - centre) > 0)
    assert np.abs(np.linalg.norm(p - centre, axis=1) - radius).max() < np.sqrt(3) * voxel
    assert np.array_equal(ref.sort_records(mref.axis_vertices(got)), ref.sort_records(ref.extract(vol)))
    assert vertices[:, 3:].max() > 100                                     # the colours are interpolated, not zero
    # the canonical form does not depend on the order of either array
    rng = np.random.default_rng(0)
    order = rng.permutation(len(vertices))
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    shuffled = np.roll(rank[triangles], 1, axis=1)[rng.permutation(len(triangles))]
    assert np.array_equal(mref.canonical(vertices[order], shuffled), mref.canonical(vertices, triangles))
    assert not np.array_equal(mref.canonical(vertices, triangles[:, ::-1]), mref.canonical(vertices, triangles))      # the winding counts


def test_a_hole_in_the_weights_opens_the_mesh_only_there(sphere):
    vol = mref.with_hole(sphere[0])
    got = mref.mesh(vol)
    topo = mref.topology(got["triangles"])
    assert topo["repeated"] == [] and all(n < 2 for _, _, n in topo["open"])
    assert len(topo["open"]) > 0 and len(got["triangles"]) < len(sphere[1]["triangles"])
    print(f"hole: {len(topo['open'])} edges used once")
    nx, ny, nz = vol["dims"]
    steps = np.array(mref.EDGES)
    for i, j, _ in topo["open"]:
        ends = []
        for x, y, z, e in got["keys"][[i, j]]:
            ends += [(x, y, z), tuple(np.array((x, y, z)) + steps[e])]
        ends = np.array(ends)
        low, high = ends.min(axis=0), ends.max(axis=0)
        assert np.all(high - low <= 1)
        unseen = False
        for base in np.ndindex(*(2 - (high - low))):                       # every cube that holds both grid edges
            b = low - np.array(base) * (1 - (high - low))
            if np.any(b < 0) or np.any(b + 1 >= (nx, ny, nz)):
                continue
            unseen |= bool((vol["weight"][b[2]:b[2] + 2, b[1]:b[1] + 2, b[0]:b[0] + 2] == 0).any())
        assert unseen, (i, j)


@pytest.fixture(scope="module")
def fused():
    """The small volume after the ten frames that see the scene (test_tsdf_fusion.py's fixture)."""
    frames = ref.make_frames(ref.INTRINSICS_60)
    vol = ref.new_volume(**ref.SMALL)
    for pose, depth, colour in frames[:10]:
        ref.integrate(vol, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, colour)
    return vol


@pytest.mark.parametrize("min_weight", [0, 2])
def test_the_fused_volume_meshes_without_a_fin(fused, min_weight):
    got = mref.mesh(fused, min_weight)
    topo = mref.topology(got["triangles"])
    assert len(got["triangles"]) > 0 and topo["repeated"] == [] and all(n <= 2 for _, _, n in topo["open"])
    assert np.array_equal(ref.sort_records(mref.axis_vertices(got)), ref.sort_records(ref.extract(fused, min_weight)))
    assert got["triangles"].max() < len(got["vertices"])


# ------------------------------------------------------------------------------------------ vertices across tile seams
def _older_fixtures():
    """The volumes test_gpu_tsdf_mesh.py meshed before the pattern volumes: both spheres, both fused volumes at min_weight 0 and 2."""
    sphere = mref.sphere_volume(**mref.SPHERE_VOLUME)
    yield sphere, 0
    yield mref.with_hole(sphere), 0
    frames = ref.make_frames(ref.INTRINSICS_60)
    for spec in (ref.SMALL, ref.WIDE):
        vol = ref.new_volume(**spec)
        for i in [0, 10, 1, 2, 3, 4, 5, 6, 7, 8, 9]:
            pose, depth, image = frames[i]
            ref.integrate(vol, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, image)
        yield vol, 0
        yield vol, 2


def _per_axis(pairs):
    return [sum(1 for p in pairs if p[0] == axis) for axis in range(3)]


def test_the_pattern_volumes_reach_every_mask_and_edge_type_across_every_seam():
    """A triangle vertex whose owner lies in the next 32 x 8 x 4 tile is ranked with a mask from the second halo layer of the triangle
    kernel's staged codes and offset by a vertex_base another workgroup wrote; a wrong rank there still gives indices in range.  Per
    axis there are 192 (owner mask, edge type) pairs for such a vertex (mref.seam_pairs).  The spheres and fused volumes the GPU test
    meshed before reach 15 / 53 / 89 of them across the x / y / z seams (the sphere spans x = 14 .. 29 and never touches x = 31 | 32);
    the twelve pattern volumes - all 256 sign patterns of a cube whose base is the first voxel of the second tile, or the last of the
    first, on a background of either sign - reach 192 / 192 / 192."""
    older = set()
    for vol, min_weight in _older_fixtures():
        older |= mref.seam_pairs(vol, mref.mesh(vol, min_weight))
    assert _per_axis(older) == [15, 53, 89]
    for axis, tile in enumerate(mref.TILE):
        reached = set()
        for seam in (tile, tile - 1):
            for background in (1, -1):
                vol = mref.pattern_volume(axis, seam, background)
                assert vol["dims"][axis] == seam + 3 and sorted(vol["dims"])[1:] == [49, 49] and np.prod(vol["dims"]) < 100000
                assert (vol["weight"] > 0).all() and (np.abs(vol["tsdf"]) >= np.float32(0.05)).all()
                got = mref.mesh(vol)
                assert len(got["triangles"]) > 20000 and got["triangles"].max() < len(got["vertices"])
                assert (got["cubes"] >= 0).all() and (got["cubes"] < np.array(vol["dims"]) - 1).all() and set(got["tets"]) == set(range(6))
                reached |= {p for p in mref.seam_pairs(vol, got) if p[0] == axis}
        assert len(reached) == mref.SEAM_PAIRS == 192, (axis, len(reached))
        assert {(m, e) for _, m, e in reached} == {(m, e) for m in range(128) for e in range(7) if m >> e & 1 and not mref.EDGES[e][axis]}


@pytest.mark.parametrize("dims", ref.SEAM_DIMS)
def test_the_noise_volumes_mesh_with_indices_in_range(dims):
    """Independent random signs, a tenth unseen, exact zeros of both signs: nearly every tetrahedron of every cube has a triangle."""
    vol = mref.noise_volume(dims, seed=1)
    assert ((vol["tsdf"] == 0) & np.signbit(vol["tsdf"])).sum() == 8 == ((vol["tsdf"] == 0) & ~np.signbit(vol["tsdf"])).sum()
    assert 0.05 < (vol["weight"] == 0).mean() < 0.15 and set(np.unique(vol["weight"])) == {0.0, 1.0, 2.0, 3.0}
    got = mref.mesh(vol)
    assert len(got["triangles"]) > 1000 and got["triangles"].min() >= 0 and got["triangles"].max() < len(got["vertices"])
    assert np.array_equal(ref.sort_records(mref.axis_vertices(got)), ref.sort_records(ref.extract(vol)))
    # +0 and -0 are outside: next to a positive voxel along x they own no vertex on that edge, next to a seen negative one they do
    zero, seen = (vol["tsdf"] == 0)[:, :, :-1], ((vol["weight"] > 0)[:, :, :-1] & (vol["weight"] > 0)[:, :, 1:])
    owns = (got["masks"][:, :, :-1] & 1) != 0
    assert zero.sum() > 8 and np.array_equal(owns[zero], (seen & (vol["tsdf"][:, :, 1:] < 0))[zero])
