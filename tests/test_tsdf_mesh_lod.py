"""CPU: the restatement of the mesh normals and of the clustered level of detail (tests/tsdf_mesh_lod_ref.py) has the properties the
rules promise, on tiny fields; the argument checks that need no device; the .ply with and without normals."""
import io

import numpy as np
import pytest

import tsdf_mesh_lod_ref as lod
import tsdf_mesh_ref as mref
from monorec_amd import pointcloud, tsdf_fusion as tf

F = np.float32


def _sphere16():
    """A ball of radius 5.7 voxels well inside a 16^3 grid, every voxel seen."""
    vol = lod.field_volume((16, 16, 16), "sphere")
    assert (vol["tsdf"] < 0).any() and (vol["weight"] > 0).all()
    border = np.ones(vol["tsdf"].shape, bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert (vol["tsdf"][border] > 0).all()                                    # fully inside
    return vol


def test_cell_one_is_the_full_mesh():
    vol = lod.field_volume((17, 13, 9), "pockets", seed=3)
    full = mref.mesh(vol, 1.0)
    got = lod.mesh(vol, 1.0, cell=1)
    assert len(full["triangles"]) > 100 and got["normals"] is None and got["clusters"] is None
    assert np.array_equal(mref.canonical(got["vertices"], got["triangles"]), mref.canonical(full["vertices"], full["triangles"]))
    assert lod.same(lod.canonical(got["vertices"], got["triangles"]), lod.canonical(full["vertices"], full["triangles"]))
    with_normals = lod.mesh(vol, 1.0, cell=1, normals=True)
    assert np.array_equal(with_normals["vertices"], full["vertices"]) and with_normals["normals"].shape == (len(full["vertices"]), 3)


@pytest.mark.parametrize("cell", [2, 4, 8])
def test_every_directed_edge_of_a_clustered_sphere_is_matched_by_its_reverse(cell):
    vol = _sphere16()
    full = mref.mesh(vol)
    assert mref.topology(full["triangles"])["open"] == []                     # the full mesh is closed
    got = lod.mesh(vol, cell=cell, normals=True)
    edges = lod.directed_edges(got["triangles"])
    assert len(got["triangles"]) >= 4 and len(got["triangles"]) < len(full["triangles"])
    assert all(edges.get((b, a), 0) == n for (a, b), n in edges.items())
    assert all(a != b for a, b in edges)
    # one vertex per cluster that owns a vertex of the full mesh, counted from the masks alone
    assert len(got["vertices"]) == got["clusters"] == lod.owning_clusters(vol, 0.0, cell) < len(full["vertices"])
    assert got["triangles"].min() >= 0 and got["triangles"].max() < len(got["vertices"])
    lengths = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert np.all((np.abs(lengths - 1) < 1e-6) | (lengths == 0))


@pytest.mark.parametrize("dims,cell", [((17, 13, 9), 2), ((17, 13, 9), 4), ((17, 13, 9), 8), ((16, 16, 16), 4)])
@pytest.mark.parametrize("kind", ["sphere", "plane", "pockets"])
def test_one_vertex_per_cluster_that_owns_one(dims, cell, kind):
    vol = lod.field_volume(dims, kind, seed=1)
    for min_weight in (0.0, 1.0):
        got = lod.mesh(vol, min_weight, cell=cell)
        assert len(got["vertices"]) == got["clusters"] == lod.owning_clusters(vol, min_weight, cell) > 0
        corners = got["triangles"]
        assert np.all((corners[:, 0] != corners[:, 1]) & (corners[:, 1] != corners[:, 2]) & (corners[:, 0] != corners[:, 2]))


def test_normals_of_a_plane_are_its_normal_to_fp32_rounding():
    """tsdf = (N . index - 40) / 64 with N = (2, 3, 6), |N| = 7.  Where both ends of a vertex's edge have all six neighbours in the
    grid, both gradients are 2 N / 64 exactly (differences of multiples of 1 / 64 below 2^24 / 64), m = g_a + s * 0 = g_a exactly, the
    squares and their sums are exact, sqrtf(49 / 1024) = 7 / 32 exactly, and m_i / len is ONE correctly rounded division: the normal
    is within half an ulp of N_i / 7, so within one ulp of its fp32 value.  (At the border of the grid the differences are one-sided
    along some axes and central along others: those normals are not the plane's, by the rule.)"""
    vol = lod.integer_plane((12, 11, 10))
    full = mref.mesh(vol)
    normals = lod.vertex_normals(vol, full)
    keys = full["keys"]
    ends = np.stack([keys[:, :3], keys[:, :3] + np.asarray(mref.EDGES)[keys[:, 3]]])
    inner = np.all((ends >= 1) & (ends <= np.asarray(vol["dims"]) - 2), axis=(0, 2))
    assert inner.sum() > 100 and (~inner).sum() > 10
    want = np.array([2.0, 3.0, 6.0]) / 7.0
    ulp = np.spacing(want.astype(F)).astype(np.float64)
    assert np.all(np.abs(normals[inner].astype(np.float64) - want) <= ulp)
    assert np.array_equal(normals[inner], np.broadcast_to((np.array([2, 3, 6], F) * F(2 / 64)) / F(7 / 32), normals[inner].shape))
    # tsdf grows along N: the normals point where the winding of the triangles does
    tri = full["vertices"][full["triangles"]][:, :, :3].astype(np.float64)
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.all(cross @ want >= -1e-12) and (cross @ want > 0).any()
    # a cluster sums count <= 7 * 8 unit vectors that are all the same u: every partial sum is within count roundings of half an ulp of
    # the running length <= count, the normalisation adds three more - (count + 3) * 2^-24 * count / count per component, relative to 1
    # (a cluster vertex at index 3 or more and dims - 4 or less has members in voxels 2 .. dims - 3 only, with far ends up to dims - 2)
    vol = lod.integer_plane((20, 18, 16), offset=96)
    got = lod.mesh(vol, cell=2, normals=True)
    index = got["vertices"][:, :3] / float(vol["voxel"])
    inner = np.all((index >= 3) & (index <= np.asarray(vol["dims"]) - 4), axis=1)
    assert inner.sum() > 30
    assert np.all(np.abs(got["normals"][inner].astype(np.float64) - want) <= (56 + 3) * 2.0 ** -24)


def test_one_sided_differences_where_a_neighbour_is_unseen_or_outside():
    vol = lod.integer_plane((6, 5, 4))
    vol["weight"][2, 2, 3] = 0
    g = lod.gradients(vol)
    t = vol["tsdf"]
    assert g[0][1, 1, 0] == t[1, 1, 1] - t[1, 1, 0] and g[0][1, 1, 5] == t[1, 1, 5] - t[1, 1, 4]           # outside the grid
    assert g[0][2, 2, 2] == t[2, 2, 2] - t[2, 2, 1] and g[0][2, 2, 4] == t[2, 2, 5] - t[2, 2, 4]           # unseen
    assert g[1][2, 1, 3] == t[2, 1, 3] - t[2, 0, 3] and g[2][1, 2, 3] == t[1, 2, 3] - t[0, 2, 3]
    assert g[0][1, 1, 2] == t[1, 1, 3] - t[1, 1, 1] and g[2][1, 1, 2] == t[2, 1, 2] - t[0, 1, 2]           # central


def test_a_bad_cell_raises_before_anything_else():
    volume = tf.TSDFVolume.__new__(tf.TSDFVolume)                              # no device, no arrays: the check comes first
    for bad in (3, 0, 16, -2, True, 2.5, "4"):
        for call in (lambda: volume.mesh(cell=bad), lambda: volume.mesh_counts(cell=bad), lambda: volume.save_mesh_ply(io.BytesIO(), cell=bad),
                     lambda: tf.SparseTSDFVolume.__new__(tf.SparseTSDFVolume).mesh(0, bad, True)):
            with pytest.raises(ValueError, match=r"must be one of 1, 2, 4, 8"):
                call()
    assert tf.MESH_CELLS == (1, 2, 4, 8) and all(tf.BLOCK % c == 0 for c in tf.MESH_CELLS)
    with pytest.raises(ValueError):
        lod.mesh(lod.integer_plane((4, 4, 4)), cell=3)


def test_runner_keys_are_checked():
    config = {"max_d": 30}
    assert tf.mesh_settings(config) == {} and tf.mesh_settings(dict(config, mesh_cell=1, mesh_normals=False)) == {}
    assert tf.mesh_settings(dict(config, mesh_cell=4, mesh_normals=True)) == {"cell": 4, "normals": True}
    assert tf.fusion_settings(dict(config, mesh_cell=4, mesh_normals=True)) == tf.fusion_settings(config)      # checked there, returned by mesh_settings
    for bad in (3, 0, "2", True, 16):
        with pytest.raises(ValueError, match=r"mesh_cell .* must be one of 1, 2, 4, 8"):
            tf.fusion_settings(dict(config, mesh_cell=bad))
    for bad in (1, 0, "true", None):
        with pytest.raises(ValueError, match=r"mesh_normals .* must be true or false"):
            tf.fusion_settings(dict(config, mesh_normals=bad))


def _tiny_mesh():
    vertices = np.arange(24, dtype=F).reshape(4, 6) * F(0.25) - F(1.5)
    triangles = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    normals = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 0], [0.6, 0, 0.8]], F)
    return vertices, triangles, normals


def test_ply_with_normals_round_trips():
    vertices, triangles, normals = _tiny_mesh()
    data = io.BytesIO()
    pointcloud.write_mesh_ply(data, vertices, triangles, normals)
    text = data.getvalue()
    assert b"property float blue\nproperty float nx\nproperty float ny\nproperty float nz\nelement face 2\n" in text
    got = lod.parse_mesh_ply(text)
    assert np.array_equal(got[0], vertices) and np.array_equal(got[1], triangles) and np.array_equal(got[2], normals)
    assert len(text) == text.index(b"end_header\n") + 11 + 4 * 36 + 2 * 13
    with pytest.raises(ValueError, match="3 normals for 4 vertices"):
        pointcloud.write_mesh_ply(io.BytesIO(), vertices, triangles, normals[:3])
    empty = io.BytesIO()
    pointcloud.write_mesh_ply(empty, np.zeros((0, 6), F), np.zeros((0, 3), np.int32), np.zeros((0, 3), F))
    assert lod.parse_mesh_ply(empty.getvalue())[2].shape == (0, 3)


# what write_mesh_ply(file, vertices, triangles) wrote for _tiny_mesh() before it took normals
RECORDED_HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                   b"property float red\nproperty float green\nproperty float blue\nelement face 2\nproperty list uchar int vertex_indices\n"
                   b"end_header\n")
RECORDED_FACES = bytes([3, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3, 2, 0, 0, 0, 1, 0, 0, 0, 3, 0, 0, 0])


def test_ply_without_normals_is_byte_identical_to_the_recorded_call():
    vertices, triangles, _ = _tiny_mesh()
    recorded = RECORDED_HEADER + vertices.astype("<f4").tobytes() + RECORDED_FACES
    for call in (lambda f: pointcloud.write_mesh_ply(f, vertices, triangles), lambda f: pointcloud.write_mesh_ply(f, vertices, triangles, None),
                 lambda f: pointcloud.write_mesh_ply(f, vertices, triangles, normals=None)):
        data = io.BytesIO()
        call(data)
        assert data.getvalue() == recorded
    got = mref.parse_mesh_ply(recorded)
    assert np.array_equal(got[0], vertices) and np.array_equal(got[1], triangles)
