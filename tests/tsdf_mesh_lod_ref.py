"""Helper of test_tsdf_mesh_lod.py / test_gpu_tsdf_mesh_lod.py: the vertex normals and the clustered level of detail of the TSDF mesh
as include/monorec_hip.h states them, restated in numpy over a volume dict of tsdf_fusion_ref (every array float32, every operation
rounded on its own).  The full mesh, its owner voxels and edge types come from tsdf_mesh_ref.mesh.  A sparse volume is restated by the
dense volume it stands for (tsdf_sparse_ref: a block without storage has weight 0, so it is unseen for min_weight >= 0)."""
import numpy as np

import tsdf_fusion_ref as ref
import tsdf_mesh_ref as mref

F = np.float32
CELLS = (1, 2, 4, 8)


def gradients(vol, min_weight=0.0):
    """(3, nz, ny, nx) fp32: g_i = tsdf[v + e_i] - tsdf[v - e_i], a neighbour outside the grid or not seen replaced by v itself."""
    tsdf, seen = vol["tsdf"], vol["weight"] > F(min_weight)
    g = np.zeros((3,) + tsdf.shape, F)
    for i in range(3):
        axis = 2 - i                                               # the arrays are [z][y][x]
        near = tuple(slice(0, -1) if a == axis else slice(None) for a in range(3))
        far = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
        hi, lo = tsdf.copy(), tsdf.copy()
        hi[near] = np.where(seen[far], tsdf[far], tsdf[near])
        lo[far] = np.where(seen[near], tsdf[near], tsdf[far])
        g[i] = hi - lo
    return g


def _normalised(m):
    """m / |m| with |m| = sqrt((m_0 m_0 + m_1 m_1) + m_2 m_2) in fp32, 0 where that is not above 0."""
    m = m.astype(F)
    with np.errstate(all="ignore"):
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]).astype(F)
        unit = (m / length[:, None]).astype(F)
    return np.where((length > 0)[:, None], unit, F(0)).astype(F)


def vertex_normals(vol, full, min_weight=0.0):
    """(n, 3) fp32: the normal of every vertex of `full` = mref.mesh(vol, min_weight), in its order."""
    keys, tsdf = full["keys"], vol["tsdf"]
    if not len(keys):
        return np.zeros((0, 3), F)
    g = gradients(vol, min_weight)
    step = np.asarray(mref.EDGES, np.int64)[keys[:, 3]]
    ax, ay, az = keys[:, 0], keys[:, 1], keys[:, 2]
    bx, by, bz = ax + step[:, 0], ay + step[:, 1], az + step[:, 2]
    ta, tb = tsdf[az, ay, ax], tsdf[bz, by, bx]
    with np.errstate(all="ignore"):
        s = (ta / (ta - tb)).astype(F)
        ga, gb = g[:, az, ay, ax].T, g[:, bz, by, bx].T
        m = (ga + s[:, None] * (gb - ga)).astype(F)
    return _normalised(m)


RUN = 8                                        # voxels of one run of a cluster's sum


def _serial_sums(group, values):
    """(the distinct values of the sorted `group`, per group the fp32 sum of its rows of `values`, taken from 0 in the order given)."""
    ids, start, count = np.unique(group, return_index=True, return_counts=True)
    sums = np.zeros((len(ids), values.shape[1]), F)
    for j in range(int(count.max())):                                                  # member j of every group that has one
        pick = count > j
        sums[pick] = sums[pick] + values[start[pick] + j]
    return ids, sums


def mesh(vol, min_weight=0.0, cell=1, normals=False):
    """dict(vertices (n, 6) fp32, triangles (m, 3) int64, normals (n, 3) fp32 or None, clusters: how many clusters own a vertex of the
    full mesh - None for cell 1) of `mesh(min_weight, cell, normals)`; the order of both arrays is this function's own."""
    if cell not in CELLS:
        raise ValueError(f"cell {cell!r} must be one of {CELLS}")
    full = mref.mesh(vol, min_weight)
    unit = vertex_normals(vol, full, min_weight) if normals else None
    if cell == 1:
        return dict(vertices=full["vertices"], triangles=full["triangles"], normals=unit, clusters=None)
    keys = full["keys"]
    if not len(keys):
        return dict(vertices=np.zeros((0, 6), F), triangles=np.zeros((0, 3), np.int64), normals=np.zeros((0, 3), F) if normals else None, clusters=0)
    nx, ny, _ = vol["dims"]
    cx, cy = -(-nx // cell), -(-ny // cell)
    cid = ((keys[:, 2] // cell) * cy + keys[:, 1] // cell) * cx + keys[:, 0] // cell
    # voxel i of its cluster, z outermost, x fastest; run i // 8 of the cluster.  A run is summed serially, then the runs of a cluster
    local = ((keys[:, 2] % cell) * cell + keys[:, 1] % cell) * cell + keys[:, 0] % cell
    runs_per = max(cell ** 3 // RUN, 1)
    run = cid * runs_per + local // RUN
    order = np.lexsort((keys[:, 3], local, run))                                       # by run, then voxel, then edge
    values = full["vertices"] if unit is None else np.concatenate([full["vertices"], unit], axis=1)
    values = np.concatenate([values.astype(F), np.ones((len(values), 1), F)], axis=1)[order]      # the count beside them
    run_ids, run_sums = _serial_sums(run[order], values)
    owners, sums = _serial_sums(run_ids // runs_per, run_sums)
    count = sums[:, -1]
    vertices = (sums[:, :6] / count[:, None]).astype(F)
    mapped = np.searchsorted(owners, cid)[full["triangles"]]                            # every corner's cluster, as a vertex index
    keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    return dict(vertices=vertices, triangles=mapped[keep], normals=_normalised(sums[:, 6:9]) if normals else None, clusters=len(owners))


def owning_clusters(vol, min_weight, cell):
    """How many clusters hold a voxel whose mask is not 0, from the masks alone."""
    masks = mref.mesh(vol, min_weight)["masks"] != 0
    pad = [(0, -d % cell) for d in masks.shape]
    masks = np.pad(masks, pad)
    nz, ny, nx = masks.shape
    return int(masks.reshape(nz // cell, cell, ny // cell, cell, nx // cell, cell).any(axis=(1, 3, 5)).sum())


# ------------------------------------------------------------------------------------------ comparing meshes
def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _sorted_rows(rows):
    return rows[np.lexsort(tuple(rows[:, k] for k in range(rows.shape[1] - 1, -1, -1)))] if len(rows) else rows


def records(vertices, normals=None):
    """(n, 6 or 9) fp32: the vertex records with their normals beside them."""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 6)
    return vertices if normals is None else np.concatenate([vertices, np.asarray(normals, dtype=F).reshape(-1, 3)], axis=1)


def canonical(vertices, triangles, normals=None):
    """(sorted vertex records, sorted triangles) as uint32 bit patterns: the vertices sorted by their bytes, every triangle as the
    records of its three vertices, rotated (winding kept) to the rotation that sorts first, the triangles sorted - repeated ones stay.
    Two meshes are the same vertices, surface, winding and normals, bit for bit, iff both arrays are equal."""
    rec = _bits(records(vertices, normals))
    triangles = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    m, w = len(triangles), rec.shape[1]
    if m == 0:
        return _sorted_rows(rec), np.zeros((0, 3 * w), np.uint32)
    corners = rec[triangles]                                                           # (m, 3, w)
    rotations = np.stack([np.roll(corners, -r, axis=1).reshape(m, 3 * w) for r in range(3)], axis=1).reshape(3 * m, 3 * w)
    owner = np.repeat(np.arange(m), 3)
    order = np.lexsort(tuple(rotations[:, k] for k in range(3 * w - 1, -1, -1)) + (owner,))      # by triangle, then by its words
    return _sorted_rows(rec), _sorted_rows(rotations[order[::3]])


def same(got, want):
    """Are two canonical meshes equal?"""
    return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def directed_edges(triangles):
    """{(a, b): count} over the directed edges of the triangles."""
    triangles = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    directed = np.concatenate([triangles[:, [0, 1]], triangles[:, [1, 2]], triangles[:, [2, 0]]])
    pairs, counts = np.unique(directed, axis=0, return_counts=True) if len(directed) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    return {(int(a), int(b)): int(n) for (a, b), n in zip(pairs, counts)}


def parse_mesh_ply(data):
    """(vertices (n, 6) fp32, triangles (m, 3) int32, normals (n, 3) fp32 or None) of a file `write_mesh_ply` wrote; asserts its layout."""
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    names = [line.split()[-1] for line in lines if line.startswith("property float ")]
    assert names in (["x", "y", "z", "red", "green", "blue"], ["x", "y", "z", "red", "green", "blue", "nx", "ny", "nz"])
    w = len(names)
    n, m = int(lines[2].split()[-1]), int(lines[3 + w].split()[-1])
    assert lines == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property float {f}" for f in names] + \
        [f"element face {m}", "property list uchar int vertex_indices"]
    assert len(data) == len(head) + len(b"end_header\n") + 4 * w * n + 13 * m
    rows = np.frombuffer(body[:4 * w * n], "<f4").reshape(n, w)
    faces = np.frombuffer(body[4 * w * n:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert np.all(faces["n"] == 3)
    return rows[:, :6], faces["v"].astype(np.int32), rows[:, 6:] if w == 9 else None


# ------------------------------------------------------------------------------------------ fields
def field_volume(dims, kind, seed=0, colour=True):
    """A volume of `dims` voxels of 0.06 m, trunc 3 voxels, random colours:
    sphere   a ball of 0.38 of the shortest side round a point a little off the centre, every weight 2
    plane    an oblique plane through the middle that leaves the grid on every side, every weight 2
    pockets  the sphere with weights 1 .. 3 and a tenth of the voxels unseen (weight 0) - some of them next to the surface"""
    vol = ref.new_volume(dims, (-0.3, 0.2, 1.0), 0.06, 0.18, colour=colour)
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if kind == "plane":
        normal = np.array([2.0, 3.0, 6.0]) / 7.0
        dist = normal[0] * (x - 0.5 * (nx - 1) - 0.21) + normal[1] * (y - 0.5 * (ny - 1) + 0.13) + normal[2] * (z - 0.5 * (nz - 1) - 0.37)
    else:
        centre = (0.5 * (nx - 1) + 0.3, 0.5 * (ny - 1) - 0.4, 0.5 * (nz - 1) + 0.1)
        dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - 0.38 * (min(dims) - 1)
    vol["tsdf"] = np.clip(dist / 3.0, -1.0, 1.0).astype(F)
    vol["weight"] = np.full(vol["tsdf"].shape, 2, F)
    if kind == "pockets":
        vol["weight"] = np.where(rng.random(vol["tsdf"].shape) < 0.1, 0.0, rng.integers(1, 4, vol["tsdf"].shape)).astype(F)
    if colour:
        vol["colour"][..., :3] = rng.integers(0, 256, size=vol["tsdf"].shape + (3,), dtype=np.uint8)
    return vol


def integer_plane(dims, normal=(2, 3, 6), offset=40):
    """tsdf = (N . index - offset) / 64 with an integer N: every value, every difference of two and the squared length of the gradient
    are exact in fp32.  Every weight 1, no colour.  The unit normal is N / |N| (|(2, 3, 6)| = 7)."""
    vol = ref.new_volume(dims, (0.0, 0.0, 0.0), 0.0625, 0.1875, colour=False)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol["tsdf"] = ((normal[0] * x + normal[1] * y + normal[2] * z - offset) / 64.0).astype(F)
    vol["weight"] = np.ones(vol["tsdf"].shape, F)
    return vol
