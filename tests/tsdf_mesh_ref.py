"""Helper of test_tsdf_mesh.py / test_gpu_tsdf_mesh.py: the rules of mr_tsdf_mesh_vertices_f32 / mr_tsdf_mesh_triangles_f32 as
include/monorec_hip.h states them - marching tetrahedra over the Kuhn split of every cube of eight voxels - restated in numpy over
a volume dict of tsdf_fusion_ref (every array float32, every operation rounded on its own), and what the tests need to compare
meshes whose vertex and triangle order is unspecified."""
import numpy as np

import tsdf_fusion_ref as ref

F = np.float32

# the seven edge types a voxel owns, as (dx, dy, dz) steps to the far end
EDGES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# one tetrahedron per permutation (a, b, c) of the axes: c0 = v, c1 = c0 + e_a, c2 = c1 + e_b, c3 = c2 + e_c; the three even ones first
PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))
ODD = (False, False, False, True, True, True)
# the six edges of a tetrahedron as (near corner, far corner): E01 E12 E23 E02 E13 E03.  The near corner owns the edge.
TET_EDGES = ((0, 1), (1, 2), (2, 3), (0, 2), (1, 3), (0, 3))
E01, E12, E23, E02, E13, E03 = range(6)
# case = sum of 1 << i over the corners c_i that are inside (tsdf < 0); triangles of an EVEN tetrahedron (an odd one swaps the last two
# vertices of each).  Quads are split along their first-listed vertex.
CASES = {
    0: (),
    1: ((E01, E02, E03),),
    2: ((E01, E13, E12),),
    3: ((E12, E02, E03), (E12, E03, E13)),
    4: ((E02, E12, E23),),
    5: ((E01, E12, E23), (E01, E23, E03)),
    6: ((E01, E13, E23), (E01, E23, E02)),
    7: ((E03, E13, E23),),
    8: ((E03, E23, E13),),
    9: ((E01, E02, E23), (E01, E23, E13)),
    10: ((E01, E03, E23), (E01, E23, E12)),
    11: ((E02, E23, E12),),
    12: ((E12, E13, E03), (E12, E03, E02)),
    13: ((E01, E12, E13),),
    14: ((E01, E03, E02),),
    15: (),
}


def _unit(axis):
    return tuple(1 if k == axis else 0 for k in range(3))


def _shifted(array, step, extent=None):
    """array[z + dz, y + dy, x + dx] over the voxels for which that neighbour exists (`extent`: over that many voxels per axis
    instead), as a view.  step = (dx, dy, dz)."""
    nz, ny, nx = array.shape[:3]
    dx, dy, dz = step
    ex, ey, ez = extent if extent is not None else (nx - dx, ny - dy, nz - dz)
    return array[dz:dz + ez, dy:dy + ey, dx:dx + ex]


def edge_type(step):
    return EDGES.index(tuple(step))


def mesh(vol, min_weight=0.0):
    """dict(keys (n, 4) int64: x y z edge of every vertex, vertices (n, 6) fp32, triangles (m, 3) int64 into them; per triangle cubes
    (m, 3) int64: x y z of the base voxel of its cube, and tets (m,) int64: its tetrahedron, an index into PERMS; masks (nz, ny, nx)
    uint8: bit e set where the voxel owns a vertex on its edge EDGES[e]).  The order of vertices and triangles is this function's own."""
    nx, ny, nz = vol["dims"]
    tsdf, weight = vol["tsdf"], vol["weight"]
    seen = weight > F(min_weight)
    neg = tsdf < 0
    px, py, pz = ref.positions(vol)
    pos = [np.broadcast_to(p, tsdf.shape) for p in (px, py, pz)]
    index = np.full((7, nz, ny, nx), -1, np.int64)             # vertex number of (edge, z, y, x)
    keys, records, count = [], [], 0
    masks = np.zeros((nz, ny, nx), np.uint8)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for e, step in enumerate(EDGES):
        extent = (nx - step[0], ny - step[1], nz - step[2])
        if min(extent) < 1:
            continue
        lo = lambda a: _shifted(a, (0, 0, 0), extent)
        hi = lambda a: _shifted(a, step)
        tv, tn = lo(tsdf), hi(tsdf)
        active = lo(seen) & hi(seen) & (lo(neg) != hi(neg))
        with np.errstate(all="ignore"):
            s = tv / (tv - tn)
            rec = np.zeros(tv.shape + (6,), F)
            for k in range(3):
                rec[..., k] = lo(pos[k]) + s * vol["voxel"] if step[k] else lo(pos[k])
            if vol["colour"] is not None:
                for c in range(3):
                    cv, cn = lo(vol["colour"])[..., c].astype(F), hi(vol["colour"])[..., c].astype(F)
                    rec[..., 3 + c] = np.floor(cv + s * (cn - cv) + F(0.5))
        n = int(active.sum())
        lo(index[e])[active] = count + np.arange(n)
        lo(masks)[active] |= np.uint8(1 << e)
        keys.append(np.stack([lo(xx)[active], lo(yy)[active], lo(zz)[active], np.full(n, e)], axis=1))
        records.append(rec[active])
        count += n
    keys = np.concatenate(keys) if keys else np.zeros((0, 4), np.int64)
    records = np.concatenate(records).astype(F) if records else np.zeros((0, 6), F)

    triangles, bases, tets = [], [], []
    cubes = (nx - 1, ny - 1, nz - 1)
    if min(cubes) >= 1:
        for number_of_tet, (perm, odd) in enumerate(zip(PERMS, ODD)):
            corner = [(0, 0, 0)]
            for axis in perm:
                corner.append(tuple(p + q for p, q in zip(corner[-1], _unit(axis))))
            whole = np.ones(cubes[::-1], bool)
            case = np.zeros(cubes[::-1], np.int64)
            for i, c in enumerate(corner):
                whole &= _shifted(seen, c, cubes)
                case |= _shifted(neg, c, cubes).astype(np.int64) << i
            for number, tris in CASES.items():
                pick = whole & (case == number)
                if not tris or not pick.any():
                    continue
                for tri in tris:
                    if odd:
                        tri = (tri[0], tri[2], tri[1])
                    ids = []
                    for edge in tri:
                        near, far = TET_EDGES[edge]
                        step = tuple(q - p for p, q in zip(corner[near], corner[far]))
                        ids.append(_shifted(index[edge_type(step)], corner[near], cubes)[pick])
                    triangles.append(np.stack(ids, axis=1))
                    bases.append(np.stack([_shifted(a, (0, 0, 0), cubes)[pick] for a in (xx, yy, zz)], axis=1))
                    tets.append(np.full(int(pick.sum()), number_of_tet, np.int64))
    triangles = np.concatenate(triangles) if triangles else np.zeros((0, 3), np.int64)
    bases = np.concatenate(bases) if bases else np.zeros((0, 3), np.int64)
    tets = np.concatenate(tets) if tets else np.zeros(0, np.int64)
    assert records.dtype == F and (triangles >= 0).all() and len(bases) == len(tets) == len(triangles)
    return dict(keys=keys, vertices=records, triangles=triangles, cubes=bases, tets=tets, masks=masks)


def axis_vertices(result):
    """The records on the three axis edges: what `extract` returns."""
    return result["vertices"][result["keys"][:, 3] < 3]


# ------------------------------------------------------------------------------------------ vertices across tile seams
TILE = (32, 8, 4)                              # the workgroup tile of the mesh kernels
SEAM_PAIRS = 192                               # per axis: the 3 edge types without a step along it x the 64 masks that contain one type


def seam_pairs(vol, result, tile=TILE):
    """The set of (axis, owner mask, edge type) over the triangle vertices of `result` = mesh(vol, ...) whose owner voxel lies in the
    next tile along `axis` than the base voxel of the triangle's cube: the triangle kernel ranks such a vertex with a mask from the
    second halo layer of its staged codes and adds a vertex_base another workgroup wrote.  The owner is then a corner of the cube one
    step along `axis` from its base, so the edge has no step along `axis`: 3 types x 64 masks = SEAM_PAIRS per axis."""
    keys, masks = result["keys"], result["masks"]
    pairs = set()
    for corner in range(3):
        owner = keys[result["triangles"][:, corner]]
        mask = masks[owner[:, 2], owner[:, 1], owner[:, 0]]
        for axis in range(3):
            across = owner[:, axis] // tile[axis] == result["cubes"][:, axis] // tile[axis] + 1
            pairs |= {(axis, int(m), int(e)) for m, e in np.unique(np.stack([mask[across], owner[across, 3]], axis=1), axis=0)}
    assert all(m >> e & 1 and not EDGES[e][axis] for axis, m, e in pairs)
    return pairs


def pattern_volume(axis, seam, background, seed=0):
    """Every sign pattern of a cube whose base is voxel `seam` of `axis`: all voxels seen, magnitudes 0.05 .. 1, the sign `background`
    (+1 or -1) except on a 16 x 16 grid of sites 3 voxels apart along the other two axes, where corner dx + 2 dy + 4 dz of the cube is
    negative iff that bit of the site's number is set.  seam + 3 voxels along `axis`, 49 along the others, random colours."""
    dims = tuple(seam + 3 if a == axis else 49 for a in range(3))
    vol = ref.new_volume(dims, (-0.3, 0.2, 1.0), 0.06, 0.18)
    rng = np.random.default_rng(seed)
    shape = vol["tsdf"].shape
    sign = np.full(shape, float(background))
    others = [a for a in range(3) if a != axis]
    for site in range(256):
        base = [0, 0, 0]
        base[axis], base[others[0]], base[others[1]] = seam, 3 * (site % 16), 3 * (site // 16)
        for corner in range(8):
            x, y, z = base[0] + (corner & 1), base[1] + (corner >> 1 & 1), base[2] + (corner >> 2)
            sign[z, y, x] = -1.0 if site >> corner & 1 else 1.0
    vol["tsdf"] = (sign * (0.05 + 0.95 * rng.random(shape))).astype(F)
    vol["weight"] = np.ones(shape, F)
    vol["colour"][..., :3] = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    return vol


def noise_volume(dims, seed, unseen=0.1, colour=True):
    """Independent random signs, magnitudes 0.02 .. 1, weights 1 .. 3 with a share `unseen` at 0, random colours; eight voxels hold
    exactly 0.0 and eight -0.0 (both count as outside).  No NaN, no denormal."""
    vol = ref.new_volume(dims, (-0.3, 0.2, 1.0), 0.06, 0.18, colour=colour)
    rng = np.random.default_rng(seed)
    shape = vol["tsdf"].shape
    tsdf = (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * (0.02 + 0.98 * rng.random(shape))).astype(F).reshape(-1)
    zeros = rng.choice(tsdf.size, 16, replace=False)
    tsdf[zeros[:8]], tsdf[zeros[8:]] = F(0.0), F(-0.0)
    vol["tsdf"] = tsdf.reshape(shape)
    vol["weight"] = np.where(rng.random(shape) < unseen, 0.0, rng.integers(1, 4, shape)).astype(F)
    if colour:
        vol["colour"][..., :3] = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    assert np.isfinite(vol["tsdf"]).all() and (np.abs(vol["tsdf"][vol["tsdf"] != 0]) >= 0.02).all()
    return vol


# ------------------------------------------------------------------------------------------ comparing meshes
def canonical(vertices, triangles):
    """(m, 18) fp32: every triangle as its three vertex records, rotated (winding kept) to the rotation that sorts first, the
    triangles sorted.  Two meshes are the same surface with the same winding and diagonals iff these are equal."""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 6)
    triangles = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    m = len(triangles)
    if m == 0:
        return np.zeros((0, 18), F)
    recs = vertices[triangles]                                            # (m, 3, 6)
    rotations = np.stack([np.roll(recs, -r, axis=1).reshape(m, 18) for r in range(3)], axis=1).reshape(3 * m, 18)
    owner = np.repeat(np.arange(m), 3)
    order = np.lexsort(tuple(rotations[:, k] for k in range(17, -1, -1)) + (owner,))      # by triangle, then by the 18 floats
    best = rotations[order[::3]]                                          # the first of each triangle's three
    return best[np.lexsort(tuple(best[:, k] for k in range(17, -1, -1)))]


def topology(triangles):
    """dict(V, E, F, open: the undirected edges (i, j), i < j, whose use count is not 2, with that count; repeated: the directed edges
    used more than once)."""
    triangles = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    directed = np.concatenate([triangles[:, [0, 1]], triangles[:, [1, 2]], triangles[:, [2, 0]]])
    pairs, counts = np.unique(directed, axis=0, return_counts=True) if len(directed) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    undirected, uses = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True) if len(directed) else (pairs, counts)
    return dict(V=len(np.unique(triangles)), E=len(undirected), F=len(triangles),
                open=[(int(i), int(j), int(n)) for (i, j), n in zip(undirected[uses != 2], uses[uses != 2])],
                repeated=[(int(i), int(j)) for i, j in pairs[counts > 1]])


def parse_mesh_ply(data):
    """(vertices (n, 6) fp32, triangles (m, 3) int32) of a file `write_mesh_ply` wrote; asserts its layout."""
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    n, m = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    assert lines == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + \
        [f"property float {f}" for f in ("x", "y", "z", "red", "green", "blue")] + [f"element face {m}", "property list uchar int vertex_indices"]
    assert len(data) == len(head) + len(b"end_header\n") + 24 * n + 13 * m
    vertices = np.frombuffer(body[:24 * n], "<f4").reshape(n, 6)
    faces = np.frombuffer(body[24 * n:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert np.all(faces["n"] == 3)
    return vertices, faces["v"].astype(np.int32)


# ------------------------------------------------------------------------------------------ an analytic volume
def sphere_volume(dims, origin, voxel, colour=True):
    """tsdf = clip((|p - c| - r) / 0.18, -1, 1) in fp32 round `ref.SPHERE`, every weight 1, a colour ramp."""
    vol = ref.new_volume(dims, origin, voxel, 0.18, colour=colour)
    px, py, pz = ref.positions(vol)
    cx, cy, cz, r = (F(v) for v in ref.SPHERE)
    dist = np.sqrt((px - cx) * (px - cx) + (py - cy) * (py - cy) + (pz - cz) * (pz - cz)).astype(F)
    vol["tsdf"] = np.clip((dist - r) / F(0.18), F(-1), F(1)).astype(F)
    vol["weight"] = np.ones_like(vol["tsdf"])
    if colour:
        nx, ny, nz = dims
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        vol["colour"][..., 0] = (x * 6) % 256
        vol["colour"][..., 1] = (y * 12 + 3) % 256
        vol["colour"][..., 2] = (z * 11 + x) % 256
    return vol


SPHERE_VOLUME = dict(dims=(41, 19, 21), origin=(-1.2, -0.6, 2.3), voxel=0.06)


def with_hole(vol):
    """A copy with two z slices of a band of rows unseen."""
    vol = ref.copy_volume(vol)
    nz = vol["dims"][2]
    vol["weight"][nz // 2 - 1:nz // 2 + 1, 2:6, :] = 0
    return vol
