"""Helper of test_tsdf_sparse_render.py / test_gpu_tsdf_sparse_render.py: mr_tsdf_sparse_render_f32 as include/monorec_hip.h states it,
restated in numpy - the march of tests/tsdf_render_ref.py's `render` on the virtual dense volume of a block table, with the corner
lookup going through the table: a voxel of a block without storage reads tsdf 1, weight 0, colour 0.  The table may be far larger than
anything a dense array could hold: only the allocated blocks of a small restatement volume placed somewhere inside it exist."""
import numpy as np

import tsdf_render_ref as rref

F = np.float32
B = 8                                          # MR_TSDF_BLOCK


def render_virtual(sub, offset, origin, blocks, pose, intrinsics, height, width, t_min, t_max, step, min_weight=0.0):
    """One view of the sparse volume of `blocks` = (nbx, nby, nbz) blocks at `origin` whose only allocated blocks are those of `sub` - a
    sparsified restatement volume (tsdf_sparse_ref.sparsify / fuse: whole blocks, with its `allocated` grid) - placed at voxel `offset`
    (whole blocks).  pose: camera -> world (4, 4); intrinsics (fx, fy, cx, cy).  Returns dict(depth (h, w) fp32, normal (h, w, 3) fp32,
    colour (h, w, 3) uint8, hit (h, w) bool, base (h, w, 3) int64: the cell base i of the hit sample in voxels of the whole volume, -1
    where nothing was hit)."""
    m = np.asarray(pose, dtype=F)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    t_min, t_max, step, min_weight = F(t_min), F(t_max), F(step), F(min_weight)
    dims = tuple(B * int(b) for b in blocks)
    off = tuple(int(v) for v in offset)
    sx, sy, sz = sub["dims"]
    assert all(v % B == 0 for v in off + (sx, sy, sz)) and all(v >= 0 and v + d <= n for v, d, n in zip(off, (sx, sy, sz), dims))
    allocated, tsdf, weight, colour = sub["allocated"], sub["tsdf"], sub["weight"], sub["colour"]
    inv = F(1.0) / sub["voxel"]
    o = [(m[a, 3] - F(origin[a])) * inv for a in range(3)]
    v, u = np.meshgrid(np.arange(height, dtype=F), np.arange(width, dtype=F), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    n = u.size
    with np.errstate(all="ignore"):
        rx, ry = (u - cx) / fx, (v - cy) / fy
        e = [((m[a, 0] * rx + m[a, 1] * ry) + m[a, 2]) * inv for a in range(3)]
    assert all(x.dtype == F for x in e) and all(isinstance(x, F) for x in o)

    def fetch(x, y, z):
        """(weight, tsdf, colour (n, 4)) of the voxels (x, y, z) of the whole volume, through (offset, allocated)."""
        lx, ly, lz = x - off[0], y - off[1], z - off[2]
        in_sub = (lx >= 0) & (lx < sx) & (ly >= 0) & (ly < sy) & (lz >= 0) & (lz < sz)
        lx, ly, lz = (np.where(in_sub, a, 0) for a in (lx, ly, lz))
        have = in_sub & allocated[lz >> 3, ly >> 3, lx >> 3]
        rgb = np.where(have[:, None], colour[lz, ly, lx], np.uint8(0)) if colour is not None else None
        return np.where(have, weight[lz, ly, lx], F(0.0)), np.where(have, tsdf[lz, ly, lx], F(1.0)), rgb

    depth, normal, rgb = np.zeros(n, F), np.zeros((n, 3), F), np.zeros((n, 3), np.uint8)
    hit, base = np.zeros(n, bool), np.full((n, 3), -1, np.int64)
    active, prev_valid, f_prev = np.ones(n, bool), np.zeros(n, bool), np.zeros(n, F)
    corner_steps = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    lerp, trilinear = rref.lerp, rref.trilinear
    for k in range(rref.sample_count(t_min, t_max, step)):
        if not active.any():
            break
        with np.errstate(all="ignore"):
            t = t_min + F(k) * step
            g = [o[a] + t * e[a] for a in range(3)]
            i = [np.floor(x) for x in g]
            f = [g[a] - i[a] for a in range(3)]
            inside = np.ones(n, bool)
            for a in range(3):
                inside &= (i[a] >= 0) & (i[a].astype(np.float64) + 1 <= dims[a] - 1)
            if not (inside & active).any():                                    # no ray that still marches has a valid sample here
                prev_valid = np.zeros(n, bool)
                continue
            ii = [np.where(inside, i[a], 0).astype(np.int64) for a in range(3)]
            corners = {(dz, dy, dx): fetch(ii[0] + dx, ii[1] + dy, ii[2] + dz) for dz, dy, dx in corner_steps}
            valid = inside.copy()
            for c in corner_steps:
                valid &= corners[c][0] > min_weight
            T = [[[corners[(dz, dy, dx)][1] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
            value = trilinear(T, f[0], f[1], f[2])
            assert value.dtype == F and t.dtype == F
            hit_now = active & valid & prev_valid & ~(f_prev < 0) & (value < 0)
            stop_now = active & valid & prev_valid & (f_prev < 0) & ~(value < 0)
            s = f_prev / (f_prev - value)
            d = (t_min + F(k - 1) * step) + s * step
            depth = np.where(hit_now, d, depth)
            if hit_now.any():
                gx = lerp(lerp(T[0][0][1] - T[0][0][0], T[0][1][1] - T[0][1][0], f[1]), lerp(T[1][0][1] - T[1][0][0], T[1][1][1] - T[1][1][0], f[1]), f[2])
                gy = lerp(lerp(T[0][1][0] - T[0][0][0], T[0][1][1] - T[0][0][1], f[0]), lerp(T[1][1][0] - T[1][0][0], T[1][1][1] - T[1][0][1], f[0]), f[2])
                gz = lerp(lerp(T[1][0][0] - T[0][0][0], T[1][0][1] - T[0][0][1], f[0]), lerp(T[1][1][0] - T[0][1][0], T[1][1][1] - T[0][1][1], f[0]), f[1])
                length = np.sqrt((gx * gx + gy * gy) + gz * gz)
                assert length.dtype == F
                for a, comp in enumerate((gx, gy, gz)):
                    normal[:, a] = np.where(hit_now, np.where(length > 0, comp / length, F(0)), normal[:, a])
                    base[:, a] = np.where(hit_now, ii[a], base[:, a])
                if colour is not None:
                    for ch in range(3):
                        C = [[[corners[(dz, dy, dx)][2][:, ch].astype(F) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
                        byte = np.minimum(F(255.0), np.floor(trilinear(C, f[0], f[1], f[2]) + F(0.5)))
                        rgb[:, ch] = np.where(hit_now, byte, rgb[:, ch].astype(F)).astype(np.uint8)
            hit |= hit_now
            active &= ~(hit_now | stop_now)
            prev_valid, f_prev = valid, value
    return dict(depth=depth.reshape(height, width), normal=normal.reshape(height, width, 3), colour=rgb.reshape(height, width, 3),
                hit=hit.reshape(height, width), base=base.reshape(height, width, 3))
