"""Helper of test_tsdf_render.py / test_gpu_tsdf_render.py: mr_tsdf_skip_grid_u8 / mr_tsdf_render_f32 as include/monorec_hip.h states
them, restated in numpy on the volume dicts of tests/tsdf_fusion_ref.py - every array is float32, so every operation is rounded on its
own, in the order of the header.  `render` visits every sample of every ray; with `bricks` it also plays the skipping rule beside the
full march and reports what the rule would have spared and whether it could have changed anything."""
import numpy as np

import tsdf_fusion_ref as ref

F = np.float32
BRICK = 4


def brick_flags(vol, min_weight=0.0, brick=BRICK):
    """(bz, by, bx) uint8: 1 where a voxel with weight > min_weight and tsdf < 0 lies in [B b, B b + B] on every axis (clipped)."""
    nx, ny, nz = vol["dims"]
    neg = (vol["weight"] > F(min_weight)) & (vol["tsdf"] < 0)
    counts = [(n + brick - 1) // brick for n in (nx, ny, nz)]
    out = np.zeros((counts[2], counts[1], counts[0]), np.uint8)
    for bz in range(counts[2]):
        for by in range(counts[1]):
            for bx in range(counts[0]):
                out[bz, by, bx] = neg[brick * bz:brick * bz + brick + 1, brick * by:brick * by + brick + 1, brick * bx:brick * bx + brick + 1].any()
    return out


def sample_count(t_min, t_max, step):
    """Number of samples k = 0, 1, ... with t_k = t_min + (float)k * step <= t_max."""
    t_min, t_max, step = F(t_min), F(t_max), F(step)
    k = 0
    while t_min + F(k) * step <= t_max:
        k += 1
    return k


def lerp(a, b, f):
    return a + f * (b - a)


def trilinear(c, fx, fy, fz):
    """c[z][y][x] (each an array over the pixels), lerped along x, then y, then z."""
    y0 = lerp(lerp(c[0][0][0], c[0][0][1], fx), lerp(c[0][1][0], c[0][1][1], fx), fy)
    y1 = lerp(lerp(c[1][0][0], c[1][0][1], fx), lerp(c[1][1][0], c[1][1][1], fx), fy)
    return lerp(y0, y1, fz)


def render(vol, pose, intrinsics, height, width, t_min, t_max, step, min_weight=0.0, bricks=None, brick=BRICK):
    """One view.  pose: camera -> world (4, 4); intrinsics (fx, fy, cx, cy).  Returns dict(depth (h, w) fp32, normal (h, w, 3) fp32,
    colour (h, w, 3) uint8, hit (h, w) bool, evaluations: cells evaluated by the full march, up to each ray's end) and, with `bricks`,
    brick_depth (the depth of the march that skips), brick_evaluations and skipped_negative (skipped samples that were valid and
    negative: must be 0)."""
    m = np.asarray(pose, dtype=F)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    t_min, t_max, step, min_weight = F(t_min), F(t_max), F(step), F(min_weight)
    nx, ny, nz = vol["dims"]
    dims = (nx, ny, nz)
    tsdf, weight = vol["tsdf"].reshape(-1), vol["weight"].reshape(-1)
    colour = vol["colour"].reshape(-1, 4) if vol["colour"] is not None else None
    inv = F(1.0) / vol["voxel"]
    o = [(m[a, 3] - F(vol["origin"][a])) * inv for a in range(3)]
    v, u = np.meshgrid(np.arange(height, dtype=F), np.arange(width, dtype=F), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    n = u.size
    with np.errstate(all="ignore"):
        rx, ry = (u - cx) / fx, (v - cy) / fy
        e = [((m[a, 0] * rx + m[a, 1] * ry) + m[a, 2]) * inv for a in range(3)]
    assert all(x.dtype == F for x in e) and all(isinstance(x, F) for x in o)

    depth, normal, rgb = np.zeros(n, F), np.zeros((n, 3), F), np.zeros((n, 3), np.uint8)
    hit = np.zeros(n, bool)
    active, prev_valid, f_prev = np.ones(n, bool), np.zeros(n, bool), np.zeros(n, F)
    evaluations = 0
    # the march that skips, beside the full one: state 0 prev not valid, 1 valid, 2 skipped
    b_active, b_state, b_prev = np.ones(n, bool), np.zeros(n, np.int8), np.zeros(n, F)
    b_depth, b_evaluations, skipped_negative = np.zeros(n, F), 0, 0
    last_valid, last_f = np.zeros(n, bool), np.zeros(n, F)             # sample k - 1 in full, whatever the states
    corner_steps = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    for k in range(sample_count(t_min, t_max, step)):
        with np.errstate(all="ignore"):
            t = t_min + F(k) * step
            g = [o[a] + t * e[a] for a in range(3)]
            i = [np.floor(x) for x in g]
            f = [g[a] - i[a] for a in range(3)]
            inside = np.ones(n, bool)
            for a in range(3):
                inside &= (i[a] >= 0) & (i[a].astype(np.float64) + 1 <= dims[a] - 1)
            ii = [np.where(inside, i[a], 0).astype(np.int64) for a in range(3)]
            base = (ii[2] * ny + ii[1]) * nx + ii[0]
            base = np.where(inside, base, 0)
            at = {(dz, dy, dx): np.where(inside, base + dx + dy * nx + dz * nx * ny, 0) for dz, dy, dx in corner_steps}
            valid = inside.copy()
            for c in corner_steps:
                valid &= weight[at[c]] > min_weight
            T = [[[tsdf[at[(dz, dy, dx)]] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
            value = trilinear(T, f[0], f[1], f[2])
            assert value.dtype == F and t.dtype == F
            evaluations += int((active & inside).sum())
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
                if colour is not None:
                    for ch in range(3):
                        C = [[[colour[at[(dz, dy, dx)], ch].astype(F) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
                        byte = np.minimum(F(255.0), np.floor(trilinear(C, f[0], f[1], f[2]) + F(0.5)))
                        rgb[:, ch] = np.where(hit_now, byte, rgb[:, ch].astype(F)).astype(np.uint8)
            hit |= hit_now
            active &= ~(hit_now | stop_now)
            if bricks is not None:
                byte = bricks[ii[2] // brick, ii[1] // brick, ii[0] // brick] != 0
                skip = b_active & inside & ~byte & ~((b_state == 1) & (b_prev < 0))
                skipped_negative += int((skip & valid & (value < 0)).sum())
                full = b_active & inside & ~skip
                again = full & (b_state == 2)                              # sample k - 1 in full, as prev
                b_evaluations += int(full.sum()) + int(again.sum())
                b_state = np.where(again, last_valid.astype(np.int8), b_state)
                b_prev = np.where(again, last_f, b_prev)
                b_hit = full & valid & (b_state == 1) & ~(b_prev < 0) & (value < 0)
                b_stop = full & valid & (b_state == 1) & (b_prev < 0) & ~(value < 0)
                b_depth = np.where(b_hit, (t_min + F(k - 1) * step) + (b_prev / (b_prev - value)) * step, b_depth)
                b_active &= ~(b_hit | b_stop)
                b_state = np.where(~inside, 0, np.where(skip, 2, valid.astype(np.int8))).astype(np.int8)
                b_prev = np.where(full, value, b_prev)
            prev_valid, f_prev = valid, value
            last_valid, last_f = valid, value
    out = dict(depth=depth.reshape(height, width), normal=normal.reshape(height, width, 3), colour=rgb.reshape(height, width, 3),
               hit=hit.reshape(height, width), evaluations=evaluations)
    if bricks is not None:
        out.update(brick_depth=b_depth.reshape(height, width), brick_evaluations=b_evaluations, skipped_negative=skipped_negative)
    return out


def scene_depth(pose, intrinsics, height, width):
    """The camera-z depth of the analytic scene of tests/tsdf_fusion_ref.py in metres (0: nothing), before its centimetre rounding."""
    depth_cm, _ = ref.render(pose, intrinsics, height, width, zero_rows=())
    return depth_cm.astype(np.float64) / 100.0


def inside_pose():
    """A camera inside the SMALL volume, in front of the wall and beside the sphere, turned half a radian about y towards the sphere."""
    t = np.eye(4, dtype=F)
    t[:3, 0], t[:3, 2] = (np.cos(0.5), 0.0, -np.sin(0.5)), (np.sin(0.5), 0.0, np.cos(0.5))
    t[:3, 3] = (-0.75, -0.2, 2.55)
    return t


def slab_volume(dims=(21, 19, 30), colour=True):
    """Two slabs of negative tsdf across z (4 .. 9 and 16 .. 21), positive elsewhere, all seen but one column: a ray that starts inside
    the first slab leaves it through a back face and must not report the second; one from z < 4 hits the first."""
    vol = ref.new_volume(dims, (-0.6, -0.5, 1.0), 0.06, 0.18, colour=colour)
    z = np.arange(dims[2]).reshape(-1, 1, 1)
    inside = ((z >= 4) & (z <= 9)) | ((z >= 16) & (z <= 21))
    y, x = np.arange(dims[1]).reshape(1, -1, 1), np.arange(dims[0]).reshape(1, 1, -1)
    vol["tsdf"] = np.where(inside, -0.4, 0.7).astype(F) + (F(0.01) * ((x * 3 + y * 5 + z) % 7)).astype(F)
    vol["weight"] = np.ones(vol["tsdf"].shape, F)
    vol["weight"][:, 3, 5] = 0
    if colour:
        vol["colour"][..., 0], vol["colour"][..., 1], vol["colour"][..., 2] = (x * 11 + z) % 256, (y * 13 + z * 3) % 256, (x + y + z * 7) % 256
    return vol


def slab_pose(z):
    """A camera on the axis of `slab_volume` at height z, looking along +z."""
    t = np.eye(4, dtype=F)
    t[:3, 3] = (0.0, 0.05, z)
    return t


def behind_pose():
    """A camera behind the wall, looking back at it (-z): it sees the surfaces from inside."""
    t = np.eye(4, dtype=F)
    t[0, 0], t[2, 2] = -1.0, -1.0
    t[:3, 3] = (0.05, 0.02, 3.6)
    return t
