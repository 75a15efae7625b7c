"""Helper of test_tsdf_render.py / test_gpu_tsdf_render.py: mr_tsdf_skip_grid_u8 / mr_tsdf_render_f32 as include/monorec_hip.h states
them, restated in numpy on the volume dicts of tests/tsdf_fusion_ref.py - every array is float32, so every operation is rounded on its
own, in the order of the header.  `render` visits every sample of every ray; with `bricks` it also plays the skipping rule beside the
full march and reports what the rule would have spared and whether it could have changed anything.  `clip_range` restates the kernels'
clip to the volume's box, and CLIP_CASES are the views in which that clip decides."""
import functools

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


def rays(vol, pose, intrinsics, height, width):
    """(o, e): the camera centre in voxel units (three fp32 scalars) and every pixel's direction per metre of camera z (three (h w,)
    fp32 arrays), as `ray_of_pixel` and the host's `prepare_march` round them."""
    m = np.asarray(pose, dtype=F)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    inv = F(1.0) / vol["voxel"]
    with np.errstate(all="ignore"):
        o = [(m[a, 3] - F(vol["origin"][a])) * inv for a in range(3)]
        v, u = np.meshgrid(np.arange(height, dtype=F), np.arange(width, dtype=F), indexing="ij")
        u, v = u.reshape(-1), v.reshape(-1)
        rx, ry = (u - cx) / fx, (v - cy) / fy
        e = [((m[a, 0] * rx + m[a, 1] * ry) + m[a, 2]) * inv for a in range(3)]
    assert all(x.dtype == F for x in e) and all(isinstance(x, F) for x in o)
    return o, e


def clip_range(vol, pose, intrinsics, height, width, t_min, t_max, step, exact=False):
    """`clip_to_box` of monorec_amd/csrc/tsdf_render.h in fp32, operation by operation: (k_lo, k_hi), two (h, w) int64 arrays - the
    samples the kernels march; k_hi = -1 where the ray is parallel to a pair of faces and lies outside them.  np.fmax / np.fmin are
    fmaxf / fminf: they drop a NaN.  `exact`: the same box without the slack and without the extra sample on either side - what a
    clip with no safety margin would march."""
    t_min, step = F(t_min), F(step)
    last = sample_count(t_min, t_max, step) - 1
    o, e = rays(vol, pose, intrinsics, height, width)
    n = height * width
    t_lo, t_hi = np.full(n, t_min, F), np.full(n, t_min + F(last) * step, F)
    empty = np.zeros(n, bool)
    extra = F(0.0) if exact else F(1.0)
    with np.errstate(all="ignore"):
        for q in range(3):
            lim = F(vol["dims"][q] - 2)
            assert float(lim) == vol["dims"][q] - 2
            top = lim + F(2.0)
            zero = e[q] == 0
            empty |= zero & ~((o[q] >= 0) & (o[q] <= top))
            ta, tb = (F(0.0) - o[q]) / e[q], (top - o[q]) / e[q]
            slack = np.zeros(n, F) if exact else F(1e-5) * np.fmax(np.abs(ta), np.abs(tb)) + step
            t_lo = np.where(zero, t_lo, np.fmax(t_lo, np.fmin(ta, tb) - slack))
            t_hi = np.where(zero, t_hi, np.fmin(t_hi, np.fmax(ta, tb) + slack))
        k_lo = np.fmin(np.fmax(np.floor((t_lo - t_min) / step) - extra, F(0.0)), F(last) + F(1.0))
        k_hi = np.fmin(np.fmax(np.ceil((t_hi - t_min) / step) + extra, F(-1.0)), F(last))
    assert k_lo.dtype == F and k_hi.dtype == F and t_lo.dtype == F and np.isfinite(k_lo).all() and np.isfinite(k_hi).all()
    k_hi = np.where(empty, F(-1.0), k_hi)
    return k_lo.astype(np.int64).reshape(height, width), k_hi.astype(np.int64).reshape(height, width)


def render(vol, pose, intrinsics, height, width, t_min, t_max, step, min_weight=0.0, bricks=None, brick=BRICK, k_range=None):
    """One view.  pose: camera -> world (4, 4); intrinsics (fx, fy, cx, cy).  Returns dict(depth (h, w) fp32, normal (h, w, 3) fp32,
    colour (h, w, 3) uint8, hit (h, w) bool, evaluations: cells evaluated by the full march, up to each ray's end; hit_k (h, w) int64:
    the hit sample, -1 without a hit; end_k: the sample at which the march ended - the hit, the back-face stop, or the last sample;
    first_in, last_in: the first and the last sample at which the ray, still marching, was inside the volume, -1 if never) and, with
    `bricks`, brick_depth (the depth of the march that skips), brick_evaluations and skipped_negative (skipped samples that were valid
    and negative: must be 0).  `k_range` = (k_lo, k_hi) per pixel: the march of a kernel clipped to those samples - the others are not
    visited, which is what a sample outside the volume amounts to."""
    t_min, t_max, step, min_weight = F(t_min), F(t_max), F(step), F(min_weight)
    nx, ny, nz = vol["dims"]
    dims = (nx, ny, nz)
    tsdf, weight = vol["tsdf"].reshape(-1), vol["weight"].reshape(-1)
    colour = vol["colour"].reshape(-1, 4) if vol["colour"] is not None else None
    o, e = rays(vol, pose, intrinsics, height, width)
    n = height * width
    samples = sample_count(t_min, t_max, step)
    in_range = (lambda k: np.ones(n, bool)) if k_range is None else \
        (lambda k: (np.asarray(k_range[0]).reshape(-1) <= k) & (k <= np.asarray(k_range[1]).reshape(-1)))

    depth, normal, rgb = np.zeros(n, F), np.zeros((n, 3), F), np.zeros((n, 3), np.uint8)
    hit = np.zeros(n, bool)
    active, prev_valid, f_prev = np.ones(n, bool), np.zeros(n, bool), np.zeros(n, F)
    evaluations = 0
    hit_k, end_k = np.full(n, -1, np.int64), np.full(n, samples - 1, np.int64)
    first_in, last_in = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    # the march that skips, beside the full one: state 0 prev not valid, 1 valid, 2 skipped
    b_active, b_state, b_prev = np.ones(n, bool), np.zeros(n, np.int8), np.zeros(n, F)
    b_depth, b_evaluations, skipped_negative = np.zeros(n, F), 0, 0
    last_valid, last_f = np.zeros(n, bool), np.zeros(n, F)             # sample k - 1 in full, whatever the states
    corner_steps = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    for k in range(samples):
        with np.errstate(all="ignore"):
            t = t_min + F(k) * step
            g = [o[a] + t * e[a] for a in range(3)]
            i = [np.floor(x) for x in g]
            f = [g[a] - i[a] for a in range(3)]
            inside = in_range(k)
            for a in range(3):
                inside &= (i[a] >= 0) & (i[a].astype(np.float64) + 1 <= dims[a] - 1)
            first_in = np.where(active & inside & (first_in < 0), k, first_in)
            last_in = np.where(active & inside, k, last_in)
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
            hit_k = np.where(hit_now, k, hit_k)
            end_k = np.where(hit_now | stop_now, k, end_k)
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
               hit=hit.reshape(height, width), evaluations=evaluations, hit_k=hit_k.reshape(height, width), end_k=end_k.reshape(height, width),
               first_in=first_in.reshape(height, width), last_in=last_in.reshape(height, width))
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


# ------------------------------------------------------------------------------------------ where the clip decides
# The cases of test_tsdf_render.py (which proves on the CPU that they bite), test_gpu_tsdf_render.py and test_gpu_tsdf_sparse_render.py.
# Voxels of 2^-4 m and origins, camera centres, t_min and steps on multiples of 2^-6 m: a camera on a lattice line that looks along an
# axis has o, e_axis = +-16 and every t_k exact, so a sample lies ON a face of the box, not near it.
CLIP_H, CLIP_W = 23, 37
CLIP_VOXEL = 0.0625
CLIP_DIMS = (24, 16, 16)
CLIP_ORIGIN = (-0.75, -0.5, 1.0)
CLIP_CENTRE = (12.0, 8.0, 8.0)                 # a lattice point in the middle of CLIP_DIMS, in voxels
NEAR, FAR_SIDE = 0.3, -0.7                     # tsdf either side of a surface at 0.3 of a cell


def layer_volume(dims, axis, high, leave=False, colour=True):
    """All seen (weights 1 .. 3).  With d the distance of a voxel's layer from the low (`high`: the high) face of `axis`: positive at
    d = 0 and negative behind it, the surface at about 0.3 of the first cell layer behind that face - or, with `leave`, negative at
    d = 0 and positive everywhere else, the surface in the last cell layer a ray towards that face crosses.  The magnitudes vary by a
    few per cent from voxel to voxel, so that normals and interpolation fractions matter; a colour pattern."""
    vol = ref.new_volume(dims, CLIP_ORIGIN, CLIP_VOXEL, 3 * CLIP_VOXEL, colour=colour)
    z, y, x = np.meshgrid(*(np.arange(n) for n in dims[::-1]), indexing="ij")
    d = (x, y, z)[axis]
    d = dims[axis] - 1 - d if high else d
    base = np.where(d == 0, FAR_SIDE if leave else NEAR, NEAR if leave else FAR_SIDE)
    vol["tsdf"] = (base * (1.0 + 0.04 * ((3 * x + 5 * y + z) % 7))).astype(F)
    vol["weight"] = (1 + (x + 2 * y + 3 * z) % 3).astype(F)
    if colour:
        vol["colour"][..., 0], vol["colour"][..., 1], vol["colour"][..., 2] = (x * 11 + z) % 256, (y * 13 + z * 3) % 256, (x + y + z * 7) % 256
    return vol


def sparse_negative_volume(dims, seed, negative=0.005):
    """Nothing like a scene: independent voxels, about one in 200 negative (-1 .. -0.3, the others 0.02 .. 1), weights 3, one in ten 1,
    a few 0 (unseen), random colours.  A brick holds a seen negative voxel or not by chance."""
    rng = np.random.default_rng(seed)
    vol = ref.new_volume(dims, CLIP_ORIGIN, CLIP_VOXEL, 3 * CLIP_VOXEL)
    shape = vol["tsdf"].shape
    vol["tsdf"] = np.where(rng.random(shape) < negative, -0.3 - 0.7 * rng.random(shape), 0.02 + 0.98 * rng.random(shape)).astype(F)
    draw = rng.random(shape)
    vol["weight"] = np.where(draw < 0.03, 0.0, np.where(draw < 0.13, 1.0, 3.0)).astype(F)
    vol["colour"][..., :3] = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    return vol


def at_voxels(g, origin=CLIP_ORIGIN, voxel=CLIP_VOXEL):
    """The world position of the point g (in voxels) of a volume at `origin`."""
    return tuple(float(o) + float(v) * voxel for o, v in zip(origin, g))


def axis_pose(axis, sign, centre, turn=(0.0, 0.0)):
    """Camera -> world (4, 4) fp32 of a camera at `centre` (world) that looks along sign * e_axis: its x axis is e_(axis + 1), its y axis
    sign * e_(axis + 2), so the other entries of the rotation are exactly 0.  `turn` = (about its own y, then about its own x), radians."""
    r = np.zeros((3, 3))
    r[(axis + 1) % 3, 0], r[(axis + 2) % 3, 1], r[axis, 2] = 1.0, sign, sign
    ay, ax = turn
    if ay or ax:
        ry = np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]])
        rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
        r = r @ ry @ rx
    t = np.eye(4)
    t[:3, :3], t[:3, 3] = r, centre
    return t.astype(F)


def _on_axis(axis, value, centre=CLIP_CENTRE):
    return tuple(value if a == axis else c for a, c in enumerate(centre))


def _face_name(axis, high):
    return "xyz"[axis] + ("hi" if high else "lo")


def _t_max_at_hit(case, below):
    """t_max = the fp32 t_k of the hit sample of `case` with a generous range (every hit ray of these views hits at the same k), or
    the float just below it."""
    full = render(case["volume"](), case["pose"], case["intrinsics"], CLIP_H, CLIP_W, case["t_min"], 4.0, case["step"])
    ks = np.unique(full["hit_k"][full["hit"]])
    assert len(ks) == 1, ks
    t = F(case["t_min"]) + F(ks[0]) * F(case["step"])
    return float(np.nextafter(t, F(0.0)) if below else t)


def _clip_cases():
    V, dims, cases = CLIP_VOXEL, CLIP_DIMS, []
    volume = functools.lru_cache(maxsize=None)(layer_volume)
    noise = functools.lru_cache(maxsize=None)(sparse_negative_volume)

    def add(group, name, vol, pose, intrinsics, t_min, t_max, step):
        cases.append(dict(group=group, id=f"{group}-{name}", volume=vol, pose=pose, intrinsics=intrinsics, t_min=t_min, t_max=t_max, step=step))

    wide, narrow = (40.0, 40.0, 18.0, 11.0), (80.0, 80.0, 18.0, 11.0)          # integer principal point: row 11 and column 18 are axis-parallel
    for axis in range(3):
        n = dims[axis]
        for high in (False, True):
            face, sign = _face_name(axis, high), (-1.0 if high else 1.0)       # the camera looks at the face from 16 voxels outside
            outside = at_voxels(_on_axis(axis, n - 1 + 16.0 if high else -16.0))
            enter = functools.partial(volume, dims, axis, high)
            # 1. entering: half-voxel steps.  Low faces: sample 16 lies ON the face (tsdf 0.3), sample 17 half a voxel in (negative):
            # the hit's `prev` is the first sample in the box.  High faces: the box of the clip ends at n_a, a voxel beyond the last
            # cell, so there it is t_min that puts sample 0 a quarter voxel inside the first cell layer; "face" below has the same view
            # with the face deciding (two samples spare under an exact clip).
            add(1, f"enter-{face}", enter, axis_pose(axis, sign, outside), wide, (16.25 if high else 8.0) * V, (n + 18) * V, V / 2)
            if high:
                add(3, f"enter-{face}-face", enter, axis_pose(axis, sign, outside), wide, 8.25 * V, (n + 18) * V, V / 2)
            # 3. the same volume from a camera turned half a radian, 18 voxels from the middle of the face: edges and corners of the box
            middle = np.array(_on_axis(axis, n - 1.0 if high else 0.0))
            turned = axis_pose(axis, sign, (0, 0, 0), turn=(0.5, -0.35))
            centre = at_voxels(middle - 18.0 * turned[:3, 2].astype(np.float64))
            add(3, f"oblique-{face}", enter, axis_pose(axis, sign, centre, turn=(0.5, -0.35)), (25.0, 25.0, 18.0, 11.0), 0.0, 48 * V, V / 2)
            # 2. leaving through this face: steps of 2.5 voxels from a camera beyond the opposite face.  Low faces: a sample lies ON the face,
            # in the negative layer: the hit sample is the last one in the box.  High faces: the last cell ends a voxel before the clip's
            # box, so the hit sample (half a voxel before the last layer) is made the last by t_max; "face" has the face deciding.
            leave = functools.partial(volume, dims, axis, high, True)
            opposite = at_voxels(_on_axis(axis, -16.0 if high else n - 1 + 16.0))
            reach = n + 14.5 if high else n + 15.0                              # voxels from the camera to the hit sample
            t_min = (reach % 2.5) * V
            add(2, f"leave-{face}", leave, axis_pose(axis, -sign, opposite), narrow, t_min, (reach if high else reach + 3) * V, 2.5 * V)
            if high:
                add(3, f"leave-{face}-face", leave, axis_pose(axis, -sign, opposite), narrow, t_min, (reach + 3) * V, 2.5 * V)
    # 3. origins on the box: a camera centre exactly on the x = 0 face (column 18 runs in the face, the columns left of it leave at once),
    # and one exactly on an interior lattice point with t_min = 0
    leave_z = functools.partial(volume, dims, 2, True, True)
    add(3, "centre-on-face", leave_z, axis_pose(2, 1.0, at_voxels((0.0, 7.5, 2.25))), narrow, 0.0, 16 * V, V / 2)
    add(3, "centre-on-lattice", leave_z, axis_pose(2, 1.0, at_voxels((12.0, 8.0, 4.0)), turn=(0.5, 0.2)), wide, 0.0, 24 * V, V / 2)
    # 4. beside the box, looking along it: column 18 has e_x == 0 and o_x outside (the `empty` branch), its neighbours enter through the side
    for high in (False, True):
        beside = at_voxels((dims[0] + 0.5 if high else -0.5, 8.25, -16.0))
        add(4, f"beside-{_face_name(0, high)}", functools.partial(volume, dims, 0, high), axis_pose(2, 1.0, beside), wide, 8 * V, 40 * V, V / 2)
    # 5. thin volumes: two voxels are one cell layer (lim = 0), one voxel is none (lim = -1)
    for axis, thin in ((2, (24, 16, 2)), (0, (2, 16, 16))):
        vol = functools.partial(volume, thin, axis, False)
        outside = at_voxels(_on_axis(axis, -16.0))
        add(5, f"two-{'xyz'[axis]}", vol, axis_pose(axis, 1.0, outside), wide, 8 * V, 20 * V, V / 2)
        add(5, f"two-{'xyz'[axis]}-oblique", vol, axis_pose(axis, 1.0, at_voxels(_on_axis(axis, -6.0)), turn=(0.9, 0.3)), wide, 0.0, 40 * V, V / 4)
    for axis, thin in ((2, (24, 16, 1)), (0, (1, 16, 16))):
        add(5, f"one-{'xyz'[axis]}", functools.partial(volume, thin, (axis + 1) % 3, False), axis_pose(axis, 1.0, at_voxels(_on_axis(axis, -16.0))),
            wide, 8 * V, 20 * V, V / 2)
    # 6. far cameras: 600 m and 60 km from the z = 0 face, off the lattice, the focal length grown with the distance; steps of 0.05 voxel,
    # 1500 samples from just in front of the box.  At 60 km an ulp of t is longer than the step.
    for name, distance in (("600m", 600.0), ("60km", 60000.0)):
        focal = 24.0 * distance
        far = (CLIP_ORIGIN[0] + 12.3 * V, CLIP_ORIGIN[1] + 7.8 * V, CLIP_ORIGIN[2] - distance)
        step = 0.05 * V
        t_min = float(F(distance - 3 * V))
        t_max = float(F(t_min) + F(1499) * F(step))
        add(6, f"far-{name}", functools.partial(volume, dims, 2, False), axis_pose(2, 1.0, far), (focal, focal, 18.0, 11.0), t_min, t_max, step)
    # 7. where t_max decides: the z-low entering view off the lattice in t; t_max the fp32 t_k of the hit sample, and the float below it
    base = dict(volume=functools.partial(volume, dims, 2, False), pose=axis_pose(2, 1.0, at_voxels(_on_axis(2, -16.0))), intrinsics=wide,
                t_min=0.47, step=0.03)
    for name, below in (("found", False), ("lost", True)):
        add(7, f"t_max-{name}", base["volume"], base["pose"], wide, 0.47, functools.partial(_t_max_at_hit, base, below), 0.03)
    # 8. poses that are no rotation, on the fused SMALL volume round the origin and far from it (tests/tsdf_fusion_ref.py)
    for kind in ("scaled", "sheared", "wild"):
        for world, shift in (("origin", ref.ORIGIN), ("far", ref.FAR)):
            frames, ks = ref.camera_cases(ref.SMALL, 0, kind, shift=shift)
            for j, ((pose, _, _), k) in enumerate(zip(frames, ks)):
                add(8, f"{kind}-{world}-{j}", functools.partial(fused_small, shift), pose, k, 0.0, 3.0, 0.06)
            # those look anywhere; the middle pose of the arc, its rotation block scaled the same way, sees the scene
            arc = ref.arc_poses()[5].astype(np.float64)
            arc[:3, :3] *= dict(scaled=1.5, sheared=np.array([0.8, 1.0, 1.3]), wild=3.0)[kind]
            arc[:3, 3] += np.asarray(shift)
            add(8, f"{kind}-{world}-arc", functools.partial(fused_small, shift), arc.astype(F), ref.INTRINSICS_60, 0.0, 6.0, 0.06)
    # the brick rule where the volume is no scene (the cases of the brick tests, marched like any other)
    for dims_n, seed in (((37, 19, 17), 1), ((9, 6, 5), 3)):                 # seeds whose views have hits at min_weight 0 and 1
        vol = functools.partial(noise, dims_n, seed)
        middle = tuple((n - 1) / 2 + 0.3 for n in dims_n)
        add("noise", "x".join(map(str, dims_n)), vol, axis_pose(2, 1.0, at_voxels(_on_axis(2, -6.0, middle)), turn=(0.2, 0.1)),
            (30.0, 30.0, 18.0, 11.0), 0.0, 40 * V, V / 2)
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


_FUSED = {}


def fused_small(shift=ref.ORIGIN):
    """ref.SMALL after the ten arc frames that see the scene (60-pixel focal length), its origin moved by `shift`: the same voxels
    in another world."""
    if "vol" not in _FUSED:
        vol = ref.new_volume(**ref.SMALL)
        for pose, depth, image in ref.make_frames(ref.INTRINSICS_60)[:10]:
            ref.integrate(vol, ref.world_to_camera(pose), ref.INTRINSICS_60, depth, image)
        _FUSED["vol"] = vol
    key = tuple(shift)
    if key not in _FUSED:
        _FUSED[key] = dict(_FUSED["vol"], origin=tuple(F(v) for v in ref.shifted(ref.SMALL, shift)["origin"]))
    return _FUSED[key]


CLIP_CASES = _clip_cases()


def case_inputs(case):
    """(volume dict, pose, intrinsics, (t_min, t_max, step)) of a CLIP_CASES entry; volumes and a derived t_max are made once."""
    if callable(case["t_max"]):
        case["t_max"] = case["t_max"]()
    return case["volume"](), case["pose"], case["intrinsics"], (case["t_min"], case["t_max"], case["step"])
