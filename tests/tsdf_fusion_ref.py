"""Helper of test_tsdf_fusion.py / test_gpu_tsdf_fusion.py: the arithmetic of mr_tsdf_integrate_f32 / mr_tsdf_extract_f32 as
include/monorec_hip.h states it, restated in numpy - every array is float32, so every operation is rounded on its own, in the order
of the header - and a small analytic scene (a wall and a sphere seen by a pinhole camera) to feed it."""
import numpy as np

F = np.float32


def roundf(x):
    """C roundf (halves away from zero) from floor / abs / copysign; the fraction `|x| - floor(|x|)` is exact in fp32."""
    with np.errstate(invalid="ignore"):                          # inf - inf
        a = np.abs(x)
        whole = np.floor(a)
        return np.copysign(whole + ((a - whole) >= F(0.5)).astype(F), x)


# ------------------------------------------------------------------------------------------ the volume
def new_volume(dims, origin, voxel_size, trunc, colour=True, offset=(0, 0, 0)):
    """`offset`: the volume restates the block of `dims` voxels that starts at voxel index `offset` of a larger volume at `origin`."""
    nx, ny, nz = dims
    return dict(dims=(nx, ny, nz), origin=tuple(F(v) for v in origin), voxel=F(voxel_size), trunc=F(trunc), offset=tuple(offset),
                tsdf=np.ones((nz, ny, nx), F), weight=np.zeros((nz, ny, nx), F),
                colour=np.zeros((nz, ny, nx, 4), np.uint8) if colour else None)


def copy_volume(vol):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vol.items()}


def positions(vol):
    """p_a = origin_a + (float)i_a * voxel_size as broadcastable (1,1,nx), (1,ny,1), (nz,1,1) arrays."""
    nx, ny, nz = vol["dims"]
    ox, oy, oz = vol["origin"]
    x0, y0, z0 = vol.get("offset", (0, 0, 0))
    px = (ox + np.arange(x0, x0 + nx, dtype=F) * vol["voxel"]).reshape(1, 1, nx)
    py = (oy + np.arange(y0, y0 + ny, dtype=F) * vol["voxel"]).reshape(1, ny, 1)
    pz = (oz + np.arange(z0, z0 + nz, dtype=F) * vol["voxel"]).reshape(nz, 1, 1)
    return px, py, pz


def world_to_camera(cam_to_world):
    """The 3 x 4 fp32 matrix the host passes: torch.inverse(cam_to_world) in fp32."""
    import torch
    return torch.inverse(torch.as_tensor(np.asarray(cam_to_world, dtype=F)).reshape(4, 4))[:3, :4].numpy().copy()


def integrate(vol, m, intrinsics, depth_cm, colour, max_depth_m=np.inf):
    """One frame into `vol`, in place.  m: (3, 4) fp32 world -> camera; intrinsics (fx, fy, cx, cy); depth_cm (h, w) int16; colour
    (h, w, 3) uint8 or None.  Returns the masks of what happened: dict(behind, outside, nodepth, occluded, updated, band, clamped)."""
    m = np.asarray(m, dtype=F)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    h, w = depth_cm.shape
    px, py, pz = positions(vol)
    shape = vol["tsdf"].shape
    with np.errstate(all="ignore"):
        cam = [np.broadcast_to(((m[r, 0] * px + m[r, 1] * py) + m[r, 2] * pz) + m[r, 3], shape) for r in range(3)]
        front = cam[2] > 0
        u = roundf(fx * (cam[0] / cam[2]) + cx)
        v = roundf(fy * (cam[1] / cam[2]) + cy)
        inside = front & (u >= 0) & (u < F(w)) & (v >= 0) & (v < F(h))
        ui = np.where(inside, u, F(0)).astype(np.int64)
        vi = np.where(inside, v, F(0)).astype(np.int64)
        d = depth_cm[vi, ui].astype(F) / F(100.0)
        has_depth = inside & ~(d <= 0) & ~(d > F(max_depth_m))
        diff = d - cam[2]
        updated = has_depth & ~(diff <= -vol["trunc"])
        dist = np.minimum(F(1.0), diff / vol["trunc"])
        w_old = vol["weight"]
        w_new = w_old + F(1.0)
        tsdf = (vol["tsdf"] * w_old + dist) / w_new
        if vol["colour"] is not None:
            for c in range(3):
                blend = np.minimum(F(255.0), np.floor((vol["colour"][..., c].astype(F) * w_old + colour[vi, ui, c].astype(F)) / w_new + F(0.5)))
                vol["colour"][..., c] = np.where(updated, blend, vol["colour"][..., c].astype(F)).astype(np.uint8)
        vol["tsdf"] = np.where(updated, tsdf, vol["tsdf"]).astype(F)
        vol["weight"] = np.where(updated, w_new, w_old).astype(F)
    assert vol["tsdf"].dtype == F and tsdf.dtype == F and dist.dtype == F and u.dtype == F
    return dict(behind=~front, outside=front & ~inside, nodepth=inside & ~has_depth, occluded=has_depth & ~updated, updated=updated,
                band=updated & (dist < 1), clamped=updated & ~(dist < 1), inside=inside)


def extract(vol, min_weight=0.0):
    """Every edge crossing as (n, 6) fp32 records x y z red green blue, in no particular order."""
    px, py, pz = positions(vol)
    shape = vol["tsdf"].shape
    pos = [np.broadcast_to(p, shape) for p in (px, py, pz)]
    records = []
    for axis, dim in ((0, 2), (1, 1), (2, 0)):                 # x is the last array dimension
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[dim], hi[dim] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        tv, tn = vol["tsdf"][lo], vol["tsdf"][hi]
        hit = (vol["weight"][lo] > F(min_weight)) & (vol["weight"][hi] > F(min_weight)) & ((tv < 0) != (tn < 0))
        with np.errstate(all="ignore"):
            s = tv / (tv - tn)
            rec = np.zeros(tv.shape + (6,), F)
            for a in range(3):
                rec[..., a] = pos[a][lo]
            rec[..., axis] = pos[axis][lo] + s * vol["voxel"]
            if vol["colour"] is not None:
                for c in range(3):
                    cv, cn = vol["colour"][lo + (c,)].astype(F), vol["colour"][hi + (c,)].astype(F)
                    rec[..., 3 + c] = np.floor(cv + s * (cn - cv) + F(0.5))
        records.append(rec[hit])
    return np.concatenate(records).astype(F)


def sort_records(records):
    """Records in a canonical order (the device's order is unspecified)."""
    records = np.asarray(records, dtype=F).reshape(-1, 6)
    return records[np.lexsort(tuple(records[:, k] for k in range(5, -1, -1)))]


# ------------------------------------------------------------------------------------------ volumes loaded directly
def crossing_owners(vol, min_weight=0.0):
    """[x, y, z] boolean (nz, ny, nx) arrays: voxel v owns a crossing along that axis (`extract`'s rule, on v and v + e_axis)."""
    seen, neg = vol["weight"] > F(min_weight), vol["tsdf"] < 0
    owners = []
    for dim in (2, 1, 0):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[dim], hi[dim] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        own = np.zeros(seen.shape, bool)
        own[lo] = seen[lo] & seen[hi] & (neg[lo] != neg[hi])
        owners.append(own)
    return owners


def slab(dims, axis, zero=False):
    """All seen; negative on the low half of `axis` (or 0 everywhere)."""
    vol = new_volume(dims, (-0.3, 0.2, 1.0), 0.06, 0.18)
    index = np.arange(dims[axis]).reshape([-1 if k == 2 - axis else 1 for k in range(3)])
    vol["tsdf"] = np.broadcast_to(np.where(index < dims[axis] // 2, -0.25, 0.5), vol["tsdf"].shape).astype(F)
    if zero:
        vol["tsdf"] = np.zeros_like(vol["tsdf"])
    vol["weight"] = np.ones_like(vol["tsdf"])
    vol["colour"][..., :3] = 90
    return vol


def seam_volume(dims, colour=True, seed=0):
    """A closed surface across every kind of seam of the 32 x 8 x 4 tiles of a volume a little larger than whole tiles: the union of a
    ball in the low x third of the volume and of balls of 0.7 voxels round single voxels - the last of the first tile (31, 7, 3), the
    first past it (32, 8, 4) and the volume's last - so that edges 31|32, 7|8, 3|4 and last-but-one|last along x, y, z are crossed.
    tsdf = clip(distance / 3 voxels, -1, 1); weights 3, about one in ten 1, a few 0 (unseen), all 3 next to the small balls; random
    colours."""
    nx, ny, nz = dims
    vol = new_volume(dims, (-0.3, 0.2, 1.0), 0.06, 0.18, colour=colour)
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    marks = [(31, 7, 3), (32, 8, 4), (nx - 1, ny - 1, nz - 1)]
    balls = [(0.3 * (nx - 1), (ny - 1) / 2 + 0.1, (nz - 1) / 2 - 0.2, 0.45 * min(dims) + 0.3)] + [m + (0.7,) for m in marks]
    dist = np.min([np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r for cx, cy, cz, r in balls], axis=0)
    vol["tsdf"] = np.clip(dist / 3.0, -1.0, 1.0).astype(F)
    draw = rng.random((nz, ny, nx))
    vol["weight"] = np.where(draw < 0.03, 0.0, np.where(draw < 0.13, 1.0, 3.0)).astype(F)
    for mx, my, mz in marks:
        vol["weight"][max(mz - 1, 0):mz + 2, max(my - 1, 0):my + 2, max(mx - 1, 0):mx + 2] = 3.0
    if colour:
        vol["colour"][..., :3] = rng.integers(0, 256, size=(nz, ny, nx, 3), dtype=np.uint8)
    return vol


SEAM_DIMS = [(33, 9, 5), (34, 10, 6), (65, 17, 9)]


# ------------------------------------------------------------------------------------------ the scene
WALL_Z = 3.0
SPHERE = (0.1, -0.05, 2.95, 0.45)              # centre and radius; it pokes through the wall


def surface_distance(points):
    """Distance of world points to the visible surface (wall z = WALL_Z or the sphere), in double."""
    p = np.asarray(points, dtype=np.float64)
    to_sphere = np.abs(np.linalg.norm(p[..., :3] - np.array(SPHERE[:3]), axis=-1) - SPHERE[3])
    return np.minimum(np.abs(p[..., 2] - WALL_Z), to_sphere)


def arc_poses(count=11, radius=0.35):
    """Camera -> world poses (4, 4) fp32 on a small arc round the z axis at z = 0, looking at (0, 0, 3); the LAST one looks away from
    the scene (turned half round about y): every voxel of the test volumes is behind it."""
    poses = []
    for i in range(count):
        a = -0.5 + i / max(count - 2, 1)                       # -0.5 .. 0.5 over the first count - 1 poses
        centre = np.array([radius * np.sin(2 * a), 0.1 * a, 0.0])
        z = np.array([0.0, 0.0, 3.0]) - centre
        if i == count - 1:
            z = -z
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        t = np.eye(4)
        t[:3, 0], t[:3, 1], t[:3, 2], t[:3, 3] = x, y, z, centre
        poses.append(t.astype(F))
    return poses


def render(pose, intrinsics, height, width, zero_rows=(3, 17)):
    """(depth_cm (h, w) int16, colour (h, w, 3) uint8) of the scene from `pose`: the camera-z depth of the nearest hit in centimetres
    (0 where the ray hits nothing in front of the camera, and on `zero_rows`), and a colour pattern that depends on pixel and pose."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    t = np.asarray(pose, dtype=np.float64)
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    rays = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ t[:3, :3].T        # per unit of camera z
    c = t[:3, 3]
    with np.errstate(all="ignore"):
        wall = (WALL_Z - c[2]) / rays[..., 2]
        oc = c - np.array(SPHERE[:3])
        qa, qb, qc = (rays * rays).sum(-1), 2 * (rays @ oc), oc @ oc - SPHERE[3] ** 2
        disc = qb * qb - 4 * qa * qc
        sphere = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
    wall = np.where(wall > 0, wall, np.inf)
    sphere = np.where(sphere > 0, sphere, np.inf)
    depth = np.minimum(wall, sphere)
    depth_cm = np.where(np.isfinite(depth), np.round(depth * 100), 0).clip(0, 32767).astype(np.int16)
    for r in zero_rows:
        if r < height:
            depth_cm[r] = 0
    shade = int(round(float(t[0, 3]) * 100)) % 40
    colour = np.stack([(u * 6 + v * 3 + shade) % 256, (u * 2 + v * 9 + 40) % 256, (255 - u * 5 + v + shade) % 256], axis=-1).astype(np.uint8)
    return depth_cm, colour


def make_frames(intrinsics, height=24, width=40, count=11):
    """[(cam_to_world fp32 (4, 4), depth_cm, colour)] of arc_poses."""
    return [(pose,) + render(pose, intrinsics, height, width) for pose in arc_poses(count)]


# the two volumes of the tests: odd nx (the scalar tail, rows off the 16-byte boundary); nx a multiple of 4 and wider than any frustum
SMALL = dict(dims=(37, 21, 13), origin=(-1.1, -0.6, 2.45), voxel_size=0.06, trunc=0.18)
WIDE = dict(dims=(128, 24, 12), origin=(-3.81, -0.7, 2.5), voxel_size=0.06, trunc=0.18)
INTRINSICS_30 = (30.0, 30.0, 19.5, 11.5)
INTRINSICS_60 = (60.0, 60.0, 19.5, 11.5)


# ------------------------------------------------------------------------------------------ hard cameras
CAMERA_KINDS = ("rigid", "scaled", "sheared", "wild", "offcentre", "aniso")
ORIGIN, FAR = (0.0, 0.0, 0.0), (812.3, -41.7, 1203.9)      # the two worlds: round the origin, and where an fp32 ulp is a tenth of a millimetre
CASE_H, CASE_W = 24, 40


def shifted(spec, shift):
    """`spec` moved by `shift` metres."""
    return dict(spec, origin=tuple(float(o) + float(s) for o, s in zip(spec["origin"], shift)))


def camera_cases(spec, seed, kind="rigid", max_depth_m=None, shift=ORIGIN):
    """Eight cameras for culling to be wrong about, for the volume `shifted(spec, shift)`: (frames, ks), frames = [(cam_to_world (4, 4)
    fp32, depth_cm (24, 40) int16, colour (24, 40, 3) uint8)] and ks = [(fx, fy, cx, cy)], one per frame.
    Centres uniform in the volume's box grown by 0.3 m, turned any way (the Q of a normal matrix, det +1), fx from {12, 30, 90} and
    fy = 1.1 fx, the principal point within a pixel of the middle, depth uniform in 20 .. 400 cm with one pixel in ten 0, random colours.
    The outermost ring of every depth map holds min(max_depth_m, 4 m) - written before the zeros are drawn -, so that voxels out to
    max_depth_m + trunc along the corner rays are updated.  `kind`:
      rigid      as above
      scaled     the rotation block of cam_to_world times 1.5 (even frames) or 0.7 (odd): world -> camera has rows of 0.67 or 1.43
      sheared    its columns times 0.8, 1.0, 1.3
      wild       times 3: the rows of world -> camera are 1 / 3 long, beyond what culling takes for a rotation
      offcentre  on frames 0, 2, 4, 6 the principal point outside the image: cx from {-15, w + 10}, cy from {-9, h + 6}
      aniso      fy = 4 fx"""
    assert kind in CAMERA_KINDS, kind
    rng = np.random.default_rng(seed)
    h, w = CASE_H, CASE_W
    lo = np.array(shifted(spec, shift)["origin"], dtype=np.float64)
    hi = lo + (np.array(spec["dims"]) - 1) * spec["voxel_size"]
    depth = rng.integers(20, 400, size=(8, h, w)).astype(np.int16)
    ring = int(round(100 * min(np.inf if max_depth_m is None else float(max_depth_m), 4.0)))
    depth[:, 0, :] = depth[:, -1, :] = ring
    depth[:, :, 0] = depth[:, :, -1] = ring
    depth[rng.random((8, h, w)) < 0.1] = 0
    image = rng.integers(0, 256, size=(8, h, w, 3)).astype(np.uint8)
    frames, ks = [], []
    for i in range(8):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        centre = lo - 0.3 + rng.random(3) * (hi - lo + 0.6)
        focal = float(rng.choice([12.0, 30.0, 90.0]))
        cx, cy = 19.5 + rng.normal(), 11.5 + rng.normal()
        out_x, out_y = float(rng.choice([-15.0, w + 10.0])), float(rng.choice([-9.0, h + 6.0]))
        if kind == "scaled":
            q = q * (1.5 if i % 2 == 0 else 0.7)
        elif kind == "sheared":
            q = q * np.array([0.8, 1.0, 1.3])
        elif kind == "wild":
            q = q * 3.0
        elif kind == "offcentre" and i % 2 == 0:
            cx, cy = out_x, out_y
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = q, centre
        frames.append((pose.astype(F), depth[i], image[i]))
        ks.append((focal, focal * (4.0 if kind == "aniso" else 1.1), float(cx), float(cy)))
    return frames, ks


def k_matrix(k):
    """(fx, fy, cx, cy) as the 3 x 3 matrix."""
    fx, fy, cx, cy = k
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)
