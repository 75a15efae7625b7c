"""Helper of test_depth_consistency.py / test_gpu_depth_consistency.py: the arithmetic of mr_depth_consistency_f32 as
include/monorec_hip.h states it, restated in numpy - every array is float32, so every operation is rounded on its own, in the order of
the header - on the analytic scene of tests/tsdf_fusion_ref.py (a wall and a sphere seen from an arc of cameras)."""
import numpy as np

from tsdf_fusion_ref import F, FAR, INTRINSICS_30, ORIGIN, SMALL, arc_poses, camera_cases, make_frames, render, roundf  # noqa: F401

OUTCOMES = ("behind", "outside", "nodepth", "depth", "reproj", "hit")


def valid_depth(inv):
    """(valid, d): inv > 0 and d = 1 / inv finite and > 0."""
    with np.errstate(all="ignore"):
        d = F(1.0) / inv
        return (inv > 0) & (d > 0) & np.isfinite(d), d


def _rows(m, x, y, z):
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]


def filter_depth(inv_depth, intrinsics, views, rel_tol, max_reproj_px, min_views, average):
    """inv_depth (h, w) fp32; intrinsics (fx, fy, cx, cy); views: [(m (3, 4), back (3, 4), (fx, fy, cx, cy), inv_depth_j (h, w))] in launch
    order.  Returns (out (h, w) fp32, hits (h, w) uint8, [per view: dict of the boolean outcome masks OUTCOMES over the VALID reference
    pixels - exactly one of them holds at each -, and of the values the decisions were taken on: u_raw / v_raw (before roundf), q2, dn,
    diff (|dn - q2|), bound (rel_tol * q2), err2 (ex * ex + ey * ey)])."""
    inv = np.asarray(inv_depth)
    assert inv.dtype == F and inv.ndim == 2
    h, w = inv.shape
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    rel_tol, reproj = F(rel_tol), F(max_reproj_px)
    x = np.broadcast_to(np.arange(w, dtype=F).reshape(1, w), (h, w))
    y = np.broadcast_to(np.arange(h, dtype=F).reshape(h, 1), (h, w))
    traces = []
    with np.errstate(all="ignore"):
        valid, d = valid_depth(inv)
        X, Y, Z = ((x - cx) / fx) * d, ((y - cy) / fy) * d, d
        total, n = d.copy(), np.zeros((h, w), np.int32)
        for m, back, kj, inv_j in views:
            m, back, inv_j = np.asarray(m, dtype=F).reshape(3, 4), np.asarray(back, dtype=F).reshape(3, 4), np.asarray(inv_j)
            assert inv_j.dtype == F and inv_j.shape == (h, w)
            fxj, fyj, cxj, cyj = (F(v) for v in kj)
            q = _rows(m, X, Y, Z)
            front = valid & (q[2] > 0)
            u_raw, v_raw = fxj * (q[0] / q[2]) + cxj, fyj * (q[1] / q[2]) + cyj
            u, v = roundf(u_raw), roundf(v_raw)
            inside = front & (u >= 0) & (u < F(w)) & (v >= 0) & (v < F(h))
            ui, vi = np.where(inside, u, F(0)).astype(np.int64), np.where(inside, v, F(0)).astype(np.int64)
            valid_n, dn = valid_depth(inv_j[vi, ui])
            has_depth = inside & valid_n
            diff, bound = np.abs(dn - q[2]), rel_tol * q[2]
            agrees = has_depth & (diff <= bound)
            Xn, Yn = ((u - cxj) / fxj) * dn, ((v - cyj) / fyj) * dn
            p = _rows(back, Xn, Yn, dn)
            hit = agrees & (p[2] > 0)
            ex, ey = (fx * (p[0] / p[2]) + cx) - x, (fy * (p[1] / p[2]) + cy) - y
            err2 = ex * ex + ey * ey
            if not np.isposinf(reproj):
                hit = hit & (err2 <= reproj * reproj)
            n = n + hit
            total = np.where(hit, total + p[2], total)
            for a in (u_raw, q[2], dn, diff, bound, err2, total):
                assert a.dtype == F
            traces.append(dict(behind=valid & ~front, outside=front & ~inside, nodepth=inside & ~has_depth, depth=has_depth & ~agrees,
                               reproj=agrees & ~hit, hit=hit, u_raw=u_raw, v_raw=v_raw, q2=q[2], dn=dn, diff=diff, bound=bound, err2=err2))
        kept = valid & (n >= int(min_views))
        value = F(1.0) / (total / (1 + n).astype(F)) if average else inv
        out = np.where(kept, value, F(0)).astype(F)
    return out, n.astype(np.uint8), traces


def relative(pose, pose_j):
    """(m, back) (3, 4) fp32: neighbour camera <- reference camera and its inverse, from the camera -> world poses in double, rounded once."""
    m = np.linalg.inv(np.asarray(pose_j, dtype=np.float64).reshape(4, 4)) @ np.asarray(pose, dtype=np.float64).reshape(4, 4)
    return m[:3].astype(F), np.linalg.inv(m)[:3].astype(F)


def inverse_depth(depth_cm):
    """The scene's inverse depth: 100 / depth_cm in fp32, 0 where there is no depth."""
    cm = np.asarray(depth_cm).astype(F)
    with np.errstate(all="ignore"):
        return np.where(cm > 0, F(100.0) / cm, F(0)).astype(F)


def outcome_counts(traces):
    return {name: int(sum(t[name].sum() for t in traces)) for name in OUTCOMES}


def scene(reference, neighbours, count=11, radius=0.35, intrinsics=INTRINSICS_30, height=24, width=40):
    """The arc scene at one size: (inv_depth of frame `reference`, its pose, [(inv_depth_j, pose_j) for j in neighbours])."""
    poses = arc_poses(count, radius)
    maps = {j: inverse_depth(render(poses[j], intrinsics, height, width)[0]) for j in [reference] + list(neighbours)}
    return maps[reference], poses[reference], [(maps[j], poses[j]) for j in neighbours]


def views_of(pose, neighbours, intrinsics):
    """`scene`'s neighbours (or any [(inv_depth_j, pose_j)]) as filter_depth's views, all with the same intrinsics."""
    return [relative(pose, pose_j) + (intrinsics, inv_j) for inv_j, pose_j in neighbours]


# the two scenes of the issue
SCENE_A = dict(reference=5, neighbours=(3, 4, 6, 10), radius=1.0, rel_tol=0.01, max_reproj_px=0.5)
SCENE_B = dict(reference=4, neighbours=(2, 3, 5, 6), radius=0.35, rel_tol=0.01, max_reproj_px=1.0, min_views=2, block=(8, 14, 10, 20), factor=1.25)
