"""Camera geometries for the cost-volume tests (host side, no GPU), and the projection of the reference restated in plain fp32.

Every other cost-volume test runs on the one geometry monorec_amd.synth.make_batch builds: source frames that differ from the keyframe by a
translation along z (+ 1 cm in x / y), one unskewed upper-triangular K for all images.  There 4 of the 12 entries of every `proj` and 4 of
the 9 of every `kinv` are zero or round-off, the third ray component is exactly 1, no hypothesis lies behind a source camera and no sample
falls on a pixel centre - an error in the terms those zeros multiply is invisible.  The builders here return the same dict:

    general          per-sample keyframe poses (tens of degrees about oblique axes, large translations), every source pose = kf_pose @ rel
                     with rel a rotation of a few degrees about an axis near (1, 2, 3) and a translation in x, y and z, different for every
                     (sample, frame); skewed K with off-centre principal points, different for every image; the last sample's keyframe
                     "intrinsics" is K @ R (a rectifying rotation): all nine kinv entries non-zero.
    general_far      the same with rel at 3 x the angle and 6 x the translation: a good share of the hypotheses lies BEHIND a source camera.
    pixel_exact      identity poses, identity keyframe K, source "intrinsics" [[s, 0, s (.5 + kx)], [0, t, t (.5 + ky)], [0, 0, 1]] with
                     s = (W - 1) / W, t = (H - 1) / H at 32 x 64 and power-of-two depths >= 4 (`exact_depths`): every operation of the chain is
                     exact, the unnormalised sample position is exactly (x + kx, y + ky).  The frame is the keyframe moved by the same shift.
    zero_denominator `general` about an identity keyframe pose; frame 0 has the identity pose too and the third "intrinsics" row
                     (0, 0, 0, -1e-7f): pcz + 1e-7 == 0 at every point.  Frame 1 is an ordinary frame.
    planted_zeros    pixel_exact(0, 0) with frame = keyframe and pixels that are exactly 0 in both images / in the frame only: both clauses of
                     the sfcv_mult_mask=False validity `any(warped != 0) | all(warped == keyframe)` decide somewhere.

The restatement (`rays`, `project`, `div_const`, `unnormalise`, `valid_fma`, `valid_bool`) is written from the reference's lines
(model/layers.py:63-71, model/monorec/monorec_model.py:198-219 and F.grid_sample's unnormalise) in numpy fp32 with an exact fmaf;
tests/test_cost_volume_geometry.py pins it on the CPU oracle bit for bit and shows which mutations of it each geometry can see.  The two
matrix products are k-ascending chains on every host seen, but whether the CPU's matmul FUSES each multiply-add depends on the host
(`host_fuses`): the kernels fuse, as the hosts of the reference fixtures do."""
import functools
import math

import numpy as np
import torch

from pointcloud_paths import fmaf

F32 = np.float32
H_GENERAL, W_GENERAL = 48, 80
H_EXACT, W_EXACT = 32, 64
MUTATIONS = ("r2_one", "x2_depth", "drop_ki1", "swap_p1_p4")


# ---- builders -------------------------------------------------------------------------------------------------------------------------------------
def _rotation(axis, degrees):
    """Rodrigues rotation (3 x 3, float64) about `axis`."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ang = math.radians(degrees)
    return np.eye(3) + math.sin(ang) * ax + (1 - math.cos(ang)) * (ax @ ax)


def _rigid(axis, degrees, translation):
    m = np.eye(4)
    m[:3, :3] = _rotation(axis, degrees)
    m[:3, 3] = translation
    return torch.from_numpy(m).float()


def _intrinsics(h, w, fx, fy, skew, cx, cy):
    """4 x 4 K with skew; focal lengths as fractions of the KITTI example's at this size (synth.make_intrinsics)."""
    k = torch.eye(4, dtype=torch.float32)
    k[0, 0], k[0, 1], k[0, 2] = 489.23 * w / 512.0 * fx, skew, cx * w
    k[1, 1], k[1, 2] = 489.23 * h / 256.0 * fy, cy * h
    return k


def general(b=2, h=H_GENERAL, w=W_GENERAL, frames=2, seed=5, far=False, rig=True):
    """`rig=False`: the keyframe poses are the identity (the source poses are then `rel` itself)."""
    from monorec_amd import synth
    batch = synth.make_batch(b, h, w, frames, seed=seed)          # the textures
    angle, reach = (3.0, 6.0) if far else (1.0, 1.0)
    kf_pose = torch.stack([_rigid((2 - 3 * n, -1 + 4 * n, 3 - n), 35 + 22 * n, (-41.0 + 60 * n, 7.0 - 3 * n, 19.0 + 11 * n)) for n in range(b)])
    if not rig:
        kf_pose = torch.eye(4).repeat(b, 1, 1)
    kf_k = torch.stack([_intrinsics(h, w, 1 + 0.03 * n, 1 - 0.02 * n, 1.3 + 0.4 * n, 0.46 + 0.02 * n, 0.55 - 0.03 * n) for n in range(b)])
    rectify = torch.eye(4)
    rectify[:3, :3] = torch.from_numpy(_rotation((3, 1, 2), 4.0)).float()
    kf_k[b - 1] = kf_k[b - 1] @ rectify                            # "intrinsics" K @ R: a full 3 x 3
    poses, intrs = [], []
    for f in range(frames):
        sign = -1.0 if f % 2 == 0 else 1.0
        step = f // 2 + 1
        rel = torch.stack([_rigid((1 + 0.1 * n, 2 - 0.2 * f, 3), -sign * angle * (1.6 + 0.5 * n + 0.3 * f),
                                  (reach * (0.05 + 0.02 * f - 0.09 * n), reach * (-0.04 + 0.07 * f - 0.01 * n), sign * reach * step * (0.55 + 0.1 * n)))
                           for n in range(b)])
        poses.append((kf_pose @ rel).contiguous())
        intrs.append(torch.stack([_intrinsics(h, w, 1 + 0.02 * f - 0.015 * n, 0.99 + 0.01 * n + 0.015 * f, -0.9 + 0.7 * n + 1.1 * f,
                                              0.52 - 0.03 * n + 0.01 * f, 0.47 + 0.02 * n + 0.02 * f) for n in range(b)]).contiguous())
    batch.update(keyframe_pose=kf_pose.contiguous(), keyframe_intrinsics=kf_k.contiguous(), poses=poses, intrinsics=intrs)
    return batch


def general_far(b=2, h=H_GENERAL, w=W_GENERAL, frames=2, seed=6):
    return general(b, h, w, frames, seed, far=True)


def zero_denominator(b=2, h=H_GENERAL, w=W_GENERAL, seed=7):
    """Frame 0: third "intrinsics" row (0, 0, 0, -1e-7f) and - like the keyframe - the identity pose, whose fp32 inverse is exact, so that
    proj[2] is (0, 0, 0, -1e-7f) to the bit and pcz + 1e-7f is exactly 0 at every point.  (The fp32 inverse of a pose far from the origin
    has a last row that is off by ~1e-7: the sum is then tiny instead of 0 and the quotient finite.)  Frame 1: an ordinary `general` frame."""
    batch = general(b, h, w, 2, seed, rig=False)
    k = batch["intrinsics"][0].clone()
    k[:, 2, :] = torch.tensor([0.0, 0.0, 0.0, -1e-7], dtype=torch.float32)
    batch["intrinsics"] = [k.contiguous(), batch["intrinsics"][1]]
    batch["poses"] = [torch.eye(4).repeat(b, 1, 1), batch["poses"][1]]
    return batch


def exact_depths(d):
    """Powers of two from 4 up: depth * ray and every product with a `proj` entry of pixel_exact are exact, and pcz + 1e-7 == pcz."""
    return torch.tensor([2.0 ** (2 + i) for i in range(d)], dtype=torch.float32)


def per_pixel(depths, b, h, w):
    """The hypothesis ladder `depths` (D) as the per-pixel input (B, D, H, W)."""
    return depths.view(1, -1, 1, 1).expand(b, -1, h, w).contiguous()


def exact_intrinsics(kx, ky, h=H_EXACT, w=W_EXACT):
    s, t = (w - 1) / w, (h - 1) / h
    return torch.tensor([[s, 0, s * (0.5 + kx), 0], [0, t, t * (0.5 + ky), 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64).float()


def pixel_exact(kx, ky, more=(), seed=9):
    """One sample, one source frame per shift ((kx, ky), then `more`).  Frame f is the keyframe moved by the integer part of its shift:
    frame[y + ky, x + kx] = keyframe[y, x] wherever that lands inside the image."""
    from monorec_amd import synth
    h, w = H_EXACT, W_EXACT
    shifts = ((kx, ky),) + tuple(more)
    batch = synth.make_batch(1, h, w, 1, seed=seed)
    eye = torch.eye(4).unsqueeze(0)
    kf = batch["keyframe"]
    batch.update(keyframe_pose=eye.clone(), keyframe_intrinsics=eye.clone(), poses=[eye.clone() for _ in shifts],
                 intrinsics=[exact_intrinsics(sx, sy).unsqueeze(0) for sx, sy in shifts],
                 frames=[torch.roll(kf, shifts=(math.floor(sy) % h, math.floor(sx) % w), dims=(2, 3)).contiguous() for sx, sy in shifts])
    return batch


PLANTED_BOTH = (slice(8, 12), slice(10, 18))          # (rows, columns) exactly 0 in keyframe and frame
PLANTED_FRAME = (slice(18, 22), slice(30, 38))        # exactly 0 in the frame only
PLANTED_PIXELS_BOTH = ((5, 40), (25, 7))
PLANTED_PIXELS_FRAME = ((14, 52), (27, 44))


def planted_zeros(seed=9):
    batch = pixel_exact(0, 0, seed=seed)
    kf = batch["keyframe"].clone()
    assert bool((kf != 0).all())
    kf[0, :, PLANTED_BOTH[0], PLANTED_BOTH[1]] = 0
    for y, x in PLANTED_PIXELS_BOTH:
        kf[0, :, y, x] = 0
    frame = kf.clone()
    frame[0, :, PLANTED_FRAME[0], PLANTED_FRAME[1]] = 0
    for y, x in PLANTED_PIXELS_FRAME:
        frame[0, :, y, x] = 0
    batch.update(keyframe=kf.contiguous(), frames=[frame.contiguous()])
    return batch


def planted_invalid(h=H_EXACT, w=W_EXACT):
    """(H, W) bool: where the sfcv_mult_mask=False validity of planted_zeros is false - the frame is 0 and the keyframe is not."""
    m = np.zeros((h, w), dtype=bool)
    m[PLANTED_FRAME] = True
    for y, x in PLANTED_PIXELS_FRAME:
        m[y, x] = True
    return m


def exact_valid(shift, n, br):
    """Closed form along one axis of pixel_exact: pixel i inside the border frame [br, n - br) and a tap of non-zero weight inside it too.
    INTEGER shift: the one tap i + shift (weight one; the neighbour of weight zero does not count).  Half-integer shift: the two taps
    floor(i + shift) and the next (weight one half each).  The position is clamped where the grid is (|g| <= 2): to -n / 2 - 0.5 and
    3 n / 2 - 0.5, half-integers outside the image."""
    assert float(2 * shift) == int(2 * shift)
    i = np.arange(n)
    pos = np.clip(i + float(shift), -0.5 * n - 0.5, 1.5 * n - 0.5)
    first = np.floor(pos).astype(np.int64)
    tap = _in_frame(first, n, br) | ((pos != first) & _in_frame(first + 1, n, br))
    return _in_frame(i, n, br) & tap


def exact_valid_map(shift, br, h=H_EXACT, w=W_EXACT):
    """(H, W) bool: the validity of pixel_exact's frame with shift (kx, ky) at border radius `br`."""
    return exact_valid(shift[1], h, br)[:, None] & exact_valid(shift[0], w, br)[None, :]


# ---- the reference's projection, restated -----------------------------------------------------------------------------------------------------------
def host_matrices(batch):
    """kinv (B, 9) and proj (B, F, 12) as numpy fp32, formed by the reference's lines (monorec_model.py:171,198,207, layers.py:65)."""
    b, nf = batch["keyframe"].shape[0], len(batch["frames"])
    kinv = np.stack([torch.inverse(batch["keyframe_intrinsics"][n]).unsqueeze(0)[0, :3, :3].reshape(9).numpy() for n in range(b)])
    proj = np.zeros((b, nf, 12), dtype=F32)
    for n in range(b):
        for f in range(nf):
            t = torch.inverse(batch["poses"][f][n]) @ batch["keyframe_pose"][n]
            proj[n, f] = torch.matmul(batch["intrinsics"][f][n].unsqueeze(0), t.unsqueeze(0))[0, :3, :].reshape(12).numpy()
    return kinv.astype(F32), proj


def mac(a, b, c, fused=True):
    """One step of a k-ascending fp32 dot product: fma(a, b, c), or - `fused=False` - the rounded product plus c, rounded again."""
    if fused:
        return fmaf(a, b, c)
    with np.errstate(all="ignore"):
        return (np.asarray(a, dtype=F32) * np.asarray(b, dtype=F32)).astype(F32) + np.asarray(c, dtype=F32)


@functools.lru_cache(None)
def host_fuses():
    """Does this host's torch.matmul accumulate the small products of the reference's lines ((1, 3, 3) @ (1, 3, HW), (1, 3, 4) @ (D, 4, HW))
    k-ascending with fused multiply-adds (True: MKL on the Intel hosts the reference fixtures come from, and what the kernels do) or with
    separately rounded products and sums (False: MKL on AMD EPYC hosts)?  Anything else is an error: the restatement would not know the order."""
    gen = torch.Generator().manual_seed(77)
    a3, x3 = torch.rand(1, 3, 3, generator=gen) - 0.5, torch.rand(1, 3, 3840, generator=gen) * 80
    a4, x4 = torch.rand(1, 3, 4, generator=gen) * 90 - 45, torch.rand(8, 4, 3840, generator=gen) * 400 - 100
    verdict = []
    for a, x in ((a3, x3), (a4, x4)):
        want = torch.matmul(a, x).numpy()
        a, x = a[0].numpy(), x.numpy()
        same = {}
        for fused in (True, False):
            acc = a[:, 0, None] * x[:, None, 0]
            for k in range(1, a.shape[1]):
                acc = mac(a[:, k, None], x[:, None, k], acc, fused)
            same[fused] = bool((acc.view(np.int32) == want.view(np.int32)).all())
        assert same[True] != same[False], ("torch.matmul is neither k-ascending chain on this host", same)
        verdict.append(same[True])
    assert verdict[0] == verdict[1], verdict
    return verdict[0]


def rays(ki, h, w, mutate=None, fused=True):
    """inv(K)[:3, :3] @ [x; y; 1] (monorec_model.py:199) as the k-ascending fp32 chain of the CPU's matmul (`fused`: see host_fuses): three
    (H, W) arrays."""
    y, x = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    out = []
    for i in range(3):
        acc = F32(ki[3 * i]) * x
        if not (mutate == "drop_ki1" and i == 0):
            acc = mac(F32(ki[3 * i + 1]), y, acc, fused)
        out.append(mac(F32(ki[3 * i + 2]), F32(1), acc, fused))
    if mutate == "r2_one":
        out[2] = np.ones_like(out[2])
    return out


def project(ray, depth, p, h, w, mutate=None, division=None, fused=True):
    """point_projection + normalise + clamp (monorec_model.py:200-201,208, layers.py:65-70) for depths (D,) or (D, H, W): the normalised grid
    (D, H, W, 2) and pcz (D, H, W).  `division(a, d)`: the division by W - 1 / H - 1 (None: true division and Tensor.clamp, the reference's; else that
    division and C's fminf / fmaxf, as a kernel has them)."""
    depth = np.asarray(depth, dtype=F32)
    depth = depth.reshape(-1, 1, 1) if depth.ndim == 1 else depth
    p = np.asarray(p, dtype=F32).copy()
    if mutate == "swap_p1_p4":
        p[1], p[4] = p[4], p[1]
    with np.errstate(all="ignore"):
        x0, x1, x2 = depth * ray[0], depth * ray[1], depth * ray[2]
        if mutate == "x2_depth":
            x2 = np.broadcast_to(depth, x0.shape).astype(F32)
        pc = [mac(p[4 * j + 3], F32(1), mac(p[4 * j + 2], x2, mac(p[4 * j + 1], x1, p[4 * j] * x0, fused), fused), fused) for j in range(3)]
        z = pc[2] + F32(1e-7)
        div = division or (lambda a, d: a / F32(d))
        u = div(pc[0] / z, w - 1)
        v = div(pc[1] / z, h - 1)
        # Tensor.clamp hands a NaN on (np.clip too); C's fminf(fmaxf(a, -2), 2) - what goes with `division` - answers -2 for a NaN
        clamp = (lambda a: np.clip(a, F32(-2), F32(2))) if division is None else (lambda a: np.fmin(np.fmax(a, F32(-2)), F32(2)))
        u = clamp((u - F32(0.5)) * F32(2))
        v = clamp((v - F32(0.5)) * F32(2))
    return np.stack([u, v], -1).astype(F32), pc[2]


def div_const(a, d):
    """The three-operation division by a constant that the kernels use where the host has checked it: q0 = a y, r = fma(-d, q0, a),
    q = fma(r, y, q0), y = fp32(1 / d)."""
    d = F32(d)
    y = F32(1) / d
    with np.errstate(all="ignore"):
        q0 = np.asarray(a, dtype=F32) * y
        return fmaf(fmaf(-d, q0, a), y, q0)


def unnormalise(grid, h, w):
    """F.grid_sample(align_corners=False): sample position, integer corner and the four bilinear weights of a normalised grid."""
    sx = fmaf(grid[..., 0] + F32(1), F32(w * 0.5), F32(-0.5))
    sy = fmaf(grid[..., 1] + F32(1), F32(h * 0.5), F32(-0.5))
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = sx - fx, sy - fy
    return dict(sx=sx, sy=sy, x0=fx.astype(np.int64), y0=fy.astype(np.int64), w=wx, e=F32(1) - wx, n=wy, s=F32(1) - wy)


def _in_frame(i, n, br):
    return (i >= br) & (i < n - br)


def valid_fma(grid, h, w, br=2):
    """monorec_model.py:218: the bilinear sample of the border mask (ones inside a `br` wide zero frame, zeros outside the image) as
    grid_sample's four-term chain, != 0.  (D, H, W) bool."""
    u = unnormalise(grid, h, w)
    ml, mr = _in_frame(u["x0"], w, br).astype(F32), _in_frame(u["x0"] + 1, w, br).astype(F32)
    mt, mb = _in_frame(u["y0"], h, br).astype(F32), _in_frame(u["y0"] + 1, h, br).astype(F32)
    nw, ne, sw, se = u["s"] * u["e"], u["s"] * u["w"], u["n"] * u["e"], u["n"] * u["w"]
    return fmaf(mr * mb, se, fmaf(ml * mb, sw, fmaf(mr * mt, ne, (ml * mt) * nw))) != 0


def valid_bool(grid, h, w, br=2, zero_weight_clauses=True):
    """The same as logic: a tap counts when it is inside the frame and its weight is not zero."""
    u = unnormalise(grid, h, w)
    on = (lambda v: v != 0) if zero_weight_clauses else (lambda v: np.ones(v.shape, dtype=bool))
    lft, rgt = _in_frame(u["x0"], w, br) & on(u["e"]), _in_frame(u["x0"] + 1, w, br) & on(u["w"])
    top, bot = _in_frame(u["y0"], h, br) & on(u["s"]), _in_frame(u["y0"] + 1, h, br) & on(u["n"])
    return (lft | rgt) & (top | bot)


def pixel_valid(hit, h, w, br=2):
    """monorec_model.py:219: border mask of the pixel itself times the AND over all depths.  hit (D, H, W) -> (H, W) bool."""
    inside = np.zeros((h, w), dtype=bool)
    inside[br:h - br, br:w - br] = True
    return inside & hit.all(0)


def restated(batch, depths, mutate=None, division=None, fused=True):
    """The restatement over a whole batch: `depths` (D) or per-pixel (B, D, H, W).  Returns grid (B, F, D, H, W, 2) and pcz (B, F, D, H, W).
    `fused=True` is the arithmetic of the kernels; pass host_fuses() to compare with this host's oracle."""
    b, _, h, w = batch["keyframe"].shape
    kinv, proj = host_matrices(batch)
    depths = depths.numpy() if isinstance(depths, torch.Tensor) else np.asarray(depths)
    grids, pcz = [], []
    for n in range(b):
        ray = rays(kinv[n], h, w, mutate, fused)
        out = [project(ray, depths if depths.ndim == 1 else depths[n], proj[n, f], h, w, mutate, division, fused) for f in range(proj.shape[1])]
        grids.append(np.stack([g for g, _ in out]))
        pcz.append(np.stack([np.broadcast_to(z, g.shape[:-1]) for g, z in out]))
    return np.stack(grids), np.stack(pcz)


# ---- what the GPU tests run ------------------------------------------------------------------------------------------------------------------------
INTEGER_SHIFTS = ((0, 0), (-1, 2), (1, -1), (3, -3))
OTHER_SHIFTS = ((-1.5, 0.5), (0.5, -1.5), (1000, -1000))        # two half-integer shifts; one far outside: u clamps at +2, v at -2
SCENES = {
    "general": general,
    "general_far": general_far,
    "zero_denominator": zero_denominator,
    "exact_integer": lambda: pixel_exact(*INTEGER_SHIFTS[0], more=INTEGER_SHIFTS[1:]),
    "exact_other": lambda: pixel_exact(*OTHER_SHIFTS[0], more=OTHER_SHIFTS[1:]),
    "planted_zeros": planted_zeros,
}
EXACT_SHIFTS = {"exact_integer": INTEGER_SHIFTS, "exact_other": OTHER_SHIFTS, "planted_zeros": ((0, 0),)}
RANDOM_SCENES = ("general", "general_far", "zero_denominator")


def runs(scene):
    """The launches of one scene as cost_volume_paths cases, named `<entry>_d<D>[_pixd][_p<P>]`: the exact entry at D 8 and at every depth
    count with a register-resident fusion kernel, the tiled entry, the relaxed / B8 / lean entries, the patch entry at P 5 and P 1, each family
    with and without per-pixel depths.  planted_zeros is for sfcv_mult_mask=False, which only the tiled and the patch kernels serve."""
    import cost_volume_paths as cp
    batch = SCENES[scene]()
    b, _, h, w = batch["keyframe"].shape
    f = len(batch["frames"])
    fuse_d = cp.constants()["fuse_depths"]
    mm = scene != "planted_zeros"
    spec = [("mode", 8, False, 3), ("mode", 8, True, 3), ("tiled", 8, False, 3), ("tiled", 8, True, 3),
            ("mode", 8, False, 5), ("mode", 8, True, 5), ("mode", 8, False, 1)]
    if mm:
        spec += [("mode", d, False, 3) for d in fuse_d] + [("relaxed", 8, False, 3), ("b8", fuse_d[0], False, 3), ("lean", fuse_d[0], False, 3)]
    out = []
    for entry, d, pixd, patch in spec:
        name = f"{entry}_d{d}" + ("_pixd" if pixd else "") + (f"_p{patch}" if patch != 3 else "")
        out.append(cp.Case(name, None, None, entry, b, f, d, h, w, 1, pixd, mm, patch, True, 0))
    return out

