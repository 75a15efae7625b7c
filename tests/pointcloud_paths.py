"""Launch paths of the point-cloud append (host side, no GPU): `pointcloud_append_kernel` and the host entry `mr_pointcloud_append_f32`
of csrc/pointcloud.hip - the back-projection and ordered compaction behind `PLYSaver.add_depthmap`.

As tests/pointwise_paths.py and tests/data_paths.py do for their kernels, this module holds
    * `constants()`: workgroup size, wave count, grid, MR_MAX_VOTE_MASKS and the error codes, read from the sources by regular expression,
    * `rule_roi`: the python-slice clamp of the host entry restated,
    * PATHS[entry] / UNREACHED: the branch combinations of kernel and entry, one table per dimension (plane against the workgroup, keep
      pattern per pass, masks, uniform, roi, batch, cursor and capacity, depth values); CASES: each case NAMES the path it is there for and
      `path_of(case)` re-derives it from the case's shape and from the reference's keep decisions,
    * a GENERAL camera (skewed K with nine non-zero inverse entries, a rotation about (1, 2, 3) with nine distinct non-zero entries, a
      translation, another camera per batch element) - `synth.make_pointcloud_case` has eleven structural zeros a wrong kernel hides behind,
    * `operands(case)` (uniform data, general camera) and `operands(case, exact=True)` (powers of two and small dyadic rationals: every
      intermediate of the kernel is exact),
    * two references of the documented operation (include/monorec_hip.h, "One PLYSaver.add_depthmap ..."): `append_ref`, numpy fp32 with the
      kernel's roundings and an exactly emulated fmaf, and `append_ref64`, the same in fp64 with the absolute sums S the derived bound needs.
tests/test_pointcloud_paths.py checks the census and the references on the host, tests/test_gpu_pointcloud_paths.py runs every case on the
device."""
import collections
import functools
import json
import os
import re

import numpy as np
import torch

from pointwise_paths import MAX_DEVICE_BYTES  # noqa: F401  (the GPU file keeps its allocations under it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of fp32
BOUND_ROUNDINGS = 10                 # |fp32 - fp64| <= 10 u S: 1 (1/d) + 3 (kinv chain) + 1 (depth product) + 4 (pose chain) + 1 for the second-order terms
QNAN_BITS = 0x7fc00000               # every NaN is compared as this one: IEEE 754 leaves sign and payload of the NaN of an invalid operation open
DROPOUT = 0.75

Case = collections.namedtuple("Case", "entry name path args")
Ref = collections.namedtuple("Ref", "records cursor admitted batch pixel")


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@functools.lru_cache(None)
def constants():
    """What the compaction rests on, read from the sources."""
    pc, hdr = _src("monorec_amd", "csrc", "pointcloud.hip"), _src("include", "monorec_hip.h")
    wg = int(re.search(r"__launch_bounds__\((\d+)\) void pointcloud_append_kernel", pc).group(1))
    step = int(re.search(r"for \(long long p0 = 0; p0 < plane; p0 \+= (\d+)\)", pc).group(1))
    launch = re.search(r"hipLaunchKernelGGL\(pointcloud_append_kernel, dim3\((\d+)\), dim3\((\d+)\), 0,", pc)
    assert step == wg == int(launch.group(2)), (wg, step, launch.group(2))
    waves = int(re.search(r"__shared__ int wave_tot\[(\d+)\];", pc).group(1))
    assert int(re.search(r"for \(int w = 0; w < (\d+); \+\+w\) \{ const int t = wave_tot\[w\];", pc).group(1)) == waves
    lane = re.search(r"lane = tid & (\d+), wave = tid >> (\d+);", pc)
    wave_size = int(lane.group(1)) + 1
    assert 1 << int(lane.group(2)) == wave_size and waves * wave_size == wg, (waves, wave_size, wg)
    return dict(wg=wg, waves=waves, wave_size=wave_size, grid=int(launch.group(1)),
                max_masks=int(re.search(r"#define MR_MAX_VOTE_MASKS (\d+)", hdr).group(1)),
                err_bad_argument=int(re.search(r"#define MR_ERR_BAD_ARGUMENT \((-\d+)\)", hdr).group(1)),
                err_unsupported=int(re.search(r"#define MR_ERR_UNSUPPORTED\s+\((-\d+)\)", hdr).group(1)),
                err_lds_budget=int(re.search(r"#define MR_ERR_LDS_BUDGET\s+\((-\d+)\)", hdr).group(1)))


# ---- rules ------------------------------------------------------------------------------------------------------------------------------------
def rule_roi(roi, h, w):
    """The host entry's `if (roi)` block: (y0, y1, x0, x1) by the slicing semantics of `mask[:, :, :roi[0]] = False` etc. (ply_utils.py:39-43)."""
    if roi is None:
        return 0, h, 0, w
    out = []
    for i, v in enumerate(roi):
        n = h if i < 2 else w
        if v < 0:
            v += n
        out.append(0 if v < 0 else n if v > n else v)
    return tuple(out)


def plane_class(h, w):
    """Where h * w stands against wave and workgroup."""
    c = constants()
    n, wg, ws = h * w, c["wg"], c["wave_size"]
    if n < ws:
        return "under_one_wave"
    if n == ws:
        return "one_wave"
    if n < wg:
        return "partial_wave_one_pass" if n % ws else None
    if n == wg:
        return "one_pass"
    if n == wg + 1:
        return "one_pass_plus_one"
    return "passes_partial_wave" if n // wg >= 2 and n % ws else None


def segments(plane):
    """(first, last + 1) pixel of every pass of the kernel's `p0` loop."""
    wg = constants()["wg"]
    return [(p0, min(p0 + wg, plane)) for p0 in range(0, plane, wg)]


def keep_pattern(name, b, plane):
    """The keep pattern `name` as a (b, plane) bool array, the same in every pass of every batch element."""
    ws = constants()["wave_size"]
    k = np.zeros((b, plane), dtype=bool)
    for p0, p1 in segments(plane):
        n = p1 - p0
        if name == "all":
            k[:, p0:p1] = True
        elif name == "lane0_wave0":
            k[:, p0] = True
        elif name == "lane63_last_full_wave":
            if n >= ws:
                k[:, p0 + n // ws * ws - 1] = True
        elif name == "empty_waves_between":
            for wv in range(0, (n + ws - 1) // ws, 3):                 # waves 0, 3, 6, ... full, two empty ones between them
                k[:, p0 + wv * ws:min(p0 + (wv + 1) * ws, p1)] = True
        elif name != "none":
            raise KeyError(name)
    return k


def keep_class(keep):
    """The pattern a (b, plane) keep array shows, judged per pass: one of the names of `keep_pattern`, else "random"."""
    b, plane = keep.shape
    for name in ("all", "none", "lane0_wave0", "lane63_last_full_wave", "empty_waves_between"):
        if np.array_equal(keep, keep_pattern(name, b, plane)):
            return name
    return "random"


def position(pixel):
    """(pass, wave, lane) of a pixel index."""
    c = constants()
    return int(pixel) // c["wg"], int(pixel) % c["wg"] // c["wave_size"], int(pixel) % c["wave_size"]


# ---- exact fmaf -------------------------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """fp32 fused multiply-add, exactly: the fp64 product of two fp32 numbers is exact; the fp64 sum is rounded TO ODD by its TwoSum residual
    (53 >= 24 + 2 bits), so that the final rounding to fp32 is the single rounding of the exact a * b + c."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c)))
    shape = a.shape
    a, b, c = (np.atleast_1d(v) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F32).reshape(shape)


# ---- cameras ----------------------------------------------------------------------------------------------------------------------------------
def general_camera(b, h, w):
    """(intrinsics (b, 4, 4), pose (b, 4, 4), kinv (b, 9)) fp32.  K: skew, fx != fy, a small non-zero lower row (so that all nine entries of its
    inverse are non-zero); kinv is the fp32 result of the host's torch.inverse, as PLYSaver.add_depthmap computes it, handed on AS GIVEN.
    Pose: Rodrigues rotation about (1, 2, 3) / sqrt(14) - nine non-zero entries of pairwise distinct magnitude - and a translation.
    Every batch element has another camera."""
    k4 = torch.eye(4, dtype=torch.float32).repeat(b, 1, 1)
    pose = torch.eye(4, dtype=torch.float32).repeat(b, 1, 1)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    ax = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    for i in range(b):
        k3 = [[45.0 + 3 * i, 1.5 + 0.7 * i, w / 2 + 1.3 * i], [0.6 + 0.2 * i, 52.0 - 2 * i, h / 2 - 0.9 * i], [2e-4 * (1 + i), -3e-4 * (1 + i), 1.0]]
        k4[i, :3, :3] = torch.tensor(k3, dtype=torch.float64).float()
        ang = 0.7 + 0.3 * i
        rot = np.eye(3) + np.sin(ang) * ax + (1 - np.cos(ang)) * (ax @ ax)
        pose[i, :3, :3] = torch.from_numpy(rot).float()
        pose[i, :3, 3] = torch.tensor([3.1 + i, -2.2 - 0.5 * i, 5.3 + 0.25 * i])
    kinv = torch.inverse(k4)[:, :3, :3].contiguous()
    return k4, pose, kinv.reshape(b, 9)


_KINV_NUM = [9, -3, 5, 2, 11, -7, -1, 4, 13]        # / 32
_ROT_NUM = [7, -2, 3, -5, 6, 1, 4, -9, 8]           # / 8
_TRANS_NUM = [11, -13, 10]                          # / 8


def exact_camera(b):
    """(kinv (b, 9), pose (b, 16)) of small dyadic rationals: skewed, all rotation entries non-zero and distinct, another set per batch
    element.  Not an inverse and not orthonormal: the kernel does not care."""
    kinv = np.stack([np.roll(_KINV_NUM, i) for i in range(b)]).astype(F32) / F32(32)
    pose = np.zeros((b, 4, 4), dtype=F32)
    for i in range(b):
        pose[i, :3, :3] = np.roll(_ROT_NUM, 2 * i).reshape(3, 3) / 8.0
        pose[i, :3, 3] = (np.array(_TRANS_NUM) + 3 * i) / 8.0
        pose[i, 3, 3] = 1
    return kinv, pose.reshape(b, 16)


# ---- paths ------------------------------------------------------------------------------------------------------------------------------------
def _mask_paths():
    top = constants()["max_masks"]
    return ["n0", "n1-hits1"] + [f"n{n}-hits{m}" for n in (5, top) for m in (1, 2, n)] + ["at_vote_above"]


PATHS = {
    "plane": ["under_one_wave", "one_wave", "partial_wave_one_pass", "one_pass", "one_pass_plus_one", "passes_partial_wave"],
    "keep": ["all", "none", "lane0_wave0", "lane63_last_full_wave", "empty_waves_between", "random"],
    "masks": _mask_paths(),
    "uniform": ["null", "dropout", "equal_dropout"],
    "roi": ["null", "interior", "negative", "beyond", "empty"],
    "batch": ["b1", "b3_cameras_differ"],
    "cursor": ["start0", "start_nonzero", "cap_inside_wave_middle_pass", "cap_at_pass_boundary", "start_ge_capacity", "capacity0", "start_2p31"],
    "depth": [f"{v}-{m}" for v in ("edges", "open", "inexact_max") for m in ("unmasked", "masked")],
}
# declared by the code but run by no case, with the reason
UNREACHED = {
    "cursor/record_index_beyond_2p31_written": "a capacity above 2^31 records is a 48 GiB buffer: over MAX_DEVICE_BYTES; `rec * 6` in 64 bits is read, not run",
    "grid/more_than_one_workgroup": "the launch is dim3(1) by construction (the compaction is ordered through one cursor)",
}
EDGE_VALUES = ("zero", "minus_zero", "negative", "nan", "inf", "at_min", "at_max", "below_min", "above_max")


def inv_for_depth(target, offset=0):
    """An fp32 inverse depth v with fp32(1 / v) == the fp32 number `offset` steps above fp32(target)."""
    t = F32(target)
    for _ in range(abs(offset)):
        t = np.nextafter(t, F32(np.inf if offset > 0 else -np.inf), dtype=F32)
    v = F32(1) / t
    for cand in (v, np.nextafter(v, F32(0)), np.nextafter(v, F32(np.inf)), np.nextafter(np.nextafter(v, F32(0)), F32(0)),
                 np.nextafter(np.nextafter(v, F32(np.inf)), F32(np.inf))):
        if F32(1) / cand == t:
            return F32(cand)
    return None


def edge_values(min_d, max_d):
    """name -> fp32 inverse depth of EDGE_VALUES (below_min / above_max: the depth is the fp32 neighbour just outside the inclusive range)."""
    out = {"zero": F32(0.0), "minus_zero": F32(-0.0), "negative": F32(-0.25), "nan": F32(np.nan), "inf": F32(np.inf),
           "at_min": inv_for_depth(min_d), "at_max": inv_for_depth(max_d)}
    for name, target, direction in (("below_min", min_d, -1), ("above_max", max_d, 1)):
        out[name] = next(v for v in (inv_for_depth(target, direction * k) for k in (1, 2, 3, 4)) if v is not None)
    assert all(v is not None for v in out.values()), out
    return out


def path_of(case, exact=False):
    """The path the restated rules and the reference's keep decisions put `case` on (None: on none of the declared ones)."""
    a, e, c = case.args, case.entry, constants()
    ops = operands(case, exact)
    keep, _ = decisions(ops)
    plane = a["h"] * a["w"]
    if e == "plane":
        return plane_class(a["h"], a["w"])
    if e == "keep":
        return keep_class(keep) if len(segments(plane)) >= 2 else None
    if e == "masks":
        n, hits = len(ops["masks"]), a["min_hits"]
        if n == 0:
            return "n0"
        sums = np.sum(ops["masks"], axis=0)
        if ops["vote_above"] > 0 and set(np.unique(sums)) == {ops["vote_above"], ops["vote_above"] + 1}:
            return "at_vote_above"
        return f"n{n}-hits{hits}" if ops["vote_above"] == n - hits else None
    if e == "uniform":
        if ops["uniform"] is None:
            return "null"
        return "equal_dropout" if (ops["uniform"] == F32(ops["dropout"])).any() else "dropout" if ops["dropout"] == DROPOUT else None
    if e == "roi":
        if a["roi"] is None:
            return "null"
        y0, y1, x0, x1 = rule_roi(a["roi"], a["h"], a["w"])
        if y1 <= y0 or x1 <= x0:
            return "empty"
        if min(a["roi"]) < 0:
            return "negative"
        if a["roi"][1] > a["h"] or a["roi"][3] > a["w"]:
            return "beyond"
        return "interior" if 0 < y0 < y1 < a["h"] and 0 < x0 < x1 < a["w"] else None
    if e == "batch":
        if a["b"] == 1:
            return "b1"
        differ = all(not np.array_equal(ops[k][i], ops[k][j]) for k in ("kinv", "pose") for i in range(a["b"]) for j in range(i))
        return "b3_cameras_differ" if a["b"] == 3 and differ else None
    if e == "cursor":
        start, cap, kept = ops["start"], ops["capacity"], int(keep.sum())
        if start >= 2 ** 31:
            return "start_2p31" if 0 < cap < 2 ** 31 else None
        if cap == 0:
            return "capacity0"
        if start >= cap:
            return "start_ge_capacity"
        if start + kept <= cap:
            return "start0" if start == 0 else "start_nonzero"
        bi, pi = np.nonzero(keep)
        cut = cap - start                                  # record `cut - 1` is the last one admitted, record `cut` the first one refused
        (b0, p0), (b1, p1) = (bi[cut - 1], pi[cut - 1]), (bi[cut], pi[cut])
        if b0 != b1:
            return None
        last = len(segments(plane)) - 1
        if position(p0)[:2] == position(p1)[:2]:
            return "cap_inside_wave_middle_pass" if 0 < position(p0)[0] < last else None
        return "cap_at_pass_boundary" if position(p0)[0] < position(p1)[0] else None        # all of one pass admitted, none of the next
    if e == "depth":
        form = "masked" if ops["masks"] else "unmasked"
        if float(F32(ops["max_d"])) != ops["max_d"]:                                       # (as python doubles: numpy would compare in fp32)
            at = (F32(1) / ops["inv_depth"] == F32(ops["max_d"])).any() if np.isfinite(ops["max_d"]) else False
            return f"inexact_max-{form}" if at else None
        vals = edge_values(*(edge_range(ops)))
        have = all((ops["inv_depth"].view(np.uint32) == v.view(np.uint32)).any() for v in vals.values())
        if not have:
            return None
        return f"{'open' if np.isinf(ops['min_d']) and np.isinf(ops['max_d']) else 'edges'}-{form}"
    raise KeyError(e)


def edge_range(ops):
    """The finite range the boundary values of a depth case are built for (an open case keeps its data around 1.5 .. 12 too)."""
    return (ops["min_d"], ops["max_d"]) if np.isfinite(ops["min_d"]) and np.isfinite(ops["max_d"]) else (1.5, 12.0)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(b=1, h=9, w=50, masks=0, min_hits=1, masks_kind="random", uniform=None, dropout=0.0, roi=None, start=0, capacity=("slack", 5),
                keep="random", depth="plain", min_d=1.5, max_d=12.0, certified=True)


def _cases():
    c = constants()
    wg, ws, top = c["wg"], c["wave_size"], c["max_masks"]
    out = []

    def add(entry, name, path, **args):
        unknown = set(args) - set(DEFAULTS)
        assert not unknown, unknown
        out.append(Case(entry, name, path, dict(DEFAULTS, **args)))

    # -- plane against the workgroup (derived from wave size 64 / workgroup 1024 at the present constants: 63, 64, 450, 1024, 1025, 2079 pixels)
    assert (ws, wg) == (64, 1024), "re-derive the shapes below from the constants"
    for h, w in ((7, 9), (8, 8), (9, 50), (16, 64), (25, 41), (33, 63)):
        add("plane", f"{h}x{w}", plane_class(h, w), h=h, w=w)
    # -- keep pattern per pass, on three passes (33 x 63: two whole passes and 31 pixels), start cursor 3
    for pat in PATHS["keep"]:
        add("keep", pat, pat, h=35, w=61, keep=pat, start=3)
    # -- masks
    add("masks", "n0", "n0")
    add("masks", "n1_hits1", "n1-hits1", masks=1, min_hits=1)
    for n in (5, top):
        for m in (1, 2, n):
            add("masks", f"n{n}_hits{m}", f"n{n}-hits{m}", masks=n, min_hits=m, h=25, w=41)
    add("masks", "sum_at_vote_above", "at_vote_above", masks=5, min_hits=2, masks_kind="at_vote")
    # -- uniform
    add("uniform", "null", "null")
    add("uniform", "dropout_075", "dropout", uniform="random", dropout=DROPOUT, h=25, w=41)
    add("uniform", "entries_equal_dropout", "equal_dropout", uniform="equal", dropout=DROPOUT, h=25, w=41)
    # -- roi
    add("roi", "null", "null", h=20, w=30)
    add("roi", "interior", "interior", h=20, w=30, roi=[3, 17, 4, 27])
    add("roi", "negative", "negative", h=20, w=30, roi=[-18, -2, 2, -3])
    add("roi", "far_negative_and_beyond", "negative", h=20, w=30, roi=[-25, 40, -31, 29])
    add("roi", "beyond", "beyond", h=20, w=30, roi=[2, 25, 1, 31])
    add("roi", "empty_rows", "empty", h=20, w=30, roi=[12, 12, 2, 28])
    add("roi", "empty_reversed_columns", "empty", h=20, w=30, roi=[2, 18, -5, 10])
    # -- batch: per-element cameras; b3 runs more than one pass per element and carries the negative roi of the reference fixture
    add("batch", "b1", "b1", h=25, w=41)
    add("batch", "b3_negative_roi", "b3_cameras_differ", b=3, h=25, w=41, roi=[2, -2, -38, -1])
    add("batch", "b3_masks_dropout", "b3_cameras_differ", b=3, h=9, w=50, masks=5, min_hits=2, uniform="random", dropout=0.4)
    # -- cursor and capacity
    add("cursor", "start0", "start0")
    add("cursor", "start37", "start_nonzero", start=37)
    add("cursor", "cap_inside_wave_of_pass1", "cap_inside_wave_middle_pass", h=33, w=63, start=5, capacity=("cut_wave", 1, 7))
    add("cursor", "cap_after_pass0", "cap_at_pass_boundary", h=33, w=63, start=5, capacity=("pass_end", 0))
    add("cursor", "cap_after_pass1_b3", "cap_at_pass_boundary", b=3, h=33, w=63, start=0, capacity=("pass_end", 1))
    add("cursor", "start40_capacity24", "start_ge_capacity", start=40, capacity=("abs", 24))
    add("cursor", "start_equals_capacity", "start_ge_capacity", start=24, capacity=("abs", 24))
    add("cursor", "capacity0", "capacity0", capacity=("abs", 0))
    add("cursor", "start_2p31_plus_5", "start_2p31", start=2 ** 31 + 5, capacity=("abs", 16), h=25, w=41)
    # -- depth values.  "edges": every EDGE_VALUES entry under a finite inclusive range; "open": the same data under (-inf, +inf), where
    # 1 / 0, 1 / -0 and 1 / inf are KEPT and give inf / NaN coordinates; "inexact_max": max_d = 0.1 is no fp32 number, a depth of fp32(0.1)
    for form, n in (("unmasked", 0), ("masked", 2)):
        add("depth", f"edges_{form}", f"edges-{form}", depth="edges", masks=n, min_hits=n)
        add("depth", f"open_{form}", f"open-{form}", depth="edges", masks=n, min_hits=n, min_d=-np.inf, max_d=np.inf, certified=False)
        add("depth", f"max_d_0.1_{form}", f"inexact_max-{form}", depth="inexact_max", masks=n, min_hits=n, min_d=0.01, max_d=0.1, certified=False)
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def _seed(case, exact):
    return 5000 + 11 * [(c.entry, c.name) for c in CASES].index((case.entry, case.name)) + (1 if exact else 0)


@functools.lru_cache(None)
def _operands(key, exact):
    case = next(c for c in CASES if (c.entry, c.name) == key)
    a = case.args
    b, h, w = a["b"], a["h"], a["w"]
    plane = h * w
    rng = np.random.default_rng(_seed(case, exact))
    min_d, max_d = a["min_d"], a["max_d"]
    if exact and a["depth"] == "edges" and np.isfinite(min_d):
        min_d, max_d = 2.0, 8.0                                # the same decisions on powers of two, boundaries that are powers of two
    if exact:
        inv = (2.0 ** -rng.integers(0, 6, size=(b, plane))).astype(F32)                     # depth 1 .. 32, kept: 2, 4, 8
        valid = (2.0 ** -rng.integers(1, 4, size=(b, plane))).astype(F32)
        image = (rng.integers(-128, 129, size=(b, 3, plane)) / 256.0).astype(F32)
        kinv, pose = exact_camera(b)
        k4 = None
    else:
        lo, hi = (0.02, 1.0) if a["depth"] != "inexact_max" else (5.0, 50.0)                 # depth 1 .. 50 around [1.5, 12], or .02 .. .2 around [.01, .1]
        inv = rng.uniform(lo, hi, size=(b, plane)).astype(F32)
        valid = rng.uniform(0.1, 0.6, size=(b, plane)).astype(F32)
        image = rng.uniform(-0.5, 0.5, size=(b, 3, plane)).astype(F32)
        k4, pose4, kinv = general_camera(b, h, w)
        k4, pose, kinv = k4.numpy(), pose4.numpy().reshape(b, 16).copy(), kinv.numpy().copy()
    if a["keep"] != "random":
        pat = keep_pattern(a["keep"], b, plane)
        inv = np.where(pat, valid, F32(0.0))
    if a["depth"] == "edges":
        vals = list(edge_values(*((min_d, max_d) if np.isfinite(min_d) else (1.5, 12.0))).values())
        idx = np.arange(2, b * plane, 5)                       # every fifth pixel: the edges in turn (9 values against 2 mask states: all pairs meet)
        inv.reshape(-1)[idx] = np.array(vals, dtype=F32)[np.arange(idx.size) % len(vals)]
    if a["depth"] == "inexact_max":
        inv.reshape(-1)[np.arange(1, b * plane, 7)] = inv_for_depth(0.1)
        inv.reshape(-1)[np.arange(3, b * plane, 7)] = inv_for_depth(0.1, 1)
    n = a["masks"]
    vote_above = float(n - a["min_hits"])
    masks = []
    if a["masks_kind"] == "at_vote":
        masks = [np.ones((b, plane), dtype=F32) for _ in range(3)] + [(rng.random((b, plane)) < 0.6).astype(F32), np.zeros((b, plane), dtype=F32)]
    elif n:
        need = n - a["min_hits"] + 1                           # masks that must be 1
        q = 0.7 ** (1.0 / n) if need == n else 1 - 0.3 ** (1.0 / n) if need == 1 else 0.85
        masks = [(rng.random((b, plane)) < q).astype(F32) for _ in range(n)]
    uniform = None
    if a["uniform"] is not None:
        uniform = rng.random((b, plane)).astype(F32)
        if a["uniform"] == "equal":
            uniform.reshape(-1)[::3] = F32(a["dropout"])
    ops = dict(b=b, h=h, w=w, inv_depth=np.ascontiguousarray(inv, dtype=F32), masks=masks, vote_above=vote_above, image=image, kinv=kinv, pose=pose,
               intrinsics=k4, uniform=uniform, dropout=float(a["dropout"]), min_d=float(min_d), max_d=float(max_d), roi=a["roi"], start=int(a["start"]),
               min_hits=a["min_hits"])
    keep, _ = decisions(ops)
    kind = a["capacity"]
    kept = int(keep.sum())
    if kind[0] == "slack":
        cap = ops["start"] + kept + kind[1]
    elif kind[0] == "abs":
        cap = kind[1]
    elif kind[0] == "pass_end":                                # everything batch element 0 keeps up to the end of that pass
        cap = ops["start"] + int(keep[0, :segments(plane)[kind[1]][1]].sum())
    else:                                                      # cut_wave: half of what that wave of that pass keeps (batch element 0)
        c = constants()
        first = kind[1] * c["wg"] + kind[2] * c["wave_size"]
        cap = ops["start"] + int(keep[0, :first].sum()) + int(keep[0, first:first + c["wave_size"]].sum()) // 2
    ops["capacity"] = int(cap)
    for v in ops.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for m in masks:
        m.setflags(write=False)
    return ops


def operands(case, exact=False):
    """The operands of a case as numpy arrays (read-only, computed once): inv_depth / uniform (b, plane), image (b, 3, plane), masks, kinv
    (b, 9), pose (b, 16), intrinsics (b, 4, 4; general camera only), the scalars of the call, `start` and the resolved `capacity`.
    exact=True: the certified operands - inv_depth a power of two, dyadic camera, image values multiples of 2^-8."""
    return _operands((case.entry, case.name), bool(exact))


# ---- references -------------------------------------------------------------------------------------------------------------------------------
def decisions(ops):
    """(keep (b, plane) bool, depth (b, plane) fp32): the vote, `depth *= mask`, the correctly rounded 1 / d, the inclusive range, the roi and
    the strict `uniform > dropout` - applied whenever `uniform` is given, as the header documents."""
    h, w = ops["h"], ops["w"]
    d = ops["inv_depth"].astype(F32)
    with np.errstate(all="ignore"):
        if ops["masks"]:
            s = ops["masks"][0].astype(F32)
            for m in ops["masks"][1:]:
                s = s + m
            d = d * np.where(s > F32(ops["vote_above"]), F32(1), F32(0))
        depth = F32(1) / d
        keep = (F32(ops["min_d"]) <= depth) & (depth <= F32(ops["max_d"]))
    y0, y1, x0, x1 = rule_roi(ops["roi"], h, w)
    p = np.arange(h * w)
    y, x = p // w, p % w
    keep = keep & ((y >= y0) & (y < y1) & (x >= x0) & (x < x1))[None, :]
    if ops["uniform"] is not None:
        keep = keep & (ops["uniform"] > F32(ops["dropout"]))
    return keep, depth


def canonical_bits(rec):
    """The bit patterns of fp32 records with every NaN replaced by QNAN_BITS.  +-inf, +-0 and every finite value keep their bits; sign and payload
    of a NaN that inf - inf or 0 * inf produced differ between x86 (0xffc00000) and other hardware and are no part of the documented operation."""
    bits = np.array(np.ascontiguousarray(rec, dtype=F32).view(np.uint32), copy=True)
    bits[np.isnan(bits.view(F32))] = QNAN_BITS
    return bits


def append_ref(ops, capacity=None, kinv=None, pose=None):
    """numpy fp32 restatement with the kernel's roundings: K[0] * fx then two fmaf, the product with depth, T[0] * c0 then three fmaf, the
    colour add and multiply apart.  Ref(records (n, 6), new cursor, admitted (n,) under `capacity`, batch and pixel index of each record);
    the records are in batch-major, pixel row-major order.  NaN coordinates are canonical (`canonical_bits`)."""
    keep, depth = decisions(ops)
    kinv = ops["kinv"] if kinv is None else kinv
    pose = ops["pose"] if pose is None else pose
    capacity = ops["capacity"] if capacity is None else capacity
    bi, pi = np.nonzero(keep)
    w = ops["w"]
    fx, fy, one = (pi % w).astype(F32), (pi // w).astype(F32), F32(1)
    K, T, dep = kinv[bi].astype(F32), pose[bi].astype(F32), depth[bi, pi]
    rec = np.empty((bi.size, 6), dtype=F32)
    with np.errstate(all="ignore"):
        cam = []
        for j in range(3):
            n = K[:, 3 * j] * fx
            n = fmaf(K[:, 3 * j + 1], fy, n)
            n = fmaf(K[:, 3 * j + 2], one, n)
            cam.append(dep * n)
        for i in range(3):
            v = T[:, 4 * i] * cam[0]
            v = fmaf(T[:, 4 * i + 1], cam[1], v)
            v = fmaf(T[:, 4 * i + 2], cam[2], v)
            rec[:, i] = fmaf(T[:, 4 * i + 3], one, v)
        for ch in range(3):
            rec[:, 3 + ch] = (ops["image"][bi, ch, pi] + F32(0.5)) * F32(255.0)
    rec = canonical_bits(rec).view(F32)
    return Ref(rec, ops["start"] + bi.size, ops["start"] + np.arange(bi.size, dtype=np.int64) < capacity, bi, pi)


def append_ref64(ops):
    """(records (n, 6) fp64, S (n, 3)): the same operation in fp64 from the same fp32 inputs and the same keep decisions, and per coordinate the
    absolute sum S_i = sum_j |T_ij| depth sum_k |K_jk| |p_k| + |T_i3| that the rounding bound scales with."""
    keep, _ = decisions(ops)
    bi, pi = np.nonzero(keep)
    w = ops["w"]
    p = np.stack([(pi % w).astype(np.float64), (pi // w).astype(np.float64), np.ones(bi.size)], 1)
    K = ops["kinv"].astype(np.float64).reshape(-1, 3, 3)[bi]
    T = ops["pose"].astype(np.float64).reshape(-1, 4, 4)[bi]
    with np.errstate(all="ignore"):
        d = ops["inv_depth"].astype(np.float64)
        if ops["masks"]:
            d = d * (np.sum([m.astype(np.float64) for m in ops["masks"]], axis=0) > ops["vote_above"])
        dep = 1.0 / d[bi, pi]
        cam = dep[:, None] * np.einsum("njk,nk->nj", K, p)
        xyz = np.einsum("nij,nj->ni", T[:, :3, :3], cam) + T[:, :3, 3]
        S = np.einsum("nij,nj->ni", np.abs(T[:, :3, :3]), np.abs(dep)[:, None] * np.einsum("njk,nk->nj", np.abs(K), p)) + np.abs(T[:, :3, 3])
        col = (ops["image"].astype(np.float64)[bi, :, pi] + 0.5) * 255.0
    return np.concatenate([xyz, col], 1), S


def oracle_records(ops):
    """oracle.monorec_oracle.pointcloud_records (the reference's own expressions in torch) on the operands of a general-camera case: dropout > 0
    and `uniform` wherever the case thins."""
    from oracle import monorec_oracle as orc
    b, h, w = ops["b"], ops["h"], ops["w"]
    t = lambda x, *s: torch.from_numpy(np.array(x, copy=True)).view(*s)                       # noqa: E731
    masks = [t(m, b, 1, h, w) for m in ops["masks"]] or None
    uniform = None if ops["uniform"] is None else t(ops["uniform"], b, 1, h, w)
    return orc.pointcloud_records(t(ops["inv_depth"], b, 1, h, w), t(ops["image"], b, 3, h, w), t(ops["intrinsics"], b, 4, 4), t(ops["pose"], b, 4, 4),
                                  ops["min_d"], ops["max_d"], ops["roi"], ops["dropout"] if uniform is not None else 0.0, uniform, masks, ops["min_hits"])


def first_difference(got_bits, want_bits, ref, w):
    """Text naming the first record whose bits differ: its index, (b, y, x), pass, wave and lane."""
    bad = np.nonzero((got_bits != want_bits).any(1))[0]
    if bad.size == 0:
        return "no difference"
    i = int(bad[0])
    ps, wave, lane = position(ref.pixel[i])
    return (f"{bad.size} of {len(want_bits)} records differ; first: record {i} = (b {int(ref.batch[i])}, y {int(ref.pixel[i]) // w}, x {int(ref.pixel[i]) % w}), "
            f"pass {ps}, wave {wave}, lane {lane}: got {[hex(int(v)) for v in got_bits[i]]}, want {[hex(int(v)) for v in want_bits[i]]}")


# ---- the committed fixture of the reference's own PLYSaver on two general-camera cases (tools/make_golden_pointcloud_general.py) ---------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "pointcloud_general.npz")
FIXTURE_CASES = ["batch.b3_negative_roi", "uniform.null"]              # "<entry>.<name>": three cameras under a negative roi; dropout 0


def fixture_cases():
    with open(os.path.join(GOLDEN, "pointcloud_general.json")) as f:
        return json.load(f)["cases"]


def fixture_ops(z, name, meta):
    """The operands dict of a fixture case from the committed arrays (kinv: this host's torch.inverse of the stored intrinsics, as given)."""
    b, h, w = meta["b"], meta["h"], meta["w"]
    k4 = z[f"{name}.intrinsics"]
    kinv = torch.inverse(torch.from_numpy(k4))[:, :3, :3].contiguous().numpy().reshape(b, 9)
    return dict(b=b, h=h, w=w, inv_depth=z[f"{name}.inv_depth"].reshape(b, h * w), masks=[], vote_above=0.0, image=z[f"{name}.image"].reshape(b, 3, h * w),
                kinv=kinv, pose=z[f"{name}.pose"].reshape(b, 16), intrinsics=k4, uniform=None, dropout=0.0, min_d=meta["min_d"], max_d=meta["max_d"],
                roi=meta["roi"], start=0, capacity=2 ** 62, min_hits=1)


CASES = []
CASES = _cases()


def cases_of(entry):
    return [c for c in CASES if c.entry == entry]


def ids(cases):
    return [f"{c.entry}-{c.name}" for c in cases]


def certified_cases():
    return [c for c in CASES if c.args["certified"]]


def device_bytes(case):
    """Bytes the GPU test of a case allocates: depth, image, masks, uniform, cameras, the record buffer with its guards, the cursor pair."""
    a = case.args
    px = a["b"] * a["h"] * a["w"]
    return 4 * px * (1 + 3 + a["masks"] + 1) + a["b"] * 100 + 24 * (px + 64) + 16


def table():
    lines = []
    for entry, paths in PATHS.items():
        for p in paths:
            names = [c.name for c in cases_of(entry) if c.path == p]
            lines.append(f"{entry:8s} {p:30s} {', '.join(names) if names else '-- NO CASE --'}")
    return "\n".join(lines)
