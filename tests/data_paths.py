"""Launch paths of the kernels at the two ENDS of the pipeline (host side, no GPU): csrc/preprocess.hip (the Pillow-exact resize, the lidar /
D(V)SO targets, the frame-store unpack and scatter), csrc/select.hip (median select, stage ratios, stage-scaled metric sums) and
mr_sparse_metric_sums_f32 (csrc/eltwise.hip).

As tests/pointwise_paths.py does for the kernels around the convolutions, this module holds
    * `constants()`: what the launch rules rest on, read from the sources by regular expression, never typed in,
    * `rule_*`: every launch rule restated in plain Python, and a numpy restatement of the three-digit radix select,
    * PATHS[entry]: the branch combinations rule and kernel can take; UNREACHED: declared paths no case runs, with the reason,
    * CASES: the cases, each NAMING its path - `path_of(case)` re-derives it; shapes on a threshold are derived from the constants,
    * the operands of every case and the CPU references tests/test_gpu_data_paths.py compares the kernels with.
tests/test_data_paths.py checks the census on the host, tests/test_gpu_data_paths.py runs every case on the device."""
import collections
import functools
import math
import os
import re

import numpy as np
import torch

from oracle import input_oracle as io_ref
from pointwise_paths import MAX_DEVICE_BYTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_LOG = 2e-5              # column 4 (logf of the device's against the host's math library): the project's bar of tests/test_gpu_metrics.py
INF, NAN = float("inf"), float("nan")

Case = collections.namedtuple("Case", "entry name path args")


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@functools.lru_cache(None)
def constants():
    """What the launch rules rest on, read from the sources."""
    pre, sel, elt = _src("monorec_amd", "csrc", "preprocess.hip"), _src("monorec_amd", "csrc", "select.hip"), _src("monorec_amd", "csrc", "eltwise.hip")
    hdr = _src("include", "monorec_hip.h")
    tile = re.search(r"constexpr int PT_H = (\d+), PT_W = (\d+);", pre)
    # the four elect / write launches and the unpack / scatter launches: ceil(items / wg) workgroups, capped
    capped = re.findall(r"\(\((n|cells) \+ (\d+)\) / (\d+) < (\d+) \? \(\1 \+ \2\) / \3 : \4\)", pre)
    assert sorted(c[0] for c in capped) == ["cells", "cells", "n", "n"], capped
    capped2 = re.findall(r"blocks > (\d+) \? \1 : blocks", pre)
    assert len(capped2) == 2, capped2
    wgs = {int(c[2]) for c in capped} | {int(c[1]) + 1 for c in capped} | {int(v) for v in re.findall(r"const long long blocks = \(n(?: / 16)? \+ 255\) / (\d+);", pre)}
    caps = {int(c[3]) for c in capped} | {int(v) for v in capped2}
    assert len(wgs) == 1 and len(caps) == 1, (wgs, caps)
    lds = re.search(r"if \(lds > (\d+) \* (\d+)\) return MR_ERR_LDS_BUDGET;", pre)
    table = re.search(r"const size_t lds = \(size_t\)max_tile_rows \* PT_W \* channels \+ \(with_lut \? (\d+) \* sizeof\(float\) : 0\);", pre)
    step = re.search(r"for \(int base = 0; base < n; base \+= (\d+) \* kThreads\)", sel)
    return dict(
        pt_h=int(tile.group(1)), pt_w=int(tile.group(2)), pre_threads=int(re.search(r"constexpr int PRE_THREADS = (\d+);", pre).group(1)),
        wg=wgs.pop(), grid_cap=caps.pop(), lds_limit=int(lds.group(1)) * int(lds.group(2)), lut_bytes=int(table.group(1)) * 4,
        k_threads=int(re.search(r"constexpr int kThreads = (\d+);", sel).group(1)), k_bins=int(re.search(r"constexpr int kBins = (\d+);", sel).group(1)),
        select_step=int(step.group(1)) * int(re.search(r"constexpr int kThreads = (\d+);", sel).group(1)),
        metric_wg=int(re.search(r"__launch_bounds__\((\d+)\) void sparse_metric_sums_kernel", elt).group(1)),
        max_stages=int(re.search(r"#define MR_MAX_METRIC_STAGES (\d+)", hdr).group(1)),
        metric_dense=int(re.search(r"#define MR_METRIC_DENSE (0x[0-9a-fA-F]+)", hdr).group(1), 16),
        err_bad_argument=int(re.search(r"#define MR_ERR_BAD_ARGUMENT \((-\d+)\)", hdr).group(1)),
        err_unsupported=int(re.search(r"#define MR_ERR_UNSUPPORTED\s+\((-\d+)\)", hdr).group(1)),
        err_lds_budget=int(re.search(r"#define MR_ERR_LDS_BUDGET\s+\((-\d+)\)", hdr).group(1)))


# ---- launch rules ---------------------------------------------------------------------------------------------------------------------------
def pass_items():
    """Work items one pass of a grid-stride loop of csrc/preprocess.hip covers at the capped grid."""
    c = constants()
    return c["grid_cap"] * c["wg"]


def rule_grid(items):
    """The elect / write / scatter / unpack launches: (workgroups, passes of the grid-stride loop the busiest thread makes)."""
    c = constants()
    blocks = min(max((items + c["wg"] - 1) // c["wg"], 1), c["grid_cap"])
    return blocks, (items + blocks * c["wg"] - 1) // (blocks * c["wg"])


def is_second_pass(items):
    """Strictly between one and two passes: some threads loop twice, some once, none three times."""
    return pass_items() < items < 2 * pass_items()


def tile_rows(vb, out_h):
    """Source rows each row of output tiles reads: the horizontal pass writes that many LDS rows (preprocess_kernel: r_end - r_first)."""
    th = constants()["pt_h"]
    return [int(vb[min(t + th - 1, out_h - 1), 0] + vb[min(t + th - 1, out_h - 1), 1] - vb[t, 0]) for t in range(0, out_h, th)]


def rule_resize(entry, channels, crop_h, crop_w, out_h, out_w, vb=None):
    """launch_preprocess with the max_tile_rows of ImagePreprocessor.__init__: the grid, the last tile, the LDS bytes or the error code,
    and the passes of the horizontal-pass loop over the busiest tile."""
    c = constants()
    if vb is None:
        vb = io_ref.resample_coeffs(crop_h, 0, crop_h, out_h)[1]
    rows = tile_rows(vb, out_h)
    tiles_x, tiles_y = (out_w + c["pt_w"] - 1) // c["pt_w"], (out_h + c["pt_h"] - 1) // c["pt_h"]
    assert len(rows) == tiles_y
    cols = [min(c["pt_w"], out_w - t * c["pt_w"]) for t in range(tiles_x)]
    lds = max(rows) * c["pt_w"] * channels + (c["lut_bytes"] if entry == "lut" else 0)
    busiest = max(rows) * max(cols)
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, last_cols=cols[-1], last_rows=out_h - (tiles_y - 1) * c["pt_h"], max_tile_rows=max(rows), lds=lds,
                code=c["err_lds_budget"] if lds > c["lds_limit"] else 0, h_passes=(busiest + c["pre_threads"] - 1) // c["pre_threads"],
                v_passes=(c["pt_h"] * max(cols) + c["pre_threads"] - 1) // c["pre_threads"])


def largest_tile_rows(entry, channels):
    """The most LDS rows the budget accepts for (entry, channels)."""
    c = constants()
    return (c["lds_limit"] - (c["lut_bytes"] if entry == "lut" else 0)) // (c["pt_w"] * channels)


def rule_target(src_h, src_w, box, extent):
    """The host checks of mr_lidar_inverse_depth_u16_f32 / mr_dso_inverse_depth_u16_f32 in their order (`extent`: what a NULL box means)."""
    c = constants()
    if src_h * src_w >= 2 ** 31:
        return c["err_unsupported"]
    x0, y0, x1, y1 = box if box is not None else (0, 0, extent[1], extent[0])
    return c["err_bad_argument"] if x1 <= x0 or y1 <= y0 else 0


def rule_select(n, m, le=None):
    """masked_select_kernel on n pixels of which m are selected: steps of the compaction loop, whether the last one is partial, the m == 0
    exit, and - for the prediction, given `le` = how many selected keys are <= the lower median - where hi comes from: the same key
    ("prefix_odd": m is odd; "prefix_le": more than lo_rank + 1 keys are <= it) or the smallest key above it ("above", s_above)."""
    step = constants()["select_step"]
    hi_from = None if m == 0 or le is None else "prefix_odd" if m & 1 else "prefix_le" if le > (m - 1) // 2 + 1 else "above"
    return dict(steps=(n + step - 1) // step, partial=n % step != 0, empty=m == 0, hi_from=hi_from)


def key_of(x):
    """Order-preserving key of fp32 bit patterns (numpy float32 -> uint32): negatives flipped, the rest get the sign bit."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def float_of(k):
    k = np.uint32(k)
    return np.array([k & np.uint32(0x7fffffff) if k & np.uint32(0x80000000) else ~k], dtype=np.uint32).view(np.float32)[0]


def _digits():
    bits = constants()["k_bins"].bit_length() - 1
    return ((32 - bits, bits), (32 - 2 * bits, bits), (0, 32 - 2 * bits))         # (shift, width), most significant first: 11, 11, 10 bits


def find_bin(hist, rank):
    """find_bin of select.hip: the bin holding `rank` (0-based from the smallest key) and the rank within it."""
    incl = np.cumsum(hist)
    b = int(np.searchsorted(incl, rank, side="right"))
    return b, int(rank - (incl[b] - hist[b]))


def radix_select(values):
    """The kernel's selection restated: (lo, hi, where hi came from) of a non-empty float32 selection without NaN."""
    keys = key_of(values)
    m = keys.size
    lo_rank = (m - 1) // 2
    prefix, rank = 0, lo_rank
    for d, (shift, width) in enumerate(_digits()):
        top = shift + width
        live = keys if d == 0 else keys[(keys >> np.uint32(top)) == np.uint32(prefix >> top)] if top < 32 else keys
        hist = np.bincount(((live >> np.uint32(shift)) & np.uint32((1 << width) - 1)).astype(np.int64), minlength=1 << width)
        b, rank = find_bin(hist, rank)
        prefix |= b << shift
    le = int((keys <= np.uint32(prefix)).sum())
    above = int(keys[keys > np.uint32(prefix)].min()) if le < m else 0xffffffff
    source = rule_select(m, m, le)["hi_from"]
    return float_of(prefix), float_of(prefix if source != "above" else above), source


STAGE_BRANCHES = ("positive", "negative", "zero_meets_inf", "zero_without_inf", "inf_meets_zero", "inf_without_zero", "nan")


def rule_stage(count, target_median, lo, hi, nans, zeros, infs, stages):
    """stage_scales_kernel: the branch taken at each stage, from the statistics of the selection."""
    f = np.float32
    tm, lo, hi = f(target_median), f(lo), f(hi)
    out = []
    with np.errstate(all="ignore"):
        for _ in range(stages):
            if count == 0 or nans:
                out.append("nan")
                continue
            r = tm / lo
            if np.isnan(r):
                out.append("nan")
                nans = 1
            elif r == 0:
                out.append("zero_meets_inf" if infs else "zero_without_inf")
                nans, zeros, infs = (1, zeros, infs) if infs else (0, count, 0)
            elif np.isinf(r):
                out.append("inf_meets_zero" if zeros else "inf_without_zero")
                nans, zeros, infs = (1, zeros, infs) if zeros else (0, 0, count)
            else:
                out.append("negative" if r < 0 else "positive")
            if not nans:
                a, c = lo * r, hi * r
                lo, hi = (c, a) if np.signbit(r) else (a, c)
    return out


def _collapse(branches):
    out = []
    for b in branches:
        if not out or out[-1] != b:
            out.append(b)
    return ">".join(out)


# ---- paths ------------------------------------------------------------------------------------------------------------------------------------
RESIZE_ENTRIES = ("f32", "lut", "u8")
RESIZE_GEOMETRIES = ("upscale_one_tile", "tiles2x2_ragged", "one_pixel_out", "one_pixel_wide_crop", "all_0", "all_255", "checker")
TARGET_PATHS = ["nobox", "box", "ties", "collisions", "elect2_tiny_grid", "elect2_write2", "upscale", "every_value", "refuse_empty_box", "refuse_2p31"]
SELECT_PATHS = (["step1_partial-m0", "step1_full-m0", "step2-m0"] + [f"step1_partial-m{m}-{s}" for m, s in ((1, "prefix_odd"), (2, "above"), (2, "prefix_le"), (3, "prefix_odd"))] +
                ["step1_partial-dense-prefix_odd", "step1_full-dense-above", "step2-dense-prefix_odd", "step4-dense-prefix_odd"] +
                [f"{st}-sparse-{s}" for st in ("step1_partial", "step1_full", "step2", "step4") for s in ("prefix_odd", "above")] +
                ["step1_partial-dense-prefix_le", "step2-sparse-prefix_le", "step1_partial-sparse-nan", "step2-dense-nan"])
PATHS = {
    "resize": ([f"{g}-{e}-c{c}" for g in RESIZE_GEOMETRIES for e in RESIZE_ENTRIES for c in (1, 3)] + [f"odd_crop_padded_rows-{e}-c3" for e in RESIZE_ENTRIES] +
               [f"lds_{k}-{e}-c{c}" for k in ("accept", "refuse") for e, c in (("f32", 1), ("f32", 3), ("lut", 1))] + ["plane_padded-u8-c1", "plane_padded-u8-c3"]),
    "lidar": TARGET_PATHS,
    "dso": TARGET_PATHS + ["png_smaller_edges", "png_larger_edges"],
    "scatter": ["empty", "one", "all_cells", "second_pass_dropped"],
    "unpack": [f"{t}-c{c}-{l}" for t in ("under_one_wave", "chunks_only", "chunks_and_tail") for c in (1, 3) for l in ("plain", "lut")] + ["second_pass"],
    "select": SELECT_PATHS,
    "stage": ["positive", "negative>positive", "zero_meets_inf>nan", "zero_without_inf>inf_meets_zero>nan", "inf_meets_zero>nan",
              "inf_without_zero>zero_meets_inf>nan", "nan"],
    "sparse_sums": [f"{s}-{r}-{d}-{k}" for s, r, d, k in (
        ("under_wave", "full", "nomax", "plain"), ("under_wave", "full", "max", "plain"), ("ragged", "roi", "max", "plain"), ("ragged", "roi", "nomax", "plain"),
        ("ragged", "full", "max", "clamped"), ("ragged", "full", "nomax", "clamped"), ("ragged", "full", "max", "inf"), ("ragged", "full", "nomax", "inf"),
        ("ragged", "roi", "max", "nan_valid"), ("ragged", "full", "nomax", "nan_valid"), ("ragged", "full", "max", "nan_masked"))],
    "stage_sums": ["all_columns-noscale-full-nomax", "all_columns-noscale-roi-max", "one_stage-noscale-full-max", "one_stage-scaled-roi-max",
                   "max_stages-scaled-roi-max", "max_stages-scaled-full-nomax", "sparse7-noscale-full-max-nan_valid", "sparse7-noscale-full-max-nan_masked",
                   "sparse7-noscale-roi-nomax-inf"],
}
# declared, not run: (entry, path) -> why
UNREACHED = {("unpack", "second_pass"): "a second pass of unpack_frame_kernel's chunk loop needs more than grid_cap * wg 16-byte chunks in one plane: an 8 MiB plane and "
                                        "a 100 MB fp32 output, above MAX_DEVICE_BYTES and above every frame the project stores"}


def tie_counts(case):
    """Source coordinates of the case that land exactly on k + 0.5 in the target grid, per axis (rows, columns): np.around decides them."""
    a = case.args
    (h, w), (th, tw) = a["src"], a["out"]
    if case.entry == "dso":
        oh, ow = a["orig"]
        ry = np.clip(np.arange(h, dtype=np.float64) / h * oh, 0, oh - 1)
        rx = np.clip(np.arange(w, dtype=np.float64) / w * ow, 0, ow - 1)
        x0, y0, x1, y1 = a["box"] if a["box"] is not None else (0, 0, ow, oh)
    else:
        ry, rx = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
        x0, y0, x1, y1 = a["box"] if a["box"] is not None else (0, 0, w, h)
    ry, rx = ry[(y0 <= ry) & (ry < y1)], rx[(x0 <= rx) & (rx < x1)]
    ty, tx = (ry - y0) / (y1 - y0) * th, (rx - x0) / (x1 - x0) * tw
    ty, tx = ty[ty <= th - 1], tx[tx <= tw - 1]                     # (beyond the clip nothing is rounded)
    return int((ty - np.floor(ty) == 0.5).sum()), int((tx - np.floor(tx) == 0.5).sum())


def edge_hits(case):
    """D(V)SO: how many rescaled row / column coordinates equal y0, y1, x0, x1 exactly (the half-open crop test on doubles decides them)."""
    a = case.args
    (h, w), (oh, ow) = a["src"], a["orig"]
    ry = np.clip(np.arange(h, dtype=np.float64) / h * oh, 0, oh - 1)
    rx = np.clip(np.arange(w, dtype=np.float64) / w * ow, 0, ow - 1)
    x0, y0, x1, y1 = a["box"]
    return [int((ry == y0).sum()), int((ry == y1).sum()), int((rx == x0).sum()), int((rx == x1).sum())]


def select_features(case):
    """What the selection of a select case exercises: (m, where hi comes from or "nan" / None, digit in which lo and hi first differ)."""
    pred, gt = select_operands(case)
    sel = pred[gt > 0]
    m = sel.size
    if m == 0:
        return 0, None, None
    if np.isnan(sel).any():
        return m, "nan", None
    lo, hi, source = radix_select(sel)
    diff = int(key_of(lo)[0]) ^ int(key_of(hi)[0])
    digit = None if diff == 0 else next(i for i, (shift, width) in enumerate(_digits()) if diff >> shift)
    return m, source, digit


def path_of(case):
    """The path the restated rules put `case` on (None: on none of the declared ones)."""
    a, e, c = case.args, case.entry, constants()
    if e == "resize":
        x0, y0, x1, y1 = a["box"] if a["box"] is not None else (0, 0, a["src"][1], a["src"][0])
        ch, cw, (oh, ow) = y1 - y0, x1 - x0, a["out"]
        r = rule_resize(a["kernel"], a["channels"], ch, cw, oh, ow)
        tag = f"-{a['kernel']}-c{a['channels']}"
        top = largest_tile_rows(a["kernel"], a["channels"])
        if r["code"] != 0:
            return "lds_refuse" + tag if r["max_tile_rows"] == top + 1 == ch else None
        if r["max_tile_rows"] == top:
            return "lds_accept" + tag if ch == top and r["lds"] + c["pt_w"] * a["channels"] > c["lds_limit"] else None
        if a.get("plane_pad"):
            return "plane_padded" + tag if a["kernel"] == "u8" else None
        if a.get("row_pad"):
            return "odd_crop_padded_rows" + tag if x0 & 1 and y0 & 1 and a["channels"] == 3 else None
        if a["fill"] != "random":
            return a["fill"] + tag
        if (oh, ow) == (1, 1):
            return "one_pixel_out" + tag
        if cw == 1:
            return "one_pixel_wide_crop" + tag
        if (r["tiles_x"], r["tiles_y"], r["last_cols"], r["last_rows"]) == (2, 2, 1, 1) and r["h_passes"] > 1:
            return "tiles2x2_ragged" + tag
        ksize = io_ref.resample_coeffs(cw, 0, cw, ow)[0], io_ref.resample_coeffs(ch, 0, ch, oh)[0]
        if (r["tiles_x"], r["tiles_y"]) == (1, 1) and ow < c["pt_w"] and oh > ch and ow > cw and ksize == (3, 3) and r["h_passes"] == 1:
            return "upscale_one_tile" + tag
        return None
    if e in ("lidar", "dso"):
        (h, w), (th, tw) = a["src"], a["out"]
        code = rule_target(h, w, a["box"], a["orig"] if e == "dso" else a["src"])
        if code == c["err_unsupported"]:
            return "refuse_2p31"
        if code != 0:
            return "refuse_empty_box"
        elect, write = rule_grid(h * w)[1], rule_grid(th * tw)[1]
        if a["fill"] == "every_value":
            return "every_value" if (h * w, th * tw) == (65536, 65536) and (elect, write) == (1, 1) else None
        if elect > 1:
            if not (is_second_pass(h * w) and elect == 2):
                return None
            return "elect2_write2" if is_second_pass(th * tw) and write == 2 else "elect2_tiny_grid" if th * tw <= 16 else None
        if write != 1:
            return None
        if e == "dso" and a["src"] != a["orig"]:
            return ("png_smaller_edges" if h < a["orig"][0] and w < a["orig"][1] else "png_larger_edges") if min(edge_hits(case)) > 0 else None
        if a["fill"] == "all" and h * w >= 50 * th * tw:
            return "collisions"
        if min(tie_counts(case)) > 0:
            return "ties"
        if max(tie_counts(case)) > 0:
            return None
        if th > h and tw > w:
            return "upscale"
        return "nobox" if a["box"] is None else "box"
    if e == "scatter":
        n, passes = a["n"], rule_grid(a["n"])[1]
        if n == 0:
            return "empty"
        if passes == 2 and is_second_pass(n) and n % c["wg"] and a["dropped"] > 0 and a["cells"] == n + 7:
            return "second_pass_dropped"
        return None if passes != 1 or a["dropped"] else "one" if n == 1 else "all_cells" if n == a["cells"] else None
    if e == "unpack":
        n = a["h"] * a["w"]
        if rule_grid(n // 16)[1] != 1:
            return None
        tail = "under_one_wave" if n < 64 else "chunks_only" if n % 16 == 0 else "chunks_and_tail"
        return f"{tail}-c{a['channels']}-{'lut' if a['lut'] else 'plain'}"
    if e == "select":
        m, source, _ = select_features(case)
        r = rule_select(a["n"], m)
        if r["empty"] != (source is None):
            return None
        step = {(1, True): "step1_partial", (1, False): "step1_full", (2, True): "step2", (4, True): "step4"}.get((r["steps"], r["partial"]))
        if step is None:
            return None
        if m == 0:
            return f"{step}-m0"
        kind = a["kind"] if a["kind"] in ("dense", "sparse") else f"m{m}" if m <= 3 else "dense" if m == a["n"] else "sparse"
        if kind == "dense" and m != a["n"]:
            return None
        return f"{step}-{kind}-{source}"
    if e == "stage":
        pred, gt = stage_operands(case)
        return _collapse(rule_stage(*selection_stats(pred, gt), c["max_stages"]))
    if e in ("sparse_sums", "stage_sums"):
        b, h, w = a["shape"]
        y0, y1, x0, x1 = a["roi"] if a["roi"] is not None else (0, h, 0, w)
        n = (y1 - y0) * (x1 - x0)
        if a["roi"] is not None and not (y0 > 0 and x0 > 0 and y1 < h and x1 < w):
            return None
        size = "under_wave" if n < 64 else "ragged" if n % c["metric_wg"] else None
        if size is None:
            return None
        tail = f"{'roi' if a['roi'] is not None else 'full'}-{'max' if a['max_distance'] else 'nomax'}"
        if e == "sparse_sums":
            return f"{size}-{tail}-{a['data']}"
        cols = a["columns"]
        dense = c["metric_dense"]
        if len(cols) == 1:
            head = "one_stage"
        elif len(cols) == c["max_stages"]:
            head = "max_stages"
        elif list(cols) == list(range(1, 8)) + [k | dense for k in range(1, 8)]:
            head = "all_columns"
        elif list(cols) == list(range(1, 8)):
            head = "sparse7"
        else:
            return None
        return f"{head}-{'scaled' if a['scaled'] else 'noscale'}-{tail}" + ("" if a["data"] == "plain" else f"-{a['data']}")
    raise KeyError(e)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def _cases():
    c = constants()
    one_pass, step = pass_items(), c["select_step"]
    out = []

    def add(entry, name, path, **args):
        out.append(Case(entry, name, path, args))

    # -- the resize: (source h, w), crop box (x0, y0, x1, y1) or None, output (h, w)
    geoms = {"upscale_one_tile": ((7, 9), None, (12, 20)), "tiles2x2_ragged": ((40, 150), None, (c["pt_h"] + 1, c["pt_w"] + 1)),
             "one_pixel_out": ((5, 6), None, (1, 1)), "one_pixel_wide_crop": ((9, 8), (3, 0, 4, 9), (4, 3)),
             "all_0": ((11, 13), None, (5, 20)), "all_255": ((11, 13), None, (5, 20)), "checker": ((11, 13), None, (5, 20))}
    for g in RESIZE_GEOMETRIES:
        src, box, o = geoms[g]
        for e in RESIZE_ENTRIES:
            for ch in (1, 3):
                add("resize", f"{g}-{e}-c{ch}", f"{g}-{e}-c{ch}", kernel=e, channels=ch, src=src, box=box, out=o,
                    fill=g if g in ("all_0", "all_255", "checker") else "random")
    for e in RESIZE_ENTRIES:            # both crop origins odd, three channels, 5 bytes of padding behind every source row
        add("resize", f"odd_crop_padded_rows-{e}", f"odd_crop_padded_rows-{e}-c3", kernel=e, channels=3, src=(23, 31), box=(3, 5, 28, 20), out=(9, 13), fill="random", row_pad=5)
    # the LDS edge: a strong downscale to one tile row reads the whole crop height.  The source is 12 columns wide, not 4: a Pillow from 11 on
    # resizes an image more than 100 times as tall as wide vertically FIRST (Image.resize), the Pillow of the reference's days and the
    # restatement never do; no image of the project is that narrow, and the cases stay clear of it so that both references hold
    for e, ch in (("f32", 1), ("f32", 3), ("lut", 1)):
        top = largest_tile_rows(e, ch)
        add("resize", f"lds_accept-{e}-c{ch}", f"lds_accept-{e}-c{ch}", kernel=e, channels=ch, src=(top, 12), box=None, out=(c["pt_h"], 3), fill="random")
        add("resize", f"lds_refuse-{e}-c{ch}", f"lds_refuse-{e}-c{ch}", kernel=e, channels=ch, src=(top + 1, 12), box=None, out=(c["pt_h"], 3), fill="random")
    for ch in (1, 3):
        add("resize", f"plane_padded-u8-c{ch}", f"plane_padded-u8-c{ch}", kernel="u8", channels=ch, src=(19, 27), box=(2, 1, 25, 18), out=(7, 11), fill="random", plane_pad=37)
    # -- lidar / D(V)SO targets: (png h, w), box, target grid; D(V)SO: original image size and f_x
    big = (one_pass // 1024 + 1, 1024)                                  # 513 x 1024: strictly between one and two elect passes
    side = math.isqrt(one_pass) + 1                                      # 725 x 725 cells: strictly between one and two write passes
    for e in ("lidar", "dso"):
        def target(name, path, src, box, o, fill, orig=None, focal=707.0912):
            kw = dict(src=src, box=box, out=o, fill=fill)
            if e == "dso":
                kw.update(orig=orig or src, focal=focal)
            add(e, name, path, **kw)
        target("nobox_37x53", "nobox", (37, 53), None, (16, 24), 0.3)
        target("box_37x53", "box", (37, 53), (3, 2, 50, 35), (16, 24), 0.3)
        target("ties_64x96", "ties", (64, 96), None, (32, 48), 0.5)
        target("collisions_40x60", "collisions", (40, 60), None, (4, 6), "all")
        target("elect2_tiny_grid", "elect2_tiny_grid", big, None, (2, 3), 0.5)
        target("elect2_write2", "elect2_write2", big, None, (side, side), 0.5)
        target("upscale_5x7", "upscale", (5, 7), None, (16, 24), 0.6)
        target("every_value", "every_value", (256, 256), None, (256, 256), "every_value")
        target("empty_box", "refuse_empty_box", (37, 53), (10, 5, 10, 30), (16, 24), 0.3)
        target("pixels_2p31", "refuse_2p31", (65536, 32768), None, (16, 24), 0.3)
    add("dso", "every_value_focal_2", "every_value", src=(256, 256), box=None, out=(256, 256), fill="every_value", orig=(256, 256), focal=431.7)
    add("dso", "png_32x64_of_64x128", "png_smaller_edges", src=(32, 64), box=(10, 6, 50, 40), out=(13, 17), fill=0.7, orig=(64, 128), focal=707.0912)
    add("dso", "png_128x256_of_64x128", "png_larger_edges", src=(128, 256), box=(10, 6, 50, 40), out=(13, 17), fill=0.7, orig=(64, 128), focal=707.0912)
    # -- scatter
    add("scatter", "n0", "empty", n=0, cells=35, dropped=0)
    add("scatter", "n1", "one", n=1, cells=35, dropped=0)
    add("scatter", "n35", "all_cells", n=35, cells=35, dropped=0)
    add("scatter", "second_pass", "second_pass_dropped", n=one_pass + 3, cells=one_pass + 10, dropped=5)
    # -- unpack (the geometries of tests/test_gpu_frame_store.py)
    for (h, w), t in (((5, 7), "under_one_wave"), ((16, 64), "chunks_only"), ((33, 130), "chunks_and_tail")):
        for ch in (1, 3):
            for lut in (False, True):
                add("unpack", f"{h}x{w}_c{ch}_{'lut' if lut else 'plain'}", f"{t}-c{ch}-{'lut' if lut else 'plain'}", h=h, w=w, channels=ch, lut=lut)
    # -- median select: one sample per case; the GPU test launches the samples of one size together
    sizes = {"step1_partial": 63, "step1_full": step, "step2": step + 1, "step4": 3 * step + 5}
    add("select", "n1_m0", "step1_partial-m0", n=1, kind="m0")
    add("select", "n1_m1", "step1_partial-m1-prefix_odd", n=1, kind="m1")
    for st, n in sizes.items():
        if st != "step4":
            add("select", f"n{n}_m0", f"{st}-m0", n=n, kind="m0")
        add("select", f"n{n}_dense", f"{st}-dense-{'prefix_odd' if n & 1 else 'above'}", n=n, kind="dense")
        add("select", f"n{n}_dense_drop1", f"{st}-sparse-{'above' if n & 1 else 'prefix_odd'}", n=n, kind="drop1")
        add("select", f"n{n}_sparse_odd", f"{st}-sparse-prefix_odd", n=n, kind="sparse_odd")
        add("select", f"n{n}_sparse_even", f"{st}-sparse-above", n=n, kind="sparse_even")
    for m, kind, s in ((1, "m1", "prefix_odd"), (2, "m2_sign", "above"), (2, "m2_equal", "prefix_le"), (3, "m3", "prefix_odd")):
        add("select", f"n63_{kind}", f"step1_partial-m{m}-{s}", n=63, kind=kind)
    for n, st in ((63, "step1_partial"), (step + 1, "step2")):
        add("select", f"n{n}_low10", f"{st}-sparse-above", n=n, kind="low10")
        add("select", f"n{n}_mid11", f"{st}-sparse-above", n=n, kind="mid11")
        add("select", f"n{n}_top", f"{st}-sparse-above", n=n, kind="top")
        add("select", f"n{n}_sign", f"{st}-sparse-above", n=n, kind="sign")
        add("select", f"n{n}_extremes", f"{st}-sparse-above", n=n, kind="extremes")
    add("select", "n62_all_equal_even", "step1_partial-dense-prefix_le", n=62, kind="all_equal")
    add("select", f"n{step + 1}_median_duplicates", "step2-sparse-prefix_le", n=step + 1, kind="dup")
    add("select", "n63_nan_prediction", "step1_partial-sparse-nan", n=63, kind="nan_sparse")
    add("select", f"n{step + 1}_nan_prediction", "step2-dense-nan", n=step + 1, kind="nan_dense")
    # -- stage ratios: samples of 1 x 8 pixels
    for name, path in (("positive", "positive"), ("negative", "negative>positive"), ("median_inf", "zero_meets_inf>nan"),
                       ("ratio_underflows", "zero_without_inf>inf_meets_zero>nan"), ("median_zero", "inf_meets_zero>nan"),
                       ("ratio_overflows", "inf_without_zero>zero_meets_inf>nan"), ("nan_prediction", "nan"), ("no_target", "nan"),
                       ("subnormal_median", "positive"), ("negative_inf_median", "zero_meets_inf>nan")):
        add("stage", name, path, kind=name)
    # -- metric sums: (batch, H, W), roi (y0, y1, x0, x1)
    for name, shape, roi, maxd, data in (
            ("5x9_nomax", (2, 5, 9), None, None, "plain"), ("5x9_max80", (2, 5, 9), None, 80, "plain"),
            ("roi_max80", (2, 41, 67), (3, 38, 5, 66), 80, "plain"), ("roi_nomax", (2, 41, 67), (3, 38, 5, 66), None, "plain"),
            ("clamped_max80", (2, 37, 61), None, 80, "clamped"), ("clamped_nomax", (2, 37, 61), None, None, "clamped"),
            ("inf_max80", (2, 37, 61), None, 80, "inf"), ("inf_nomax", (2, 37, 61), None, None, "inf"),
            ("nan_at_valid_pixel_roi_max80", (2, 41, 67), (3, 38, 5, 66), 80, "nan_valid"), ("nan_at_valid_pixel_nomax", (2, 37, 61), None, None, "nan_valid"),
            ("nan_at_masked_pixel", (2, 37, 61), None, 80, "nan_masked")):
        path = f"{'under_wave' if shape[1] * shape[2] < 64 else 'ragged'}-{'roi' if roi else 'full'}-{'max' if maxd else 'nomax'}-{data}"
        add("sparse_sums", name, path, shape=shape, roi=roi, max_distance=maxd, data=data)
    dense, every = c["metric_dense"], list(range(1, 8))
    sixteen = [1, 2 | dense, 3, 4 | dense, 5, 6 | dense, 7, 1 | dense, 2, 3 | dense, 4, 5 | dense, 6, 7 | dense, 1, 4][:c["max_stages"]]
    for name, path, shape, roi, maxd, cols, scaled, data in (
            ("all_columns_nomax", "all_columns-noscale-full-nomax", (2, 37, 61), None, None, every + [k | dense for k in every], False, "plain"),
            ("all_columns_roi", "all_columns-noscale-roi-max", (2, 41, 67), (3, 38, 5, 66), 80, every + [k | dense for k in every], False, "plain"),
            ("one_stage", "one_stage-noscale-full-max", (2, 5, 9), None, 80, [4], False, "plain"),
            ("one_stage_scaled", "one_stage-scaled-roi-max", (5, 41, 67), (3, 38, 5, 66), 80, [2 | dense], True, "plain"),
            ("max_stages_scaled_roi", "max_stages-scaled-roi-max", (5, 41, 67), (3, 38, 5, 66), 80, sixteen, True, "plain"),
            ("max_stages_scaled_nomax", "max_stages-scaled-full-nomax", (5, 37, 61), None, None, sixteen, True, "plain"),
            ("nan_at_valid_pixel", "sparse7-noscale-full-max-nan_valid", (2, 37, 61), None, 80, every, False, "nan_valid"),
            ("nan_at_masked_pixel", "sparse7-noscale-full-max-nan_masked", (2, 37, 61), None, 80, every, False, "nan_masked"),
            ("inf_roi_nomax", "sparse7-noscale-roi-nomax-inf", (2, 41, 67), (3, 38, 5, 66), None, every, False, "inf")):
        add("stage_sums", name, path, shape=shape, roi=roi, max_distance=maxd, columns=cols, scaled=scaled, data=data)
    return out


CASES = _cases()


def cases_of(entry, run_only=False):
    """Cases of an entry; `run_only`: without the refusals (those are asserted on the host, nothing is launched)."""
    return [c for c in CASES if c.entry == entry and not (run_only and c.path.startswith(("refuse", "lds_refuse")))]


def case_ids(entry, run_only=False):
    return [c.name for c in cases_of(entry, run_only)]


def gen(case, extra=0):
    return np.random.RandomState(5000 + 11 * CASES.index(case) + extra)


def device_bytes(case):
    """Bytes the GPU test of the case allocates on the device (operands, outputs, scratch)."""
    a, e = case.args, case.entry
    if e == "resize":
        (h, w), (oh, ow) = a["src"], a["out"]
        return h * (w * a["channels"] + a.get("row_pad", 0)) + 12 * oh * ow + 16 * (oh + ow) * 70 + 1024 + 3 * a.get("plane_pad", 0) + 64
    if e in ("lidar", "dso"):
        return 2 * a["src"][0] * a["src"][1] + 8 * a["out"][0] * a["out"][1]
    if e == "scatter":
        return 8 * a["n"] + 4 * a["cells"]
    if e == "unpack":
        n = a["h"] * a["w"]
        return a["channels"] * ((n + 15) // 16 * 16) + 12 * n + 64 + 1024
    if e == "select":
        return 16 * a["n"] + 32
    if e == "stage":
        return 16 * 8 + 32 + 4 * constants()["max_stages"] + 32
    if e in ("sparse_sums", "stage_sums"):
        b, h, w = a["shape"]
        return 8 * b * h * w + 8 * b * (2 + constants()["max_stages"]) + 4 * b * constants()["max_stages"]
    raise KeyError(e)


def table():
    """The path / case table as text: one line per path with the cases that are there for it."""
    lines = []
    for entry, paths in PATHS.items():
        for p in paths:
            names = [c.name for c in cases_of(entry) if c.path == p]
            note = "-- UNREACHED (declared) --" if (entry, p) in UNREACHED else "-- NO CASE --"
            lines.append(f"{entry:12s} {p:44s} {', '.join(names) if names else note}")
    return "\n".join(lines)


# ---- operands and references: the resize ------------------------------------------------------------------------------------------------------
def response_table():
    """256 floats, not monotone: a wrong index shows."""
    return (np.random.RandomState(77).rand(256) * 255).astype(np.float32)


PAD_BYTE = 0xEE             # what the padding behind a source row holds: read by mistake it changes the result
CANARY = 0xAB               # what the padding behind an 8-bit output plane holds before the launch


def resize_image(case):
    """uint8 (H, W[, 3]) source of a resize case."""
    a = case.args
    h, w = a["src"]
    shape = (h, w) if a["channels"] == 1 else (h, w, 3)
    if a["fill"] == "all_0":
        return np.zeros(shape, np.uint8)
    if a["fill"] == "all_255":
        return np.full(shape, 255, np.uint8)
    if a["fill"] == "checker":
        board = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
        return board if a["channels"] == 1 else np.stack([board, 255 - board, board], 2)
    return gen(case).randint(0, 256, size=shape).astype(np.uint8)


def resize_box(case):
    a = case.args
    return a["box"] if a["box"] is not None else (0, 0, a["src"][1], a["src"][0])


def resize_reference_u8(case, img):
    """The integer restatement of Pillow on the crop: uint8 (channels, out_h, out_w)."""
    x0, y0, x1, y1 = resize_box(case)
    oh, ow = case.args["out"]
    out = io_ref.resize_bilinear_u8(np.ascontiguousarray(img[y0:y1, x0:x1]), oh, ow)
    return out.reshape(oh, ow, case.args["channels"]).transpose(2, 0, 1)


def resize_reference_pillow(case, img):
    """Pillow itself, where it is installed (else None)."""
    try:
        from PIL import Image
    except ImportError:
        return None
    oh, ow = case.args["out"]
    out = np.asarray(Image.fromarray(img).crop(resize_box(case)).resize((ow, oh), Image.BILINEAR))
    return out.reshape(oh, ow, case.args["channels"]).transpose(2, 0, 1)


def resize_reference_f32(case, img):
    """What the f32 / lut entries write: float32 (3, out_h, out_w)."""
    a = case.args
    if a["kernel"] == "lut":      # tum_mono_vo_dataset.py:92-94 as tests/test_gpu_tum_mono_vo.py states it: the 8-bit result indexes the table
        u = torch.from_numpy(resize_reference_u8(case, img).copy())
        want = torch.from_numpy(response_table())[u.long()] / 255 - .5
        return want.expand(3, *a["out"]).contiguous() if a["channels"] == 1 else want
    return io_ref.preprocess_image(img, a["box"], *a["out"])


# ---- operands and references: targets, scatter, unpack ----------------------------------------------------------------------------------------
def target_png(case):
    """uint16 (H, W) depth PNG of a lidar / D(V)SO case."""
    a = case.args
    h, w = a["src"]
    rng = gen(case)
    if a["fill"] == "every_value":
        return rng.permutation(65536).astype(np.uint16).reshape(h, w)
    values = rng.randint(1, 65536, size=(h, w)).astype(np.uint16)
    return values if a["fill"] == "all" else np.where(rng.rand(h, w) < a["fill"], values, 0).astype(np.uint16)


def target_reference(case, png):
    a = case.args
    if case.entry == "lidar":
        return io_ref.lidar_inverse_depth(png, a["box"], *a["out"])
    return io_ref.dso_inverse_depth(png, (*a["orig"], a["focal"]), a["box"], *a["out"])


def scatter_operands(case):
    """(uint32 index, float32 value): a permutation into the cells, `dropped` of the indices replaced by values >= cells."""
    a = case.args
    rng = gen(case)
    n, cells = a["n"], a["cells"]
    index = {0: np.zeros(0, np.uint32), 1: np.array([cells - 1], np.uint32)}.get(n)
    if index is None:
        index = rng.permutation(cells)[:n].astype(np.uint32)
    value = rng.rand(n).astype(np.float32) + 0.25
    if a["dropped"]:
        where = rng.permutation(n)[:a["dropped"]]
        index[where] = np.array([cells, cells + 1, 0xffffffff, 0x80000000, cells + 12345], np.uint32)[np.arange(a["dropped"]) % 5]
    return index, value


def scatter_reference(index, value, cells):
    out = np.zeros(cells, np.float32)
    keep = index.astype(np.int64) < cells
    out[index[keep]] = value[keep]
    return out


def unpack_record(case):
    """uint8 (channels, plane_stride) as tests/test_gpu_frame_store.py builds it: every byte value where there is room, 0xAB in the padding."""
    a = case.args
    rng = gen(case)
    n = a["h"] * a["w"]
    rec = np.full((a["channels"], (n + 15) // 16 * 16), CANARY, dtype=np.uint8)
    for ch in range(a["channels"]):
        values = np.concatenate([rng.permutation(256), rng.randint(0, 256, size=max(n - 256, 0))])[:n]
        rec[ch, :n] = rng.permutation(values).astype(np.uint8)
    return rec


def unpack_reference(case, rec):
    a = case.args
    u = torch.from_numpy(rec[:, :a["h"] * a["w"]].reshape(a["channels"], a["h"], a["w"]).copy())
    want = (torch.from_numpy(response_table())[u.long()] if a["lut"] else u.float()) / 255 - .5
    return want.expand(3, a["h"], a["w"]).contiguous() if a["channels"] == 1 else want


# ---- operands and references: median select and stage ratios -----------------------------------------------------------------------------------
def bits_f32(b):
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


def _unselected(rng, n):
    """Targets that are never selected: NaN, negative, -0 and +0."""
    return np.array([NAN, -1.5, -0.0, 0.0, -INF], dtype=np.float32)[rng.randint(0, 5, size=n)]


def _around(rng, m, lo, hi, below=(0.1, 0.5), above=(2.5, 3.0)):
    """m (even) values whose two middle ones are lo, hi: half of the rest below, half above, shuffled."""
    assert m % 2 == 0 and m >= 2
    k = m // 2 - 1
    v = np.concatenate([rng.uniform(*below, size=k), rng.uniform(*above, size=k), [lo, hi]]).astype(np.float32)
    return v[rng.permutation(m)]


def select_operands(case):
    """(prediction, target) float32 (n,) of a select case."""
    a = case.args
    n, kind = a["n"], a["kind"]
    rng = gen(case)
    gt = _unselected(rng, n)
    pred = rng.randn(n).astype(np.float32)
    pos = lambda k: (rng.rand(k) * 3 + 0.01).astype(np.float32)

    def choose(m):
        where = np.sort(rng.permutation(n)[:m])
        gt[where] = pos(m)
        return where
    if kind == "m0":
        pred[rng.randint(0, n)] = NAN                  # a NaN prediction at an unselected pixel is not counted
    elif kind in ("m1", "m3"):
        choose(int(kind[1]))
    elif kind == "m2_sign":
        pred[choose(2)] = np.array([1.0, -1.0], np.float32)
    elif kind == "m2_equal":
        pred[choose(2)] = np.float32(0.37)
    elif kind == "dense":
        gt[:] = pos(n)
    elif kind == "drop1":
        gt[:] = pos(n)
        gt[rng.randint(0, n)] = 0.0
    elif kind in ("sparse_odd", "sparse_even"):
        m = max(int(0.3 * n), 4)
        m += (m & 1) != (kind == "sparse_odd")
        choose(m)
    elif kind in ("low10", "mid11", "top", "sign", "extremes"):
        m = max(int(0.3 * n), 4) & ~1
        where = choose(m)
        if kind == "low10":
            pred[where] = _around(rng, m, bits_f32(0x3f800001), bits_f32(0x3f8003ff))
        elif kind == "mid11":
            pred[where] = _around(rng, m, bits_f32(0x3f800400), bits_f32(0x3f9ffc00))
        elif kind == "top":
            pred[where] = _around(rng, m, np.float32(1.0), np.float32(2.0))
        elif kind == "sign":
            pred[where] = _around(rng, m, np.float32(-1.0), np.float32(1.0), below=(-3.0, -2.0))
        else:       # subnormals, +-inf, 3e38 and zeros of one sign around a subnormal pair of middle values
            v = _around(rng, m, bits_f32(0x00000001), bits_f32(0x00000002), below=(-3.0, -2.0))
            order = np.argsort(v)
            v[order[0]], v[order[1]], v[order[-1]], v[order[-2]] = -INF, -3e38, INF, 3e38
            if m >= 8:
                v[order[m // 2 - 2]] = 0.0
                v[order[m // 2 + 1]] = bits_f32(0x007fffff)
            pred[where] = v
            gt[where[0]], gt[where[1]] = INF, bits_f32(0x00000001)
    elif kind == "all_equal":
        gt[:] = pos(n)
        pred[:] = np.float32(0.37)
    elif kind == "dup":
        m = max(int(0.3 * n), 4) & ~1
        where = choose(m)
        v = _around(rng, m, np.float32(1.25), np.float32(1.25))
        v[np.nonzero(v > 2)[0][:m // 8]] = 1.25            # the median value 2 + m / 8 times: more than lo_rank + 1 keys are <= it
        pred[where] = v
    elif kind == "nan_sparse":
        where = choose(max(int(0.3 * n), 4))
        pred[where[::5]] = NAN
    elif kind == "nan_dense":
        gt[:] = pos(n)
        pred[::1000] = NAN
    else:
        raise KeyError(kind)
    return pred, gt


def selection_stats(pred, gt):
    """(count, target_median, lo, hi, nans, zeros, infs) of one sample by sorting - mr_median_stats from the definition."""
    sel = gt > 0
    m = int(sel.sum())
    if m == 0:
        return 0, np.float32(NAN), np.float32(NAN), np.float32(NAN), 0, 0, 0
    t, p = np.sort(gt[sel]), np.sort(pred[sel])
    return (m, t[(m - 1) // 2], p[(m - 1) // 2], p[m // 2], int(np.isnan(pred[sel]).sum()), int((pred[sel] == 0).sum()), int(np.isinf(pred[sel]).sum()))


def stage_operands(case):
    """(prediction, target) float32 (8,) of a stage case."""
    kind = case.args["kind"]
    rng = gen(case)
    gt = (rng.rand(8) * 3 + 0.5).astype(np.float32)
    pred = (rng.rand(8) * 3 + 0.5).astype(np.float32)
    if kind == "negative":
        pred = -pred
    elif kind == "median_inf":
        pred[:5] = INF
    elif kind == "negative_inf_median":
        pred[:5] = -INF
    elif kind == "ratio_underflows":
        gt[:] = bits_f32(0x00000001)
        pred[:] = (rng.rand(8) * 1e38 + 2e38).astype(np.float32)
    elif kind == "median_zero":
        pred[:5] = 0.0
    elif kind == "ratio_overflows":
        gt[:] = (rng.rand(8) * 1e38 + 2e38).astype(np.float32)
        pred[:] = (rng.rand(8) * 1e-30 + 1e-30).astype(np.float32)
    elif kind == "nan_prediction":
        pred[3] = NAN
    elif kind == "no_target":
        gt[:] = np.array([0.0, -0.0, -1.0, NAN, 0.0, -2.0, 0.0, -INF], np.float32)
    elif kind == "subnormal_median":
        pred[:] = (np.arange(1, 9) * 3).astype(np.uint32).view(np.float32)[rng.permutation(8)]
        gt[:] = (np.arange(1, 9) * 5).astype(np.uint32).view(np.float32)[rng.permutation(8)]
    elif kind != "positive":
        raise KeyError(kind)
    return pred, gt


def median_scaling_chain(pred, gt, stages):
    """The reference's median_scaling (utils/util.py:135-142) applied `stages` times with CPU torch.median, as _median_scaling_cpu of
    tests/test_gpu_median_scaling.py: (B, stages) float32 ratios.  pred, gt: (B, n) float32 tensors."""
    res = pred.clone()
    mask = gt > 0
    rows = []
    for _ in range(stages):
        r = torch.stack([torch.median(gt[i, mask[i]]) / torch.median(res[i, mask[i]]) if bool(mask[i].any()) else torch.tensor(NAN) for i in range(gt.shape[0])]).float()
        rows.append(r)
        res = res * r.view(-1, 1)
    return torch.stack(rows, 1)


# ---- operands and references: the metric sums ----------------------------------------------------------------------------------------------------
def metric_operands(case):
    """(prediction, target) float32 (B, 1, H, W) tensors of a metric case, and for a scaled stage case the (B, stages) ratios."""
    a = case.args
    b, h, w = a["shape"]
    rng = gen(case)
    gt = (rng.rand(b, 1, h, w) * 0.3 + 0.004).astype(np.float32)
    gt[rng.rand(b, 1, h, w) < 0.4] = 0.0                                       # sparse target
    gt[(rng.rand(b, 1, h, w) < 0.1) & (gt > 0)] = 0.011                          # beyond 80 m: masked with max_distance, valid without
    pred = (gt * (1 + 0.3 * rng.randn(b, 1, h, w)) + 0.002 * rng.rand(b, 1, h, w)).astype(np.float32)
    pred = np.where(gt == 0, (rng.rand(b, 1, h, w) * 0.3 + 0.004).astype(np.float32), np.abs(pred) + np.float32(1e-4)).astype(np.float32)
    y0, y1, x0, x1 = a["roi"] if a["roi"] is not None else (0, h, 0, w)
    inside = np.zeros((b, 1, h, w), bool)
    inside[:, :, y0:y1, x0:x1] = True
    valid = np.argwhere(inside & (gt > 0.02))
    masked = np.argwhere(inside & (gt == 0))
    pick = lambda rows, k: [tuple(rows[i]) for i in rng.permutation(len(rows))[:k]]
    valid0 = valid[valid[:, 0] == 0]                                            # the odd values go into sample 0: the others stay finite
    if a["data"] == "clamped":          # negative predictions and predictions below 1 / max_distance, at valid pixels
        for i, p in enumerate(pick(valid0, 40)):
            pred[p] = (-0.1, 1e-4, -3.0, 0.0124)[i % 4]
    elif a["data"] == "inf":
        for i, p in enumerate(pick(valid0, 6) + pick(masked, 2)):
            pred[p] = INF if i % 2 == 0 else -INF
    elif a["data"] == "nan_valid":
        pred[pick(valid0, 1)[0]] = NAN
    elif a["data"] == "nan_masked":
        pred[pick(masked, 1)[0]] = NAN
    scales = None
    if case.entry == "stage_sums" and a["scaled"]:
        k = len(a["columns"])
        scales = (0.7 + 0.6 * rng.rand(b, k)).astype(np.float32)
        for row, (j, v) in zip(range(1, b), ((min(1, k - 1), -1.3), (min(2, k - 1), 0.0), (min(3, k - 1), INF), (0, NAN))):
            scales[row, j] = v                                                  # sample 0 plain; 1 negative, 2 zero, 3 inf, 4 NaN ratio
    return torch.from_numpy(pred), torch.from_numpy(gt), None if scales is None else torch.from_numpy(scales)


def inv_max_distance(max_distance):
    """The kernel's 1.0f / max_distance (fp32), 0 for None."""
    return torch.tensor(0.0) if not max_distance else torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(max_distance), dtype=torch.float32)


def metric_terms(v, g, inv):
    """The per-element terms in fp32, in the kernels' documented order: (masked, [q1 .. q7]).  v, g: fp32 tensors; inv: fp32 0-dim (0 = None)."""
    masked = (g == 0) | (g < inv) if inv > 0 else g == 0                        # get_mask
    gg, pp = torch.relu(g), torch.relu(v)                                       # get_positive_depth
    if inv > 0:
        gg, pp = torch.clamp_min(gg, inv), torch.clamp_min(pp, inv)             # get_absolute_depth
    dg, dp = 1.0 / gg, 1.0 / pp
    d = dp - dg
    lg = torch.log(dp) - torch.log(dg)
    th = torch.max(dg / dp, dp / dg)
    t = [torch.tensor(x, dtype=torch.float32) for x in (1.25, 1.25 * 1.25, 1.25 * 1.25 * 1.25)]
    return masked, [d.abs() / dg, (d * d) / dg, d * d, lg * lg, (th < t[0]).float(), (th < t[1]).float(), (th < t[2]).float()]


def _crop(t, roi):
    return t if roi is None else t[:, :, roi[0]:roi[1], roi[2]:roi[3]]


def sparse_sums_reference(pred, gt, roi, max_distance):
    """(B, 8) float64: the layout of mr_sparse_metric_sums_f32, fp32 terms summed in fp64 over the unmasked pixels."""
    v, g = _crop(pred, roi), _crop(gt, roi)
    masked, q = metric_terms(v, g, inv_max_distance(max_distance))
    keep = (~masked).double()
    cols = [keep.sum((1, 2, 3))] + [torch.where(masked, torch.zeros((), dtype=torch.float64), t.double()).sum((1, 2, 3)) for t in q]
    return torch.stack(cols, 1)


def stage_sums_reference(pred, gt, roi, max_distance, columns, scales):
    """(B, 2 + k) float64: the layout of mr_metric_stage_sums_f32; stage j sees the prediction after j + 1 fp32 multiplies."""
    v, g = _crop(pred, roi).clone(), _crop(gt, roi)
    inv = inv_max_distance(max_distance)
    dense = constants()["metric_dense"]
    masked = (g == 0) | (g < inv) if inv > 0 else g == 0
    out = [(~masked).double().sum((1, 2, 3)), torch.full((g.shape[0],), float(g[0].numel()), dtype=torch.float64)]
    for j, col in enumerate(columns):
        if scales is not None:
            v = v * scales[:, j].view(-1, 1, 1, 1)
        q = metric_terms(v, g, inv)[1][(col & 0xff) - 1].double()
        out.append((q if col & dense else torch.where(masked, torch.zeros((), dtype=torch.float64), q)).sum((1, 2, 3)))
    return torch.stack(out, 1)
