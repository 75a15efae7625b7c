"""Launch paths of the kernels AROUND the convolutions (host side, no GPU): csrc/eltwise.hip, csrc/heads.hip, the B8 / lean entry points of
csrc/cost_volume.hip, the element-wise companions of csrc/conv_b8.hip and mr_static_mask_f32 (csrc/pointcloud.hip).

For every entry point this module holds
    * `rule_*`: the host launch rule restated in plain Python (which instantiation, how many passes of a grid-stride loop, which loop of a
      kernel runs a 16-block and which a tail, what is refused),
    * PATHS[entry]: the branch combinations the rule and the kernel can take,
    * CASES: the test cases, each NAMING the path it is there for - `path_of(case)` re-derives the path from the case's shape through the
      rule, tests/test_pointwise_paths.py asserts that both agree and that no path is without a case,
    * the CPU references tests/test_gpu_pointwise_paths.py compares the kernels with, and the operands of every case.
The constants the rules rest on (`constants()`) are read from the sources by regular expression, never typed in: the shapes of the
threshold / grid-stride / LDS-budget cases are DERIVED from them, so a changed constant moves the cases along with it or fails them.
tests/test_gpu_pointwise_paths.py runs every case on the device against these references."""
import collections
import functools
import math
import os
import re
import struct

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DEVICE_BYTES = 64 * 1000 * 1000         # no case allocates more than this on the device
MASK_TOL = HEAD_TOL = 2e-6                  # the project's bar of the fp32 one-channel kernels (tests/test_gpu_kernels.py)

Case = collections.namedtuple("Case", "entry name path args")


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@functools.lru_cache(None)
def constants():
    """What the launch rules rest on, read from the sources."""
    elt, heads, pc = _src("monorec_amd", "csrc", "eltwise.hip"), _src("monorec_amd", "csrc", "heads.hip"), _src("monorec_amd", "csrc", "pointcloud.hip")
    hdr = _src("include", "monorec_hip.h")
    wg = int(re.search(r"long long blocks = \(work_items \+ (\d+)\) / (\d+);", elt).group(2))
    assert int(re.search(r"long long blocks = \(work_items \+ (\d+)\) / (\d+);", elt).group(1)) == wg - 1
    cap = re.search(r"if \(blocks > (\d+) \* (\d+)\) blocks = \1 \* \2;", elt)
    quad_min = [int(v) for v in re.findall(r"const long long quad_min = (\d+)ll;", heads)]
    assert len(quad_min) == 1
    thr = re.search(r"\(long long\)batch \* plane <= (\d+)ll \* (\d+) \* (\d+) \? 1 : 2;", heads)
    sm = re.search(r"constexpr int SM_TH = (\d+), SM_TW = (\d+);", pc)
    lds = re.search(r"const size_t lds = \(size_t\)\(SM_TH \+ 2 \* r\) \* \(SM_TW \+ 2 \* r\) \+ \(size_t\)\(SM_TH \+ 2 \* r\) \* SM_TW;\s*"
                    r"if \(lds > (\d+) \* 1024\) return MR_ERR_LDS_BUDGET;", pc)
    frames = int(re.search(r"#define MR_MAX_FRAMES\s+(\d+)", hdr).group(1))
    g = re.search(r"#define MR_MAX_GATHER \((\d+) \+ (\d+) \* MR_MAX_FRAMES\)", hdr)
    fuse_d = sorted({int(v) for v in re.findall(r"cv_fuse_reg_kernel<(\d+), true>", _src("monorec_amd", "csrc", "cost_volume.hip"))})
    return dict(wg=wg, grid_cap=int(cap.group(1)) * int(cap.group(2)), quad_min=quad_min[0],
                vec2_above=int(thr.group(1)) * int(thr.group(2)) * int(thr.group(3)), sm_th=int(sm.group(1)), sm_tw=int(sm.group(2)),
                static_mask_lds=int(lds.group(1)) * 1024, max_frames=frames, max_gather=int(g.group(1)) + int(g.group(2)) * frames,
                max_heads=int(re.search(r"#define MR_MAX_HEADS\s+(\d+)", hdr).group(1)), fuse_depths=tuple(fuse_d),
                err_bad_argument=int(re.search(r"#define MR_ERR_BAD_ARGUMENT \((-\d+)\)", hdr).group(1)),
                err_unsupported=int(re.search(r"#define MR_ERR_UNSUPPORTED\s+\((-\d+)\)", hdr).group(1)),
                err_lds_budget=int(re.search(r"#define MR_ERR_LDS_BUDGET\s+\((-\d+)\)", hdr).group(1)))


# ---- launch rules ---------------------------------------------------------------------------------------------------------------------------
def pass_items():
    """Work items one pass of a grid-stride loop of csrc/eltwise.hip covers at the capped grid."""
    c = constants()
    return c["grid_cap"] * c["wg"]


def rule_grid(work_items):
    """grid_for(): (workgroups, passes of the grid-stride loop the busiest thread makes)."""
    c = constants()
    blocks = min(max((work_items + c["wg"] - 1) // c["wg"], 1), c["grid_cap"])
    return blocks, (work_items + blocks * c["wg"] - 1) // (blocks * c["wg"])


def is_second_pass(work_items):
    """Strictly between one and two passes: some threads loop twice, some once, none three times."""
    return pass_items() < work_items < 2 * pass_items()


def pool3_out(n):
    return (n + 2 - 3) // 2 + 1


def work_items(case):
    """Work items of an eltwise.hip launch (what grid_for() is given)."""
    a = case.args
    if case.entry == "maxpool3x3s2":
        return a["planes"] * pool3_out(a["h"]) * pool3_out(a["w"])
    if case.entry in ("maxpool2x2", "pool2x2_framemax"):            # two outputs per item; mr_maxpool2x2_f32 takes frames * planes planes
        return (a["frames"] if case.entry == "maxpool2x2" else 1) * a["planes"] * (a["h"] // 2) * (a["w"] // 4)
    if case.entry in ("max_over_frames", "resnet_normalize", "nonzero_mean"):
        return a["count"] // 4
    if case.entry == "apply_mask":
        return a["batch"] * a["depths"] * a["plane"] // 4
    raise KeyError(case.entry)


def rule_classifier(batch, plane):
    """mask_classifier_launch: (VEC, planev, totalv, workgroups)."""
    c = constants()
    vec = 1 if batch * plane <= c["vec2_above"] else 2
    planev = plane // vec
    return vec, planev, batch * planev, (batch * planev + 255) // 256


def loop16(n):
    """Which of the two loops `for (; i + 16 <= n; i += 16)` / `for (; i < n; ++i)` run: "blocks", "tail", "both" or "none" (n == 0)."""
    return "none" if n == 0 else "blocks" if n % 16 == 0 else "tail" if n < 16 else "both"


def rule_head(b, c, h, w):
    """mr_depth_heads_f32 per head: (quad mode, workgroups)."""
    pixels = b * h * w
    quad = w % 4 == 0 and pixels >= constants()["quad_min"]
    return quad, ((pixels // 4 + 63) // 64 if quad else (pixels + 15) // 16)


def rule_static_mask(mask_fill):
    """mr_static_mask_f32: 0 and the LDS bytes, or the error code."""
    c = constants()
    if mask_fill < 0 or mask_fill & 1:
        return c["err_bad_argument"], None
    r = mask_fill // 2
    lds = (c["sm_th"] + 2 * r) * (c["sm_tw"] + 2 * r) + (c["sm_th"] + 2 * r) * c["sm_tw"]
    return (c["err_lds_budget"], lds) if lds > c["static_mask_lds"] else (0, lds)


def largest_mask_fill():
    fill = 0
    while rule_static_mask(fill + 2)[0] == 0:
        fill += 2
    return fill


def rule_cost_volume_b8(depths):
    """mr_cost_volume_b8_f32 / _lean_f32: 0 where a register-held fusion kernel with B8 output exists, else MR_ERR_UNSUPPORTED."""
    c = constants()
    return 0 if depths in c["fuse_depths"] else c["err_unsupported"]


# ---- paths ------------------------------------------------------------------------------------------------------------------------------------
CLASSIFIER_PATHS = ([f"vec{v}-c_{cp}-d_{dp}-plain" for v in (1, 2) for cp in ("blocks", "tail", "both") for dp in ("blocks", "tail", "both", "none")] +
                    [f"vec{v}-c_{cp}-d_blocks-b8" for v in (1, 2) for cp in ("blocks", "tail", "both")])      # (a B8 copy needs D % 16 == 0)
PATHS = {
    "maxpool3x3s2": ["even", "odd", "h1", "w1", "second_pass", "second_pass_whole_blocks"],
    "maxpool2x2": ["minimal", "frames3", "second_pass"],
    "pool2x2_framemax": ["minimal", "frames3", "second_pass"],
    "max_over_frames": ["one_item-f1", "one_item-f3", "second_pass-f1", "second_pass-f3"],
    "resnet_normalize": ["one_item", "second_pass"],
    "nonzero_mean": [f"{p}-f{f}" for p in ("one_item", "second_pass") for f in (1, 2, 4)],
    "apply_mask": [f"{w}-{p}" for w in ("one_quad_plane", "wrap") for p in ("in_place", "out_of_place")],
    "gather_small": [f"{i}-{n}" for i in ("iters1", "iters2", "iters3") for n in ("one", "max")],
    "mask_classifier": CLASSIFIER_PATHS,
    "depth_heads": ["quad_one_channel", "alternating_quad_pixel"],
    "cost_volume_b8": ["d32-ragged", "d48-ragged", "d64-ragged", "d32-ragged-f1", "unsupported"],
    "f32_to_b8": ["partial_block", "whole_block", "whole_and_partial"],
    "b8_max": ["frames1", "minimal", "frames3"],
    "static_mask": ["r0", "r1", "r16", "r_max", "refuse_lds", "refuse_odd"],
}
GRID_STRIDE_ENTRIES = ("maxpool3x3s2", "maxpool2x2", "pool2x2_framemax", "max_over_frames", "resnet_normalize", "nonzero_mean", "apply_mask")


def path_of(case):
    """The path the restated rules put `case` on (None: on none of the declared ones)."""
    a, e = case.args, case.entry
    if e in GRID_STRIDE_ENTRIES:
        items = work_items(case)
        blocks, passes = rule_grid(items)
        second = is_second_pass(items) and passes == 2
        if not second and passes != 1:
            return None
    if e == "maxpool3x3s2":
        if second:
            return "second_pass" if items % constants()["wg"] else "second_pass_whole_blocks"
        if a["h"] == 1 or a["w"] == 1:
            return "h1" if a["h"] == 1 and a["w"] > 1 else "w1" if a["h"] > 1 else None
        return {(0, 0): "even", (1, 1): "odd"}.get((a["h"] & 1, a["w"] & 1))
    if e in ("maxpool2x2", "pool2x2_framemax"):
        if second:
            return "second_pass" if items % constants()["wg"] else None
        if (a["planes"], a["h"], a["w"], a["frames"]) == (1, 2, 4, 1):
            return "minimal"
        return "frames3" if a["frames"] == 3 else None
    if e in ("max_over_frames", "resnet_normalize", "nonzero_mean"):
        size = "second_pass" if second and items % constants()["wg"] else "one_item" if items == 1 else None
        if size is None:
            return None
        return size if e == "resnet_normalize" else f"{size}-f{a['frames']}"
    if e == "apply_mask":
        plane4 = a["plane"] // 4
        if second and items % constants()["wg"]:
            # the wrap of a thread (i -> i + one pass) must change b for some threads and d for all of them: i / (plane4 * D) and the
            # plane index both move; every (b, d) pair is met in the first pass
            size = "wrap" if a["batch"] >= 2 and a["depths"] >= 2 and pass_items() % plane4 != 0 and pass_items() >= (a["batch"] * a["depths"] - 1) * plane4 else None
        else:
            size = "one_quad_plane" if plane4 == 1 else None
        return None if size is None else f"{size}-{'in_place' if a['in_place'] else 'out_of_place'}"
    if e == "gather_small":
        iters = (a["floats_each"] + 63) // 64
        num = "one" if a["num"] == 1 else "max" if a["num"] == constants()["max_gather"] else None
        return None if num is None or not 1 <= iters <= 3 else f"iters{iters}-{num}"
    if e == "mask_classifier":
        vec = rule_classifier(a["batch"], a["plane"])[0]
        if a["b8"] and (a["depths"] == 0 or a["depths"] % 16):
            return None
        return f"vec{vec}-c_{loop16(a['channels'])}-d_{loop16(a['depths'])}-{'b8' if a['b8'] else 'plain'}"
    if e == "depth_heads":
        modes = [rule_head(*s)[0] for s in a["heads"]]
        if modes == [True] and a["heads"][0][1] == 1:
            return "quad_one_channel"
        if len(modes) == constants()["max_heads"] and modes == [True, False, True, False]:
            return "alternating_quad_pixel"
        return None
    if e == "cost_volume_b8":
        if rule_cost_volume_b8(a["depths"]) != 0:
            return "unsupported"
        ragged = (a["h"] * a["w"]) % 256 != 0 and a["h"] * a["w"] > 256
        return f"d{a['depths']}-ragged{'-f1' if a['frames'] == 1 else ''}" if ragged and a["frames"] in (1, 2) else None
    if e == "f32_to_b8":
        c = a["c"]
        return "partial_block" if c < 8 else "whole_block" if c % 8 == 0 else "whole_and_partial"
    if e == "b8_max":
        if (a["h"], a["w"]) == (2, 2):
            return "minimal"
        return {1: "frames1", 3: "frames3"}.get(a["frames"])
    if e == "static_mask":
        code, _ = rule_static_mask(a["mask_fill"])
        c = constants()
        if code == c["err_bad_argument"]:
            return "refuse_odd"
        if code == c["err_lds_budget"]:
            return "refuse_lds" if a["mask_fill"] == largest_mask_fill() + 2 else None
        r = a["mask_fill"] // 2
        return "r_max" if a["mask_fill"] == largest_mask_fill() else {0: "r0", 1: "r1", 16: "r16"}.get(r)
    raise KeyError(e)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def _smallest(pred, start):
    n = start
    while not pred(n):
        n += 1
    return n


def _second_pass_count4():
    """Smallest float4 count strictly above one pass that is no multiple of the workgroup size... + 3: `524288 + 3` at the present constants."""
    return pass_items() + 3


def _cases():
    c = constants()
    one_pass, wg = pass_items(), c["wg"]
    out = []

    def add(entry, name, path, **args):
        out.append(Case(entry, name, path, args))

    # -- mr_maxpool3x3s2_f32: (planes, H, W).  second pass: 9 planes, output rows of 230 - the fewest output rows that exceed one pass, one
    # fewer input row where that count is a whole number of workgroups (9 x 256 x 230 = 529 920 = 2070 x 256 at the present constants)
    add("maxpool3x3s2", "even_6x8", "even", planes=6, h=6, w=8)
    add("maxpool3x3s2", "odd_17x23", "odd", planes=15, h=17, w=23)
    add("maxpool3x3s2", "h1", "h1", planes=6, h=1, w=9)
    add("maxpool3x3s2", "w1", "w1", planes=6, h=9, w=1)
    ho = _smallest(lambda n: 9 * n * 230 > one_pass and (9 * n * 230) % wg != 0, 1)
    add("maxpool3x3s2", "second_pass_ragged", "second_pass", planes=9, h=2 * ho - 1, w=459)
    ho = _smallest(lambda n: 9 * n * 230 > one_pass and (9 * n * 230) % wg == 0, 1)
    add("maxpool3x3s2", "second_pass_511x459", "second_pass_whole_blocks", planes=9, h=2 * ho - 1, w=459)
    # -- mr_maxpool2x2_f32 / mr_pool2x2_framemax_f32: (frames, planes, H, W); an item = 2 rows x 4 columns
    hh = _smallest(lambda n: 5 * n * 410 > one_pass and (5 * n * 410) % wg != 0, 1)             # 257 -> 514 x 1640: 526 850 items
    for entry in ("maxpool2x2", "pool2x2_framemax"):
        add(entry, "minimal_2x4", "minimal", frames=1, planes=1, h=2, w=4)
        add(entry, "frames3_12x16", "frames3", frames=3, planes=10, h=12, w=16)
    add("pool2x2_framemax", "second_pass_514x1640", "second_pass", frames=2, planes=5, h=2 * hh, w=1640)
    add("maxpool2x2", "second_pass_514x1640", "second_pass", frames=1, planes=5, h=2 * hh, w=1640)
    # -- 16 bytes per lane over `count` floats
    big = 4 * _second_pass_count4()
    for f in (1, 3):
        add("max_over_frames", f"count4_f{f}", f"one_item-f{f}", frames=f, count=4)
        add("max_over_frames", f"second_pass_f{f}", f"second_pass-f{f}", frames=f, count=big)
    add("resnet_normalize", "count4", "one_item", frames=1, count=4)
    add("resnet_normalize", "second_pass", "second_pass", frames=1, count=big)
    for f in (1, 2, 4):
        add("nonzero_mean", f"count4_f{f}", f"one_item-f{f}", frames=f, count=4)
        add("nonzero_mean", f"second_pass_f{f}", f"second_pass-f{f}", frames=f, count=big)
    # -- mr_apply_mask_f32: B 2, D 5, a tenth of a pass + 3 float4 per plane (52 431): 22 items wrap, path_of() checks the rest
    plane4 = one_pass // 10 + 3
    for in_place in (True, False):
        tag = "in_place" if in_place else "out_of_place"
        add("apply_mask", f"plane4_{tag}", f"one_quad_plane-{tag}", batch=2, depths=5, plane=4, in_place=in_place)
        add("apply_mask", f"wrap_{tag}", f"wrap-{tag}", batch=2, depths=5, plane=4 * plane4, in_place=in_place)
    # -- mr_gather_small_f32
    for floats, iters in ((1, 1), (65, 2), (130, 3)):
        add("gather_small", f"floats{floats}_one", f"iters{iters}-one", num=1, floats_each=floats)
        add("gather_small", f"floats{floats}_max", f"iters{iters}-max", num=c["max_gather"], floats_each=floats)
    # -- mask classifier.  VEC 2: batch 3 and the smallest plane 210 x W (W even) with 3 x plane above the threshold whose thread count is no
    # multiple of 256 (210 x 212, W % 4 == 0: totalv 66 780); VEC 1: the same at 10 x 14.  C 32 / 13 / 19 and D 16 / 5 / 20 / none: blocks, tail, both.
    w2 = _smallest(lambda w: w % 4 == 0 and 3 * 210 * w > c["vec2_above"] and (3 * 210 * w // 2) % 256 != 0, 4)
    for vec, (h, w) in ((1, (10, 14)), (2, (210, w2))):
        for ch in (32, 13, 19):
            for d in (16, 5, 20, 0):
                add("mask_classifier", f"vec{vec}_c{ch}_d{d}", f"vec{vec}-c_{loop16(ch)}-d_{loop16(d)}-plain", batch=3, channels=ch, plane=h * w, hw=(h, w), depths=d, b8=False)
            add("mask_classifier", f"vec{vec}_c{ch}_d16_b8", f"vec{vec}-c_{loop16(ch)}-d_blocks-b8", batch=3, channels=ch, plane=h * w, hw=(h, w), depths=16, b8=True)
    add("mask_classifier", "vec2_c19_d32_b8", "vec2-c_both-d_blocks-b8", batch=3, channels=19, plane=210 * w2, hw=(210, w2), depths=32, b8=True)
    add("mask_classifier", "at_threshold", "vec1-c_both-d_both-plain", batch=1, channels=35, plane=c["vec2_above"], hw=(1, c["vec2_above"]), depths=20, b8=False)
    add("mask_classifier", "threshold_plus_2", "vec2-c_both-d_both-plain", batch=1, channels=35, plane=c["vec2_above"] + 2, hw=(1, c["vec2_above"] + 2), depths=20,
        b8=False)
    # -- depth heads: C = 1 in quad mode at exactly quad_min pixels; four heads alternating quad / pixel
    side = math.isqrt(c["quad_min"])
    assert side * side == c["quad_min"] and side % 4 == 0
    add("depth_heads", "quad_c1", "quad_one_channel", heads=[(1, 1, side, side)])
    add("depth_heads", "quad_pixel_quad_pixel", "alternating_quad_pixel", heads=[(1, 3, side, side), (1, 5, 7, 9), (1, 2, side, side + 4), (1, 4, 3, 5)])
    # -- mr_cost_volume_b8_f32 / _lean_f32: 45 x 70 = 3150 pixels = 12 workgroups and 78 pixels
    for d in c["fuse_depths"]:
        add("cost_volume_b8", f"d{d}_45x70", f"d{d}-ragged", batch=2, h=45, w=70, frames=2, depths=d)
    add("cost_volume_b8", "d32_45x70_f1", "d32-ragged-f1", batch=2, h=45, w=70, frames=1, depths=c["fuse_depths"][0])
    add("cost_volume_b8", "d20_refused", "unsupported", batch=2, h=45, w=70, frames=2, depths=20)
    # -- layout conversions and the B8 max kernels
    for ch, path in ((1, "partial_block"), (8, "whole_block"), (44, "whole_and_partial")):
        add("f32_to_b8", f"c{ch}", path, n=2, c=ch, hw=331)
    add("b8_max", "frames1", "frames1", frames=1, batch=2, c=12, h=6, w=10)
    add("b8_max", "minimal_2x2", "minimal", frames=2, batch=1, c=8, h=2, w=2)
    add("b8_max", "frames3_inf", "frames3", frames=3, batch=2, c=44, h=12, w=20)
    # -- mr_static_mask_f32
    top = largest_mask_fill()
    for shape in ((1, 17, 65), (2, 33, 130)):
        for fill in (0, 2, 32):
            add("static_mask", f"fill{fill}_{shape[1]}x{shape[2]}", f"r{fill // 2}", shape=shape, mask_fill=fill)
    add("static_mask", "largest_fill_20x70", "r_max", shape=(3, 20, 70), mask_fill=top)
    add("static_mask", "largest_fill_20x260", "r_max", shape=(2, 20, 260), mask_fill=top)
    add("static_mask", "fill_beyond_lds", "refuse_lds", shape=(3, 20, 70), mask_fill=top + 2)
    add("static_mask", "odd_fill", "refuse_odd", shape=(1, 17, 65), mask_fill=3)
    return out


CASES = _cases()


def cases_of(entry):
    return [c for c in CASES if c.entry == entry]


def case_ids(entry):
    return [c.name for c in cases_of(entry)]


def device_bytes(case):
    """Bytes the GPU test of the case allocates on the device (inputs, outputs, and the second output set where two entry points run)."""
    a, e = case.args, case.entry
    if e == "maxpool3x3s2":
        return 4 * a["planes"] * (a["h"] * a["w"] + pool3_out(a["h"]) * pool3_out(a["w"]))
    if e == "maxpool2x2":
        return 5 * a["frames"] * a["planes"] * a["h"] * a["w"]                                   # source + a quarter of it
    if e == "pool2x2_framemax":
        return a["planes"] * a["h"] * a["w"] * (5 * a["frames"] + 4)                             # source, pooled, frame maximum
    if e in ("max_over_frames", "resnet_normalize", "nonzero_mean"):
        return 4 * a["count"] * (a["frames"] + 1)
    if e == "apply_mask":
        return 4 * a["batch"] * a["plane"] * (2 * a["depths"] + 1)
    if e == "gather_small":
        return 4 * a["num"] * a["floats_each"] * 2
    if e == "mask_classifier":
        per = a["batch"] * a["plane"]
        return 4 * per * (a["channels"] + 2 * (1 + a["depths"])) + 2 * per * a["depths"]        # both entry points' outputs side by side
    if e == "depth_heads":
        return sum(4 * b * (ch + 1) * h * w for b, ch, h, w in a["heads"])
    if e == "cost_volume_b8":
        per = a["batch"] * a["depths"] * a["h"] * a["w"]
        return 2 * (4 * per * (1 + a["frames"]) + 2 * per * a["frames"]) + 4 * 3 * a["batch"] * a["h"] * a["w"] * (1 + a["frames"])
    if e == "f32_to_b8":
        return a["n"] * a["hw"] * (8 * a["c"] + 16 * ((a["c"] + 7) // 8))
    if e == "b8_max":
        per = a["batch"] * ((a["c"] + 7) // 8) * a["h"] * a["w"] * 16
        return per * a["frames"] * 5 // 4 + 2 * per
    if e == "static_mask":
        b, h, w = a["shape"]
        return 8 * b * h * w
    raise KeyError(e)


def table():
    """The path / case table as text: one line per path with the cases that are there for it."""
    lines = []
    for entry, paths in PATHS.items():
        for p in paths:
            names = [c.name for c in cases_of(entry) if c.path == p]
            lines.append(f"{entry:18s} {p:34s} {', '.join(names) if names else '-- NO CASE --'}")
    return "\n".join(lines)


# ---- operands and references --------------------------------------------------------------------------------------------------------------------
INF = float("inf")


def gen(case, extra=0):
    return torch.Generator().manual_seed(1000 + 7 * CASES.index(case) + extra)


def sprinkle(x, g, values, every=97):
    """`values` written over x (flat) at a stride of about `every`, cyclically: the same positions in no two frames."""
    flat = x.view(-1)
    n = flat.numel()
    start = int(torch.randint(0, min(every, n), (1,), generator=g))
    idx = torch.arange(start, n, every)
    if idx.numel():
        flat[idx] = torch.tensor(values, dtype=x.dtype)[torch.arange(idx.numel()) % len(values)]
    return x


def max_input(shape, g):
    """Gaussian data with +-inf sprinkled in (no NaN: the references of the max kernels then agree with torch bit for bit)."""
    x = torch.randn(*shape, generator=g)
    return sprinkle(x, g, [INF, -INF, 0.0, -0.0], every=61) if x.numel() > 4 else x


def nonzero_mean_input(frames, count, g):
    """(frames, count): per position one of - all frames zero; some frames -0.0; some frames exactly 0; one +-inf; plain Gaussian."""
    x = torch.randn(frames, count, generator=g)
    kind = torch.arange(count) % 5 if count > 4 else torch.arange(count)         # count == 4: the first four kinds, one position each
    x[:, kind == 0] = 0.0
    which = torch.randint(0, frames, (count,), generator=g)
    rows = torch.arange(frames).unsqueeze(1)
    x = torch.where((kind == 1) & (rows == which), torch.tensor(-0.0), x)
    x = torch.where((kind == 2) & (rows != which), torch.tensor(0.0), x)           # all but one frame exactly 0 (F = 1: none)
    sign = torch.where(torch.arange(count) % 2 == 0, INF, -INF)
    x = torch.where((kind == 3) & (rows == which), sign, x)
    return x.contiguous()


def nonzero_mean_exact(x):
    """The kernel's own order in torch: sequential fp32 sum over the frames / max(count of != 0, 1)."""
    s = x[0].clone()
    n = (x[0] != 0).float()
    for f in range(1, x.shape[0]):
        s = s + x[f]
        n = n + (x[f] != 0).float()
    return s / n.clamp_min(1.0)


def nonzero_mean_bound(x):
    """(fp64 value, bound): |fp32 sequential result - fp64 value| <= (F - 1) 2^-24 sum|x_f| / max(n, 1) + 2^-24 |result| (F - 1 roundings of
    partial sums, each <= sum|x_f|, and one of the quotient).  Positions with an infinity are compared exactly by the caller."""
    xd = x.double()
    n = (xd != 0).sum(0).clamp_min(1).double()
    val = xd.sum(0) / n
    return val, (x.shape[0] - 1) * 2.0 ** -24 * xd.abs().sum(0) / n + 2.0 ** -24 * val.abs()


def classifier_operands(case):
    a = case.args
    g = gen(case)
    b, c, d = a["batch"], a["channels"], a["depths"]
    h, w = a["hw"]
    x = torch.randn(b, c, h, w, generator=g)
    wt = torch.randn(1, c, 1, 1, generator=g) * (1.0 / math.sqrt(c))
    bias = torch.randn(1, generator=g) * 0.1
    cv = torch.randn(b, max(d, 1), h, w, generator=g)
    return x, wt, bias, cv


def classifier_mask_reference(x, wt, bias, dtype=torch.float64):
    """sigmoid(conv1x1) in `dtype` (monorec_model.py:340-343,383)."""
    return torch.sigmoid(F.conv2d(x.to(dtype), wt.to(dtype), bias.to(dtype)))


def head_operands(case):
    g = gen(case)
    out = []
    for b, c, h, w in case.args["heads"]:
        out.append((torch.randn(b, c, h, w, generator=g), torch.randn(1, c, 3, 3, generator=g) * (0.5 / math.sqrt(9 * c)), torch.randn(1, generator=g) * 0.1))
    return out


HEAD_LO, HEAD_HI = 0.0025, 0.33


def head_reference(x, wt, bias, dtype=torch.float64):
    """Conv2d(C, 1, 3, padding=1), abs(tanh), inverse-depth affine (monorec_model.py:520-523,554-557,716-717) in `dtype`."""
    t = torch.abs(torch.tanh(F.conv2d(x.to(dtype), wt.to(dtype), bias.to(dtype), padding=1)))
    return (1 - t) * HEAD_LO + t * HEAD_HI


def to_b8(x):
    """dense (N, C, H, W) fp32 -> (N, ceil(C / 8), H, W, 8) bf16 by torch's rounding (padded channels zero)."""
    n, c, h, w = x.shape
    cb = (c + 7) // 8
    p = torch.zeros(n, cb * 8, h, w, dtype=torch.float32)
    p[:, :c] = x
    return p.view(n, cb, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def from_b8(t, c):
    n, cb, h, w, _ = t.shape
    return t.float().permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)[:, :c].contiguous()


def b8_bits(t, c):
    """The bf16 bit patterns of a B8 tensor as (N, C, H, W) int32."""
    n, cb, h, w, _ = t.shape
    return (t.view(torch.int16).to(torch.int32) & 0xffff).permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)[:, :c].contiguous()


def bf(x):
    return x.to(torch.bfloat16).float()


def f32_from_bits(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# fp32 bit patterns placed in the data of the layout-conversion cases: (class, fp32 bits, bf16 bits where the issue names them)
BF16_EDGES = [
    ("tie_to_even_down", 0x3f808000, 0x3f80), ("tie_to_even_up", 0x3f818000, 0x3f82),
    ("below_tie", 0x3f807fff, 0x3f80), ("above_tie", 0x3f808001, 0x3f81),
    ("overflow_to_inf", 0x7f7f8000, 0x7f80), ("largest_that_stays_finite", 0x7f7f7fff, 0x7f7f),
    ("plus_inf", 0x7f800000, 0x7f80), ("minus_inf", 0xff800000, 0xff80), ("minus_zero", 0x80000000, 0x8000),
    ("denormal_smallest", 0x00000001, 0x0000), ("denormal_half", 0x00400000, 0x0040), ("denormal_largest", 0x007fffff, 0x0080),
    ("denormal_tie_down", 0x00008000, 0x0000), ("denormal_tie_up", 0x00018000, 0x0002),
    ("quiet_nan", 0x7fc00000, None), ("signalling_nan", 0x7f800001, None), ("negative_quiet_nan", 0xffc12345, None),
]


def edge_tensor():
    """The fp32 values of BF16_EDGES (built from the bit patterns: no arithmetic touches them)."""
    return torch.tensor([b if b < 2 ** 31 else b - 2 ** 32 for _, b, _ in BF16_EDGES], dtype=torch.int32).view(torch.float32)


def conversion_input(case):
    """Unrounded Gaussian data with the edge table written over the first elements of every (sample, channel) plane."""
    a = case.args
    g = gen(case)
    x = torch.randn(a["n"], a["c"], a["hw"], 1, generator=g)
    e = edge_tensor()
    for ch in range(a["c"]):
        x[:, ch, ch:ch + e.numel(), 0] = e                   # another offset per channel: every element slot of a group meets every edge
    return x


def bf16_bits(x):
    """torch's fp32 -> bf16 conversion as bit patterns (int32, 0..65535)."""
    return x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xffff


def is_nan_bf16_bits(bits):
    return ((bits & 0x7f80) == 0x7f80) & ((bits & 0x007f) != 0)


def static_mask_input(case):
    """cv_mask with few moving pixels: values below the threshold, some exactly AT it (they count as moving), some above.  Sample 0 of
    the three-sample cases has no moving pixel at all."""
    b, h, w = case.args["shape"]
    g = gen(case)
    thr = torch.tensor(0.1, dtype=torch.float32)
    x = torch.rand(b, 1, h, w, generator=g) * 0.09
    n = max(1, h * w // 400)
    wide = case.args["mask_fill"] > 64                         # a wide box: moving pixels in the left eighth only, so that the right stays static
    for s in range(b):
        if b == 3 and s == 0:
            continue
        ys, xs = torch.randint(0, h, (n,), generator=g), torch.randint(0, w // 8 if wide else w, (n,), generator=g)
        x[s, 0, ys, xs] = torch.where(torch.arange(n) % 2 == 0, thr, torch.tensor(0.7))
    x[b - 1, 0, 0, 0] = thr                                    # a corner, exactly at the threshold
    below = torch.tensor(0.1, dtype=torch.float32).view(torch.int32) - 1
    x[b - 1, 0, h - 1, w - 1] = below.view(torch.float32)      # the largest fp32 below the threshold: not moving
    return x, float(thr)


def cost_volume_finalise(raw, border=2):
    """What cv_fuse_reg_kernel stores as a single-frame volume, from the raw per-frame costs (B, D, H, W) it reads (csrc/cost_volume.hip:
    `(1 - 2 |raw|) * vm`): vm = 1 inside the border of width `border` where no raw value of the pixel has its sign bit set, else 0."""
    b, d, h, w = raw.shape
    inside = torch.zeros(h, w, dtype=torch.bool)
    inside[border:h - border, border:w - border] = True
    signed = (raw.view(torch.int32) < 0).any(1, keepdim=True)
    vm = (inside.view(1, 1, h, w) & ~signed).float()
    return (1.0 - raw.abs() * 2.0) * vm
