"""Launch paths of csrc/cost_volume.hip (host side, no GPU): which kernel instantiations an mr_cost_volume_* call runs and with which geometry.

    * `rule()`: the launch decision (entry checks, the one-plane-per-wave rule, march_geometry, both depth-chunk loops, the patch LDS formula,
      the choice of the fusion kernel) restated in plain Python.  tests/test_cost_volume_paths.py compares it FIELD BY FIELD with what the
      library itself answers (mr_cost_volume_launch_query - the function the launcher consumes) for every case and for a few hundred
      pseudo-random argument sets, refused ones included.
    * `constants()`: what the rules rest on, read from the source by regular expression, never typed in.
    * `instantiations()`: every kernel instantiation NAMED IN THE KERNEL TABLES of the source (the one launcher, launch_cv, launches nothing
      else).  Each is either run by at least one case or listed in UNREACHABLE with the reason - those are run by NO test.
    * CASES: each names the sad-kernel instantiation and the fusion instantiation it is there for; `path_of(case)` re-derives both from the
      shape through `rule()`.  SUBPATHS: the branches inside a path key (strip counts, row-loop residues, chunking, ...), each with a predicate
      over (case, rule) that at least one case must satisfy.
    * the operands of a case (`operands`) and its CPU reference (`oracle_of`) with the bars of tests/test_gpu_kernels.py (`bars`).
tests/test_gpu_cost_volume_paths.py runs every case on the device."""
import collections
import functools
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DEVICE_BYTES = 100 * 1000 * 1000        # no case holds more than this on the device at once (the fusion second-pass case needs ~84 MB)

FAMILY = {1: "march", 2: "tiled", 3: "patch"}


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _one(pattern, text, flags=0):
    found = re.findall(pattern, text, flags)
    assert len(found) == 1, (pattern, found)
    return found[0]


@functools.lru_cache(None)
def constants():
    """What the launch rules rest on, read from csrc/cost_volume.hip and include/monorec_hip.h."""
    s, hdr = _src("monorec_amd", "csrc", "cost_volume.hip"), _src("include", "monorec_hip.h")
    strip = _one(r"g\.strips = \(W \+ (\d+)\) / (\d+);", s)
    ty = _one(r"for \(int ty = (\d+); ty <= (\d+); \+\+ty\)", s)
    fuse = _one(r"\(total \+ (\d+)\) / (\d+) < (\d+) \? \(total \+ \1\) / \2 : \3\);", s)
    assert int(strip[0]) == int(strip[1]) - 1 and int(fuse[0]) == int(fuse[1]) - 1
    chunk = _one(r"while \(\(long long\)L\.tiles \* F \* B \* nchunk < (\d+) && \(D / \(nchunk \* 2\)\) >= (\d+) && \(D % \(nchunk \* even\)\) == 0\) nchunk \*= 2;", s)
    even = _one(r"const int even = patch \? (\d+) : (\d+);", s)
    tiled = _one(r"constexpr int CV_TX = (\d+), CV_TY = (\d+);", s)
    patch = _one(r"constexpr int CVP_TX = (\d+), CVP_TY = (\d+);", s)
    assert _one(r"constexpr int TX = (\d+), TY = (\d+), NT = TX \* TY;", s) == patch           # the patch kernel's own tile
    fuse_d = sorted({int(v) for v in re.findall(r"cv_fuse_reg_kernel<(\d+), (?:true|false)>", s)})
    assert _one(r"if \(!plane_flags && !tiled && \(D == (\d+) \|\| D == (\d+) \|\| D == (\d+)\)\) \{", s) == tuple(str(v) for v in fuse_d)
    return dict(strip=int(strip[1]), ty_min=int(ty[0]), ty_max=int(ty[1]), ty_default=int(_one(r"int best_ty = (\d+);", s)),
                simds=float(_one(r"const double simds = ([\d.]+);", s)), full_rounds=float(_one(r"rounds >= ([\d.]+) \? 1\.0", s)),
                dp1_below=int(_one(r"dp_env != 2 && waves2 < (\d+)\)", s)), kfs_min_d=int(_one(r"if \(!pixd && D >= (\d+)\) \{", s)),
                fuse_cap=int(fuse[2]), fuse_wg=int(fuse[1]), chunk_grid=int(chunk[0]), chunk_min_planes=int(chunk[1]),
                even_patch=int(even[0]), even_tiled=int(even[1]), tiled_tile=(int(tiled[0]), int(tiled[1])), patch_tile=(int(patch[0]), int(patch[1])),
                fuse_depths=tuple(fuse_d), max_frames=int(_one(r"#define MR_MAX_FRAMES\s+(\d+)", hdr)),
                err_bad_argument=int(_one(r"#define MR_ERR_BAD_ARGUMENT \((-\d+)\)", hdr)),
                err_unsupported=int(_one(r"#define MR_ERR_UNSUPPORTED\s+\((-\d+)\)", hdr)))


# ---- the launch rules, restated ---------------------------------------------------------------------------------------------------------------
def march_geometry(F, B, D, H, W, dp):
    c = constants()
    strips = (W + c["strip"] - 1) // c["strip"]
    pitch = (W + strips - 1) // strips
    npairs = (D + dp - 1) // dp
    per_seg = strips * F * B * npairs
    best, best_ty = -1.0, c["ty_default"]
    for ty in range(c["ty_min"], c["ty_max"] + 1):
        segs = (H + ty - 1) // ty
        rounds = float(per_seg * segs) / c["simds"]
        balance = 1.0 if rounds >= c["full_rounds"] else rounds / float(int(rounds + 0.999999))
        rows = float(H) / (float(segs) * (ty + 4))
        score = balance * rows
        if score > best + 1e-9:
            best, best_ty = score, ty
    return dict(strips=strips, pitch=pitch, npairs=npairs, ty=best_ty, ysegs=(H + best_ty - 1) // best_ty)


def rule_fuse(B, D, H, W, plane_flags, tiled, b8, lean):
    c = constants()
    if not plane_flags and not tiled and D in c["fuse_depths"]:
        return dict(fuse=1, fuse_depths=D, fuse_b8=int(b8), fuse_lean=int(b8 and lean), fuse_pflag=0, fuse_grid=[(H * W + 255) // 256, B])
    blocks = min((B * H * W + c["fuse_wg"] - 1) // c["fuse_wg"], c["fuse_cap"])
    return dict(fuse=2, fuse_depths=0, fuse_b8=0, fuse_lean=0, fuse_pflag=int(plane_flags), fuse_grid=[blocks, 1])


FIELDS = ("status family mode opt sad_grid sad_block dp pixd kfs fd relaxed strips pitch ty ysegs npairs kf_prepass kf_grid tile_w tile_h tiles_x "
          "tiles nchunk dchunk radius lds_bytes flag_memset fuse fuse_depths fuse_b8 fuse_lean fuse_pflag fuse_grid").split()
_ARRAYS = {"sad_grid": 3, "kf_grid": 2, "fuse_grid": 2}


def _blank(status=0):
    out = {k: ([0] * _ARRAYS[k] if k in _ARRAYS else 0) for k in FIELDS}
    out["status"] = status
    return out


def rule(F, B, D, H, W, use_ssim=1, pixd=False, mult_mask=True, patch=3, tiled=False, b8=False, relaxed=False, lean=False,
         exact_division=lambda divisor: True):
    """cv_decide() of csrc/cost_volume.hip: every field of mr_cv_launch.  `exact_division(d)`: the verdict of mr_exact_const_division."""
    c = constants()
    bad, unsupported = c["err_bad_argument"], c["err_unsupported"]
    if use_ssim < 0 or use_ssim > 3:
        return _blank(bad)
    if patch < 1 or patch > 7 or patch % 2 == 0:
        return _blank(unsupported)
    if not mult_mask and D < F:
        return _blank(unsupported)
    if F < 1 or F > c["max_frames"] or B < 1 or H < 5 or W < 5:
        return _blank(bad)
    if D < 2:
        return _blank(bad)
    if b8 and not (patch == 3 and mult_mask and not tiled and D in c["fuse_depths"]):
        return _blank(unsupported)
    border = patch // 2 + 1
    if H < 2 * border + 1 or W < 2 * border + 1:
        return _blank(bad)
    plane_flags = not mult_mask
    L = _blank()
    L["mode"], L["opt"] = use_ssim, int(pixd) | (2 if plane_flags else 0)
    if patch == 3 and use_ssim == 1 and not plane_flags and not tiled:
        dp1 = False
        if not pixd and D >= c["kfs_min_d"]:
            g2 = march_geometry(F, B, D, H, W, 2)
            dp1 = g2["strips"] * g2["ysegs"] * F * B * g2["npairs"] < c["dp1_below"]
        g = march_geometry(F, B, D, H, W, 1 if dp1 else 2)
        fd = bool(exact_division(W - 1)) and bool(exact_division(H - 1))
        kfs = dp1 or D >= c["kfs_min_d"]
        L.update(family=1, dp=1 if dp1 else 2, pixd=int(pixd), kfs=int(kfs), fd=int(fd), relaxed=int((b8 or relaxed) and fd and kfs and not pixd),
                 sad_grid=[g["strips"] * g["ysegs"], F * ((g["npairs"] + 3) // 4), B], sad_block=256, kf_prepass=int(kfs),
                 kf_grid=[(H * W + 255) // 256, B] if kfs else [0, 0], **g)
        L.update(rule_fuse(B, D, H, W, False, False, b8, lean))
        return L
    is_patch = patch != 3
    tw, th = c["patch_tile"] if is_patch else c["tiled_tile"]
    tiles_x = (W + tw - 1) // tw
    tiles = tiles_x * ((H + th - 1) // th)
    even = c["even_patch"] if is_patch else c["even_tiled"]
    nchunk = 1
    while tiles * F * B * nchunk < c["chunk_grid"] and D // (nchunk * 2) >= c["chunk_min_planes"] and D % (nchunk * even) == 0:
        nchunk *= 2
    r = patch // 2
    if is_patch:
        lds = 4 * (6 * (th + 2 * (r + 1)) * (tw + 2 * (r + 1)) + 7 * (th + 2 * r) * (tw + 2 * r))
    else:     # cv_sad_kernel's static arrays: kf[3 HY HX], wr[2 * 3 HY HX], es[2 SY SX]
        lds = 4 * (9 * (th + 4) * (tw + 4) + 2 * (th + 2) * (tw + 2))
    L.update(family=3 if is_patch else 2, tile_w=tw, tile_h=th, tiles_x=tiles_x, tiles=tiles, nchunk=nchunk, dchunk=D // nchunk,
             sad_grid=[tiles, F * nchunk, B], sad_block=tw * th, radius=r, lds_bytes=lds, flag_memset=int(plane_flags))
    L.update(rule_fuse(B, D, H, W, plane_flags, False if is_patch else tiled, b8, lean))
    return L


def query(lib, F, B, D, H, W, use_ssim=1, pixd=False, mult_mask=True, patch=3, tiled=False, b8=False, relaxed=False, lean=False):
    """The library's own answer (mr_cost_volume_launch_query) as the same dict."""
    import ctypes
    from monorec_amd import _lib
    out = _lib.CvLaunch()
    rc = lib.mr_cost_volume_launch_query(F, B, D, H, W, use_ssim, int(pixd), int(mult_mask), patch, int(tiled), int(b8), int(relaxed), int(lean), ctypes.byref(out))
    got = {k: (list(getattr(out, k)) if k in _ARRAYS else int(getattr(out, k))) for k in FIELDS}
    assert rc == got["status"]        # (a decision the kernel tables have no entry for would answer MR_ERR_UNSUPPORTED with status 0)
    return got


# ---- kernel instantiations named in the kernel tables ---------------------------------------------------------------------------------------------
def _bools(text):
    return text.replace("true", "1").replace("false", "0").replace(" ", "")


def _table(name, s):
    """The initialiser of the constant table `name` (up to its closing `};`)."""
    return _one(r"\nconst \w+ %s(?:\[\d*\])+ = \{(.*?)\};" % name, s, re.S)


@functools.lru_cache(None)
def instantiations():
    """Every kernel instantiation the kernel tables of csrc/cost_volume.hip name, as strings like `cv_sad_march_kernel<2,0,1,1,0>`
    (DP, PIXD, KFS, FD, RELAXED), `cv_sad_kernel<32,16,MODE,OPT>`, `cv_sad_patch_kernel<MODE,OPT>`, `cv_fuse_reg_kernel<DD,B8OUT>`,
    `cv_fuse_kernel<PFLAG>`, `cv_kf_stats_kernel`.  One pattern per table; the launcher launches table entries and the prepass, nothing else."""
    s = _src("monorec_amd", "csrc", "cost_volume.hip")
    tw, th = constants()["tiled_tile"]
    tiled = [f"cv_sad_kernel<{tw},{th},{m},{o}>" for m, o in re.findall(r"cv_sad_kernel<CV_TX, CV_TY, (\d), (\d)>", _table("TILED", s))]
    patch = [f"cv_sad_patch_kernel<{m},{o}>" for m, o in re.findall(r"cv_sad_patch_kernel<(\d), (\d)>", _table("PATCH", s))]
    assert "cv_sad_march_kernel<DP, PIXD, KFS, FD, RELAXED>}; }" in s          # march_entry<...>() names the instantiation of its own arguments
    march = [_bools(f"cv_sad_march_kernel<{a}>") for a in re.findall(r"march_entry<(\d(?:, (?:true|false)){4})>\(\)", _table("MARCH", s))]
    reg = [_bools(f"cv_fuse_reg_kernel<{a}>") for a in re.findall(r"cv_fuse_reg_kernel<(\d+, (?:true|false))>", _table("FUSE_REG", s))]
    gen = [_bools(f"cv_fuse_kernel<{a}>") for a in re.findall(r"cv_fuse_kernel<(true|false)>", _table("FUSE_GENERIC", s))]
    out = tiled + patch + march + reg + gen + ["cv_kf_stats_kernel"]
    assert len(set(out)) == len(out)
    # the launch sites: the prepass by name, everything else through a table entry (`kernels.`) - no instantiation is named outside the tables
    sites = re.findall(r"hipLaunchKernelGGL\((\(?\w+)", s)
    assert sorted(sites) == ["cv_kf_stats_kernel"] + ["kernels"] * 4, sites
    return tuple(sorted(out))


# FD = false: the launch takes it when mr_exact_const_division refuses W - 1 or H - 1.  The sequence passed for EVERY integer divisor from 4 to
# 1300 (tried exhaustively on a CPU), tests/test_cost_volume_paths.py asserts it through the library for every size used here and in
# no size anyone launches reaches these five kernels.  They are run by NO test.
_NO_FD = "FD = false needs a W - 1 or H - 1 that fails mr_exact_const_division: none of 4..1300 does, none of the sizes used anywhere does"
UNREACHABLE = {f"cv_sad_march_kernel<{dp},{pixd},{kfs},0,0>": _NO_FD for dp, pixd, kfs in ((1, 0, 1), (2, 1, 1), (2, 0, 1), (2, 1, 0), (2, 0, 0))}


def launched(L):
    """The instantiations a launch described by `L` (rule() or query()) runs: (sad kernel, fusion kernel, prepass or None)."""
    if L["family"] == 1:
        sad = "cv_sad_march_kernel<%d,%d,%d,%d,%d>" % (L["dp"], L["pixd"], L["kfs"], L["fd"], L["relaxed"])
    elif L["family"] == 2:
        sad = "cv_sad_kernel<%d,%d,%d,%d>" % (L["tile_w"], L["tile_h"], L["mode"], L["opt"])
    else:
        sad = "cv_sad_patch_kernel<%d,%d>" % (L["mode"], L["opt"])
    fuse = "cv_fuse_reg_kernel<%d,%d>" % (L["fuse_depths"], L["fuse_b8"]) if L["fuse"] == 1 else "cv_fuse_kernel<%d>" % L["fuse_pflag"]
    return sad, fuse, ("cv_kf_stats_kernel" if L["kf_prepass"] else None)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
# entry: "mode" (mr_cost_volume_mode_f32, or mr_cost_volume_patch_f32 when patch != 3), "tiled", "relaxed", "b8", "lean".
# oracle: the case also runs the CPU-oracle leg (every tiled / patch case; one marching anchor per instantiation).
Case = collections.namedtuple("Case", "name sad fuse entry b f d h w use_ssim pixd mult_mask patch oracle seed")


def _case(name, sad, fuse, entry, b, f, d, h, w, use_ssim=1, pixd=False, mult_mask=True, patch=3, oracle=False, seed=5):
    return Case(name, sad, fuse, entry, b, f, d, h, w, use_ssim, pixd, mult_mask, patch, oracle, seed)


def rule_of(case, exact_division=lambda divisor: True):
    return rule(case.f, case.b, case.d, case.h, case.w, case.use_ssim, case.pixd, case.mult_mask, case.patch, tiled=case.entry == "tiled",
                b8=case.entry in ("b8", "lean"), relaxed=case.entry == "relaxed", lean=case.entry == "lean", exact_division=exact_division)


def path_of(case):
    """(sad instantiation, fusion instantiation) the restated rule puts the case on."""
    return launched(rule_of(case))[:2]


def segment_rows(L, h):
    """Rows every wave of a row segment marches (its TY output rows + 2 above + 2 below), per segment."""
    return [min((s + 1) * L["ty"], h) - s * L["ty"] + 4 for s in range(L["ysegs"])]


def second_pass_shape():
    """Smallest two-sample launch of cv_fuse_kernel whose grid-stride loop makes a second pass while each sample alone makes one: B 2, W = the
    widest strip-count case, H just above cap * wg / (2 W)."""
    c = constants()
    one_pass = c["fuse_cap"] * c["fuse_wg"]
    w = 1024
    h = one_pass // (2 * w) + 1
    assert 2 * h * w > one_pass >= h * w
    return 2, h, w


def _march(dp, pixd, kfs, relaxed=0):
    return "cv_sad_march_kernel<%d,%d,%d,1,%d>" % (dp, pixd, kfs, relaxed)


def _build_cases():
    c = constants()
    tw, th = c["tiled_tile"]
    gen, reg = "cv_fuse_kernel<0>", "cv_fuse_reg_kernel<%d,%d>"
    cs = []
    # -- marching kernel, exact: one plane per wave (small shapes), every strip count, row-count parities, the minimal image, F 1 / F max
    cs += [_case("dp1_w60_one_strip", _march(1, 0, 1), gen, "mode", 1, 2, 8, 20, 60),
           _case("dp1_w61_ragged_strip", _march(1, 0, 1), gen, "mode", 1, 2, 8, 16, 61),
           _case("dp1_w120_two_full_strips", _march(1, 0, 1), gen, "mode", 2, 1, 6, 16, 120),
           _case("dp1_w121_three_strips", _march(1, 0, 1), gen, "mode", 1, 2, 7, 9, 121),
           _case("dp1_w1024_many_strips", _march(1, 0, 1), gen, "mode", 1, 1, 6, 11, 1024),
           _case("dp1_anchor_84x125", _march(1, 0, 1), gen, "mode", 1, 2, 8, 84, 125, oracle=True),
           _case("dp1_5x5_minimal", _march(1, 0, 1), gen, "mode", 1, 1, 6, 5, 5),
           _case("dp1_fmax", _march(1, 0, 1), gen, "mode", 1, c["max_frames"], 9, 21, 47),
           _case("dp1_d32_reg_fusion", _march(1, 0, 1), reg % (32, 0), "mode", 2, 2, 32, 45, 70),
           _case("dp1_d48_reg_fusion", _march(1, 0, 1), reg % (48, 0), "mode", 1, 3, 48, 17, 67),
           _case("dp1_d64_reg_fusion", _march(1, 0, 1), reg % (64, 0), "mode", 1, 1, 64, 23, 33)]
    # -- two planes per wave: per-pixel depths (always), D < 6 (no prepass), and the large launches (>= 4096 waves at two planes per wave)
    cs += [_case("dp2_pixd_kfs_anchor", _march(2, 1, 1), gen, "mode", 1, 2, 8, 84, 125, pixd=True, oracle=True),
           _case("dp2_pixd_kfs_odd_d_h9", _march(2, 1, 1), gen, "mode", 2, 2, 7, 9, 61, pixd=True),
           _case("dp2_pixd_kfs_h18", _march(2, 1, 1), gen, "mode", 1, 1, 6, 18, 40, pixd=True),
           _case("dp2_pixd_kfs_d32", _march(2, 1, 1), reg % (32, 0), "mode", 1, 2, 32, 21, 64, pixd=True),
           _case("dp2_pixd_nokfs_anchor", _march(2, 1, 0), gen, "mode", 1, 2, 5, 84, 125, pixd=True, oracle=True),
           _case("dp2_pixd_nokfs_d2_h9", _march(2, 1, 0), gen, "mode", 2, 1, 2, 9, 40, pixd=True),
           _case("dp2_pixd_nokfs_d3_h18", _march(2, 1, 0), gen, "mode", 1, 3, 3, 18, 61, pixd=True),
           _case("dp2_nokfs_anchor", _march(2, 0, 0), gen, "mode", 1, 2, 5, 84, 125, oracle=True),
           _case("dp2_nokfs_d2_5x5", _march(2, 0, 0), gen, "mode", 1, 1, 2, 5, 5),
           _case("dp2_nokfs_d4_h9", _march(2, 0, 0), gen, "mode", 2, 2, 4, 9, 121),
           _case("dp2_nokfs_d3_h18", _march(2, 0, 0), gen, "mode", 1, 3, 3, 18, 60)]
    cs += _large_march_cases()
    # -- relaxed window sums: one plane per wave on every residue of the three-row loop, the fallbacks to the exact kernels
    cs += [_case("relaxed_dp1_rows12_anchor", _march(1, 0, 1, 1), gen, "relaxed", 1, 2, 8, 80, 128, oracle=True),
           _case("relaxed_dp1_h9_rows13", _march(1, 0, 1, 1), gen, "relaxed", 2, 2, 6, 9, 61),
           _case("relaxed_dp1_h10_rows14", _march(1, 0, 1, 1), gen, "relaxed", 1, 3, 7, 10, 121),
           _case("relaxed_dp1_h11_rows7", _march(1, 0, 1, 1), gen, "relaxed", 2, 1, 9, 11, 60),
           _case("relaxed_dp1_d32", _march(1, 0, 1, 1), reg % (32, 0), "relaxed", 2, 2, 32, 13, 70),
           _case("relaxed_falls_back_pixd", _march(2, 1, 1), gen, "relaxed", 2, 2, 8, 19, 61, pixd=True),
           _case("relaxed_falls_back_d5", _march(2, 0, 0), gen, "relaxed", 2, 2, 5, 19, 61),
           _case("relaxed_falls_back_pixd_d4", _march(2, 1, 0), gen, "relaxed", 1, 2, 4, 10, 40, pixd=True)]
    # -- B8 / lean entries: the relaxed kernels + B8 fusion, the per-pixel-depth and use_ssim != 1 fallbacks
    for entry in ("b8", "lean"):
        cs += [_case(f"{entry}_d32", _march(1, 0, 1, 1), reg % (32, 1), entry, 2, 2, 32, 13, 70),
               _case(f"{entry}_d48_f1", _march(1, 0, 1, 1), reg % (48, 1), entry, 1, 1, 48, 9, 61),
               _case(f"{entry}_d64", _march(1, 0, 1, 1), reg % (64, 1), entry, 1, 3, 64, 10, 33),
               _case(f"{entry}_pixd_d32", _march(2, 1, 1), reg % (32, 1), entry, 2, 2, 32, 11, 61, pixd=True),
               _case(f"{entry}_ssim0_d32", "cv_sad_kernel<%d,%d,0,0>" % (tw, th), reg % (32, 1), entry, 2, 2, 32, 17, 40, use_ssim=0),
               _case(f"{entry}_ssim2_pixd_d48", "cv_sad_kernel<%d,%d,2,1>" % (tw, th), reg % (48, 1), entry, 1, 2, 48, 17, 40, use_ssim=2, pixd=True),
               _case(f"{entry}_ssim3_d64", "cv_sad_kernel<%d,%d,3,0>" % (tw, th), reg % (64, 1), entry, 1, 1, 64, 17, 40, use_ssim=3)]
    # -- tiled kernel: all 16 MODE x OPT (the tiled entry reaches MODE 1 OPT 0 / 1 too), oracle leg on each
    for mode in range(4):
        for opt in range(4):
            cs.append(_case(f"tiled_m{mode}_o{opt}", "cv_sad_kernel<%d,%d,%d,%d>" % (tw, th, mode, opt), "cv_fuse_kernel<%d>" % (opt >> 1), "tiled",
                            1, 2, 8, 84, 125, use_ssim=mode, pixd=bool(opt & 1), mult_mask=not opt & 2, oracle=True, seed=11 + mode))
    # -- patch kernel: all 16 at P 5; P 1 and P 7 at OPT 0 and OPT 3
    for mode in range(4):
        for opt in range(4):
            cs.append(_case(f"patch5_m{mode}_o{opt}", f"cv_sad_patch_kernel<{mode},{opt}>", "cv_fuse_kernel<%d>" % (opt >> 1), "mode",
                            1, 2, 8, 84, 125, use_ssim=mode, pixd=bool(opt & 1), mult_mask=not opt & 2, patch=5, oracle=True, seed=21 + mode))
    for p in (1, 7):
        for opt in (0, 3):
            cs.append(_case(f"patch{p}_m1_o{opt}", f"cv_sad_patch_kernel<1,{opt}>", "cv_fuse_kernel<%d>" % (opt >> 1), "mode",
                            1, 2, 8, 84, 125, pixd=bool(opt & 1), mult_mask=not opt & 2, patch=p, oracle=True, seed=31 + p))
    # -- depth chunking of the tiled / patch kernels, register fusion behind the tiled kernel, frames and samples
    cs += [_case("tiled_chunks_d_forbids", "cv_sad_kernel<%d,%d,1,0>" % (tw, th), gen, "tiled", 2, 2, 10, 20, 40),
           _case("tiled_chunks_2", "cv_sad_kernel<%d,%d,1,0>" % (tw, th), gen, "tiled", 2, 1, 20, 20, 40),
           _case("tiled_chunks_max", "cv_sad_kernel<%d,%d,1,1>" % (tw, th), gen, "tiled", 1, 2, 64, 17, 33, pixd=True),
           _case("tiled_grid_full_no_chunks", "cv_sad_kernel<%d,%d,0,0>" % (tw, th), gen, "mode", 2, c["max_frames"], 8, 113, 250, use_ssim=0),
           _case("tiled_m2_reg_fusion_d48", "cv_sad_kernel<%d,%d,2,0>" % (tw, th), reg % (48, 0), "mode", 2, 2, 48, 17, 40, use_ssim=2),
           _case("tiled_5x5_minimal", "cv_sad_kernel<%d,%d,3,2>" % (tw, th), "cv_fuse_kernel<1>", "mode", 2, 2, 2, 5, 5, use_ssim=3, mult_mask=False),
           _case("patch5_chunks_d_forbids", "cv_sad_patch_kernel<1,0>", gen, "mode", 2, 2, 9, 20, 40, patch=5),
           _case("patch5_chunks_2", "cv_sad_patch_kernel<0,0>", gen, "mode", 2, 1, 10, 20, 40, use_ssim=0, patch=5),
           _case("patch7_chunks_max_d32", "cv_sad_patch_kernel<1,1>", reg % (32, 0), "mode", 1, 2, 32, 17, 33, pixd=True, patch=7),
           _case("patch1_grid_full_no_chunks", "cv_sad_patch_kernel<2,2>", "cv_fuse_kernel<1>", "mode", 2, c["max_frames"], 8, 57, 250, use_ssim=2, mult_mask=False, patch=1),
           _case("patch7_9x9_minimal", "cv_sad_patch_kernel<3,0>", gen, "mode", 2, 1, 4, 9, 9, use_ssim=3, patch=7)]
    # -- the second pass of cv_fuse_kernel's grid-stride loop
    b, h, w = second_pass_shape()
    cs.append(_case("fuse_second_pass", _march(2, 0, 0), gen, "mode", b, 1, 2, h, w))
    return cs


def _search_large(relaxed, want_rows, odd_d=False, exclude=(), min_pixels=0):
    """Smallest launch (bytes of volumes) that runs two planes per wave with the keyframe prepass and without per-pixel depths - the kernels of
    the large configurations - with a row segment of `want_rows(rows)`; searched over the restated rule."""
    c = constants()
    best = None
    for f in (c["max_frames"],):
        for b in (2, 3, 4):
            for d in ((63,) if odd_d else (64, 48)):
                for w in (121, 181):
                    for h in range(17, 48):
                        L = rule(f, b, d, h, w, relaxed=relaxed)
                        if L["dp"] != 2 or not any(want_rows(r) for r in segment_rows(L, h)) or (b, f, d, h, w) in exclude or b * h * w < min_pixels:
                            continue
                        size = (f + 1) * b * d * h * w
                        if best is None or size < best[0]:
                            best = (size, b, f, d, h, w)
    assert best is not None
    return best[1:]


def _large_march_cases():
    cs = []
    for name, want in (("even_rows", lambda r: r % 2 == 0), ("odd_rows", lambda r: r % 2 == 1)):
        b, f, d, h, w = _search_large(False, want, odd_d=name == "odd_rows", min_pixels=10000 if name == "even_rows" else 0)      # (the oracle anchor)
        cs.append(_case(f"dp2_kfs_large_{name}", _march(2, 0, 1), "cv_fuse_kernel<0>" if d == 63 else "cv_fuse_reg_kernel<%d,0>" % d, "mode", b, f, d, h, w,
                        oracle=name == "even_rows"))
    used = []
    for res in range(3):
        b, f, d, h, w = _search_large(True, lambda r, res=res: r % 3 == res, exclude=used, min_pixels=10000 if res == 0 else 0)
        used.append((b, f, d, h, w))
        cs.append(_case(f"relaxed_dp2_large_rows{res}mod3", _march(2, 0, 1, 1), "cv_fuse_reg_kernel<%d,0>" % d, "relaxed", b, f, d, h, w, oracle=res == 0))
    return cs


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def device_bytes(case):
    """Bytes a GPU test of the case holds on the device at once: inputs, NaN-guarded outputs, per-pixel depths, B8 copies."""
    hw = case.h * case.w
    vol = case.b * case.d * hw
    n = (case.f + 1) * (case.b * 3 * hw) * 4 + (case.f + 1) * (vol + hw) * 4
    if case.pixd:
        n += vol * 4
    if case.entry in ("b8", "lean"):
        n += case.f * (vol + hw) * 2
    return n


# ---- branches inside a path key ------------------------------------------------------------------------------------------------------------------------
def _rows(case, L, relaxed, dp, pred):
    return L["family"] == 1 and L["relaxed"] == relaxed and L["dp"] == dp and any(pred(r) for r in segment_rows(L, case.h))


def _subpaths():
    c = constants()
    sp = {
        "strips_1_exactly_full": lambda k, L: L["family"] == 1 and L["strips"] == 1 and k.w == c["strip"],
        "strips_2_ragged": lambda k, L: L["family"] == 1 and L["strips"] == 2 and k.w == c["strip"] + 1,
        "strips_2_full": lambda k, L: L["family"] == 1 and L["strips"] == 2 and k.w == 2 * c["strip"],
        "strips_3": lambda k, L: L["family"] == 1 and L["strips"] == 3 and k.w == 2 * c["strip"] + 1,
        "strips_many": lambda k, L: L["family"] == 1 and L["strips"] >= 16 and k.h <= 16,
        "ysegs_1": lambda k, L: L["family"] == 1 and L["ysegs"] == 1,
        "ysegs_ragged_last": lambda k, L: L["family"] == 1 and L["ysegs"] > 1 and k.h % L["ty"] != 0,
        "npairs_multiple_of_4": lambda k, L: L["family"] == 1 and L["npairs"] % 4 == 0,
        "npairs_not_multiple_of_4": lambda k, L: L["family"] == 1 and L["npairs"] % 4 != 0,
        "odd_d_on_dp2": lambda k, L: L["family"] == 1 and L["dp"] == 2 and k.d % 2 == 1,
        "nchunk_1_d_forbids_tiled": lambda k, L: L["family"] == 2 and L["nchunk"] == 1 and L["tiles"] * k.f * k.b < c["chunk_grid"] and k.d // 2 >= c["chunk_min_planes"],
        "nchunk_1_d_forbids_patch": lambda k, L: L["family"] == 3 and L["nchunk"] == 1 and L["tiles"] * k.f * k.b < c["chunk_grid"] and k.d // 2 >= c["chunk_min_planes"],
        "nchunk_1_grid_full_tiled": lambda k, L: L["family"] == 2 and L["nchunk"] == 1 and L["tiles"] * k.f * k.b >= c["chunk_grid"] and k.d % c["even_tiled"] == 0,
        "nchunk_1_grid_full_patch": lambda k, L: L["family"] == 3 and L["nchunk"] == 1 and L["tiles"] * k.f * k.b >= c["chunk_grid"] and k.d % c["even_patch"] == 0,
        "nchunk_2_tiled": lambda k, L: L["family"] == 2 and L["nchunk"] == 2,
        "nchunk_2_patch": lambda k, L: L["family"] == 3 and L["nchunk"] == 2,
        "nchunk_max_tiled": lambda k, L: L["family"] == 2 and L["nchunk"] == 8,
        "nchunk_max_patch": lambda k, L: L["family"] == 3 and L["nchunk"] == 8,
        "minimal_image_march": lambda k, L: L["family"] == 1 and (k.h, k.w) == (5, 5),
        "minimal_image_tiled": lambda k, L: L["family"] == 2 and (k.h, k.w) == (5, 5),
        "minimal_image_patch7": lambda k, L: L["family"] == 3 and (k.h, k.w) == (9, 9) and k.patch == 7,
        "frames_1": lambda k, L: k.f == 1,
        "frames_max": lambda k, L: k.f == c["max_frames"],
        "fuse_second_pass": lambda k, L: L["fuse"] == 2 and c["fuse_cap"] * c["fuse_wg"] < k.b * k.h * k.w < 2 * c["fuse_cap"] * c["fuse_wg"] and k.h * k.w <= c["fuse_cap"] * c["fuse_wg"],
        "fuse_reg_partial_workgroup": lambda k, L: L["fuse"] == 1 and (k.h * k.w) % 256 != 0,
    }
    for dp in (1, 2):
        for res in range(3):
            sp[f"relaxed_dp{dp}_rows_{res}mod3"] = lambda k, L, dp=dp, res=res: _rows(k, L, 1, dp, lambda r: r % 3 == res)
    for dp, pixd, kfs in ((1, 0, 1), (2, 1, 1), (2, 0, 1), (2, 1, 0), (2, 0, 0)):
        for par in (0, 1):
            sp[f"exact_dp{dp}_pixd{pixd}_kfs{kfs}_rows_{'odd' if par else 'even'}"] = \
                lambda k, L, dp=dp, pixd=pixd, kfs=kfs, par=par: L["pixd"] == pixd and L["kfs"] == kfs and _rows(k, L, 0, dp, lambda r: r % 2 == par)
    return sp


SUBPATHS = _subpaths()


def table():
    lines = ["%-34s %-7s %-36s %-26s %s" % ("case", "entry", "sad kernel", "fusion kernel", "B F D HxW")]
    for k in CASES:
        lines.append("%-34s %-7s %-36s %-26s %d %d %d %dx%d%s" % (k.name, k.entry, k.sad, k.fuse, k.b, k.f, k.d, k.h, k.w, "  +oracle" if k.oracle else ""))
    return "\n".join(lines)


# ---- operands, references, bars ---------------------------------------------------------------------------------------------------------------------------
def operands(case):
    """(batch dict of monorec_amd.synth, per-pixel depths or None), seeded."""
    from monorec_amd import synth
    batch = synth.make_batch(case.b, case.h, case.w, case.f, seed=case.seed)
    pix = synth.make_pixel_depths(case.b, case.d, case.h, case.w, seed=case.seed + 100) if case.pixd else None
    return batch, pix


def select_sample(batch, pix, n):
    """Sample n alone: every tensor of the batch (and lists of tensors) sliced to [n:n+1]."""
    def cut(v):
        if isinstance(v, torch.Tensor):
            return v[n:n + 1].clone()
        if isinstance(v, (list, tuple)):
            return [cut(x) for x in v]
        return v
    return {k: cut(v) for k, v in batch.items()}, (None if pix is None else pix[n:n + 1].clone())


def select_frame(batch, f):
    """Source frame f alone."""
    out = dict(batch)
    for key in ("frames", "intrinsics", "poses"):
        out[key] = [batch[key][f]]
    return out


def oracle_of(case, batch, pix):
    from oracle import monorec_oracle as orc
    use_ssim = {0: False, 1: True}.get(case.use_ssim, case.use_ssim)
    return orc.cost_volume(batch, steps=case.d, patch_size=case.patch, use_ssim=use_ssim, cv_depths=pix, sfcv_mult_mask=case.mult_mask)


def bars(case):
    """The oracle bars tests/test_gpu_kernels.py applies to the options a case composes, per quantity a list of alternatives - each a list of
    (threshold, allowed fraction beyond it) that must ALL hold; the loosest of the options composed = ANY alternative passes.  None invented:
      base      test_cost_volume_with_any_number_of_hypotheses_matches_the_oracle (default / pixel_depths / patch5 variants)
      abs_diff  its abs_diff variant (cv) and test_cost_volume_use_ssim_variants (modes 0, 2, 3)
      pixd      test_cost_volume_per_pixel_depths
      patch     test_cost_volume_patch_sizes (P 1: 3e-4, else 1e-4; cv at 10x), composed options: test_cost_volume_patch_options_compose
    flips: 1e-4 of the pixels (all-depth validity of a single-frame volume, mult-mask paths); patch cases: the cv == 0 pattern, 5e-4."""
    sf, cv = [[(1e-4, 1e-4)]], [[(2e-4, 1e-4)]]
    if case.use_ssim != 1:
        sf.append([(1e-4, 2e-4)])
        cv.append([(1e-4, 2e-4)])
        if case.use_ssim == 0:
            cv.append([(2e-4, 5e-3)])
    if case.pixd:
        cv.append([(1e-4, 2e-4)])
    if case.patch != 3:
        loose = 3e-4 if case.patch == 1 else 1e-4
        sf.append([(loose, 1e-4)])
        cv.append([(10 * loose, 1e-4)])
        if case.use_ssim != 1 or case.pixd or not case.mult_mask:
            sf.append([(2e-5, 1e-3), (1e-3, 5e-4)])
            cv.append([(1e-3, 5e-3)])
    if case.entry == "relaxed":          # test_relaxed_cost_volume_entry_points_against_the_reference_fixture_and_the_oracle, leg 2
        sf.append([(2e-4, 1e-4)])
    return dict(sf=sf, cv=cv, flips=1e-4, cv_zero=5e-4 if case.patch != 3 else None)


def measure(got, want, alternatives):
    """(passes, max |diff|, [(threshold, fraction beyond)] of every threshold named)."""
    d = (got - want).abs()
    fr = {t: float((d > t).float().mean()) for alt in alternatives for t, _ in alt}
    ok = any(all(fr[t] <= cap for t, cap in alt) for alt in alternatives)
    return ok, float(d.max()), sorted(fr.items())
