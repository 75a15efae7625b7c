"""Host side (no GPU): the launch paths of csrc/cost_volume.hip (tests/cost_volume_paths.py) that tests/test_gpu_cost_volume_paths.py runs.
The constants the rules rest on parse and are pinned; the restated rule equals the library's own answer (mr_cost_volume_launch_query, the
function the launcher consumes) field by field; every kernel instantiation named in the kernel tables is run by a case or is on the pinned
unreachable list; every case sits on the path it names; every branch inside a path key has a case; every CPU reference runs here."""
import random
import re

import pytest
import torch

import cost_volume_paths as cp


def _query_case(lib, k):
    return cp.query(lib, k.f, k.b, k.d, k.h, k.w, k.use_ssim, k.pixd, k.mult_mask, k.patch, tiled=k.entry == "tiled", b8=k.entry in ("b8", "lean"),
                    relaxed=k.entry == "relaxed", lean=k.entry == "lean")


def test_constants_parse_and_are_pinned():
    c = cp.constants()
    assert (c["strip"], c["ty_min"], c["ty_max"], c["ty_default"], c["simds"], c["full_rounds"]) == (60, 8, 64, 64, 1024.0, 8.0)
    assert (c["dp1_below"], c["kfs_min_d"], c["fuse_cap"], c["fuse_wg"]) == (4096, 6, 8192, 256)
    assert (c["chunk_grid"], c["chunk_min_planes"], c["even_tiled"], c["even_patch"]) == (1024, 4, 4, 2)
    assert (c["tiled_tile"], c["patch_tile"], c["fuse_depths"], c["max_frames"]) == ((32, 16), (32, 8), (32, 48, 64), 8)
    assert cp.second_pass_shape() == (2, 1025, 1024)


def test_instantiations_named_at_the_launch_sites_and_the_unreachable_list_are_pinned():
    inst = cp.instantiations()
    assert len(inst) == 53
    march = [i for i in inst if i.startswith("cv_sad_march_kernel")]
    assert sorted(march) == sorted([f"cv_sad_march_kernel<{dp},{pixd},{kfs},{fd},0>" for dp, pixd, kfs in ((1, 0, 1), (2, 1, 1), (2, 0, 1), (2, 1, 0), (2, 0, 0))
                                    for fd in (0, 1)] + ["cv_sad_march_kernel<1,0,1,1,1>", "cv_sad_march_kernel<2,0,1,1,1>"])
    assert sum(i.startswith("cv_sad_kernel<32,16,") for i in inst) == 16 and sum(i.startswith("cv_sad_patch_kernel<") for i in inst) == 16
    assert sum(i.startswith("cv_fuse_reg_kernel<") for i in inst) == 6 and sum(i.startswith("cv_fuse_kernel<") for i in inst) == 2
    # run by NO test: the FD = false halves of the exact marching kernels (5 of 10), nothing else
    assert sorted(cp.UNREACHABLE) == sorted(i for i in march if re.fullmatch(r"cv_sad_march_kernel<\d,\d,\d,0,0>", i))
    assert set(cp.UNREACHABLE) <= set(inst)


def test_every_reachable_instantiation_is_run_by_a_case(hip_lib):
    print("\n" + cp.table())
    run = set()
    for k in cp.CASES:
        run |= set(cp.launched(_query_case(hip_lib, k)))
    run.discard(None)
    inst = set(cp.instantiations())
    assert run <= inst, sorted(run - inst)
    assert inst - run == set(cp.UNREACHABLE), (sorted(inst - run - set(cp.UNREACHABLE)), sorted(set(cp.UNREACHABLE) & run))


def test_every_case_sits_on_the_path_it_names(hip_lib):
    for k in cp.CASES:
        assert cp.path_of(k) == (k.sad, k.fuse), (k.name, cp.path_of(k))
        L = _query_case(hip_lib, k)
        assert L["status"] == 0 and cp.launched(L)[:2] == (k.sad, k.fuse), (k.name, cp.launched(L))
        assert cp.device_bytes(k) <= cp.MAX_DEVICE_BYTES, (k.name, cp.device_bytes(k))
        if k.oracle:            # the caps of the oracle leg (1e-4 of the entries / of the pixels) allow at least one whole entry / pixel
            assert k.b * k.h * k.w >= 10000, k.name
    small = [k for k in cp.CASES if k.b * k.h * k.w <= 48 * 80 * 3]
    assert len(small) * 2 > len(cp.CASES)


def test_every_branch_inside_a_path_key_has_a_case(hip_lib):
    rules = {k.name: _query_case(hip_lib, k) for k in cp.CASES}
    for name, pred in cp.SUBPATHS.items():
        have = [k.name for k in cp.CASES if pred(k, rules[k.name])]
        assert have, name
    # the numbers the row-loop cases were designed around: TY 8 -> 12 rows per full segment, H 9 / 10 / 11 -> last segments of 5 / 6 / 7
    for name, rows in (("relaxed_dp1_h9_rows13", [12, 5]), ("relaxed_dp1_h10_rows14", [12, 6]), ("relaxed_dp1_h11_rows7", [12, 7]),
                       ("dp2_pixd_kfs_odd_d_h9", [12, 5])):
        assert cp.segment_rows(rules[name], cp.BY_NAME[name].h) == rows, (name, cp.segment_rows(rules[name], cp.BY_NAME[name].h))
    # every tiled / patch MODE x OPT, and P 1 / P 7 at OPT 0 and 3, has an oracle case
    for fam, n in (("cv_sad_kernel", 16), ("cv_sad_patch_kernel", 16)):
        assert len({k.sad for k in cp.CASES if k.oracle and k.sad.startswith(fam + "<")}) == n
    assert {(k.patch, k.sad[-2]) for k in cp.CASES if k.oracle and k.patch in (1, 7)} == {(1, "0"), (1, "3"), (7, "0"), (7, "3")}
    # one marching anchor per reachable instantiation
    anchors = {k.sad for k in cp.CASES if k.oracle and k.sad.startswith("cv_sad_march")}
    assert anchors == {i for i in cp.instantiations() if i.startswith("cv_sad_march")} - set(cp.UNREACHABLE)


def _argument_sets():
    """The cases' own arguments and 400 seeded pseudo-random sets (sizes from a small pool: every new divisor costs the library one exhaustive
    check), valid and refused ones."""
    rng = random.Random(20)
    sizes = [5, 6, 7, 8, 9, 11, 17, 33, 60, 61, 64, 120, 121, 128, 181, 256, 512, 1024]
    out = []
    for i in range(400):
        a = dict(F=rng.choice([1, 1, 2, 2, 3, 4, 8]), B=rng.choice([1, 1, 2, 3, 4, 7]), D=rng.choice([2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 20, 24, 32, 33, 48, 63, 64, 96]),
                 H=rng.choice(sizes), W=rng.choice(sizes), use_ssim=rng.choice([0, 1, 1, 1, 1, 2, 3]), pixd=rng.random() < 0.3,
                 mult_mask=rng.random() < 0.8, patch=rng.choice([1, 3, 3, 3, 3, 5, 7]), tiled=rng.random() < 0.15, b8=rng.random() < 0.1,
                 relaxed=rng.random() < 0.25, lean=rng.random() < 0.1)
        if i % 4 == 0:          # one argument out of range (what a refusal returns depends on the ORDER of the checks: two in some sets)
            for _ in range(rng.choice([1, 1, 2])):
                key, bad = rng.choice([("F", 0), ("F", 9), ("B", 0), ("D", 1), ("D", 0), ("H", 4), ("W", 3), ("use_ssim", -1), ("use_ssim", 4), ("patch", 0),
                                       ("patch", 2), ("patch", 9), ("b8", True), ("mult_mask", False)])
                a[key] = bad
        out.append(a)
    return out


def test_the_restated_rule_equals_the_library_query_field_by_field(hip_lib):
    exact = lambda d: hip_lib.mr_exact_const_division(float(d))
    for k in cp.CASES:
        want, got = cp.rule_of(k, exact), _query_case(hip_lib, k)
        assert want == got, (k.name, {f: (want[f], got[f]) for f in cp.FIELDS if want[f] != got[f]})
    seen = {"refused": 0, 1: 0, 2: 0, 3: 0}
    for a in _argument_sets():
        kw = {k: v for k, v in a.items() if k not in "FBDHW"}
        want = cp.rule(a["F"], a["B"], a["D"], a["H"], a["W"], exact_division=exact, **kw)
        got = cp.query(hip_lib, a["F"], a["B"], a["D"], a["H"], a["W"], **kw)
        assert want == got, (a, {f: (want[f], got[f]) for f in cp.FIELDS if want[f] != got[f]})
        seen["refused" if got["status"] else got["family"]] += 1
        if got["status"]:
            assert all(v in (0, [0, 0], [0, 0, 0]) for f, v in got.items() if f != "status")
    assert min(seen.values()) >= 20, seen
    # the shape the comment above march_geometry() quotes: 2016 waves at two planes per wave -> one plane per wave, TY 37
    c2 = cp.query(hip_lib, 2, 1, 32, 256, 512)
    assert (c2["dp"], c2["ty"], c2["strips"] * c2["ysegs"] * 2 * c2["npairs"]) == (1, 37, 4032)
    assert hip_lib.mr_cost_volume_launch_query(2, 1, 32, 256, 512, 1, 0, 1, 3, 0, 0, 0, 0, None) == cp.constants()["err_bad_argument"]


def _baseline_sizes():
    text = open(cp.ROOT + "/BASELINE.md").read()
    return sorted({(int(h), int(w)) for h, w in re.findall(r"\b(\d{2,4})\s*[x×]\s*(\d{2,4})\b", text) if 5 <= int(h) <= 4096 and 5 <= int(w) <= 4096})


def test_no_size_in_use_reaches_the_fd_false_instantiations(hip_lib):
    """The five FD = false marching kernels are run by no test: every W - 1 and H - 1 of every case and of the sizes BASELINE.md names passes
    mr_exact_const_division, so does every launch anyone makes."""
    sizes = _baseline_sizes()
    assert (256, 512) in sizes
    divisors = {v - 1 for k in cp.CASES for v in (k.h, k.w)} | {v - 1 for hw in sizes for v in hw}
    assert all(hip_lib.mr_exact_const_division(float(d)) == 1 for d in sorted(divisors)), \
        [d for d in sorted(divisors) if hip_lib.mr_exact_const_division(float(d)) != 1]
    for k in cp.CASES:
        L = _query_case(hip_lib, k)
        assert L["family"] != 1 or L["fd"] == 1


@pytest.mark.parametrize("name", [k.name for k in cp.CASES if k.oracle or (k.h, k.w) in ((5, 5), (9, 9)) or k.f == cp.constants()["max_frames"] and k.b * k.h * k.w < 4000])
def test_cpu_references_run(name):
    """Every oracle case's CPU reference, and the operands of the extreme cases (5 x 5, MR_MAX_FRAMES frames), run here: finite, the right
    shapes, neither all valid nor (beyond the minimal images) all invalid."""
    k = cp.BY_NAME[name]
    batch, pix = cp.operands(k)
    cv, sf = cp.oracle_of(k, batch, pix)
    assert cv.shape == (k.b, k.d, k.h, k.w) and len(sf) == k.f and all(s.shape == cv.shape for s in sf)
    assert bool(torch.isfinite(cv).all()) and all(bool(torch.isfinite(s).all()) for s in sf)
    if k.oracle:
        valid = float((cv != 0).any(1).float().mean())
        assert 0.2 < valid < 1.0, valid
    b1, p1 = cp.select_sample(batch, pix, k.b - 1)
    assert b1["keyframe"].shape[0] == 1 and len(cp.select_frame(b1, k.f - 1)["frames"]) == 1
