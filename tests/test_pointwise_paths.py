"""Host side (no GPU): the launch paths of the kernels around the convolutions (tests/pointwise_paths.py) that
tests/test_gpu_pointwise_paths.py runs - the constants the rules rest on parse and are pinned, every declared path has a case, every case
sits on the path it names, and every reference of the GPU file runs here on the CPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import pointwise_paths as pp
from oracle import monorec_oracle as orc


def test_constants_parse_and_are_pinned():
    """Read from csrc/eltwise.hip, csrc/heads.hip, csrc/pointcloud.hip, csrc/cost_volume.hip and include/monorec_hip.h.  A change there moves
    the derived cases (or fails test_every_case_sits_on_the_path_it_names) and shows up here as a diff."""
    c = pp.constants()
    assert (c["wg"], c["grid_cap"], c["quad_min"], c["vec2_above"]) == (256, 2048, 16384, 131072)
    assert (c["sm_th"], c["sm_tw"], c["static_mask_lds"]) == (16, 64, 64 * 1024)
    assert (c["max_frames"], c["max_gather"], c["max_heads"]) == (8, 18, 4)
    assert c["fuse_depths"] == (32, 48, 64)
    assert (c["err_bad_argument"], c["err_unsupported"], c["err_lds_budget"]) == (-1, -2, -3)
    assert pp.pass_items() == 524288


def test_every_declared_path_has_a_case():
    print("\n" + pp.table())
    assert set(c.entry for c in pp.CASES) == set(pp.PATHS)
    for entry, paths in pp.PATHS.items():
        assert len(set(paths)) == len(paths)
        have = {c.path for c in pp.cases_of(entry)}
        assert have == set(paths), (entry, sorted(set(paths) - have), sorted(have - set(paths)))
    names = [(c.entry, c.name) for c in pp.CASES]
    assert len(set(names)) == len(names)


def test_every_case_sits_on_the_path_it_names():
    for case in pp.CASES:
        assert pp.path_of(case) == case.path, (case.entry, case.name, pp.path_of(case))


def test_derived_shapes_match_the_cross_checks():
    """The numbers the cases were designed around, at the present constants."""
    by = {(c.entry, c.name): c for c in pp.CASES}
    assert pp.work_items(by["maxpool3x3s2", "second_pass_511x459"]) == 529920 and by["maxpool3x3s2", "second_pass_511x459"].args["h"] == 511
    assert by["maxpool3x3s2", "odd_17x23"].args == dict(planes=15, h=17, w=23)
    sp = by["pool2x2_framemax", "second_pass_514x1640"]
    assert (sp.args["h"], sp.args["w"], sp.args["frames"], pp.work_items(sp)) == (514, 1640, 2, 526850)
    assert by["max_over_frames", "second_pass_f3"].args["count"] == 4 * (524288 + 3)
    wrap = by["apply_mask", "wrap_in_place"]
    assert (wrap.args["batch"], wrap.args["depths"], wrap.args["plane"]) == (2, 5, 4 * 52431)
    v2 = by["mask_classifier", "vec2_c19_d20"]
    assert (v2.args["batch"], v2.args["channels"], v2.args["hw"], v2.args["depths"]) == (3, 19, (210, 212), 20)
    assert pp.rule_classifier(3, 210 * 212) == (2, 22260, 66780, 261) and 66780 % 256 != 0
    assert by["mask_classifier", "at_threshold"].args["plane"] == 131072 and by["mask_classifier", "threshold_plus_2"].args["plane"] == 131074
    assert by["depth_heads", "quad_c1"].args["heads"] == [(1, 1, 128, 128)]
    assert by["depth_heads", "quad_pixel_quad_pixel"].args["heads"] == [(1, 3, 128, 128), (1, 5, 7, 9), (1, 2, 128, 132), (1, 4, 3, 5)]
    assert pp.largest_mask_fill() == 190 and by["static_mask", "fill_beyond_lds"].args["mask_fill"] == 192
    assert pp.rule_static_mask(190) == (0, 65508) and pp.rule_static_mask(192)[0] == -3 and pp.rule_static_mask(3)[0] == -1
    assert 45 * 70 == 12 * 256 + 78


def test_classifier_threshold_cases():
    """VEC = 2 strictly above the threshold: one case exactly at it (VEC 1), one at threshold + 2 (VEC 2); every vec2 case is above."""
    thr = pp.constants()["vec2_above"]
    for case in pp.cases_of("mask_classifier"):
        a = case.args
        above = a["batch"] * a["plane"] > thr
        assert case.path.startswith("vec2" if above else "vec1") and a["plane"] % 2 == 0
        assert a["hw"][0] * a["hw"][1] == a["plane"]
    sizes = sorted(c.args["batch"] * c.args["plane"] for c in pp.cases_of("mask_classifier"))
    assert thr in sizes and thr + 2 in sizes
    for vec in (1, 2):      # each instantiation meets a thread count that is no multiple of the workgroup: `i >= totalv` is true somewhere
        assert any(pp.rule_classifier(c.args["batch"], c.args["plane"])[2] % 256 for c in pp.cases_of("mask_classifier") if c.path.startswith(f"vec{vec}"))


def test_grid_stride_cases_lie_strictly_between_one_and_two_passes():
    seen = set()
    for case in pp.CASES:
        if case.entry not in pp.GRID_STRIDE_ENTRIES or not case.path.startswith(("second_pass", "wrap")):
            continue
        items = pp.work_items(case)
        blocks, passes = pp.rule_grid(items)
        assert blocks == pp.constants()["grid_cap"] and passes == 2 and pp.pass_items() < items < 2 * pp.pass_items(), (case.entry, case.name, items)
        if case.path != "second_pass_whole_blocks":            # (the one case that is a whole number of workgroups on purpose)
            assert items % pp.constants()["wg"] != 0, (case.entry, case.name, items)
        seen.add(case.entry)
    assert seen == set(pp.GRID_STRIDE_ENTRIES)
    # every other case of these entries stays within one pass
    for case in pp.CASES:
        if case.entry in pp.GRID_STRIDE_ENTRIES and not case.path.startswith(("second_pass", "wrap")):
            assert pp.rule_grid(pp.work_items(case))[1] == 1


def test_apply_mask_wrap_meets_both_samples_and_every_depth_on_each_side():
    case = next(c for c in pp.cases_of("apply_mask") if c.path == "wrap-in_place")
    a = case.args
    plane4, total = a["plane"] // 4, pp.work_items(case)
    first = {(i // (plane4 * a["depths"]), (i // plane4) % a["depths"]) for i in range(0, pp.pass_items(), plane4)} | {((pp.pass_items() - 1) // (plane4 * a["depths"]),
                                                                                                                 ((pp.pass_items() - 1) // plane4) % a["depths"])}
    assert first == {(b, d) for b in range(a["batch"]) for d in range(a["depths"])}
    # a wrapping thread: item i in the first pass, i + one pass in the second - another plane offset, another sample
    i = total - pp.pass_items() - 1
    assert i // (plane4 * a["depths"]) == 0 and (i + pp.pass_items()) // (plane4 * a["depths"]) == a["batch"] - 1
    assert i % plane4 != (i + pp.pass_items()) % plane4


def test_no_case_allocates_more_than_the_device_budget():
    worst = max(pp.CASES, key=pp.device_bytes)
    print(f"largest case: {worst.entry}/{worst.name}, {pp.device_bytes(worst) / 1e6:.1f} MB")
    for case in pp.CASES:
        assert 0 < pp.device_bytes(case) <= pp.MAX_DEVICE_BYTES, (case.entry, case.name, pp.device_bytes(case))


def test_depth_head_cases_fit_the_32_bit_descriptor_and_select_their_modes():
    for case in pp.cases_of("depth_heads"):
        for b, c, h, w in case.args["heads"]:
            assert b * c * h * w * 4 < 2 ** 31
    quad_c1 = pp.cases_of("depth_heads")[0]
    assert pp.rule_head(*quad_c1.args["heads"][0]) == (True, 64)          # (C + 3) >> 2 = 1 channel per wave: waves 1..3 have none
    firsts, blocks = [], 0
    for s in pp.cases_of("depth_heads")[1].args["heads"]:
        firsts.append(blocks)
        blocks += pp.rule_head(*s)[1]
    assert firsts == [0, 64, 68, 134] and blocks == 135


# ---- the references of the GPU file, run on the CPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pp.cases_of("mask_classifier"), ids=pp.case_ids("mask_classifier"))
def test_classifier_fp32_and_fp64_references_agree_five_times_better_than_the_tolerance(case):
    x, wt, bias, _ = pp.classifier_operands(case)
    r64 = pp.classifier_mask_reference(x, wt, bias)
    r32 = pp.classifier_mask_reference(x, wt, bias, torch.float32)
    err = float((r32.double() - r64).abs().max())
    print(f"{case.name}: fp32 vs fp64 reference {err:.2e}")
    assert not torch.isnan(r64).any() and err <= pp.MASK_TOL / 5


@pytest.mark.parametrize("case", pp.cases_of("depth_heads"), ids=pp.case_ids("depth_heads"))
def test_head_fp32_and_fp64_references_agree_five_times_better_than_the_tolerance(case):
    for x, wt, bias in pp.head_operands(case):
        r64, r32 = pp.head_reference(x, wt, bias), pp.head_reference(x, wt, bias, torch.float32)
        err = float((r32.double() - r64).abs().max())
        print(f"{case.name} {tuple(x.shape)}: fp32 vs fp64 reference {err:.2e}")
        assert not torch.isnan(r64).any() and err <= pp.HEAD_TOL / 5
        assert float(r64.min()) >= pp.HEAD_LO and float(r64.max()) <= pp.HEAD_HI


@pytest.mark.parametrize("case", [c for c in pp.cases_of("nonzero_mean") if c.args["count"] == 4] + [pp.Case("nonzero_mean", "count4000_f4", None, dict(frames=4, count=4000))],
                         ids=lambda c: c.name)
def test_nonzero_mean_references(case):
    """The bit-exact reference (the kernel's order) stays within the derived bound of the fp64 evaluation, has no NaN, and the data holds
    every class of position the issue names."""
    x = pp.nonzero_mean_input(case.args["frames"], case.args["count"], pp.gen(case) if case.path else torch.Generator().manual_seed(3))
    exact = pp.nonzero_mean_exact(x)
    val, bound = pp.nonzero_mean_bound(x)
    assert not torch.isnan(exact).any()
    fin = torch.isfinite(val)
    assert torch.equal(exact[~fin].double(), val[~fin])
    assert bool(((exact.double() - val).abs()[fin] <= bound[fin]).all())
    assert bool((x == 0).all(0).any()) and bool(torch.isinf(x).any())
    if case.args["frames"] > 1:
        assert bool((torch.signbit(x) & (x == 0)).any()) and bool(((x == 0).any(0) & (x != 0).any(0)).any())
        assert float((exact.double() - val).abs()[fin].max()) > 0 or case.args["count"] == 4       # (the bound is not vacuous: roundings do occur)
    # an independent statement of the definition (monorec_model.py:448-449)
    want = x.sum(0) / (x != 0).sum(0).clamp_min(1)
    assert bool(((exact - want).abs()[fin] <= bound[fin].float() * 2 + 1e-30).all())


def test_pooling_references_on_the_small_cases():
    """F.max_pool2d / torch.max are the references of the max kernels; on inputs without NaN they equal a plain window loop."""
    for case in pp.cases_of("maxpool3x3s2"):
        a = case.args
        if a["planes"] * a["h"] * a["w"] > 10000:
            continue
        x = pp.max_input((1, a["planes"], a["h"], a["w"]), pp.gen(case))
        ref = F.max_pool2d(x, 3, 2, 1)
        assert ref.shape[2:] == (pp.pool3_out(a["h"]), pp.pool3_out(a["w"])) and not torch.isnan(ref).any()
        xp = F.pad(x, (1, 1, 1, 1), value=-math.inf)
        for oy in range(ref.shape[2]):
            for ox in range(ref.shape[3]):
                assert torch.equal(ref[0, :, oy, ox], xp[0, :, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].amax((1, 2)))
    for case in pp.cases_of("pool2x2_framemax"):
        a = case.args
        if a["h"] > 100:
            continue
        x = pp.max_input((a["frames"], a["planes"], a["h"], a["w"]), pp.gen(case))
        ref = F.max_pool2d(x, 2)
        assert torch.equal(ref, torch.maximum(torch.maximum(x[..., 0::2, 0::2], x[..., 0::2, 1::2]), torch.maximum(x[..., 1::2, 0::2], x[..., 1::2, 1::2])))
        assert not torch.isnan(x.max(0)[0]).any()


def test_bf16_edge_table_against_torch():
    """The bit patterns of the layout-conversion cases: torch's fp32 -> bf16 conversion is round to nearest even, overflows to inf, keeps
    denormals and keeps a NaN a NaN."""
    e = pp.edge_tensor()
    assert [int(v) & 0xffffffff for v in e.view(torch.int32)] == [b for _, b, _ in pp.BF16_EDGES]
    got = pp.bf16_bits(e)
    for (name, bits, want), g in zip(pp.BF16_EDGES, got.tolist()):
        if want is None:
            assert math.isnan(pp.f32_from_bits(bits)) and bool(pp.is_nan_bf16_bits(torch.tensor(g))), name
        else:
            assert g == want, (name, hex(bits), hex(g), hex(want))
    classes = {n for n, _, _ in pp.BF16_EDGES}
    assert {"tie_to_even_down", "tie_to_even_up", "overflow_to_inf", "denormal_tie_up", "signalling_nan", "minus_zero"} <= classes
    # the data of the cases holds every edge in every channel, and is NOT bf16-representable elsewhere (rounding is exercised)
    for case in pp.cases_of("f32_to_b8"):
        x = pp.conversion_input(case)
        n = len(pp.BF16_EDGES)
        for ch in range(case.args["c"]):
            assert torch.equal(x[0, ch, ch:ch + n, 0].view(torch.int32), e.view(torch.int32))
        fin = torch.isfinite(x)
        assert float((pp.bf(x)[fin] != x[fin]).float().mean()) > 0.9
        assert (case.args["n"] * ((case.args["c"] + 7) // 8) * case.args["hw"]) % 256 != 0
    # the B8 packing helpers are each other's inverse
    x = pp.bf(torch.randn(2, 11, 3, 5, generator=torch.Generator().manual_seed(1)))
    assert torch.equal(pp.from_b8(pp.to_b8(x), 11), x) and torch.equal(pp.b8_bits(pp.to_b8(x), 11), pp.bf16_bits(x))


def test_static_mask_reference_and_inputs():
    """orc.static_mask (create_pointcloud.py:76-77) on the inputs of the cases: a value exactly at the threshold counts as moving, the largest
    fp32 below it does not; the widest box on the 20 x 70 image is all-or-nothing per sample, on the 20 x 260 image it is not."""
    for case in pp.cases_of("static_mask"):
        fill = case.args["mask_fill"]
        if pp.rule_static_mask(fill)[0] != 0:
            continue
        x, thr = pp.static_mask_input(case)
        ref = orc.static_mask(x, fill, thr)
        b, h, w = case.args["shape"]
        assert ref.shape == (b, 1, h, w) and set(ref.unique().tolist()) <= {0.0, 1.0}
        assert float(x[b - 1, 0, 0, 0]) == thr and ref[b - 1, 0, 0, 0] == 0              # at the threshold: moving
        if fill == 0:
            assert torch.equal(ref, (x < thr).float()) and ref[b - 1, 0, h - 1, w - 1] == 1      # just below: static
            assert int((x == thr).sum()) >= 1
        if case.name == "largest_fill_20x70":
            assert ref[0].min() == 1 and ref[1].max() == 0 and ref[2].max() == 0
        else:
            assert 0 < float(ref.mean()) < 1, case.name
        # independent statement: the dilation as a max-pool of the moving flags
        r = fill // 2
        dil = F.max_pool2d((x >= thr).float(), 2 * r + 1, 1, r) if r else (x >= thr).float()
        assert torch.equal(ref, 1 - dil)


def test_cost_volume_finalise_matches_a_plain_loop():
    """The expression the lean test applies to the un-finalised buffers: (1 - 2 |raw|) * vm, vm = inside the border of width 2 and no sign bit
    set among the pixel's raw values (-0.0 counts)."""
    g = torch.Generator().manual_seed(11)
    raw = torch.rand(2, 6, 9, 11, generator=g)
    raw[0, 5, 4, 4] *= -1
    raw[1, 2, 3, 6] = -0.0
    raw[1, 0, 0, 0] *= -1
    got = pp.cost_volume_finalise(raw)
    for b in range(2):
        for y in range(9):
            for x in range(11):
                ok = 2 <= y < 7 and 2 <= x < 9 and not any(math.copysign(1.0, float(v)) < 0 for v in raw[b, :, y, x])
                want = (1.0 - raw[b, :, y, x].abs() * 2.0) * (1.0 if ok else 0.0)
                assert torch.equal(got[b, :, y, x] == want, torch.ones(6, dtype=torch.bool))
    assert bool((got[0, :, 4, 4] == 0).all()) and bool((got[1, :, 3, 6] == 0).all()) and bool((got[0, :, 4, 5] != 0).any())
    for case in pp.cases_of("cost_volume_b8"):
        assert pp.rule_cost_volume_b8(case.args["depths"]) == (-2 if case.path == "unsupported" else 0)
