"""Host side (no GPU): the launch paths of the input and evaluation kernels (tests/data_paths.py) that tests/test_gpu_data_paths.py runs - the
constants the rules rest on parse and are pinned, every declared path has a case, every case sits on the path it names, the derived shapes sit
where they claim, the numpy restatement of the radix select equals np.sort on every select case, the refusals are answered without a launch,
and every reference of the GPU file runs here on the CPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import data_paths as dp
from monorec_amd import metrics
from oracle import input_oracle as io_ref
from oracle import monorec_oracle as orc


def test_constants_parse_and_are_pinned():
    """Read from csrc/preprocess.hip, csrc/select.hip, csrc/eltwise.hip and include/monorec_hip.h.  A change there moves the derived cases (or
    fails test_every_case_sits_on_the_path_it_names) and shows up here as a diff."""
    c = dp.constants()
    assert (c["pt_h"], c["pt_w"], c["pre_threads"]) == (16, 64, 1024)
    assert (c["wg"], c["grid_cap"], dp.pass_items()) == (256, 2048, 524288)
    assert (c["lds_limit"], c["lut_bytes"]) == (64 * 1024, 1024)
    assert (c["k_threads"], c["select_step"], c["k_bins"], c["metric_wg"]) == (1024, 4096, 2048, 1024)
    assert dp._digits() == ((21, 11), (10, 11), (0, 10))
    assert (c["max_stages"], c["metric_dense"]) == (16, 0x100) == (metrics.MAX_STAGES, metrics._DENSE)
    assert (c["err_bad_argument"], c["err_unsupported"], c["err_lds_budget"]) == (-1, -2, -3)


def test_every_declared_path_has_a_case_or_a_reason():
    print("\n" + dp.table())
    assert set(c.entry for c in dp.CASES) == set(dp.PATHS)
    for entry, paths in dp.PATHS.items():
        assert len(set(paths)) == len(paths)
        have = {c.path for c in dp.cases_of(entry)}
        unreached = {p for (e, p) in dp.UNREACHED if e == entry}
        assert unreached <= set(paths) and not (unreached & have)
        assert have == set(paths) - unreached, (entry, sorted(set(paths) - unreached - have), sorted(have - set(paths)))
    names = [(c.entry, c.name) for c in dp.CASES]
    assert len(set(names)) == len(names)
    assert set(dp.UNREACHED) == {("unpack", "second_pass")}             # the one declared path that is not run: its reason is in the census
    # the second pass of the unpack really is out of reach of the budget
    chunks = dp.pass_items() + 1
    assert dp.rule_grid(chunks)[1] == 2 and 12 * 16 * chunks > dp.MAX_DEVICE_BYTES


def test_every_case_sits_on_the_path_it_names():
    for case in dp.CASES:
        assert dp.path_of(case) == case.path, (case.entry, case.name, dp.path_of(case))


def test_no_case_allocates_more_than_the_device_budget():
    worst = max(dp.CASES, key=dp.device_bytes)
    print(f"largest case: {worst.entry}/{worst.name}, {dp.device_bytes(worst) / 1e6:.1f} MB")
    for case in dp.CASES:
        if not case.path.startswith("refuse"):
            assert 0 < dp.device_bytes(case) <= dp.MAX_DEVICE_BYTES, (case.entry, case.name, dp.device_bytes(case))


# ---- the resize ------------------------------------------------------------------------------------------------------------------------------------
def test_lds_edge_pairs_straddle_the_limit():
    c = dp.constants()
    by = {k.name: k for k in dp.cases_of("resize")}
    want = {("f32", 1): (1024, 65536), ("f32", 3): (341, 65472), ("lut", 1): (1008, 65536)}
    for (kernel, ch), (rows, lds) in want.items():
        ok, no = by[f"lds_accept-{kernel}-c{ch}"], by[f"lds_refuse-{kernel}-c{ch}"]
        assert ok.args["src"][0] == rows == dp.largest_tile_rows(kernel, ch) and no.args["src"][0] == rows + 1
        r_ok = dp.rule_resize(kernel, ch, rows, ok.args["src"][1], *ok.args["out"])
        r_no = dp.rule_resize(kernel, ch, rows + 1, no.args["src"][1], *no.args["out"])
        assert (r_ok["code"], r_ok["lds"], r_ok["max_tile_rows"]) == (0, lds, rows) and lds <= c["lds_limit"]
        assert r_no["code"] == c["err_lds_budget"] and r_no["lds"] > c["lds_limit"] and r_no["max_tile_rows"] == rows + 1


def test_resize_geometries_are_what_the_cases_claim():
    by = {k.name: k for k in dp.cases_of("resize")}
    r = dp.rule_resize("f32", 3, 40, 150, 17, 65)
    assert (r["tiles_x"], r["tiles_y"], r["last_cols"], r["last_rows"]) == (2, 2, 1, 1) and r["h_passes"] == 3 and r["v_passes"] == 1
    looping = sorted({k.name.split("-")[0] for k in dp.cases_of("resize", run_only=True)
                      if dp.rule_resize(k.args["kernel"], k.args["channels"], dp.resize_box(k)[3] - dp.resize_box(k)[1], dp.resize_box(k)[2] - dp.resize_box(k)[0],
                                        *k.args["out"])["h_passes"] > 1})
    assert looping == ["lds_accept", "tiles2x2_ragged"]                # the cases whose horizontal pass loops more than once: rows * cols > 1024
    up = by["upscale_one_tile-f32-c1"].args
    _, hb, _ = io_ref.resample_coeffs(up["src"][1], 0, up["src"][1], up["out"][1])
    assert hb[0, 0] == 0 and hb[0, 1] < 3 and hb[-1, 0] + hb[-1, 1] == up["src"][1] and hb[-1, 1] < 3     # bounds clipped at both edges
    odd = by["odd_crop_padded_rows-f32"].args
    assert odd["box"][0] & 1 and odd["box"][1] & 1 and odd["row_pad"] == 5 and odd["channels"] == 3
    assert dp.resize_box(by["one_pixel_wide_crop-u8-c3"])[2] - dp.resize_box(by["one_pixel_wide_crop-u8-c3"])[0] == 1
    for k in dp.cases_of("resize"):         # (where Pillow >= 11 and the reference's Pillow part: a crop more than 100 times as tall as wide)
        x0, y0, x1, y1 = dp.resize_box(k)
        assert y1 - y0 <= 100 * (x1 - x0), k.name
    img = dp.resize_image(by["checker-f32-c3"])
    assert set(np.unique(img)) == {0, 255} and img[0, 0, 0] != img[0, 1, 0] and img[0, 0, 0] != img[0, 0, 1]


@pytest.mark.parametrize("case", dp.cases_of("resize", run_only=True), ids=dp.case_ids("resize", run_only=True))
def test_resize_references_agree(hip_lib, case):
    """The integer restatement equals Pillow on every case, and the host tables of the library equal the restatement's."""
    from monorec_amd import input_pipeline
    img = dp.resize_image(case)
    ref = dp.resize_reference_u8(case, img)
    pil = dp.resize_reference_pillow(case, img)
    assert pil is None or np.array_equal(ref, pil)
    f = dp.resize_reference_f32(case, img)
    assert f.dtype == torch.float32 and tuple(f.shape) == (3, *case.args["out"]) and not torch.isnan(f).any()
    if case.args["fill"] in ("all_0", "all_255"):
        assert ref.min() == ref.max() == (0 if case.args["fill"] == "all_0" else 255)
    x0, y0, x1, y1 = dp.resize_box(case)
    for size, out in ((x1 - x0, case.args["out"][1]), (y1 - y0, case.args["out"][0])):
        ks, b, k = input_pipeline._axis_tables(hip_lib, size, out)
        ks2, b2, k2 = io_ref.resample_coeffs(size, 0, size, out)
        assert ks == ks2 and np.array_equal(b, b2) and np.array_equal(k, k2)


def _resize_call(lib, case, dst):
    """The C entry of a resize case with HOST pointers: only for arguments the entry refuses before it launches anything."""
    from monorec_amd import input_pipeline
    a = case.args
    h, w = a["src"]
    src = np.zeros((h, w * a["channels"]), np.uint8)
    hks, hb, hk = input_pipeline._axis_tables(lib, w, a["out"][1])
    vks, vb, vk = input_pipeline._axis_tables(lib, h, a["out"][0])
    args = [src.ctypes.data, h, w, a["channels"], w * a["channels"], (ctypes.c_int32 * 4)(0, 0, w, h), a["out"][0], a["out"][1],
            hb.ctypes.data, hk.ctypes.data, hks, vb.ctypes.data, vk.ctypes.data, vks, max(dp.tile_rows(vb, a["out"][0]))]
    if a["kernel"] == "lut":
        return lib.mr_preprocess_image_u8_lut_f32(*args, dp.response_table().ctypes.data, dst.ctypes.data, None)
    return lib.mr_preprocess_image_u8_f32(*args, dst.ctypes.data, None)


def test_lds_refusals_are_answered_on_the_host(hip_lib):
    refused = [k for k in dp.cases_of("resize") if k.path.startswith("lds_refuse")]
    assert len(refused) == 3
    for case in refused:
        dst = np.full(3 * case.args["out"][0] * case.args["out"][1], 7.0, np.float32)
        assert _resize_call(hip_lib, case, dst) == dp.constants()["err_lds_budget"], case.name
        assert (dst == 7.0).all()


# ---- lidar / D(V)SO, scatter ------------------------------------------------------------------------------------------------------------------------
def test_target_cases_sit_where_they_claim():
    for entry in ("lidar", "dso"):
        by = {k.name: k for k in dp.cases_of(entry)}
        ty, tx = dp.tie_counts(by["ties_64x96"])
        print(f"{entry}: ties rows {ty}, columns {tx}")
        assert ty > 0 and tx > 0
        for name in ("nobox_37x53", "box_37x53", "upscale_5x7", "every_value"):
            assert dp.tie_counts(by[name]) == (0, 0), name
        col = by["collisions_40x60"]
        png = dp.target_png(col)
        assert (png != 0).all() and png.size == 100 * col.args["out"][0] * col.args["out"][1]
        for name in ("elect2_tiny_grid", "elect2_write2"):
            h, w = by[name].args["src"]
            assert dp.pass_items() < h * w < 2 * dp.pass_items() and dp.rule_grid(h * w) == (2048, 2)
        assert by["elect2_tiny_grid"].args["src"] == (513, 1024) and by["elect2_write2"].args["out"] == (725, 725)
        assert dp.rule_grid(725 * 725) == (2048, 2) and dp.rule_grid(6)[1] == 1
        # the winners of the tiny grid's last row come from the second elect pass
        tiny = by["elect2_tiny_grid"]
        png = dp.target_png(tiny)
        last = np.flatnonzero(png.reshape(-1))[-1]
        assert last >= dp.pass_items() and dp.target_reference(tiny, png)[1, 2] != 0
        ev = dp.target_png(by["every_value"])
        assert np.array_equal(np.sort(ev.reshape(-1)), np.arange(65536)) and int((dp.target_reference(by["every_value"], ev) != 0).sum()) == 65535
        up = by["upscale_5x7"]
        assert int((dp.target_reference(up, dp.target_png(up)) == 0).sum()) > 16 * 24 - 35
    dso = {k.name: k for k in dp.cases_of("dso")}
    for name in ("png_32x64_of_64x128", "png_128x256_of_64x128"):
        hits = dp.edge_hits(dso[name])
        print(f"{name}: coordinates exactly on y0, y1, x0, x1: {hits}")
        assert min(hits) > 0
    assert dso["every_value"].args["focal"] != dso["every_value_focal_2"].args["focal"]


def test_target_refusals_are_answered_on_the_host(hip_lib):
    """As tests/test_capi_and_host.py: the entry returns before it touches the device."""
    c = dp.constants()
    png, owner, dst = np.zeros(4, np.uint16), np.zeros(4, np.int32), np.full(4, 7.0, np.float32)
    seen = set()
    for entry in ("lidar", "dso"):
        for case in [k for k in dp.cases_of(entry) if k.path.startswith("refuse")]:
            a = case.args
            box = None if a["box"] is None else (ctypes.c_int32 * 4)(*a["box"])
            want = dp.rule_target(*a["src"], a["box"], a["orig"] if entry == "dso" else a["src"])
            if entry == "lidar":
                got = hip_lib.mr_lidar_inverse_depth_u16_f32(png.ctypes.data, *a["src"], box, *a["out"], owner.ctypes.data, dst.ctypes.data, None)
            else:
                got = hip_lib.mr_dso_inverse_depth_u16_f32(png.ctypes.data, *a["src"], *a["orig"], a["focal"], box, *a["out"], owner.ctypes.data, dst.ctypes.data, None)
            assert got == want and want != 0, (entry, case.name, got, want)
            seen.add((entry, want))
    assert seen == {(e, code) for e in ("lidar", "dso") for code in (c["err_bad_argument"], c["err_unsupported"])}
    assert (dst == 7.0).all() and not owner.any()


def test_scatter_cases():
    for case in dp.cases_of("scatter"):
        index, value = dp.scatter_operands(case)
        a = case.args
        assert index.size == value.size == a["n"] and int((index.astype(np.int64) >= a["cells"]).sum()) == a["dropped"]
        kept = index[index.astype(np.int64) < a["cells"]]
        assert np.unique(kept).size == kept.size                      # a permutation: no two writes to one cell
        want = dp.scatter_reference(index, value, a["cells"])
        assert int((want != 0).sum()) == a["n"] - a["dropped"]
    big = next(k for k in dp.cases_of("scatter") if k.path == "second_pass_dropped").args
    assert dp.pass_items() < big["n"] < 2 * dp.pass_items() and big["cells"] == big["n"] + 7 and dp.rule_grid(big["n"]) == (2048, 2)


# ---- median select ------------------------------------------------------------------------------------------------------------------------------------
def test_select_restatement_equals_np_sort_on_every_case():
    skipped = []
    for case in dp.cases_of("select"):
        pred, gt = dp.select_operands(case)
        assert pred.shape == gt.shape == (case.args["n"],)
        sel = gt > 0
        m = int(sel.sum())
        assert not (sel & ~(gt > 0)).any() and not sel[np.isnan(gt) | (gt <= 0)].any()
        zeros = pred[sel][pred[sel] == 0]
        assert zeros.size == 0 or np.signbit(zeros).all() or not np.signbit(zeros).any()     # zeros of one sign only
        if m == 0:
            continue
        t = np.sort(gt[sel])
        lo, hi, _ = dp.radix_select(gt[sel])
        assert lo.view(np.uint32) == t[(m - 1) // 2].view(np.uint32) and hi.view(np.uint32) == t[m // 2].view(np.uint32), case.name
        if np.isnan(pred[sel]).any():
            skipped.append(case.name)
            continue
        p = np.sort(pred[sel])
        lo, hi, source = dp.radix_select(pred[sel])
        assert lo.view(np.uint32) == p[(m - 1) // 2].view(np.uint32) and hi.view(np.uint32) == p[m // 2].view(np.uint32), case.name
        assert source == case.path.rsplit("-", 1)[1]
        assert lo.view(np.uint32) == torch.median(torch.from_numpy(pred[sel])).numpy().view(np.uint32)
    assert sorted(skipped) == sorted(k.name for k in dp.cases_of("select") if k.args["kind"] in ("nan_sparse", "nan_dense"))   # the only lo / hi skip


def test_select_restatement_on_random_draws():
    rng = np.random.RandomState(9)
    for _ in range(200):
        m = int(rng.randint(1, 300))
        v = rng.randn(m).astype(np.float32) * np.float32(10.0) ** rng.randint(-40, 39)
        v[rng.rand(m) < 0.2] = rng.choice(v)                            # duplicates
        s = np.sort(v)
        lo, hi, _ = dp.radix_select(v)
        assert lo == s[(m - 1) // 2] and hi == s[m // 2]


def test_select_cases_hold_what_the_issue_names():
    by = {k.name: k for k in dp.cases_of("select")}
    step = dp.constants()["select_step"]
    assert sorted({k.args["n"] for k in dp.cases_of("select")}) == [1, 62, 63, step, step + 1, 3 * step + 5]
    assert {dp.select_features(k)[0] for k in dp.cases_of("select")} >= {0, 1, 2, 3}
    for n in (63, step + 1):
        assert dp.select_features(by[f"n{n}_low10"])[1:] == ("above", 2)        # lo / hi differ only in the low 10 bits,
        assert dp.select_features(by[f"n{n}_mid11"])[1:] == ("above", 1)        # only from the middle digit on,
        assert dp.select_features(by[f"n{n}_top"])[1:] == ("above", 0)          # in the top digit,
        pred, gt = dp.select_operands(by[f"n{n}_sign"])                          # across the sign flip of the key
        lo, hi, _ = dp.radix_select(pred[gt > 0])
        assert (lo, hi) == (-1.0, 1.0)
        pred, gt = dp.select_operands(by[f"n{n}_extremes"])
        sel = pred[gt > 0]
        assert np.isinf(sel).sum() == 2 and (sel == 0).sum() == 1 and (np.abs(sel) == np.float32(3e38)).sum() == 2
        assert ((sel != 0) & (np.abs(sel) < np.float32(1.1754944e-38))).sum() >= 3 and np.isinf(gt).any()
        lo, hi, _ = dp.radix_select(sel)
        assert (lo.view(np.uint32), hi.view(np.uint32)) == (1, 2)               # subnormal medians
    pred, gt = dp.select_operands(by["n63_m2_sign"])
    assert sorted(pred[gt > 0].tolist()) == [-1.0, 1.0]
    assert dp.select_features(by["n62_all_equal_even"]) == (62, "prefix_le", None)
    m, source, digit = dp.select_features(by[f"n{step + 1}_median_duplicates"])
    pred, gt = dp.select_operands(by[f"n{step + 1}_median_duplicates"])
    assert source == "prefix_le" and digit is None and (pred[gt > 0] == np.float32(1.25)).sum() == 2 + m // 8
    # a sparse mask leaves most waves with a partial ballot
    pred, gt = dp.select_operands(by[f"n{step + 1}_sparse_odd"])
    waves = (gt[:step] > 0).reshape(-1, 64).sum(1)
    assert ((waves > 0) & (waves < 64)).mean() > 0.9
    # unselected targets: NaN, negative, -0, +0
    assert np.isnan(gt).any() and (gt < 0).any() and (np.signbit(gt) & (gt == 0)).any() and (~np.signbit(gt) & (gt == 0)).any()


# ---- stage ratios ---------------------------------------------------------------------------------------------------------------------------------------
def test_stage_cases_take_every_branch_and_the_reference_chain_equals_the_recurrence():
    stages = dp.constants()["max_stages"]
    seen = set()
    for case in dp.cases_of("stage"):
        pred, gt = dp.stage_operands(case)
        stats = dp.selection_stats(pred, gt)
        branches = dp.rule_stage(*stats, stages)
        seen |= set(branches)
        chain = dp.median_scaling_chain(torch.from_numpy(pred).view(1, -1), torch.from_numpy(gt).view(1, -1), stages)[0].numpy()
        host = np.array(metrics.stage_ratios_host(*stats, stages), dtype=np.float32)
        assert np.array_equal(np.isnan(chain), np.isnan(host)), case.name
        ok = ~np.isnan(chain)
        assert np.array_equal(chain[ok].view(np.uint32), host[ok].view(np.uint32)), (case.name, chain, host)
        for j, b in enumerate(branches):
            r = chain[j]
            assert {"positive": r > 0 and np.isfinite(r), "negative": r < 0 and np.isfinite(r), "nan": np.isnan(r)}.get(b, (r == 0) if b.startswith("zero") else np.isinf(r)), (case.name, j, b, r)
        zeros = pred[gt > 0][pred[gt > 0] == 0]
        assert zeros.size == 0 or not np.signbit(zeros).any()
    assert seen == set(dp.STAGE_BRANCHES)


# ---- metric sums ----------------------------------------------------------------------------------------------------------------------------------------
def _close(got, want, rtol):
    got, want = float(got), float(want)
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= rtol * max(1.0, abs(want))


@pytest.mark.parametrize("case", dp.cases_of("sparse_sums"), ids=dp.case_ids("sparse_sums"))
def test_sparse_sums_reference_against_the_oracle(case):
    """The fp32-terms / fp64-sum reference gives the oracle's seven metrics: the same NaN pattern, the values within the project's bar."""
    a = case.args
    pred, gt, _ = dp.metric_operands(case)
    assert float(dp.inv_max_distance(80)) == float(np.float32(1 / 80)) and float(dp.inv_max_distance(None)) == 0.0
    sums = dp.sparse_sums_reference(pred, gt, a["roi"], a["max_distance"])
    got = metrics.metrics_from_sums(sums)
    want = orc.sparse_metrics(pred, gt, a["roi"], a["max_distance"])
    for name, g in zip(metrics.SPARSE_METRICS, got):
        assert math.isnan(float(g)) == math.isnan(float(want[name])), (name, float(g), float(want[name]))
        assert _close(g, want[name], 2e-5), (name, float(g), float(want[name]))
    nan = [n for n in metrics.SPARSE_METRICS if math.isnan(float(want[n]))]
    if a["data"] == "nan_valid":        # what the issue reports of the reference: the four error metrics are NaN, the three counts are not
        assert nan == ["abs_rel_sparse_metric", "sq_rel_sparse_metric", "rmse_sparse_metric", "rmse_log_sparse_metric"]
        assert torch.isnan(sums[0, 1:5]).all() and not torch.isnan(sums[1]).any() and not torch.isnan(sums[:, [0, 5, 6, 7]]).any()
    elif a["data"] in ("plain", "nan_masked") or a["max_distance"]:
        assert nan == []
    y0, y1, x0, x1 = a["roi"] if a["roi"] is not None else (0, a["shape"][1], 0, a["shape"][2])
    if a["roi"] is not None:
        assert y0 > 0 and x0 > 0 and y1 < a["shape"][1] and x1 < a["shape"][2]
    valid = gt[:, :, y0:y1, x0:x1] > 0.02
    p = pred[:, :, y0:y1, x0:x1]
    if a["data"] == "clamped":
        assert int(((p < 0) & valid).sum()) >= 10 and int(((p > 0) & (p < 1 / 80) & valid).sum()) >= 10
    if a["data"] == "inf":
        assert int((torch.isinf(p) & valid).sum()) == 6
    if a["data"] == "nan_masked":
        assert int(torch.isnan(p).sum()) == 1 and not (torch.isnan(p) & (gt[:, :, y0:y1, x0:x1] != 0)).any()


def test_stage_sums_reference_reduces_to_the_sparse_reference():
    """Columns 1..7 without scales: the stage layout holds the sparse layout's numbers; scaled cases hold every ratio class."""
    for case in dp.cases_of("stage_sums"):
        a = case.args
        pred, gt, scales = dp.metric_operands(case)
        ref = dp.stage_sums_reference(pred, gt, a["roi"], a["max_distance"], a["columns"], scales)
        assert tuple(ref.shape) == (a["shape"][0], 2 + len(a["columns"]))
        if not a["scaled"] and list(a["columns"][:7]) == list(range(1, 8)):
            sparse = dp.sparse_sums_reference(pred, gt, a["roi"], a["max_distance"])
            same = (ref[:, [0] + list(range(2, 9))] == sparse) | (torch.isnan(sparse) & torch.isnan(ref[:, [0] + list(range(2, 9))]))
            assert bool(same.all()), case.name
        if a["scaled"] and a["shape"][0] == 5:
            s = scales.numpy()
            assert np.isfinite(s[0]).all() and (s[0] > 0).all() and (s[1] < 0).any() and (s[2] == 0).any() and np.isinf(s[3]).any() and np.isnan(s[4]).any()
    cols = {c for k in dp.cases_of("stage_sums") for c in k.args["columns"]}
    assert cols == set(range(1, 8)) | {c | dp.constants()["metric_dense"] for c in range(1, 8)}
    assert {len(k.args["columns"]) for k in dp.cases_of("stage_sums")} >= {1, dp.constants()["max_stages"]}
