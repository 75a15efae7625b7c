"""Host side (no GPU): the census of reduced-multiply convolution launches (tests/reduced_conv_census.py) that
tests/test_gpu_reduced_conv_forms.py runs - what it must contain, its size pinned so that a table or dispatch change shows up as a diff
here, and the exactness certificate of every case."""
import collections
import re

import torch

import reduced_conv_census as census
from monorec_amd import engine

# instantiation keys per family, measured when the census was written
KEY_COUNTS = {"w22": 18, "w44": 5, "w44s": 5, "t22": 6, "f23": 9, "ct": 23, "up": 3}

# non-zero WINOGRAD table keys no census plan launches: none.  (An entry that stops being launched - a renamed layer, a changed signature -
# is named here with the reason, or removed from the table.)
UNREACHED = []

# forms the library carries that no table entry of the census plans selects: they run from census.EXTRA only
UNTABLED_FORMS = {("w22", 2), ("w44w", 5)}


def test_census_is_not_empty_and_its_size_is_pinned(hip_lib):
    cases = census.census()
    assert cases
    assert dict(collections.Counter(k.family for k in cases)) == KEY_COUNTS
    ids = [census.case_id(c) for c in census.all_cases()]
    assert len(set(ids)) == len(ids)                      # the readable ids the GPU file is parametrised with name the cases one to one
    assert all(k.entry == census.ENTRY[k.family] for k in cases)


def test_every_nonzero_table_key_is_launched_by_a_census_plan(hip_lib):
    sigs = {re.sub(r"_[xy]$", "", sig) if launch.stride2 else sig for launch, _, sig, _ in census.launches()}
    nonzero = [k for k, code in engine.WINOGRAD.items() if code]
    assert len(nonzero) >= 250
    missing = sorted(k for k in nonzero if k not in sigs)
    assert missing == sorted(UNREACHED), (sorted(set(missing) - set(UNREACHED)), sorted(set(UNREACHED) - set(missing)))


def test_untabled_forms_and_required_extras_are_in_the_extra_list(hip_lib):
    tabled = {(k.family, k.variant) for k in census.census()}
    extra = {(c.key.family, c.key.variant) for c in census.EXTRA}
    assert not (UNTABLED_FORMS & tabled), "a form became tabled: move it out of UNTABLED_FORMS"
    assert UNTABLED_FORMS <= extra
    keys = [c.key for c in census.EXTRA]
    assert {k.axis for k in keys if k.family == "ct" and (k.m, k.r) == (2, 7)} == {0, 1}                         # F(2,7) on both axes
    families = set(census.ENTRY)
    assert {k.family for k in keys if k.c8} == families                                                          # C % 8 != 0 per family
    assert {c.key.family for c in census.EXTRA if c.name.endswith("below_one_tile")} == families
    for c in census.EXTRA:
        if c.name.endswith("below_one_tile"):
            rows, cols = census.workgroup_tile(c.launch)
            assert c.launch.hw[0] < rows and c.launch.hw[1] < cols
    twelve = {(k.family, k.variant) for c, k in zip(census.EXTRA, keys) if c.launch.cout == 12}
    assert twelve == {("w22", 0), ("w22", 1), ("w22", 2), ("w44", 3), ("w44s", 4), ("w44w", 5), ("t22", 0), ("t22", 1), ("t22", 2)}
    assert all(k.cout_rem == "0b+t/only" for c, k in zip(census.EXTRA, keys) if c.launch.cout == 12)
    # the tables' one key with C % 8 != 0: 32 + 3 channels
    assert [c.launch.srcs_c for c in census.census().values() if c.key.c8] == [(32, 3)]


def test_representatives_keep_their_key_and_everything_but_the_image_size(hip_lib):
    origin = {}
    for launch, name, sig, where in census.launches():
        origin.setdefault((name, where), launch)
    for key, case in census.census().items():
        full, small = origin[(case.name, case.origin)], case.launch
        assert census.launch_key(full) == key == census.launch_key(small)
        assert small == full._replace(hw=small.hw, batch=small.batch), census.key_id(key)           # nothing but image size and batch
        assert small.hw[0] <= full.hw[0] and small.hw[1] <= full.hw[1] and small.batch <= max(2, full.batch)
        assert small.hw[1] % 4 == 0 and (not (key.view or key.split) or small.hw[1] % 8 == 0)
        rows, cols = census.workgroup_tile(small)
        if full.hw[0] > 2 * rows:
            assert small.hw[0] % rows, (census.key_id(key), small.hw)                               # ragged in both directions
        if full.hw[1] > 2 * cols:
            assert small.hw[1] % cols, (census.key_id(key), small.hw)
        assert census.macs(small) <= 2.5 * census.MAX_GMAC * 1e9, (census.key_id(key), census.macs(small))
        # the table value / signature the GPU test patches in decode back to the launch's form
        prefix = census.table_prefix(small)
        if prefix is not None:
            f = engine.decode_form(prefix, census.table_code(small))
            assert f.mbw == small.mbw and (small.family not in ("f23", "ct") or f.m == small.m)
            assert small.family in ("f23", "ct", "up") or f.variant == small.variant


def test_every_case_but_f47_has_certified_exact_operands(hip_lib):
    """The cap on what the exact check of the GPU file may leave out: the F(4,7) keys and nothing else."""
    exempt, seen = set(), set()
    for case in census.all_cases():
        ops = census.exact_operands(case, seed=7)
        if ops is None:
            exempt.add(census.case_id(case))
            continue
        launch = case.launch
        assert ops.bound <= census.EXACT_LIMIT
        unit = census.weight_unit(launch)
        assert tuple(ops.weight.shape) == census.weight_shape(launch) and [tuple(s.shape) for s in ops.srcs] == census.source_shapes(launch)
        assert bool(((ops.weight / unit).round() * unit == ops.weight).all()) and float(ops.weight.abs().max()) > 0
        assert all(bool((s == s.round()).all()) and float(s.abs().max()) > 0 for s in ops.srcs)
        # sparse only where the form needs it
        assert ops.attempt[2:] == (1.0, 1.0) or (case.key.m, case.key.r) in ((4, 3), (4, 4)) and case.key.family != "f23", (census.case_id(case), ops.attempt)
        seen.add(unit)
    expected = {census.case_id(c) for c in census.all_cases() if c.key.family == "ct" and (c.key.m, c.key.r) == (4, 7)}
    assert exempt == expected and expected, (exempt ^ expected)
    assert all(census.certifiable(c.key) == (census.case_id(c) not in exempt) for c in census.all_cases())
    assert seen == {1, 2, 4, 24, 90, 180, 576}, seen                      # Upconv / Refine, F(2,3), F(2x2,3x3), F(4,3), F(2,7), F(4,4), F(4x4,3x3)
    assert census.form_scales("ct", 4, 7)[1] == 90720


def test_each_certificate_is_cross_checked_by_an_exact_emulation_of_one_tile(hip_lib):
    """A^T [(G g) o (B^T d)] in Fractions over one tile - the first (zero padding in front), one in the interior and the last (ragged, zero padding behind) - reproduces the direct
    sum the layer is defined by, for the very operands of the certificate (F(4,7): for uncertified integer operands)."""
    for case in census.all_cases():
        launch = case.launch
        ops = census.exact_operands(case, seed=7)
        srcs, weight = (ops.srcs, ops.weight) if ops is not None else census._draw(launch, 7, 1, 1, 1.0, 1.0)
        cin = sum(launch.srcs_c)
        channels = sorted({0, launch.srcs_c[0] - 1, min(cin - 1, launch.srcs_c[0]), cin // 2, cin - 1})
        m = census.form_of(launch)[0]
        h, w = launch.hw
        last = ((h - 1) // (m if launch.axis != 0 else 1) if launch.family != "up" else h - 1,
                (w - 1) // (m if launch.axis != 1 else 1) if launch.family != "up" else w - 1)
        for ty, tx in ((0, 0), (last[0] // 2, last[1] // 2), last):
            form, direct = census.emulate_tile(launch, srcs, weight, launch.cout - 1, ty, tx, channels)
            assert form == direct, (census.case_id(case), ty, tx)


def test_stride2_halves_run_alone_with_the_views_their_builder_makes(hip_lib, monkeypatch):
    """The GPU file launches a stride-2 half alone through Plan._conv_winograd_1d with census.stride2_view: for every k x 1 half of the
    census, Plan.conv_relu2 - table lookup, decode_form, _conv_relu2_stride2 - builds exactly that launch for the pair (same key, same
    strided views, same destination split), and hands the 1 x k half the two column halves as its [even | odd] sources."""
    halves = [c.launch for c in census.census().values() if c.launch.view]
    assert len(halves) >= 8 and {h.split for h in halves} == {False, True}
    for half in halves:
        n, (h, w), c, cm, k = half.batch, half.hw, half.srcs_c[0], half.cout, 2 * half.r - 1
        sd = {"p.conv_y.weight": torch.zeros(cm, c, k, 1), "p.conv_y.bias": torch.zeros(cm),
              "p.conv_x.weight": torch.zeros(cm, cm, 1, k), "p.conv_x.bias": torch.zeros(cm)}
        monkeypatch.setitem(engine.WINOGRAD, engine.stride2_signature(k, cm, c, h, w // 2, n), 10 * half.mbw + int(half.split))
        plan = engine.Plan.bare("cpu", state=sd)
        plan.winograd = True
        x, mid, out = torch.zeros(n, c, 2 * h, w), torch.zeros(n, cm, h, w), torch.zeros(n, cm, h, w // 2)
        plan.conv_relu2("main", "t", [x], "p", mid, out, stride=2)
        assert len(plan.conv_log) == 2 and census.launch_of(plan.conv_log[0]) == half
        d = plan.stages["main"][0][1].native[1]
        view = census.stride2_view(half, x.data_ptr())
        assert [d.src[0], d.src[1]] == view["ptrs"] and [d.src_channels[0], d.src_channels[1]] == view["channels"] and d.num_src == 2
        assert (d.batch, d.height, d.width, d.src_row_pitch, d.src_plane_floats) == (n, h, w, view["row_pitch"], view["plane"])
        assert bool(d.dst_split_columns) == half.split and d.dst == mid.data_ptr()
        if half.split:
            other = census.launch_of(plan.conv_log[1])
            assert (other.family, other.axis, other.m, other.r, other.stride2, other.view, other.split) == ("ct", 0, 4, half.r, True, False, False)
            assert other.srcs_c == (cm, cm) and other.hw == (h, w // 2)
            dx = plan.stages["main"][1][1].native[1]
            assert [dx.src[0], dx.src[1]] == [mid.data_ptr(), mid.data_ptr() + 4 * (mid.numel() // 2)]
        else:
            assert "winograd" not in plan.conv_log[1]                  # the 1 x k half stays on the direct kernel, dense intermediate
