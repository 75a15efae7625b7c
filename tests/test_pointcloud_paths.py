"""Host side (no GPU): the census of the point-cloud append (tests/pointcloud_paths.py) that tests/test_gpu_pointcloud_paths.py runs - the
constants parse, every declared path has a case and every case sits on the path it names, the fmaf emulation is exact (constructed ties
included), the fp32 restatement says what the reference's expressions say, the certified operands are exact, and the preconditions that keep a
case from passing by emptiness hold - among them the entry-swap loop: on the general camera, swapping ANY two entries of kinv or of the pose
changes a record bit."""
import fractions
import itertools
import numpy as np
import pytest

import pointcloud_paths as pc

F32 = np.float32
_param = lambda cases: pytest.mark.parametrize("case", cases, ids=pc.ids(cases))          # noqa: E731


def test_constants_parse_and_are_pinned():
    c = pc.constants()
    assert (c["wg"], c["waves"], c["wave_size"], c["grid"]) == (1024, 16, 64, 1)
    assert c["max_masks"] == 8
    assert (c["err_bad_argument"], c["err_unsupported"], c["err_lds_budget"]) == (-1, -2, -3)


def test_every_declared_path_has_a_case():
    print("\n" + pc.table())
    assert set(c.entry for c in pc.CASES) == set(pc.PATHS)
    for entry, paths in pc.PATHS.items():
        assert len(set(paths)) == len(paths)
        have = {c.path for c in pc.cases_of(entry)}
        assert have == set(paths), (entry, sorted(set(paths) - have), sorted(have - set(paths)))
    names = [(c.entry, c.name) for c in pc.CASES]
    assert len(set(names)) == len(names)
    assert all(reason for reason in pc.UNREACHED.values())
    assert [c.args["h"] * c.args["w"] for c in pc.cases_of("plane")] == [63, 64, 450, 1024, 1025, 2079]
    assert max(pc.device_bytes(c) for c in pc.CASES) <= pc.MAX_DEVICE_BYTES


@_param(pc.CASES)
def test_every_case_sits_on_the_path_it_names(case):
    assert pc.path_of(case) == case.path, (case.entry, case.name, pc.path_of(case))
    if case.args["certified"]:
        assert pc.path_of(case, exact=True) == case.path, (case.entry, case.name, pc.path_of(case, exact=True))


def test_rule_roi_is_python_slicing():
    """`mask[:r0] = False; mask[r1:] = False` on a row of n leaves exactly range(*rule)."""
    for n in (1, 5, 20):
        for r0, r1 in itertools.product(range(-n - 3, n + 4), repeat=2):
            m = np.ones(n, dtype=bool)
            m[:r0] = False
            m[r1:] = False
            y0, y1, x0, x1 = pc.rule_roi([r0, r1, r0, r1], n, n)
            want = np.zeros(n, dtype=bool)
            want[y0:max(y1, y0)] = True
            assert np.array_equal(m, want) and (y0, y1) == (x0, x1), (n, r0, r1)


# ---- the fmaf emulation -------------------------------------------------------------------------------------------------------------------------
def _round_fraction_to_f32(q):
    """A rational correctly rounded to fp32 (nearest, ties to even) by integer arithmetic; overflow gives inf."""
    if q == 0:
        return F32(0.0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if fractions.Fraction(2) ** e > q:
        e -= 1
    assert fractions.Fraction(2) ** e <= q < fractions.Fraction(2) ** (e + 1)
    quantum = fractions.Fraction(2) ** (max(e, -126) - 23)
    n = q / quantum
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > fractions.Fraction(1, 2) or (rest == fractions.Fraction(1, 2) and lo & 1):
        lo += 1
    value = lo * quantum
    if value >= fractions.Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(value))                       # exact: an fp32 number is a double


def _fma_exact(a, b, c):
    return _round_fraction_to_f32(fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c)))


def _ties():
    """Triples whose fp64 sum a * b + c lands exactly on an fp32 midpoint while the exact sum does not: the residual decides.
    (1 + 2^-23)(1 - 2^-23) 2^-24 = 2^-24 - 2^-70, added to an fp32 number m with ulp 2^-23: the fp64 sum is the midpoint m + 2^-24, the exact
    sum lies below it.  (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a midpoint itself; c = +-2^-80 moves the exact sum off it, the fp64 sum stays."""
    out = []
    a, b = F32(1 + 2.0 ** -23), F32((1 - 2.0 ** -23) * 2.0 ** -24)
    for m in (1.0, 1 + 2.0 ** -23, 1 + 2.0 ** -22, 1.5 + 2.0 ** -23):
        for s in (1, -1):
            out.append((a, F32(s) * b, F32(s * m)))                                     # residual towards zero
    sq = F32(1 + 2.0 ** -12)
    for c in (2.0 ** -80, -2.0 ** -80):
        for s in (1, -1):
            out.append((sq, F32(s) * sq, F32(s * c)))
            out.append((sq, F32(s) * F32(1 + 2.0 ** -12 + 2.0 ** -11), F32(s * c)))    # (1 + 2^-12)(1 + 3 2^-12): another midpoint, odd below
    return out


def test_fmaf_emulation_is_exact_on_random_triples():
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(3000) * 2.0 ** rng.integers(-20, 20, 3000)).astype(F32)
    b = (rng.standard_normal(3000) * 2.0 ** rng.integers(-20, 20, 3000)).astype(F32)
    c = (rng.standard_normal(3000) * 2.0 ** rng.integers(-20, 20, 3000)).astype(F32)
    c[::3] = -(a[::3] * b[::3])                                                           # cancellation: the residual of the product is the result
    got = pc.fmaf(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert pc.fmaf(F32(3), F32(np.inf), F32(1)) == np.inf and np.isnan(pc.fmaf(F32(0), F32(np.inf), F32(1)))
    assert pc.fmaf(F32(3e38), F32(2), F32(-3e38)) == F32(3e38)                           # the product alone overflows fp32, the fused result does not


def test_fmaf_emulation_is_exact_on_the_constructed_ties_and_plain_double_rounding_is_not():
    ties = _ties()
    plain_wrong = 0
    seen = set()
    for a, b, c in ties:
        p = np.float64(a) * np.float64(b)
        s = p + np.float64(c)
        exact = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
        residual = exact - fractions.Fraction(float(s))
        assert residual != 0, (a, b, c)                                                   # the fp64 sum is inexact ...
        lo = F32(s) if np.float64(F32(s)) <= s else np.nextafter(F32(s), F32(-np.inf))
        hi = np.nextafter(lo, F32(np.inf))
        assert np.float64(lo) + (np.float64(hi) - np.float64(lo)) / 2 == s, (a, b, c)      # ... and sits on an fp32 midpoint
        seen.add(residual > 0)
        want = _fma_exact(a, b, c)
        got = pc.fmaf(a, b, c)
        assert got.view(np.uint32) == want.view(np.uint32), (a, b, c, got, want)
        plain_wrong += int(F32(s) != want)
    assert seen == {True, False}                                                         # residuals of either sign
    assert plain_wrong >= 1, "np.float32(p + c) must get a constructed tie wrong: that is why the emulation exists"
    print(f"{len(ties)} constructed ties, plain double rounding wrong on {plain_wrong}")


# ---- the restatement says what the reference says -------------------------------------------------------------------------------------------------
def _compare_with_oracle(ops, want, what):
    """`want` (n, 6) records of the reference's expressions against append_ref / append_ref64: selection, order and colours exact, coordinates
    within the derived 10 u S; non-finite coordinates must agree in kind."""
    ref = pc.append_ref(ops, capacity=2 ** 62)
    r64, S = pc.append_ref64(ops)
    assert want.shape == ref.records.shape, (what, want.shape, ref.records.shape)
    assert np.array_equal(want[:, 3:].view(np.uint32), ref.records[:, 3:].view(np.uint32)), what      # colours: also pins WHICH pixels, in which order
    fin = np.isfinite(r64[:, :3]) & np.isfinite(S)
    for got in (want[:, :3], ref.records[:, :3]):
        with np.errstate(invalid="ignore"):
            err = np.abs(got.astype(np.float64) - r64[:, :3])
        assert (err[fin] <= pc.BOUND_ROUNDINGS * pc.U * S[fin]).all(), (what, float((err[fin] / (pc.U * S[fin])).max()))
        assert np.array_equal(np.isnan(got[~fin]), np.isnan(r64[:, :3][~fin])), what
        assert np.array_equal(got[~fin][~np.isnan(got[~fin])], r64[:, :3][~fin][~np.isnan(got[~fin])]), what
    return float((err[fin] / (pc.U * S[fin])).max()) if fin.any() else 0.0


@_param(pc.CASES)
def test_restatement_equals_the_oracle(case):
    """Keep decisions and record order of append_ref equal orc.pointcloud_records exactly (the colours of distinct pixels differ, so equal colour
    columns mean equal selection and order; the count is compared too); coordinates within 10 * 2^-24 * S of the fp64 reference, both of them."""
    ops = pc.operands(case)
    keep, depth = pc.decisions(ops)
    want = pc.oracle_records(ops).numpy()
    assert want.shape[0] == int(keep.sum())
    worst = _compare_with_oracle(ops, want, case.name)
    print(f"{case.entry}/{case.name}: {want.shape[0]} records, append_ref within {worst:.2f} u S of fp64")
    if case.path.startswith("inexact_max"):
        # the decision on depth == fp32(0.1) under max_d = 0.1, taken from torch: the reference's own expression on the CPU
        import torch
        d = torch.from_numpy(depth.copy())
        torch_keep = ((ops["min_d"] <= d) & (d <= ops["max_d"])).numpy()
        at = depth == F32(0.1)
        assert at.any() and np.array_equal(keep[at], torch_keep[at]) and len(set(torch_keep[at].tolist())) == 1
        print(f"  depth == fp32(0.1) under max_d 0.1: torch keeps = {bool(torch_keep[at][0])}")


@_param(pc.certified_cases())
def test_certified_operands_are_exact(case):
    """On the certified operands the fp32 restatement EQUALS the fp64 reference: no intermediate rounds."""
    ops = pc.operands(case, exact=True)
    ref = pc.append_ref(ops)
    r64, _ = pc.append_ref64(ops)
    assert np.isfinite(r64).all()
    assert np.array_equal(ref.records.astype(np.float64), r64), case.name
    assert (np.frexp(ops["inv_depth"][pc.decisions(ops)[0]])[0] == 0.5).all()                                 # every kept inverse depth: a power of two
    assert (ops["image"] * 256 == np.round(ops["image"] * 256)).all() and np.abs(ops["image"]).max() <= 0.5
    rot = ops["pose"].reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 9)
    for i in range(ops["b"]):
        assert (rot[i] != 0).all() and len(set(np.abs(rot[i]).tolist())) == 9 and (ops["kinv"][i] != 0).all()
        assert ops["kinv"][i][1] != ops["kinv"][i][3]


# ---- preconditions: no case passes by emptiness ---------------------------------------------------------------------------------------------------
@_param(pc.CASES)
def test_preconditions(case):
    a, c = case.args, pc.constants()
    for exact in ((False, True) if a["certified"] else (False,)):
        ops = pc.operands(case, exact)
        keep, depth = pc.decisions(ops)
        ref = pc.append_ref(ops)
        frac = keep.mean()
        empty_on_purpose = a["keep"] in ("none",) or case.path in ("empty",)
        if a["keep"] != "random":
            assert pc.keep_class(keep) == a["keep"], (case.name, pc.keep_class(keep))
        elif not empty_on_purpose and a["depth"] == "plain":
            assert 0.1 <= frac <= 0.9, (case.name, exact, frac)                          # every "random" case
        elif not empty_on_purpose:                                                       # the depth cases: their own conditions below
            assert 0 < frac < 1, (case.name, exact, frac)
        assert ref.cursor == ops["start"] + int(keep.sum())
        if case.path in ("cap_inside_wave_middle_pass", "cap_at_pass_boundary"):
            cut = ops["capacity"] - ops["start"]
            assert 0 < cut < len(ref.records) and ref.admitted[cut - 1] and not ref.admitted[cut]
            same_wave = pc.position(ref.pixel[cut - 1])[:2] == pc.position(ref.pixel[cut])[:2] and ref.batch[cut - 1] == ref.batch[cut]
            assert same_wave == (case.path == "cap_inside_wave_middle_pass")
        if case.entry == "masks" and ops["masks"]:
            sums = np.sum(ops["masks"], axis=0)
            ok = np.isfinite(depth)                                                      # pixels the vote let through
            assert (sums == ops["vote_above"]).any() and not keep[sums == ops["vote_above"]].any()      # strict >
            assert keep[sums == ops["vote_above"] + 1].any() and ok.any()
        if case.path == "equal_dropout":
            at = ops["uniform"] == F32(ops["dropout"])
            unthinned = pc.decisions(dict(ops, uniform=None))[0]
            assert (at & unthinned).any() and not keep[at].any()                         # pixels only the strict `>` drops
        if case.entry == "depth":
            bits = ops["inv_depth"].view(np.uint32)
            if a["depth"] == "edges":
                vals = pc.edge_values(*pc.edge_range(ops))
                votes = np.ones_like(keep) if not ops["masks"] else np.sum(ops["masks"], axis=0) > ops["vote_above"]
                for name, v in vals.items():
                    here = bits == v.view(np.uint32)
                    for vote in ((True, False) if ops["masks"] else (True,)):
                        sel = here & (votes == vote)
                        assert sel.any(), (case.name, name, vote)
                        finite_range = np.isfinite(ops["min_d"])
                        want = vote and (name in ("at_min", "at_max") if finite_range else name != "nan")
                        if not finite_range and not vote:
                            want = name not in ("nan", "inf")                          # x * 0 = +-0 -> +-inf: kept under (-inf, inf); NaN * 0 and inf * 0 are NaN
                        assert keep[sel].all() == want and keep[sel].any() == want, (case.name, name, vote, want)
                if not np.isfinite(ops["min_d"]):
                    assert np.isnan(ref.records[:, :3]).any() or np.isinf(ref.records[:, :3]).any()
            else:
                at = depth == F32(0.1)
                assert at.any() and (depth == np.nextafter(F32(0.1), F32(1))).any()
        if ops["b"] == 3 and len(ref.records):
            # a missing `+ b * 9` / `+ b * 16`: element 0's camera for everyone changes records of the other elements
            for key in ("kinv", "pose"):
                other = pc.append_ref(ops, **{key: np.repeat(ops[key][:1], 3, axis=0)})
                changed = (other.records.view(np.uint32) != ref.records.view(np.uint32)).any(1)
                assert not changed[ref.batch == 0].any() and changed[ref.batch == 1].any() and changed[ref.batch == 2].any()


@_param([c for c in pc.CASES if c.args["keep"] != "none" and c.path != "empty"])
def test_every_kinv_and_pose_entry_contributes(case):
    """The cap on what the exact tests may miss: on the general camera, swapping ANY two of the nine kinv entries or ANY two of the twelve pose
    entries (in every batch element) changes at least one record bit of append_ref.  No pair is left out.  (Cases that keep nothing on purpose -
    keep/none and the empty rois - have no record to change and are listed out above.)"""
    ops = pc.operands(case)
    base = pc.append_ref(ops).records.view(np.uint32)
    assert len(base) > 0
    pairs = 0
    for key, n, stride in (("kinv", 9, 9), ("pose", 12, 16)):
        for i, j in itertools.combinations(range(n), 2):
            m = ops[key].copy()
            m[:, [i, j]] = m[:, [j, i]]
            assert m.shape[1] == stride
            other = pc.append_ref(ops, **{key: m}).records.view(np.uint32)
            assert (other != base).any(), (case.name, key, i, j)
            pairs += 1
    assert pairs == 36 + 66
    k4, pose, kinv = pc.general_camera(ops["b"], ops["h"], ops["w"])
    for i in range(ops["b"]):
        r = pose[i, :3, :3].numpy().reshape(-1)
        assert (r != 0).all() and len(set(np.abs(r).tolist())) == 9 and (pose[i, :3, 3] != 0).all()
        assert (kinv[i] != 0).all() and k4[i, 0, 1] != 0 and k4[i, 0, 0] != k4[i, 1, 1]
        assert np.allclose(r.reshape(3, 3) @ r.reshape(3, 3).T, np.eye(3), atol=1e-6)


def test_existing_fixture_camera_shares_one_k_and_has_the_structural_zeros():
    """What the three committed fixture cases cannot see (the reason for this census): one K for every batch element, eight zeros in kinv and
    the pose rows, kinv[8] == 1."""
    import torch
    from monorec_amd import synth
    case = synth.make_pointcloud_case(2, 64, 96, 3)
    assert torch.equal(case["intrinsics"][0], case["intrinsics"][1])
    kinv = torch.inverse(case["intrinsics"])[0, :3, :3].reshape(-1)
    assert all(float(kinv[i]) == 0 for i in (1, 3, 6, 7)) and float(kinv[8]) == 1
    assert all(float(case["pose"][0][i][j]) == 0 for i, j in ((0, 1), (1, 0), (1, 2), (2, 1)))


# ---- the committed fixture of the reference's own PLYSaver on the general camera -------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.FIXTURE_CASES)
def test_reference_fixture_on_the_general_camera(name):
    """tests/golden/pointcloud_general.npz holds what the reference's own PLYSaver appended for two general-camera cases (tools/
    make_golden_pointcloud_general.py).  Its inputs are the operands of the census case; the oracle and append_ref select the same pixels in the
    same order with the same colours, and their coordinates lie within the derived bound (the reference's sgemm order is host-dependent)."""
    z = np.load(pc.FIXTURE)
    meta = pc.fixture_cases()[name]
    case = next(c for c in pc.CASES if f"{c.entry}.{c.name}" == name)
    ops = pc.operands(case)
    fops = pc.fixture_ops(z, name, meta)
    for key in ("inv_depth", "image", "pose", "intrinsics"):
        assert np.array_equal(fops[key].reshape(-1).view(np.uint32), np.asarray(ops[key]).reshape(-1).view(np.uint32)), key
    assert (meta["roi"], meta["min_d"], meta["max_d"], meta["dropout"]) == (ops["roi"], ops["min_d"], ops["max_d"], 0)
    want = z[f"{name}.records"]
    assert want.shape == (meta["points"], 6) and meta["points"] > 100
    _compare_with_oracle(fops, want, name)
    _compare_with_oracle(fops, pc.oracle_records(fops).numpy(), name + " (oracle)")


def test_plysaver_refuses_a_capacity_below_one():
    """capacity 0 could never grow (`_ensure` doubles it): the constructor refuses it.  (Only the refusal is tested.)"""
    from monorec_amd.pointcloud import PLYSaver
    for capacity in (0, -4):
        with pytest.raises(ValueError, match="capacity"):
            PLYSaver(8, 8, capacity=capacity)
    assert PLYSaver(8, 8, capacity=1)._capacity == 1
