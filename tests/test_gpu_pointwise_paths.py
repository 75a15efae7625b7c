"""GPU (MI355X): every launch path of the kernels around the convolutions (tests/pointwise_paths.py; pinned by tests/test_pointwise_paths.py)
on its own, through the C ABI, against a plain CPU reference.  Selecting kernels and one-expression kernels are compared exactly; the two
fp32 dot-product kernels of csrc/heads.hip against an fp64 reference at the project's 2e-6.  Every output buffer starts as NaN (the references
have none), followed by a NaN guard that must survive: an element a kernel did not write, or wrote past the end, fails the test."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import pointwise_paths as pp
from monorec_amd import _lib, synth
from monorec_amd.model import depth_hypotheses, host_geometry
from oracle import monorec_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(*shape, dtype=torch.float32):
    """(backing, view): a NaN-filled output of `shape` at the front of an allocation with GUARD more NaN elements behind it."""
    n = math.prod(shape)
    backing = torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)
    return backing, backing[:n].view(*shape)


def _intact(*backings_and_views):
    """The guards behind the outputs are still NaN."""
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b[v.numel():]).all()) for b, v in backings_and_views)


def _cases(entry):
    return pytest.mark.parametrize("case", pp.cases_of(entry), ids=pp.case_ids(entry))


# ---- a. csrc/eltwise.hip ----------------------------------------------------------------------------------------------------------------------------
@_cases("maxpool3x3s2")
def test_maxpool3x3s2(hip_lib, case):
    a = case.args
    x = pp.max_input((1, a["planes"], a["h"], a["w"]), pp.gen(case))
    ref = F.max_pool2d(x, 3, 2, 1)
    xd = x.to(DEV)
    o = _out(*ref.shape)
    _lib.check(hip_lib.mr_maxpool3x3s2_f32(xd.data_ptr(), o[1].data_ptr(), a["planes"], a["h"], a["w"], _stream()), "mr_maxpool3x3s2_f32")
    assert _intact(o) and not torch.isnan(ref).any()
    assert torch.equal(o[1].cpu(), ref)


@_cases("maxpool2x2")
def test_maxpool2x2(hip_lib, case):
    a = case.args
    planes = a["frames"] * a["planes"]
    x = pp.max_input((planes, a["h"], a["w"]), pp.gen(case))
    ref = F.max_pool2d(x, 2)
    xd = x.to(DEV)
    o = _out(*ref.shape)
    _lib.check(hip_lib.mr_maxpool2x2_f32(xd.data_ptr(), o[1].data_ptr(), planes, a["h"], a["w"], _stream()), "mr_maxpool2x2_f32")
    assert _intact(o) and bool(torch.isinf(x).any()) and not torch.isnan(ref).any()
    assert torch.equal(o[1].cpu(), ref)


@_cases("pool2x2_framemax")
def test_pool2x2_framemax(hip_lib, case):
    a = case.args
    x = pp.max_input((a["frames"], a["planes"], a["h"], a["w"]), pp.gen(case))
    ref_pool, ref_max = F.max_pool2d(x, 2), x.max(0)[0]
    xd = x.to(DEV)
    po, mo = _out(*ref_pool.shape), _out(*ref_max.shape)
    _lib.check(hip_lib.mr_pool2x2_framemax_f32(xd.data_ptr(), po[1].data_ptr(), mo[1].data_ptr(), a["frames"], a["planes"], a["h"], a["w"], _stream()),
               "mr_pool2x2_framemax_f32")
    assert _intact(po, mo) and bool(torch.isinf(x).any()) and not torch.isnan(ref_pool).any()
    assert torch.equal(po[1].cpu(), ref_pool) and torch.equal(mo[1].cpu(), ref_max)


@_cases("max_over_frames")
def test_max_over_frames(hip_lib, case):
    a = case.args
    x = pp.max_input((a["frames"], a["count"]), pp.gen(case))
    xd = x.to(DEV)
    o = _out(a["count"])
    _lib.check(hip_lib.mr_max_over_frames_f32(xd.data_ptr(), o[1].data_ptr(), a["frames"], a["count"], _stream()), "mr_max_over_frames_f32")
    assert _intact(o)
    assert torch.equal(o[1].cpu(), x.max(0)[0])


@_cases("resnet_normalize")
def test_resnet_normalize(hip_lib, case):
    a = case.args
    x = torch.rand(a["count"], generator=pp.gen(case)) - 0.5
    xd = x.to(DEV)
    o = _out(a["count"])
    _lib.check(hip_lib.mr_resnet_normalize_f32(xd.data_ptr(), o[1].data_ptr(), a["count"], _stream()), "mr_resnet_normalize_f32")
    assert _intact(o)
    assert torch.equal(o[1].cpu(), ((x + 0.5) - 0.45) / 0.225)


@_cases("nonzero_mean")
def test_nonzero_mean_over_frames(hip_lib, case):
    """Bit-exact against the kernel's own order written in torch (sequential fp32 sum over the frames / max(count of != 0, 1)), and within the
    derived bound (pointwise_paths.nonzero_mean_bound) of an fp64 evaluation of SimpleMaskModule's expression (monorec_model.py:448-449)."""
    a = case.args
    x = pp.nonzero_mean_input(a["frames"], a["count"], pp.gen(case))
    xd = x.to(DEV)
    o = _out(a["count"])
    _lib.check(hip_lib.mr_nonzero_mean_over_frames_f32(xd.data_ptr(), o[1].data_ptr(), a["frames"], a["count"], _stream()), "mr_nonzero_mean_over_frames_f32")
    assert _intact(o)
    got = o[1].cpu()
    exact = pp.nonzero_mean_exact(x)
    assert not torch.isnan(exact).any() and torch.equal(got, exact)
    val, bound = pp.nonzero_mean_bound(x)
    fin = torch.isfinite(val)
    assert torch.equal(got[~fin].double(), val[~fin]) and bool(((got.double() - val).abs()[fin] <= bound[fin]).all())


@_cases("apply_mask")
def test_apply_mask(hip_lib, case):
    a = case.args
    g = pp.gen(case)
    cv = torch.randn(a["batch"], a["depths"], a["plane"], generator=g)
    mask = torch.rand(a["batch"], 1, a["plane"], generator=g)
    ref = (1 - mask) * cv
    md = mask.to(DEV)
    backing = torch.full((cv.numel() + GUARD,), NAN, device=DEV)
    src = backing[:cv.numel()].view(cv.shape)
    src.copy_(cv)
    dst = (backing, src) if a["in_place"] else _out(*cv.shape)
    _lib.check(hip_lib.mr_apply_mask_f32(src.data_ptr(), md.data_ptr(), dst[1].data_ptr(), a["batch"], a["depths"], a["plane"], _stream()), "mr_apply_mask_f32")
    assert _intact(dst, (backing, src))
    assert torch.equal(dst[1].cpu(), ref)
    if not a["in_place"]:
        assert torch.equal(src.cpu(), cv)


@_cases("gather_small")
def test_gather_small(hip_lib, case):
    a = case.args
    g = pp.gen(case)
    parts = [torch.randn(a["floats_each"], generator=g) for _ in range(a["num"])]
    dev = [torch.cat([p, torch.full((3,), NAN)]).to(DEV) for p in parts]               # scattered allocations of their own
    ptrs = (ctypes.c_void_p * a["num"])(*[d.data_ptr() for d in dev])
    o = _out(a["num"], a["floats_each"])
    _lib.check(hip_lib.mr_gather_small_f32(ptrs, a["num"], a["floats_each"], o[1].data_ptr(), _stream()), "mr_gather_small_f32")
    assert _intact(o)
    assert torch.equal(o[1].cpu(), torch.stack(parts))
    assert hip_lib.mr_gather_small_f32(ptrs, pp.constants()["max_gather"] + 1, a["floats_each"], o[1].data_ptr(), _stream()) == -1


# ---- b. csrc/heads.hip: mask classifier, both entry points ----------------------------------------------------------------------------------------------
@_cases("mask_classifier")
def test_mask_classifier(hip_lib, case):
    """mr_mask_classifier_f32 / mr_mask_classifier_b8_f32 on one path of {VEC 1, VEC 2} x {C loop: blocks / tail / both} x {D loop: blocks / tail /
    both / no volume} x {no B8 copy, B8 copy}: the mask within 2e-6 of an fp64 sigmoid(conv1x1); the volume exactly (1 - mask) * cv given the
    mask; the B8 copy exactly the bf16 rounding of that fp32 volume; both entry points bit-identical."""
    a = case.args
    b, c, d, plane = a["batch"], a["channels"], a["depths"], a["plane"]
    assert pp.rule_classifier(b, plane)[0] == int(case.path[3])
    x, wt, bias, cv = pp.classifier_operands(case)
    ref = pp.classifier_mask_reference(x, wt, bias)
    xd, wd, bd = x.to(DEV), wt.reshape(-1).to(DEV), bias.to(DEV)
    runs = {}
    for entry in (("plain", "b8") if a["b8"] else ("plain",)):
        mo = _out(*ref.shape)
        vol_backing = torch.full((cv.numel() + GUARD,), NAN, device=DEV)
        vol = vol_backing[:cv.numel()].view(cv.shape)
        vol.copy_(cv)
        if entry == "plain":
            _lib.check(hip_lib.mr_mask_classifier_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), b, c, plane, mo[1].data_ptr(), vol.data_ptr() if d else None, d,
                                                      _stream()), "mr_mask_classifier_f32")
            assert _intact(mo, (vol_backing, vol))
        else:
            bo = _out(b, d // 8, a["hw"][0], a["hw"][1], 8, dtype=torch.bfloat16)
            _lib.check(hip_lib.mr_mask_classifier_b8_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), b, c, plane, mo[1].data_ptr(), vol.data_ptr(), d, bo[1].data_ptr(),
                                                         _stream()), "mr_mask_classifier_b8_f32")
            assert _intact(mo, (vol_backing, vol), bo)
            runs["copy"] = bo[1].cpu()
        runs[entry] = (mo[1].cpu(), vol.cpu())
    got, got_cv = runs["plain"]
    err = float((got.double() - ref).abs().max())
    print(f"{case.name}: mask vs fp64 {err:.2e}")
    assert not torch.isnan(got).any() and err <= pp.MASK_TOL, err
    assert torch.equal(got_cv, (1 - got) * cv if d else cv)                       # the multiply itself is exact given the mask
    if a["b8"]:
        assert torch.equal(runs["b8"][0], got) and torch.equal(runs["b8"][1], got_cv)
        assert not torch.isnan(runs["copy"].float()).any() and torch.equal(pp.from_b8(runs["copy"], d), pp.bf(got_cv))


# ---- c. csrc/heads.hip: depth heads ------------------------------------------------------------------------------------------------------------------
@_cases("depth_heads")
def test_depth_heads(hip_lib, case):
    """C = 1 in quad mode (three of the four waves have no channel) and four heads alternating quad / pixel mode (the `first_block` selection),
    against an fp64 conv2d at the project's 2e-6."""
    shapes = case.args["heads"]
    assert [pp.rule_head(*s)[0] for s in shapes] == {"quad_one_channel": [True], "alternating_quad_pixel": [True, False, True, False]}[case.path]
    descs = (_lib.HeadDesc * len(shapes))()
    keep, outs, refs = [], [], []
    for i, ((b, c, h, w), (x, wt, bias)) in enumerate(zip(shapes, pp.head_operands(case))):
        refs.append(pp.head_reference(x, wt, bias))
        xd, wd, bd = x.to(DEV), wt.to(DEV), bias.to(DEV)
        o = _out(b, 1, h, w)
        keep += [xd, wd, bd]
        outs.append(o)
        descs[i].src, descs[i].weight, descs[i].bias, descs[i].dst = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o[1].data_ptr()
        descs[i].batch, descs[i].channels, descs[i].height, descs[i].width = b, c, h, w
    _lib.check(hip_lib.mr_depth_heads_f32(descs, len(shapes), pp.HEAD_LO, pp.HEAD_HI, _stream()), "mr_depth_heads_f32")
    assert _intact(*outs)
    for o, ref, s in zip(outs, refs, shapes):
        got = o[1].cpu()
        err = float((got.double() - ref).abs().max())
        print(f"{case.name} {s}: vs fp64 {err:.2e}")
        assert not torch.isnan(got).any() and err <= pp.HEAD_TOL, (s, err)


# ---- d. csrc/cost_volume.hip: the B8 and the lean entry point ----------------------------------------------------------------------------------------
def _cost_volume_run(lib, entry, batch, d):
    kf = batch["keyframe"].to(DEV)
    b, _, h, w = kf.shape
    nf = len(batch["frames"])
    frames = [f.to(DEV).contiguous() for f in batch["frames"]]
    kinv, proj = host_geometry(batch["keyframe_intrinsics"], batch["keyframe_pose"], batch["intrinsics"], batch["poses"])
    kinv, proj = kinv.to(DEV), proj.to(DEV)
    depths = depth_hypotheses((0.33, 0.0025), d).to(DEV)
    cv = _out(b, d, h, w)
    sf = [_out(b, d, h, w) for _ in range(nf)]
    sb = [_out(b, (d + 7) // 8, h, w, 8, dtype=torch.bfloat16) for _ in range(nf)]
    fp = (ctypes.c_void_p * nf)(*[f.data_ptr() for f in frames])
    sp = (ctypes.c_void_p * nf)(*[s[1].data_ptr() for s in sf])
    bp = (ctypes.c_void_p * nf)(*[s[1].data_ptr() for s in sb])
    cw = (ctypes.c_float * 3)(5 / 32, 16 / 32, 11 / 32)
    rc = getattr(lib, entry)(kf.data_ptr(), fp, nf, kinv.data_ptr(), proj.data_ptr(), depths.data_ptr(), b, d, h, w, 10.0, cw, 1, None, cv[1].data_ptr(), sp, bp, _stream())
    assert _intact(cv, *sf, *sb), f"{entry} wrote past the end of an output"
    return rc, cv[1].cpu(), [s[1].cpu() for s in sf], [s[1].cpu() for s in sb]


@_cases("cost_volume_b8")
def test_cost_volume_b8_and_lean_entry_points(hip_lib, case):
    """mr_cost_volume_b8_f32 and mr_cost_volume_b8_lean_f32 on the same inputs, 45 x 70 = 12 workgroups + 78 pixels (`p < HWp` false in the
    last one): fused volume and B8 copies bit-identical; the B8 copies = the bf16 rounding of the B8 entry's fp32 single-frame volumes; the lean
    run left its fp32 buffers un-finalised - raw costs from which the documented expression (1 - 2 |raw|) * vm reproduces the finalised volumes
    bit for bit.  A depth count without a register-held fusion kernel is refused by both, nothing is launched."""
    a = case.args
    batch = synth.make_batch(a["batch"], a["h"], a["w"], a["frames"], seed=5)
    d = a["depths"]
    if case.path == "unsupported":
        for entry in ("mr_cost_volume_b8_f32", "mr_cost_volume_b8_lean_f32"):
            rc, cv, sf, sb = _cost_volume_run(hip_lib, entry, batch, d)
            assert rc == pp.constants()["err_unsupported"]
            assert torch.isnan(cv).all() and all(torch.isnan(s).all() for s in sf) and all(torch.isnan(s.float()).all() for s in sb)
        return
    assert (a["h"] * a["w"]) % 256 != 0
    rc, cv, sf, sb = _cost_volume_run(hip_lib, "mr_cost_volume_b8_f32", batch, d)
    _lib.check(rc, "mr_cost_volume_b8_f32")
    rc, lcv, lsf, lsb = _cost_volume_run(hip_lib, "mr_cost_volume_b8_lean_f32", batch, d)
    _lib.check(rc, "mr_cost_volume_b8_lean_f32")
    assert not torch.isnan(cv).any() and torch.equal(cv, lcv)
    for f in range(a["frames"]):
        assert not torch.isnan(sf[f]).any() and not torch.isnan(sb[f].float()).any()
        assert torch.equal(sb[f].view(torch.int16), lsb[f].view(torch.int16))                 # the B8 copies of both runs, bit for bit
        assert torch.equal(pp.from_b8(sb[f], d), pp.bf(sf[f]))                                # = the entry's own fp32 volumes, rounded to bf16
        raw = lsf[f]
        assert not torch.isnan(raw).any()                                                     # every raw cost was written ...
        assert bool((pp.cost_volume_finalise(raw) == sf[f]).all())                            # ... and never finalised: the expression still applies
        assert not torch.equal(raw, sf[f])                                                    # (the buffers do differ from the finalised volumes)
        valid = (sf[f] != 0).any(1)
        assert 0.0 < float(valid.float().mean()) < 1.0                                        # (both kinds of pixel occur)


# ---- e. csrc/conv_b8.hip companions ------------------------------------------------------------------------------------------------------------------
@_cases("f32_to_b8")
def test_layout_conversions_round_to_nearest_even(hip_lib, case):
    """mr_f32_nchw_to_b8 on unrounded Gaussian data with the edge table (exact ties, neighbours of a tie, overflow to inf, +-inf, -0.0, denormals,
    quiet and signalling NaN) in every channel: finite and infinite inputs bit for bit like torch's .to(bfloat16), a NaN stays a NaN (payload and
    sign are not compared), padded channels are zero.  mr_b8_to_f32_nchw brings exactly those values back."""
    a = case.args
    n, c, hw = a["n"], a["c"], a["hw"]
    x = pp.conversion_input(case)
    cb = (c + 7) // 8
    xd = x.to(DEV)
    assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))                       # (the copy keeps the NaN payloads)
    o = _out(n, cb, hw, 1, 8, dtype=torch.bfloat16)
    _lib.check(hip_lib.mr_f32_nchw_to_b8(xd.data_ptr(), o[1].data_ptr(), n, c, hw, _stream()), "mr_f32_nchw_to_b8")
    assert _intact(o)
    got = o[1].cpu()
    want = pp.to_b8(x)
    got_bits, want_bits = got.view(torch.int16).to(torch.int32) & 0xffff, want.view(torch.int16).to(torch.int32) & 0xffff
    nan_in = pp.is_nan_bf16_bits(want_bits)
    assert int(nan_in.sum()) == 3 * n * c
    assert bool(pp.is_nan_bf16_bits(got_bits)[nan_in].all())
    bad = (got_bits != want_bits) & ~nan_in
    assert not bool(bad.any()), [(hex(int(g)), hex(int(w_))) for g, w_ in zip(got_bits[bad][:8], want_bits[bad][:8])]
    back = _out(n, c, hw, 1)
    _lib.check(hip_lib.mr_b8_to_f32_nchw(o[1].data_ptr(), back[1].data_ptr(), n, c, hw, _stream()), "mr_b8_to_f32_nchw")
    assert _intact(back)
    res, exp = back[1].cpu(), pp.bf(x)
    fin = ~torch.isnan(x)
    assert torch.equal(res[fin].view(torch.int32), exp[fin].view(torch.int32)) and bool(torch.isnan(res[~fin]).all())


@_cases("b8_max")
def test_b8_pool_framemax_and_max_over_frames(hip_lib, case):
    a = case.args
    frames, b, c, h, w = a["frames"], a["batch"], a["c"], a["h"], a["w"]
    x = pp.bf(pp.max_input((frames * b, c, h, w), pp.gen(case)))
    if x.numel() <= 64:
        x.view(-1)[1], x.view(-1)[6] = pp.INF, -pp.INF
    assert bool(torch.isinf(x).any())
    xb = pp.to_b8(x).to(DEV)
    cb = (c + 7) // 8
    po, fo, mo = (_out(frames * b, cb, h // 2, w // 2, 8, dtype=torch.bfloat16), _out(b, cb, h, w, 8, dtype=torch.bfloat16),
                  _out(b, cb, h, w, 8, dtype=torch.bfloat16))
    _lib.check(hip_lib.mr_pool2x2_framemax_b8(xb.data_ptr(), po[1].data_ptr(), fo[1].data_ptr(), frames, b * cb, h, w, _stream()), "mr_pool2x2_framemax_b8")
    _lib.check(hip_lib.mr_max_over_frames_b8(xb.data_ptr(), mo[1].data_ptr(), frames, b * cb * h * w, _stream()), "mr_max_over_frames_b8")
    assert _intact(po, fo, mo)
    want = x.view(frames, b, c, h, w).max(0)[0]
    assert torch.equal(pp.from_b8(po[1].cpu(), c), F.max_pool2d(x, 2))
    assert torch.equal(pp.from_b8(fo[1].cpu(), c), want) and torch.equal(pp.from_b8(mo[1].cpu(), c), want)
    for o in (po, fo, mo):                                                        # padded channels stay zero, nothing is NaN
        assert not torch.isnan(o[1].float()).any()


# ---- f. mr_static_mask_f32 ---------------------------------------------------------------------------------------------------------------------------
@_cases("static_mask")
def test_static_mask(hip_lib, case):
    """create_pointcloud.py:76-77 exactly against orc.static_mask at r = 0, 1, 16 and the largest radius the 64 KiB LDS budget admits; the next
    even mask_fill is MR_ERR_LDS_BUDGET, an odd one MR_ERR_BAD_ARGUMENT (nothing launched); values exactly at the threshold count as moving."""
    a = case.args
    b, h, w = a["shape"]
    fill = a["mask_fill"]
    x, thr = pp.static_mask_input(case)
    xd = x.to(DEV)
    o = _out(b, 1, h, w)
    rc = hip_lib.mr_static_mask_f32(xd.data_ptr(), o[1].data_ptr(), b, h, w, thr, fill, _stream())
    assert _intact(o)
    assert rc == pp.rule_static_mask(fill)[0]
    if rc != 0:
        assert rc == {"refuse_lds": pp.constants()["err_lds_budget"], "refuse_odd": pp.constants()["err_bad_argument"]}[case.path]
        assert torch.isnan(o[1]).all()
        return
    got = o[1].cpu()
    assert torch.equal(got, orc.static_mask(x, fill, thr))
    assert got[b - 1, 0, 0, 0] == 0                                              # the corner pixel sits exactly at the threshold: moving


# ---- g. NaN in the max kernels -------------------------------------------------------------------------------------------------------------------------
def _nan_expectation(x, op):
    """(expected, dropped): `op` over x with every NaN replaced by -inf - what a max that DROPS NaN gives - and NaN where that leaves -inf (the data
    has no -inf of its own: a window / frame column of nothing but NaN)."""
    assert not torch.isinf(x).any()
    ref = op(torch.where(torch.isnan(x), torch.tensor(-pp.INF), x))
    return torch.where(ref == -pp.INF, torch.tensor(NAN), ref)


def _same_with_nan(got, want):
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


def test_max_kernels_drop_nan_documented_deviation(hip_lib):
    """The six max kernels (mr_maxpool3x3s2_f32, mr_maxpool2x2_f32, mr_pool2x2_framemax_f32, mr_max_over_frames_f32, mr_pool2x2_framemax_b8,
    mr_max_over_frames_b8) take their maxima with fmaxf (v_max_f32 = maxnum), which DROPS a NaN operand: a window or frame column with one NaN
    gives the maximum of the others, where F.max_pool2d / torch.max of the reference propagate the NaN; only a window of nothing but NaN stays
    NaN (mr_maxpool3x3s2_f32: the next test).  An ACCEPTED, documented deviation (INTEGRATION.md section 5, next to the ReLU epilogue's): pinned
    here so that a change shows up."""
    lib = hip_lib
    g = torch.Generator().manual_seed(77)
    # 3x3 stride 2: one NaN inside several windows (a window of nothing but NaN: see the next test)
    x = torch.randn(1, 2, 7, 9, generator=g)
    x[0, 0, 3, 4] = NAN
    want = _nan_expectation(x, lambda t: F.max_pool2d(t, 3, 2, 1))
    o = _out(*want.shape)
    xd = x.to(DEV)
    _lib.check(lib.mr_maxpool3x3s2_f32(xd.data_ptr(), o[1].data_ptr(), 2, 7, 9, _stream()), "mr_maxpool3x3s2_f32")
    assert _intact(o) and not torch.isnan(want).any() and int(torch.isnan(F.max_pool2d(x, 3, 2, 1)).sum()) == 2
    assert torch.equal(o[1].cpu(), want)
    # 2x2 per frame and the maximum over 3 frames: a NaN in one frame / window position, one all-NaN window in every frame
    x = torch.randn(3, 2, 4, 8, generator=g)
    x[1, 0, 1, 2] = NAN
    x[:, 1, 2:4, 4:6] = NAN
    want_pool = _nan_expectation(x, lambda t: F.max_pool2d(t, 2))
    want_max = _nan_expectation(x, lambda t: t.max(0)[0])
    assert int(torch.isnan(want_pool).sum()) == 3 and int(torch.isnan(want_max).sum()) == 4
    xd = x.to(DEV)
    o = _out(*want_pool.shape)
    _lib.check(lib.mr_maxpool2x2_f32(xd.data_ptr(), o[1].data_ptr(), 6, 4, 8, _stream()), "mr_maxpool2x2_f32")
    assert _intact(o) and _same_with_nan(o[1].cpu(), want_pool)
    po, mo = _out(*want_pool.shape), _out(*want_max.shape)
    _lib.check(lib.mr_pool2x2_framemax_f32(xd.data_ptr(), po[1].data_ptr(), mo[1].data_ptr(), 3, 2, 4, 8, _stream()), "mr_pool2x2_framemax_f32")
    assert _intact(po, mo) and _same_with_nan(po[1].cpu(), want_pool) and _same_with_nan(mo[1].cpu(), want_max)
    o = _out(*want_max.shape)
    _lib.check(lib.mr_max_over_frames_f32(xd.data_ptr(), o[1].data_ptr(), 3, want_max.numel(), _stream()), "mr_max_over_frames_f32")
    assert _intact(o) and _same_with_nan(o[1].cpu(), want_max)
    assert not torch.isnan(o[1].cpu()[0, 1, 2]) and bool(torch.isnan(x.max(0)[0][0, 1, 2]))          # dropped here, propagated by torch.max
    # the B8 kernels: (frames * batch, C = 8, H, W) bf16
    x = pp.bf(torch.randn(3, 8, 4, 6, generator=g))
    x[2, 3, 0, 1] = NAN
    x[:, 5, 2:4, 2:4] = NAN
    want_pool = _nan_expectation(x, lambda t: F.max_pool2d(t, 2))
    want_max = _nan_expectation(x, lambda t: t.max(0)[0])
    assert int(torch.isnan(want_pool).sum()) == 3 and int(torch.isnan(want_max).sum()) == 4
    xb = pp.to_b8(x).to(DEV)
    po, fo, mo = _out(3, 1, 2, 3, 8, dtype=torch.bfloat16), _out(1, 1, 4, 6, 8, dtype=torch.bfloat16), _out(1, 1, 4, 6, 8, dtype=torch.bfloat16)
    _lib.check(lib.mr_pool2x2_framemax_b8(xb.data_ptr(), po[1].data_ptr(), fo[1].data_ptr(), 3, 1, 4, 6, _stream()), "mr_pool2x2_framemax_b8")
    _lib.check(lib.mr_max_over_frames_b8(xb.data_ptr(), mo[1].data_ptr(), 3, 24, _stream()), "mr_max_over_frames_b8")
    assert _intact(po, fo, mo)
    assert _same_with_nan(pp.from_b8(po[1].cpu(), 8), want_pool)
    assert _same_with_nan(pp.from_b8(fo[1].cpu(), 8)[0], want_max) and _same_with_nan(pp.from_b8(mo[1].cpu(), 8)[0], want_max)


def test_maxpool3x3s2_window_of_nothing_but_nan_gives_minus_inf_documented_deviation(hip_lib):
    """mr_maxpool3x3s2_f32 starts every window from -inf (the padding of nn.MaxPool2d(3, 2, 1)) and takes fmaxf over the taps inside the image, so
    a window whose every tap is NaN keeps that -inf where F.max_pool2d returns NaN - unlike the other five max kernels, which start from their
    first operand and hand an all-NaN window on as NaN.  Found by this file's first run; an ACCEPTED deviation of the same non-finite class
    (INTEGRATION.md section 5): the stem pools ReLU outputs, which are never NaN (the ReLU epilogue turns NaN into 0).  Pinned here."""
    g = torch.Generator().manual_seed(78)
    x = torch.randn(1, 2, 7, 9, generator=g)
    x[0, 1, 0:2, 0:2] = NAN                                      # the four pixels that are the whole (padded) window of output (0, 0)
    ref = F.max_pool2d(x, 3, 2, 1)
    want = F.max_pool2d(torch.where(torch.isnan(x), torch.tensor(-pp.INF), x), 3, 2, 1)
    assert int((want == -pp.INF).sum()) == 1 and want[0, 1, 0, 0] == -pp.INF and int(torch.isnan(ref).sum()) == 4
    o = _out(*want.shape)
    xd = x.to(DEV)
    _lib.check(hip_lib.mr_maxpool3x3s2_f32(xd.data_ptr(), o[1].data_ptr(), 2, 7, 9, _stream()), "mr_maxpool3x3s2_f32")
    assert _intact(o)
    assert torch.equal(o[1].cpu(), want)
