"""GPU (MI355X): every launch path of csrc/cost_volume.hip that tests/cost_volume_paths.py declares, each case alone.  Outputs are the front of
NaN-filled, guarded allocations; no output may hold a NaN, no guard may be touched, and the library must report the path the case names.

EXACT legs (bit for bit) - the main point:
  * every exact marching case = mr_cost_volume_tiled_f32 on the same inputs (strip / segment / plane-pair decomposition, both fusion kernels);
  * every relaxed fallback (per-pixel depths, D < 6) = the exact entry point;
  * B8 / lean entries: fp32 outputs = the entry that runs the same sad kernel (the relaxed entry; the mode entry for per-pixel depths or
    use_ssim != 1), B8 copies = torch's round-to-nearest-even bf16 of the fp32 single-frame volumes, lean leaves `sfcv` un-finalised exactly as
    cost_volume_finalise expects;
  * sample independence: sample b of a B > 1 launch = the B 1 launch of that sample alone (geometry, planes per wave, TY and nchunk may all
    differ between the two launches - that is the point; it is the whole check of the fusion second-pass case);
  * frame independence (sfcv_mult_mask paths): sfcv[f] of an F > 1 launch = the F 1 launch of frame f alone.
ORACLE leg (every tiled / patch case, one marching anchor per instantiation): oracle.cost_volume with the same options under the bars
tests/test_gpu_kernels.py applies to the options composed (cost_volume_paths.bars), sized so that every cap allows at least one whole entry.

Every exact leg held bit for bit on the MI355X, -0.0 against 0.0 included; no leg had to become a bounded one.  Measured there against the
oracle of the GPU machine's host (worst frame: max |diff| and the fraction of entries beyond the SMALLEST threshold its bars name - 1e-4 for
sfcv, 2e-5 where the composed patch options bring the (2e-5, 1e-3) + (1e-3, 5e-4) bar; validity flips;
for patch cases the mismatch of the cv == 0 pattern) - `pytest -s` prints every threshold of every case:
  dp1_anchor_84x125              sfcv 2.9e-05 (0.0e+00 beyond)  cv 4.0e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  dp2_pixd_kfs_anchor            sfcv 3.4e-05 (0.0e+00 beyond)  cv 5.4e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  dp2_pixd_nokfs_anchor          sfcv 2.7e-05 (0.0e+00 beyond)  cv 4.9e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  dp2_nokfs_anchor               sfcv 2.5e-05 (0.0e+00 beyond)  cv 2.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  dp2_kfs_large_even_rows        sfcv 4.3e-05 (0.0e+00 beyond)  cv 3.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  relaxed_dp2_large_rows0mod3    sfcv 7.2e-05 (0.0e+00 beyond)  cv 5.7e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  relaxed_dp1_rows12_anchor      sfcv 4.5e-05 (0.0e+00 beyond)  cv 4.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  tiled_m0_o0                    sfcv 1.7e-06 (0.0e+00 beyond)  cv 3.3e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m0_o1                    sfcv 2.4e-06 (0.0e+00 beyond)  cv 3.9e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m0_o2                    sfcv 4.6e-06 (0.0e+00 beyond)  cv 3.3e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m0_o3                    sfcv 2.4e-06 (0.0e+00 beyond)  cv 3.9e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m1_o0                    sfcv 5.6e-05 (0.0e+00 beyond)  cv 9.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  tiled_m1_o1                    sfcv 5.7e-05 (0.0e+00 beyond)  cv 1.9e-04 (1.9e-04 beyond 1e-04)  flips 0.0e+00
  tiled_m1_o2                    sfcv 5.6e-05 (0.0e+00 beyond)  cv 9.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  tiled_m1_o3                    sfcv 5.7e-05 (0.0e+00 beyond)  cv 1.9e-04 (1.9e-04 beyond 1e-04)  flips 0.0e+00
  tiled_m2_o0                    sfcv 4.2e-05 (0.0e+00 beyond)  cv 3.9e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m2_o1                    sfcv 5.4e-05 (0.0e+00 beyond)  cv 5.2e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m2_o2                    sfcv 4.2e-05 (0.0e+00 beyond)  cv 3.9e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m2_o3                    sfcv 5.4e-05 (0.0e+00 beyond)  cv 5.2e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m3_o0                    sfcv 1.5e-06 (0.0e+00 beyond)  cv 3.0e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m3_o1                    sfcv 8.3e-07 (0.0e+00 beyond)  cv 5.4e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m3_o2                    sfcv 2.7e-06 (0.0e+00 beyond)  cv 3.0e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  tiled_m3_o3                    sfcv 2.1e-06 (0.0e+00 beyond)  cv 5.4e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  patch5_m0_o0                   sfcv 1.8e-06 (0.0e+00 beyond)  cv 1.2e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m0_o1                   sfcv 8.3e-07 (0.0e+00 beyond)  cv 5.2e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m0_o2                   sfcv 1.9e-06 (0.0e+00 beyond)  cv 1.2e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m0_o3                   sfcv 1.2e-06 (0.0e+00 beyond)  cv 5.2e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m1_o0                   sfcv 2.8e-05 (0.0e+00 beyond)  cv 4.7e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m1_o1                   sfcv 2.6e-05 (1.1e-04 beyond)  cv 2.6e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m1_o2                   sfcv 2.8e-05 (7.1e-05 beyond)  cv 4.7e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m1_o3                   sfcv 2.6e-05 (1.8e-04 beyond)  cv 2.6e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m2_o0                   sfcv 1.8e-05 (0.0e+00 beyond)  cv 1.6e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m2_o1                   sfcv 1.4e-05 (0.0e+00 beyond)  cv 1.9e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m2_o2                   sfcv 1.8e-05 (0.0e+00 beyond)  cv 1.6e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m2_o3                   sfcv 1.5e-05 (0.0e+00 beyond)  cv 1.9e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m3_o0                   sfcv 1.2e-06 (0.0e+00 beyond)  cv 5.5e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m3_o1                   sfcv 1.7e-06 (0.0e+00 beyond)  cv 5.1e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m3_o2                   sfcv 1.9e-06 (0.0e+00 beyond)  cv 5.5e-06 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch5_m3_o3                   sfcv 2.0e-06 (0.0e+00 beyond)  cv 5.1e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch1_m1_o0                   sfcv 1.1e-04 (2.4e-05 beyond)  cv 1.8e-04 (0.0e+00 beyond 2e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch1_m1_o3                   sfcv 1.1e-04 (5.9e-02 beyond)  cv 1.8e-04 (5.1e-04 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch7_m1_o0                   sfcv 1.3e-05 (0.0e+00 beyond)  cv 1.3e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00  cv==0 0.0e+00
  patch7_m1_o3                   sfcv 1.4e-05 (0.0e+00 beyond)  cv 1.4e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00  cv==0 0.0e+00
"""
import ctypes

import pytest
import torch

import cost_volume_paths as cp
import pointwise_paths as pp
from monorec_amd import _lib
from monorec_amd.model import depth_hypotheses, host_geometry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ENTRY_SYMBOL = {"mode": "mr_cost_volume_mode_f32", "tiled": "mr_cost_volume_tiled_f32", "relaxed": "mr_cost_volume_relaxed_f32",
                "b8": "mr_cost_volume_b8_f32", "lean": "mr_cost_volume_b8_lean_f32"}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(elems, guard, dtype=torch.float32):
    """NaN-filled allocation of elems + guard elements; the output is its front (as _hip_cost_volume of tests/test_gpu_kernels.py does)."""
    return torch.full((elems + guard,), float("nan"), device=DEV, dtype=dtype)


def _run(lib, k, entry, batch, pix, depths=None):
    """One launch of `entry` with the options of case `k` on (batch, pix).  Returns dict(cv, sf [, b8]) on the CPU after checking the guards.
    `depths`: the hypothesis ladder (D) when it is not the model's."""
    kf = batch["keyframe"].to(DEV)
    b, _, h, w = kf.shape
    nf, d = len(batch["frames"]), k.d
    frames = [f.to(DEV).contiguous() for f in batch["frames"]]
    kinv, proj = host_geometry(batch["keyframe_intrinsics"], batch["keyframe_pose"], batch["intrinsics"], batch["poses"])
    kinv, proj = kinv.to(DEV), proj.to(DEV)
    depths = (depth_hypotheses((0.33, 0.0025), d) if depths is None else depths).to(DEV).contiguous()
    assert depths.shape == (d,) and depths.dtype == torch.float32
    pixd = None if pix is None else pix.to(DEV).contiguous()
    n, g = b * d * h * w, h * w
    backing = [_guarded(n, g) for _ in range(nf + 1)]
    cv, sf = backing[0][:n].view(b, d, h, w), [t[:n].view(b, d, h, w) for t in backing[1:]]
    fp = (ctypes.c_void_p * nf)(*[f.data_ptr() for f in frames])
    sp = (ctypes.c_void_p * nf)(*[s.data_ptr() for s in sf])
    cw = (ctypes.c_float * 3)(5 / 32, 16 / 32, 11 / 32)
    head = (kf.data_ptr(), fp, nf, kinv.data_ptr(), proj.data_ptr(), depths.data_ptr(), b, d, h, w, 10.0, cw, int(k.use_ssim), None if pixd is None else pixd.data_ptr())
    sym, b8back = ENTRY_SYMBOL[entry], []
    if entry in ("b8", "lean"):
        b8back = [_guarded(n, 8 * g, torch.bfloat16) for _ in range(nf)]
        bp = (ctypes.c_void_p * nf)(*[t.data_ptr() for t in b8back])
        rc = getattr(lib, sym)(*head, cv.data_ptr(), sp, bp, _stream())
    elif entry == "relaxed":
        rc = getattr(lib, sym)(*head, cv.data_ptr(), sp, _stream())
    elif entry == "mode" and k.patch != 3:
        rc = lib.mr_cost_volume_patch_f32(*head, int(k.mult_mask), int(k.patch), cv.data_ptr(), sp, _stream())
    else:
        assert k.patch == 3
        rc = getattr(lib, sym)(*head, int(k.mult_mask), cv.data_ptr(), sp, _stream())
    _lib.check(rc, sym)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[n:]).all()) for t in backing), f"{sym} wrote past the end of an fp32 output"
    assert all(bool(torch.isnan(t[n:].float()).all()) for t in b8back), f"{sym} wrote past the end of a B8 copy"
    out = dict(cv=cv.cpu(), sf=[s.cpu() for s in sf])
    if b8back:
        out["b8"] = [t[:n].view(b, d // 8, h, w, 8).cpu() for t in b8back]
        assert not any(torch.isnan(t.float()).any() for t in out["b8"]), "a B8 copy holds a NaN"
    assert not torch.isnan(out["cv"]).any() and not any(torch.isnan(s).any() for s in out["sf"]), f"{sym} left part of an output unwritten"
    return out


def _same(a, b, what):
    """Bit for bit (as integers: -0.0 != 0.0 here, NaNs are excluded before)."""
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    diff = ai != bi
    assert not bool(diff.any()), (what, int(diff.sum()), float((a - b).abs().max()), diff.nonzero()[:4].tolist())


def _same_outputs(got, want, what, b8=True):
    _same(got["cv"], want["cv"], what + " cv")
    for f, (x, y) in enumerate(zip(got["sf"], want["sf"])):
        _same(x, y, f"{what} sfcv{f}")
    if b8 and "b8" in got and "b8" in want:
        for f, (x, y) in enumerate(zip(got["b8"], want["b8"])):
            assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"{what} B8 copy {f}"


def _oracle_leg(k, got, batch, pix, oracle=None):
    """`oracle`: (cost volume, single-frame volumes) of cp.oracle_of(k, batch, pix) when the caller has them already."""
    ocv, osf = cp.oracle_of(k, batch, pix) if oracle is None else oracle
    bars = cp.bars(k)
    report, ok_all = [], True
    for f in range(k.f):
        ok, mx, fr = cp.measure(got["sf"][f], osf[f], bars["sf"])
        report.append(f"sfcv{f} max {mx:.2e} " + " ".join(f">{t:.0e}: {v:.2e}" for t, v in fr))
        ok_all &= ok
        if k.mult_mask:
            flips = float(((got["sf"][f] == 0).all(1) != (osf[f] == 0).all(1)).float().mean())
            report.append(f"flips{f} {flips:.2e}")
            ok_all &= flips <= bars["flips"]
    ok, mx, fr = cp.measure(got["cv"], ocv, bars["cv"])
    report.append(f"cv max {mx:.2e} " + " ".join(f">{t:.0e}: {v:.2e}" for t, v in fr))
    ok_all &= ok
    flips = float(((got["cv"] == 0).all(1) != (ocv == 0).all(1)).float().mean())
    report.append(f"cv flips {flips:.2e}")
    ok_all &= flips <= bars["flips"]
    if bars["cv_zero"] is not None:
        zero = float(((got["cv"] == 0) != (ocv == 0)).float().mean())
        report.append(f"cv==0 pattern {zero:.2e}")
        ok_all &= zero <= bars["cv_zero"]
    print(f"ORACLE {k.name}: " + "; ".join(report))
    assert ok_all, (k.name, report, bars)
    assert 0.2 < float((got["cv"] != 0).any(1).float().mean()) < 1.0          # not trivially all-invalid


def _exact_legs(lib, k, L, got, batch, pix, depths=None):
    """The bit-for-bit legs of the head of this file that apply to case `k` (launch decision `L`, outputs `got`); returns their names."""
    legs = []
    # -- the exact marching kernels against the tiled kernels
    if k.entry == "mode" and L["family"] == 1:
        _same_outputs(got, _run(lib, k, "tiled", batch, pix, depths), "march vs tiled")
        legs.append("tiled")
    # -- a relaxed entry that falls back to the exact kernels
    if k.entry == "relaxed" and not L["relaxed"]:
        _same_outputs(got, _run(lib, k, "mode", batch, pix, depths), "relaxed fallback vs exact entry")
        legs.append("fallback")
    # -- B8 / lean: the entry that runs the same sad kernel, the rounding of the copies, the un-finalised scratch of lean
    if k.entry in ("b8", "lean"):
        twin = _run(lib, k, "relaxed" if L["family"] == 1 and L["relaxed"] else "mode", batch, pix, depths)
        assert (L["family"] == 1 and L["relaxed"]) == (k.use_ssim == 1 and not k.pixd)
        _same(got["cv"], twin["cv"], "b8 cv vs the fp32 entry")
        for f in range(k.f):
            assert torch.equal(pp.from_b8(got["b8"][f], k.d), pp.bf(twin["sf"][f])), f"B8 copy {f} is not the bf16 rounding of the fp32 volume"
            if k.entry == "b8":
                _same(got["sf"][f], twin["sf"][f], f"b8 sfcv{f} vs the fp32 entry")
            else:
                assert bool((pp.cost_volume_finalise(got["sf"][f]) == twin["sf"][f]).all()), f"lean scratch {f} does not finalise to the fp32 volume"
                assert not torch.equal(got["sf"][f], twin["sf"][f])
        legs.append("twin")
    # -- sample independence
    if k.b > 1:
        for n in range(k.b):
            bn, pn = cp.select_sample(batch, pix, n)
            alone = _run(lib, k, k.entry, bn, pn, depths)
            part = dict(cv=got["cv"][n:n + 1], sf=[s[n:n + 1] for s in got["sf"]])
            if "b8" in got:
                part["b8"] = [t[n:n + 1] for t in got["b8"]]
            _same_outputs(part, alone, f"sample {n} alone")
        legs.append("samples")
    # -- frame independence of the single-frame volumes
    if k.f > 1 and k.mult_mask:
        for f in range(k.f):
            alone = _run(lib, k, k.entry, cp.select_frame(batch, f), pix, depths)
            _same(got["sf"][f], alone["sf"][0], f"frame {f} alone")
            if "b8" in got:
                assert torch.equal(got["b8"][f].view(torch.int16), alone["b8"][0].view(torch.int16)), f"B8 copy of frame {f} alone"
        legs.append("frames")
    return legs


@pytest.mark.parametrize("name", [k.name for k in cp.CASES])
def test_cost_volume_path(hip_lib, name):
    k = cp.BY_NAME[name]
    L = cp.query(hip_lib, k.f, k.b, k.d, k.h, k.w, k.use_ssim, k.pixd, k.mult_mask, k.patch, tiled=k.entry == "tiled", b8=k.entry in ("b8", "lean"),
                 relaxed=k.entry == "relaxed", lean=k.entry == "lean")
    assert cp.launched(L)[:2] == (k.sad, k.fuse)
    batch, pix = cp.operands(k)
    got = _run(hip_lib, k, k.entry, batch, pix)
    legs = _exact_legs(hip_lib, k, L, got, batch, pix)
    if k.oracle:
        _oracle_leg(k, got, batch, pix)
        legs.append("oracle")
    assert legs, name
    print(f"LEGS {name}: {' '.join(legs)}")
