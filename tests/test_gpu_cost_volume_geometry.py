"""GPU (MI355X): every copy of the ray / projection / validity code of csrc/cost_volume.hip on the geometries of tests/cost_volume_geometry.py -
general cameras (all 12 `proj` and all 9 `kinv` entries non-zero, third ray component != 1, different matrices for every sample and frame),
hypotheses behind a source camera, a zero denominator, and samples that fall exactly on pixel centres.  tests/test_cost_volume_geometry.py
shows on the CPU that the geometry of every other cost-volume test cannot see an error in those terms.

The launches are those of tests/test_gpu_cost_volume_paths.py (`_run`: NaN-filled guarded outputs) with its legs: the marching entry bit for
bit against the tiled entry, B8 / lean against their fp32 twins, every sample and every frame alone, and the CPU oracle under the bars of the
options composed (cost_volume_paths.bars; none invented).  `general`, `general_far` and `zero_denominator` run at 48 x 80 (two marching
strips: the seam is inside the image); the copies of the projection code that ran are asserted through the library's launch query - the
tiled kernel, the marching kernels with one and with two hypotheses per wave, the relaxed marching kernel, the patch kernel.
On `exact_integer`, `exact_other` and `planted_zeros` (32 x 64, power-of-two depths given as the ladder and per pixel) the positions are
exact on both sides, so the zero pattern of every volume equals the oracle's with NO entry flipped and equals the closed form
(cost_volume_geometry.exact_valid_map / planted_invalid); where the frame is the keyframe moved by an integer shift the valid entries are 1.
One model-level test: `general` at 64 x 96 through MonoRecModel, fp32 and bf16, against oracle.forward under the bars of tests/test_gpu_model.py.

Measured on the MI355X against the oracle of the GPU machine's host (worst frame: max |diff|, fraction of entries beyond the smallest
threshold the bars name, validity flips) - `pytest -s` prints every threshold of every case:
  general mode_d8                    sfcv 2.8e-05 (0.0e+00 beyond)  cv 4.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general mode_d8_pixd               sfcv 2.5e-05 (0.0e+00 beyond)  cv 3.4e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  general tiled_d8                   sfcv 2.8e-05 (0.0e+00 beyond)  cv 4.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general tiled_d8_pixd              sfcv 2.5e-05 (0.0e+00 beyond)  cv 3.4e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  general mode_d8_p5                 sfcv 1.6e-05 (0.0e+00 beyond)  cv 2.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general mode_d8_pixd_p5            sfcv 1.6e-05 (0.0e+00 beyond)  cv 2.4e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  general mode_d8_p1                 sfcv 9.7e-05 (0.0e+00 beyond)  cv 1.3e-04 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general mode_d32                   sfcv 3.2e-05 (0.0e+00 beyond)  cv 8.1e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general mode_d48                   sfcv 3.3e-05 (0.0e+00 beyond)  cv 7.3e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general mode_d64                   sfcv 4.4e-05 (0.0e+00 beyond)  cv 5.1e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general relaxed_d8                 sfcv 3.7e-05 (0.0e+00 beyond)  cv 6.6e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general b8_d32                     sfcv 3.7e-05 (0.0e+00 beyond)  cv 7.3e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general lean_d32                   sfcv 3.7e-05 (0.0e+00 beyond)  cv 7.3e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far mode_d8                sfcv 2.9e-05 (0.0e+00 beyond)  cv 2.9e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far mode_d8_pixd           sfcv 3.1e-05 (0.0e+00 beyond)  cv 3.1e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  general_far tiled_d8               sfcv 2.9e-05 (0.0e+00 beyond)  cv 2.9e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far tiled_d8_pixd          sfcv 3.1e-05 (0.0e+00 beyond)  cv 3.1e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  general_far mode_d8_p5             sfcv 1.7e-05 (0.0e+00 beyond)  cv 2.1e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far mode_d8_pixd_p5        sfcv 1.6e-05 (0.0e+00 beyond)  cv 1.6e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  general_far mode_d8_p1             sfcv 1.2e-04 (3.3e-05 beyond)  cv 1.2e-04 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far mode_d32               sfcv 4.3e-05 (0.0e+00 beyond)  cv 4.3e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far mode_d48               sfcv 4.2e-05 (0.0e+00 beyond)  cv 4.2e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far mode_d64               sfcv 4.5e-05 (0.0e+00 beyond)  cv 4.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far relaxed_d8             sfcv 4.5e-05 (0.0e+00 beyond)  cv 4.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far b8_d32                 sfcv 5.0e-05 (0.0e+00 beyond)  cv 5.0e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  general_far lean_d32               sfcv 5.0e-05 (0.0e+00 beyond)  cv 5.0e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator mode_d8           sfcv 2.4e-05 (0.0e+00 beyond)  cv 2.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator mode_d8_pixd      sfcv 2.3e-05 (0.0e+00 beyond)  cv 2.3e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  zero_denominator tiled_d8          sfcv 2.4e-05 (0.0e+00 beyond)  cv 2.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator tiled_d8_pixd     sfcv 2.3e-05 (0.0e+00 beyond)  cv 2.3e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  zero_denominator mode_d8_p5        sfcv 1.3e-05 (0.0e+00 beyond)  cv 1.3e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator mode_d8_pixd_p5   sfcv 1.2e-05 (0.0e+00 beyond)  cv 1.2e-05 (0.0e+00 beyond 1e-04)  flips 0.0e+00
  zero_denominator mode_d8_p1        sfcv 9.4e-05 (0.0e+00 beyond)  cv 9.4e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator mode_d32          sfcv 2.5e-05 (0.0e+00 beyond)  cv 2.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator mode_d48          sfcv 3.1e-05 (0.0e+00 beyond)  cv 3.0e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator mode_d64          sfcv 2.9e-05 (0.0e+00 beyond)  cv 2.9e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator relaxed_d8        sfcv 2.5e-05 (0.0e+00 beyond)  cv 2.5e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator b8_d32            sfcv 3.0e-05 (0.0e+00 beyond)  cv 3.0e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
  zero_denominator lean_d32          sfcv 3.0e-05 (0.0e+00 beyond)  cv 3.0e-05 (0.0e+00 beyond 2e-04)  flips 0.0e+00
On the 32 x 64 scenes (exact_integer, exact_other, planted_zeros; every run of each): 0 entries of any zero pattern differ from the oracle's, 0 from
the closed form; the exact kernels' volumes are <= 1.2e-07 from the oracle's and |1 - sfcv| <= 6.0e-08 where the frame is the shifted keyframe,
the relaxed / B8 / lean entries 1.2e-05 (integer shifts) and 2.0e-05 (half-integer shifts); the fused volume is 0 everywhere (frame weight
exactly 0) except at D 48, where 1 - fp32(1 / 47) * 47 = 6e-08 is left as the weight and the volume is valid on 0.82 of the pixels, 1.2e-07 from the oracle's.
The model at 64 x 96: depth 1.2e-06, cv_mask 2.7e-06, no volume entry beyond its bar (fp32); depth 1.6e-03 max / 2.8e-04 mean, fused volume 3.9e-03 (bf16).
Every bit-for-bit leg held.

What the file is worth, measured once: a library with X2 := depth in project(), P[1] and P[4] exchanged in the marching kernels' staged
projection, the `w != 0` clause of their validity logic dropped and the Ki[1] * y term dropped from the patch kernel's halo rays passes all 98
cost-volume tests of tests/test_gpu_cost_volume_paths.py and tests/test_gpu_b8.py; 49 of the 75 tests here fail on it (every test_general_cameras
case, the marching entries of exact_integer, both model tests).
"""
import functools

import pytest
import torch

import cost_volume_geometry as cg
import cost_volume_paths as cp
import pointwise_paths as pp
from monorec_amd import synth
from monorec_amd.model import MonoRecModel
from oracle import monorec_oracle as orc
from test_gpu_cost_volume_paths import _exact_legs, _oracle_leg, _run
from test_gpu_model import BF16_MAX_ERR, BF16_MEAN_ERR, DEV, _check_against, _model, _to_dev

pytestmark = pytest.mark.gpu

RUNS = {(scene, k.name): k for scene in cg.SCENES for k in cg.runs(scene)}


@functools.lru_cache(None)
def _batch(scene):
    return cg.SCENES[scene]()


@functools.lru_cache(None)
def _hypotheses(scene, d, pixd):
    """(ladder for the C entry or None for the model's, per-pixel depths or None, what the oracle takes as cv_depths)."""
    b, _, h, w = _batch(scene)["keyframe"].shape
    if scene in cg.EXACT_SHIFTS:
        ladder = cg.exact_depths(d)
        every = cg.per_pixel(ladder, b, h, w)
        return ladder, (every if pixd else None), every
    pix = synth.make_pixel_depths(b, d, h, w, seed=41) if pixd else None
    return None, pix, pix


@functools.lru_cache(None)
def _oracle(scene, d, patch, pixd):
    """Computed once per (scene, options), shared by the entries, never written to."""
    return orc.cost_volume(_batch(scene), steps=d, patch_size=patch, use_ssim=True, cv_depths=_hypotheses(scene, d, pixd)[2],
                           sfcv_mult_mask=scene != "planted_zeros")


def _launch(lib, scene, k):
    """Query, launch, bit-for-bit legs.  Returns (launch decision, outputs, legs)."""
    L = cp.query(lib, k.f, k.b, k.d, k.h, k.w, k.use_ssim, k.pixd, k.mult_mask, k.patch, tiled=k.entry == "tiled", b8=k.entry in ("b8", "lean"),
                 relaxed=k.entry == "relaxed", lean=k.entry == "lean")
    assert L["status"] == 0
    want_family = "patch" if k.patch != 3 else ("tiled" if k.entry == "tiled" or not k.mult_mask else "march")
    assert cp.FAMILY[L["family"]] == want_family, (k.name, L["family"])
    if want_family == "march":
        assert L["fd"] == 1 and L["relaxed"] == int(k.entry in ("relaxed", "b8", "lean")) and L["dp"] == (2 if k.pixd else 1), (k.name, L)
    ladder, pix, _ = _hypotheses(scene, k.d, k.pixd)
    batch = _batch(scene)
    got = _run(lib, k, k.entry, batch, pix, ladder)
    legs = _exact_legs(lib, k, L, got, batch, pix, ladder)
    if k.entry == "lean":         # `sf` holds the raw costs; the twin leg has shown that they finalise to the relaxed entry's volumes bit for bit
        got = dict(got, sf=[pp.cost_volume_finalise(s) for s in got["sf"]])
    return L, got, legs


def _barred(k):
    """The case whose bars apply: the fp32 outputs of the B8 / lean entries ARE the relaxed entry's (twin leg, bit for bit)."""
    return k._replace(entry="relaxed") if k.entry in ("b8", "lean") else k


def test_every_copy_of_the_projection_code_runs_on_every_geometry(hip_lib):
    for scene in cg.SCENES:
        sad = set()
        for k in cg.runs(scene):
            sad.add(cp.launched(cp.query(hip_lib, k.f, k.b, k.d, k.h, k.w, k.use_ssim, k.pixd, k.mult_mask, k.patch, tiled=k.entry == "tiled",
                                         b8=k.entry in ("b8", "lean"), relaxed=k.entry == "relaxed", lean=k.entry == "lean"))[0])
        print(f"LAUNCHED {scene}: {' '.join(sorted(sad))}")
        assert any(s.startswith("cv_sad_kernel<") for s in sad) and any(s.startswith("cv_sad_patch_kernel<") for s in sad), (scene, sad)
        if scene != "planted_zeros":      # one and two hypotheses per wave (project_batch<1>, <2>), exact and relaxed marching
            assert {"cv_sad_march_kernel<1,0,1,1,0>", "cv_sad_march_kernel<2,1,1,1,0>", "cv_sad_march_kernel<1,0,1,1,1>"} <= sad, (scene, sad)


@pytest.mark.parametrize("scene,name", [key for key in RUNS if key[0] in cg.RANDOM_SCENES])
def test_general_cameras(hip_lib, scene, name):
    k = RUNS[scene, name]
    L, got, legs = _launch(hip_lib, scene, k)
    assert "samples" in legs and "frames" in legs and (k.entry != "mode" or k.patch != 3 or "tiled" in legs) and (k.entry not in ("b8", "lean") or "twin" in legs)
    _, pix, cvd = _hypotheses(scene, k.d, k.pixd)
    _oracle_leg(_barred(k)._replace(name=f"{scene} {name}"), got, _batch(scene), pix, oracle=_oracle(scene, k.d, k.patch, k.pixd))
    if scene == "zero_denominator":
        assert bool((got["sf"][0] == 0).all())
    print(f"LEGS {scene} {name}: {' '.join(legs)} oracle")


@pytest.mark.parametrize("scene,name", [key for key in RUNS if key[0] in cg.EXACT_SHIFTS])
def test_samples_on_pixel_centres(hip_lib, scene, name):
    k = RUNS[scene, name]
    L, got, legs = _launch(hip_lib, scene, k)
    ocv, osf = _oracle(scene, k.d, k.patch, k.pixd)
    bars, br, report = cp.bars(_barred(k)), k.patch // 2 + 1, []
    for f, shift in enumerate(cg.EXACT_SHIFTS[scene]):
        sf = got["sf"][f]
        flipped = int(((sf == 0) != (osf[f] == 0)).sum())
        closed = cg.planted_invalid()[None] if scene == "planted_zeros" else ~cg.exact_valid_map(shift, br)[None]
        off_closed = int(((sf[0] == 0).numpy() != closed).sum())
        ok, mx, fr = cp.measure(sf, osf[f], bars["sf"])
        report.append(f"sfcv{f} flipped {flipped} off the closed form {off_closed} max {mx:.2e} " + " ".join(f">{t:.0e}: {v:.2e}" for t, v in fr))
        assert flipped == 0 and off_closed == 0 and ok, (scene, name, f, shift, report)
        if scene == "exact_integer":                               # the frame is the keyframe moved by the shift: sad 0, volume 1
            inside = torch.from_numpy(~closed[0])
            ok, mx, _ = cp.measure(sf[0][:, inside], torch.ones_like(sf[0][:, inside]), bars["sf"])
            report.append(f"|1 - sfcv{f}| {mx:.2e}")
            assert ok and bool(inside.any()), (scene, name, f, shift, report)
    flipped = int(((got["cv"] == 0) != (ocv == 0)).sum())
    ok, mx, fr = cp.measure(got["cv"], ocv, bars["cv"])
    report.append(f"cv flipped {flipped} valid {float((got['cv'] != 0).float().mean()):.2f} max {mx:.2e} " + " ".join(f">{t:.0e}: {v:.2e}" for t, v in fr))
    print(f"ORACLE {scene} {name}: " + "; ".join(report))
    assert flipped == 0 and ok, (scene, name, report)
    if scene != "planted_zeros":          # a pixel of the fused volume is valid only where some frame is
        some = torch.from_numpy(cg.exact_valid_map(cg.EXACT_SHIFTS[scene][0], br))
        for shift in cg.EXACT_SHIFTS[scene][1:]:
            some = some | torch.from_numpy(cg.exact_valid_map(shift, br))
        assert not bool((got["cv"][0] != 0).any(0)[~some].any())
    print(f"LEGS {scene} {name}: {' '.join(legs)} oracle")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_general_cameras_through_the_model(hip_lib, bf16):
    batch = cg.general(2, 64, 96)
    if bf16:
        model = MonoRecModel(cv_depth_steps=8, hip_in_flight=1, hip_bf16=True)
        sd = synth.seeded_state_dict(model.state_dict(), seed=0)
        model.load_state_dict(sd)
        model = model.to(DEV).eval()
    else:
        model, sd = _model(8, graph=False)
    with torch.no_grad():
        out = model(_to_dev(batch))
        out = {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in out.items() if k in
               ("result", "cv_mask", "predicted_inverse_depths", "image_features", "cost_volume", "single_frame_cvs")}
    torch.cuda.synchronize()
    ref = orc.forward(sd, batch, cv_depth_steps=8)
    assert out["result"].shape == (2, 1, 64, 96) and 0.2 < float((ref["cost_volume"] != 0).any(1).float().mean()) < 1.0
    if not bf16:
        _check_against(out, ref, "general 64x96")
        return
    err = (out["result"] - ref["result"]).abs()
    cverr = float((out["cost_volume"] - ref["cost_volume"]).abs().max())
    print("ORACLE general 64x96 bf16: result max|err| %.3e mean %.3e; cost volume max %.3e" % (err.max(), err.mean(), cverr))
    assert torch.isfinite(out["result"]).all()
    assert err.max().item() <= BF16_MAX_ERR and err.mean().item() <= BF16_MEAN_ERR and cverr < 5e-2
