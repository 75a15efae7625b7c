"""Host side (no GPU): the geometries of tests/cost_volume_geometry.py and its restatement of the reference's projection.

  * the restated grid equals the CPU oracle's `stages["grid"]` BIT FOR BIT (rays and projection as k-ascending fp32 chains, true
    divisions) on make_batch and on every new geometry - on whichever CPU runs the suite.  Whether that CPU's matmul fuses the
    multiply-adds is probed first on other data (cost_volume_geometry.host_fuses: Intel hosts do, as the kernels; MKL on AMD EPYC rounds
    product and sum separately - there the oracle's grid is one ulp off the kernels' on about a third of the entries, inside every bar);
  * both forms of the validity test - grid_sample's four-term chain and the marching kernels' logic - equal the oracle's `valid`;
  * the conditions that keep tests/test_gpu_cost_volume_geometry.py from being vacuous, on the oracle alone;
  * teeth: four mutations of the restatement (r2 := 1, X2 := depth, the Ki[1] * y term dropped, P[1] and P[4] exchanged) change the grid of
    `general`, and NONE of them changes a bit on make_batch (UNSEEN_ON_MAKE_BATCH) - which is why these geometries exist; the
    zero-weight clauses of the logic form decide only where a sample falls exactly on a pixel centre."""
import functools

import numpy as np
import pytest
import torch

import cost_volume_geometry as cg
import cost_volume_paths as cp
from monorec_amd import synth
from oracle import monorec_oracle as orc

D = 8
UNSEEN_ON_MAKE_BATCH = ("r2_one", "x2_depth", "drop_ki1", "swap_p1_p4")         # every one of them


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(None)
def _scene(name, pixd=False, patch=3):
    """(batch, hypotheses handed to the restatement, oracle outputs, oracle stages) of a scene at D hypotheses."""
    batch = synth.make_batch(2, cg.H_GENERAL, cg.W_GENERAL, 2, seed=5) if name == "make_batch" else cg.SCENES[name]()
    b, _, h, w = batch["keyframe"].shape
    if name in cg.EXACT_SHIFTS:
        depths = cg.exact_depths(D)
        cvd = cg.per_pixel(depths, b, h, w)
        given = cvd if pixd else depths
    else:
        cvd = synth.make_pixel_depths(b, D, h, w, seed=41) if pixd else None
        given = cvd if pixd else orc.depth_hypotheses(0.33, 0.0025, D)
    stages = {}
    cv, sf = orc.cost_volume(batch, steps=D, patch_size=patch, stages=stages, cv_depths=cvd, sfcv_mult_mask=name != "planted_zeros")
    stages = {k: torch.stack(v) for k, v in stages.items()}
    return batch, given, (cv, sf), stages


ALL_SCENES = ("make_batch",) + tuple(cg.SCENES)


@pytest.mark.parametrize("pixd", [False, True], ids=["ladder", "pixd"])
@pytest.mark.parametrize("name", ALL_SCENES)
def test_restated_grid_equals_the_oracle_bit_for_bit(name, pixd):
    batch, given, _, stages = _scene(name, pixd)
    grid, _ = cg.restated(batch, given, fused=cg.host_fuses())
    want = stages["grid"].numpy()
    assert grid.shape == want.shape and not np.isnan(want).any()
    diff = _bits(grid) != _bits(want)
    assert not diff.any(), (name, int(diff.sum()), grid.size)


@pytest.mark.parametrize("patch", [3, 5, 1])
@pytest.mark.parametrize("name", ALL_SCENES)
def test_both_validity_forms_equal_the_oracle(name, patch):
    batch, _, _, stages = _scene(name, False, patch)
    b, _, h, w = batch["keyframe"].shape
    br = patch // 2 + 1
    grid = stages["grid"].numpy()
    want = stages["valid"].numpy()[:, :, 0] != 0
    for n in range(b):
        for f in range(grid.shape[1]):
            chain = cg.pixel_valid(cg.valid_fma(grid[n, f], h, w, br), h, w, br)
            logic = cg.pixel_valid(cg.valid_bool(grid[n, f], h, w, br), h, w, br)
            assert (chain == want[n, f]).all() and (logic == want[n, f]).all(), (name, n, f, int((chain != want[n, f]).sum()), int((logic != want[n, f]).sum()))


def test_the_hosts_matmul_is_a_k_ascending_chain_and_both_forms_see_every_mutation():
    print("this host's torch.matmul fuses its multiply-adds:", cg.host_fuses())
    batch, given, _, _ = _scene("general")
    fused, plain = cg.restated(batch, given, fused=True)[0], cg.restated(batch, given, fused=False)[0]
    assert (_bits(fused) != _bits(plain)).any() and float(np.abs(fused - plain).max()) < 1e-4          # the two forms differ, in the last bits
    for m in cg.MUTATIONS:
        for f in (True, False):
            assert (_bits(cg.restated(batch, given, mutate=m, fused=f)[0]) != _bits(fused if f else plain)).any(), (m, f)


def test_general_fills_every_matrix_entry():
    for name in ("general", "general_far"):
        kinv, proj = cg.host_matrices(cg.SCENES[name]())
        assert np.abs(proj).min() > 1e-5, (name, np.abs(proj).min())
        assert (kinv[-1] != 0).all(), kinv[-1]                                  # the K @ R sample
        assert len({proj[n, f].tobytes() for n in range(2) for f in range(2)}) == 4 and kinv[0].tobytes() != kinv[1].tobytes()
    kinv, proj = cg.host_matrices(synth.make_batch(2, cg.H_GENERAL, cg.W_GENERAL, 2, seed=5))
    assert (np.abs(proj[..., [1, 4, 8, 9]]) < 1e-6).all() and (kinv[:, [1, 3, 6, 7]] == 0).all()         # what every other test runs on


@pytest.mark.parametrize("name,lo,hi", [("general", 0.2, 1.0), ("general_far", 0.2, 1.0), ("zero_denominator", 0.3, 0.7)])
def test_share_of_pixels_with_a_valid_fused_volume(name, lo, hi):
    (cv, _) = _scene(name)[2]
    share = float((cv != 0).any(1).float().mean())
    print(f"{name}: fused volume valid on {share:.3f} of the pixels")
    assert lo < share < hi


def test_general_far_puts_hypotheses_behind_a_source_camera():
    batch, given, _, _ = _scene("general_far")
    near, _ = _scene("general")[:2]
    pts_behind = {}
    for name, bt in (("general_far", batch), ("general", near)):
        b, _, h, w = bt["keyframe"].shape
        coord = orc.pixel_grid(h, w)
        worst = 0.0
        for n in range(b):
            rays = torch.inverse(bt["keyframe_intrinsics"][n]).unsqueeze(0)[:, :3, :3] @ coord
            pts = torch.cat([given.view(D, 1, 1) * rays, torch.ones(D, 1, h * w)], 1)
            for f in range(len(bt["frames"])):
                pc = torch.matmul(orc.projection_matrix(bt["intrinsics"][f][n], bt["poses"][f][n], bt["keyframe_pose"][n]), pts)
                worst = max(worst, float((pc[:, 2] <= 0).float().mean()))
        pts_behind[name] = worst
    print("largest share of points with pcz <= 0 in one (sample, frame):", pts_behind)
    assert pts_behind["general_far"] >= 0.05 and pts_behind["general"] == 0.0


def test_zero_denominator_in_the_oracle():
    batch, given, (cv, sf), stages = _scene("zero_denominator")
    _, proj = cg.host_matrices(batch)
    assert (proj[:, 0, 8:11] == 0).all() and (proj[:, 0, 11] == np.float32(-1e-7)).all()
    _, pcz = cg.restated(batch, given, fused=cg.host_fuses())
    assert ((pcz[:, 0] + np.float32(1e-7)) == 0).all() and ((pcz[:, 1] + np.float32(1e-7)) != 0).all()
    grid = stages["grid"]
    assert bool((grid[:, 0].abs() == 2).all()) and bool((grid[:, 0] == 2).any()) and bool((grid[:, 0] == -2).any())
    assert bool((sf[0] == 0).all()) and not torch.isnan(cv).any() and not any(torch.isnan(s).any() for s in sf)
    assert bool((sf[1] != 0).any())
    # claim 2 of the kernel header: through the three-operation constant division the infinite quotient becomes a NaN and the clamp leaves -2
    # where the reference leaves +-2; every tap is outside the image either way
    fast, _ = cg.restated(batch, given, division=cg.div_const, fused=cg.host_fuses())
    assert (fast[:, 0] == -2).all() and (_bits(fast[:, 1]) == _bits(grid[:, 1].numpy())).all()
    b, _, h, w = batch["keyframe"].shape
    for g in (fast[:, 0], grid[:, 0].numpy()):
        u = cg.unnormalise(g, h, w)
        assert ((u["x0"] + 1 < 0) | (u["x0"] >= w)).all() and ((u["y0"] + 1 < 0) | (u["y0"] >= h)).all()
        assert not cg.valid_fma(g, h, w).any() and not cg.valid_bool(g, h, w).any()


@pytest.mark.parametrize("name", ["general", "general_far", "make_batch"])
def test_constant_division_sequence_equals_true_division_on_finite_quotients(name):
    batch, given, _, _ = _scene(name)
    slow, _ = cg.restated(batch, given, fused=cg.host_fuses())
    fast, _ = cg.restated(batch, given, division=cg.div_const, fused=cg.host_fuses())
    assert (_bits(slow) == _bits(fast)).all()


@pytest.mark.parametrize("patch", [3, 5, 1])
@pytest.mark.parametrize("name", ["exact_integer", "exact_other"])
def test_pixel_exact_lands_where_intended_and_is_valid_by_the_closed_form(name, patch):
    batch, _, (cv, sf), stages = _scene(name, False, patch)
    h, w = cg.H_EXACT, cg.W_EXACT
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for f, (kx, ky) in enumerate(cg.EXACT_SHIFTS[name]):
        u = cg.unnormalise(stages["grid"][0, f].numpy(), h, w)
        assert (u["sx"] == np.clip(x + kx, -0.5 * w - 0.5, 1.5 * w - 0.5)).all() and (u["sy"] == np.clip(y + ky, -0.5 * h - 0.5, 1.5 * h - 0.5)).all()
        want = cg.exact_valid_map((kx, ky), patch // 2 + 1)
        assert ((stages["valid"][0, f, 0].numpy() != 0) == want).all(), (name, f)
        assert ((sf[f][0] != 0).numpy() == want[None]).all(), (name, f)                                  # no 1 - 2 sad is 0 by accident
        if name == "exact_integer":
            assert want.any() and float((sf[f][0][:, torch.from_numpy(want)] - 1).abs().max()) <= 1e-6   # the frame IS the keyframe there
    assert [bool(cg.exact_valid_map(s, 2).any()) for s in cg.OTHER_SHIFTS] == [True, True, False]
    assert bool((cv == 0).all())          # equal costs at every depth: the frame weight 1 - (sum_d e - 1) / (D - 1) is exactly 0 (monorec_model.py:257-269)


def test_planted_zeros_make_both_clauses_decide():
    batch, _, (cv, sf), stages = _scene("planted_zeros")
    warped, kf = stages["warped"][0][:, 0], batch["keyframe"][0]                  # (D, 3, H, W)
    assert bool((warped == batch["frames"][0][0]).all())                           # shift (0, 0): the samples ARE the frame's pixels
    nonzero, equal = (warped != 0).any(1), (warped == kf).all(1)
    for y, x in cg.PLANTED_PIXELS_BOTH:
        assert not bool(nonzero[:, y, x].any()) and bool(equal[:, y, x].all())     # kept by the second clause alone
    for y, x in cg.PLANTED_PIXELS_FRAME:
        assert not bool(nonzero[:, y, x].any()) and not bool(equal[:, y, x].any())  # dropped
    assert ((~(nonzero | equal)).numpy() == cg.planted_invalid()[None]).all()
    assert ((sf[0][0] == 0).numpy() == cg.planted_invalid()[None]).all()           # sfcv_mult_mask=False: no border frame in the single-frame volume


def test_mutations_are_seen_on_general_and_unseen_on_make_batch():
    seen = {}
    for name in ("make_batch", "general", "general_far"):
        batch, given, _, stages = _scene(name)
        want = _bits(stages["grid"].numpy())
        seen[name] = {m: int((_bits(cg.restated(batch, given, mutate=m, fused=cg.host_fuses())[0]) != want).sum()) for m in cg.MUTATIONS}
    print("grid entries a mutation changes:", seen)
    assert all(seen["general"][m] > 0 and seen["general_far"][m] > 0 for m in cg.MUTATIONS), seen
    # the record this work rests on: the geometry every other cost-volume test uses sees none of them
    assert tuple(m for m in cg.MUTATIONS if seen["make_batch"][m] == 0) == UNSEEN_ON_MAKE_BATCH, seen


def test_zero_weight_clauses_decide_only_on_pixel_centres():
    def flips(name, patch=3):
        batch, _, _, stages = _scene(name, False, patch)
        b, _, h, w = batch["keyframe"].shape
        grid, br, n = stages["grid"].numpy(), patch // 2 + 1, []
        for s in range(b):
            for f in range(grid.shape[1]):
                full = cg.pixel_valid(cg.valid_bool(grid[s, f], h, w, br), h, w, br)
                bare = cg.pixel_valid(cg.valid_bool(grid[s, f], h, w, br, zero_weight_clauses=False), h, w, br)
                n.append(int((full != bare).sum()))
        return n
    for name in ("make_batch", "general", "general_far", "zero_denominator"):
        assert flips(name) == [0, 0, 0, 0], name
    got = dict(zip(cg.INTEGER_SHIFTS, flips("exact_integer")))
    print("pixels the zero-weight clauses decide, by shift:", got)
    assert got[(0, 0)] == 0 and got[(-1, 2)] > 0 and got[(1, -1)] > 0 and got[(3, -3)] > 0      # kx = -1 (e != 0 ... w != 0) and ky = -1 (s, n)
    assert flips("exact_other") == [0, 0, 0]                                                    # half-integer: both weights one half


def test_the_gpu_runs_reach_every_copy_of_the_projection_code():
    """By the restated launch rule (tests/test_cost_volume_paths.py pins it on the library): the tiled kernel's project(), the marching
    kernels' staged projection for one and for two hypotheses per wave (compile-time constant division), the patch kernel."""
    for scene in cg.SCENES:
        sad = {cp.launched(cp.rule_of(k))[0] for k in cg.runs(scene)}
        assert any(s.startswith("cv_sad_kernel<") for s in sad) and any(s.startswith("cv_sad_patch_kernel<") for s in sad), (scene, sad)
        if scene != "planted_zeros":
            assert {"cv_sad_march_kernel<1,0,1,1,0>", "cv_sad_march_kernel<2,1,1,1,0>", "cv_sad_march_kernel<1,0,1,1,1>"} <= sad, (scene, sad)
    assert cp.march_geometry(2, 2, D, cg.H_GENERAL, cg.W_GENERAL, 1)["strips"] == 2            # the strip seam is inside the image
