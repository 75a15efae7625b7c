"""The TSDF ray-cast without a device: the two C entries' declarations and argument checks, the runner's new config keys, and the numpy
restatement (tests/tsdf_render_ref.py) held against the analytic scene of tests/tsdf_fusion_ref.py - it hits what the scene shows, at
the scene's depth, and the skipping rule spares work without changing a depth."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tsdf_fusion_ref as ref
import tsdf_render_ref as rref
from monorec_amd import _lib, tsdf_fusion as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mr_tsdf_skip_grid_u8", "mr_tsdf_render_f32")
H, W = 24, 40
RANGE = dict(t_min=0.5, t_max=6.0, step=0.06)


# ------------------------------------------------------------------------------------------ C entries
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header) and name in _lib.ABI and hasattr(hip_lib, name)
        assert any(f"`{name}`" in line for line in table), name
    assert [len(_lib.ABI[n][1]) for n in ENTRIES] == [8, 18]
    assert int(re.search(r"#define MR_TSDF_BRICK (\d+)", header).group(1)) == _lib.MR_TSDF_BRICK == tf.BRICK == rref.BRICK
    assert _lib.MR_TSDF_BRICK in (4, 8)


def test_ray_view_mirrors_the_header():
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    body = re.search(r"typedef struct mr_tsdf_ray_view \{(.*?)\} mr_tsdf_ray_view;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|uint8_t)\s*(\*?)\s*([^;]+);", body, re.M)
    size, names = 0, []
    for kind, pointer, declared in fields:
        for name in declared.split(","):
            name = name.strip()
            count = int(re.search(r"\[(\d+)\]", name).group(1)) if "[" in name else 1
            each = 8 if pointer else 4
            size = (size + each - 1) // each * each + each * count
            names.append(name.split("[")[0])
    assert names == [f[0] for f in _lib.TsdfRayView._fields_] == ["m", "fx", "fy", "cx", "cy", "depth", "normal", "colour"]
    assert ctypes.sizeof(_lib.TsdfRayView) == size == 88
    assert _lib.TsdfRayView.depth.offset == 64 and _lib.TsdfRayView.colour.offset == 80


def test_entries_reject_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    tsdf, weight, colour, bricks, depth, normal, image = (base + 4096 * i for i in range(7))
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def grid(t=tsdf, w=weight, nx=8, ny=4, nz=2, min_weight=0.0, b=bricks):
        return hip_lib.mr_tsdf_skip_grid_u8(t, w, nx, ny, nz, min_weight, b, None)

    def one_view(fx=30.0, fy=30.0, d=depth, n=normal, c=image):
        view = _lib.TsdfRayView()
        view.m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        view.fx, view.fy, view.cx, view.cy = fx, fy, 3.5, 1.5
        view.depth, view.normal, view.colour = d, n, c
        return view

    def render(t=tsdf, w=weight, c=colour, nx=8, ny=4, nz=2, o=origin, voxel=0.1, min_weight=0.0, b=bricks, views="one", count=None,
               h=4, width=8, t_min=0.5, t_max=2.0, step=0.1, **view):
        if views == "one":
            views = (_lib.TsdfRayView * 1)(one_view(**view))
        elif views == "nine":
            views = (_lib.TsdfRayView * 9)(*[one_view(**view) for _ in range(9)])
        n = count if count is not None else (len(views) if views is not None else 1)
        return hip_lib.mr_tsdf_render_f32(t, w, c, nx, ny, nz, o, voxel, min_weight, b, views, n, h, width, t_min, t_max, step, None)

    huge = [dict(nx=1 << 20, ny=1 << 20, nz=1), dict(nx=1 << 14, ny=1 << 13, nz=1 << 13), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)]
    volume = [dict(t=None), dict(w=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(t=tsdf + 2), dict(w=weight + 1), dict(min_weight=nan)] + huge
    for kw in volume:
        assert grid(**kw) == -1, ("grid", kw)
        assert render(**kw) == -1, ("render", kw)
    assert grid(b=None) == -1
    cases = [dict(c=colour + 2), dict(o=None), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=nan),
             dict(views=None), dict(count=0), dict(count=-1), dict(views="nine"), dict(d=None), dict(d=depth + 2), dict(n=normal + 1),
             dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=nan), dict(h=0), dict(width=0), dict(h=-3),
             dict(step=0.0), dict(step=-0.1), dict(step=nan), dict(t_min=-0.5), dict(t_min=nan), dict(t_max=0.25), dict(t_max=nan),
             dict(t_max=inf), dict(t_min=inf, t_max=inf), dict(t_min=0.0, t_max=2.0, step=1e-6), dict(t_min=0.0, t_max=1048576.5, step=1.0),
             dict(t_min=1000.0, t_max=1000.0, step=1e-12)]
    for kw in cases:
        assert render(**kw) == -1, ("render", kw)
    assert b"argument" in hip_lib.mr_error_string(-1).lower()


# ------------------------------------------------------------------------------------------ the runner's keys
def test_fusion_settings_accept_the_new_keys_and_reject_other_metrics():
    base = {"max_d": 30}
    plain = tf.fusion_settings(base)
    assert plain["fused_metrics"] == [] and plain["render_dir"] is None
    assert {k: v for k, v in plain.items() if k not in ("fused_metrics", "render_dir")} == dict(
        voxel_size=0.1, trunc=0.5, bounds=None, max_bytes=8 << 30, fuse_batch=4, file_name="tsdf.ply", mesh_file_name=None, save_volume=None)
    names = ["abs_rel_sparse_onlyvalid_metric", "a1_sparse_onlyvalid_metric", "rmse_log_sparse_onlyvalid_metric"]
    got = tf.fusion_settings(dict(base, fused_metrics=names, render_dir="views"))
    assert got["fused_metrics"] == names and got["render_dir"] == "views"
    assert sorted(tf.FUSED_METRICS) == sorted(f"{b}_sparse_onlyvalid_metric" for b in ("a1", "a2", "a3", "rmse", "rmse_log", "abs_rel", "sq_rel"))
    for bad in (["abs_rel_sparse_metric"], ["a1_sparse_onlydynamic_metric"], ["abs_rel_metric"], ["nothing"], "abs_rel_sparse_onlyvalid_metric", [3]):
        with pytest.raises(ValueError, match="onlyvalid"):
            tf.fusion_settings(dict(base, fused_metrics=bad))
    with pytest.raises(ValueError, match="onlyvalid"):                      # before a model or a dataset is built: neither is in this config
        tf.Fusion(dict(base, fused_metrics=["a1_sparse_metric"]))


# ------------------------------------------------------------------------------------------ the restatement on the analytic scene
@functools.lru_cache(maxsize=None)
def _fused(name, focal):
    k = ref.INTRINSICS_30 if focal == 30 else ref.INTRINSICS_60
    frames = ref.make_frames(k)
    vol = ref.new_volume(**(ref.SMALL if name == "small" else ref.WIDE))
    for pose, depth, colour in frames[:10]:
        ref.integrate(vol, ref.world_to_camera(pose), k, depth, colour)
    return vol, frames, k


@functools.lru_cache(maxsize=None)
def _view(name, focal, pose):
    vol, frames, k = _fused(name, focal)
    return rref.render(vol, frames[pose][0], k, H, W, bricks=rref.brick_flags(vol, 0.0), **RANGE)


def test_brick_flags_have_the_halo_on_the_plus_side():
    vol = ref.new_volume((17, 9, 8), (0, 0, 0), 0.1, 0.3, colour=False)
    vol["weight"][...] = 1
    assert not rref.brick_flags(vol, brick=8).any() and rref.brick_flags(vol, brick=8).shape == (1, 2, 3)
    assert rref.brick_flags(vol, brick=4).shape == (2, 3, 5) and rref.brick_flags(vol).shape == rref.brick_flags(vol, brick=rref.BRICK).shape
    vol["tsdf"][0, 8, 16] = -0.5                                           # the first voxel of brick (2, 1, 0) closes bricks 1 and 0 along x, y
    assert rref.brick_flags(vol, brick=8)[0].tolist() == [[0, 1, 1], [0, 1, 1]]
    assert rref.brick_flags(vol, brick=4)[0].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1]] and not rref.brick_flags(vol, brick=4)[1].any()
    assert not rref.brick_flags(vol, min_weight=1.0, brick=8).any()
    vol["tsdf"][0, 8, 16], vol["tsdf"][7, 7, 15] = 1.0, -0.0
    assert not rref.brick_flags(vol, brick=8).any()                        # -0 is not negative
    vol["tsdf"][7, 7, 15] = -1e-3
    assert rref.brick_flags(vol, brick=8)[0].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert rref.brick_flags(vol, brick=4).sum() == 1 and rref.brick_flags(vol, brick=4)[1, 1, 3] == 1


@pytest.mark.parametrize("name,focal,least", [("small", 30, 0.20), ("wide", 30, 0.45), ("small", 60, 0.65)])
def test_the_restatement_sees_the_scene(name, focal, least):
    vol, frames, k = _fused(name, focal)
    for pose in (0, 5, 9):
        got = _view(name, focal, pose)
        share = float(got["hit"].mean())
        scene = rref.scene_depth(frames[pose][0], k, H, W)
        both = got["hit"] & (scene > 0)
        error = np.abs(got["depth"].astype(np.float64) - scene)[both]
        print(f"{name} f={focal} pose {pose}: hit share {share:.3f}, |depth - scene| median {np.median(error) * 1000:.2f} mm max {error.max():.3f} m, "
              f"cells {got['evaluations']} -> {got['brick_evaluations']}")
        assert share >= least and both.sum() > 0.9 * got["hit"].sum()
        assert np.median(error) < 0.01
        assert np.array_equal(got["hit"], got["depth"] > 0)
        # the skipping rule: the same depth bit for bit, nothing skipped that could have mattered, and work spared
        assert np.array_equal(got["depth"], got["brick_depth"]) and got["skipped_negative"] == 0
        assert got["brick_evaluations"] < got["evaluations"]
        # unit normals that face the camera, colours from the fused images
        n = got["normal"][got["hit"]]
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1).max() < 1e-6 and not got["normal"][~got["hit"]].any()
        assert np.median(n @ frames[pose][0][:3, 2]) < -0.5
        assert got["colour"][got["hit"]].max() > 100 and not got["colour"][~got["hit"]].any()
    away = _view(name, focal, 10)
    assert not away["hit"].any() and not away["depth"].any() and away["evaluations"] == 0


def test_a_ray_that_leaves_through_a_back_face_ends():
    vol = rref.slab_volume()
    bricks = rref.brick_flags(vol)
    front = rref.render(vol, rref.slab_pose(0.9), ref.INTRINSICS_60, 23, 37, 0.0, 3.0, 0.06, bricks=bricks)
    inside = rref.render(vol, rref.slab_pose(1.4), ref.INTRINSICS_60, 23, 37, 0.0, 3.0, 0.06, bricks=bricks)
    assert front["hit"].mean() > 0.5 and np.abs(front["depth"][front["hit"]] - (1.21 - 0.9)).max() < 0.06      # the first slab's front face
    assert not inside["hit"].any()                                         # not the second slab
    for got in (front, inside):
        assert np.array_equal(got["depth"], got["brick_depth"]) and got["skipped_negative"] == 0


def test_sample_count_follows_the_rounded_t():
    assert rref.sample_count(0.5, 6.0, 0.06) == 92 and rref.sample_count(0.0, 0.0, 1.0) == 1 and rref.sample_count(1.0, 2.0, 0.25) == 5


# ------------------------------------------------------------------------------------------ the clip to the box, restated
def _existing_views():
    """(what, volume, pose, intrinsics, h, w, (t_min, t_max, step), min_weight) of every view test_gpu_tsdf_render.py had before
    rref.CLIP_CASES: the fused scene from the arc, the cameras inside and behind, the slabs, the steps and min_weights, the eight views."""
    views = []
    for name, focal in (("small", 30), ("small", 60), ("wide", 30)):
        vol, frames, k = _fused(name, focal)
        for size in ((24, 40), (23, 37)):
            views += [(f"{name}-{focal}-{p}-{size[0]}", vol, frames[p][0], k, *size, tuple(RANGE.values()), 0.0) for p in (0, 5, 9, 10)]
    vol, frames, k = _fused("small", 60)
    for which, pose, t_min, t_max in (("inside", rref.inside_pose(), 0.0, 3.0), ("behind", rref.behind_pose(), 0.0, 3.0), ("inside", rref.inside_pose(), 0.13, 0.9)):
        views.append((f"{which}-{t_min}", vol, pose, k, 23, 37, (t_min, t_max, 0.03), 0.0))
    for voxels in (0.5, 1.0, 2.5):
        views += [(f"step-{voxels}-{mw}", vol, frames[5][0], k, 23, 37, (0.5, 6.0, float(np.float32(0.06 * voxels))), mw) for mw in (0.0, 2.0)]
    for z in (0.9, 1.4):
        views.append((f"slab-{z}", rref.slab_volume(), rref.slab_pose(z), ref.INTRINSICS_60, 23, 37, (0.0, 3.0, 0.06), 0.0))
    vol, frames, _ = _fused("wide", 30)
    for j, p in enumerate((0, 2, 4, 5, 7, 9, 10, 3)):
        views.append((f"eight-{j}", vol, frames[p][0], ref.INTRINSICS_30 if j % 2 == 0 else ref.INTRINSICS_60, 23, 37, tuple(RANGE.values()), 0.0))
    return views


def _clip_views():
    for case in rref.CLIP_CASES:
        vol, pose, k, march = rref.case_inputs(case)
        yield case["id"], vol, pose, k, rref.CLIP_H, rref.CLIP_W, march, 0.0


@functools.lru_cache(maxsize=None)
def _case(case_id):
    """(inputs, the full march, the exact clip) of a CLIP_CASES entry."""
    case = next(c for c in rref.CLIP_CASES if c["id"] == case_id)
    vol, pose, k, march = rref.case_inputs(case)
    size = (rref.CLIP_H, rref.CLIP_W)
    return (vol, pose, k, march), rref.render(vol, pose, k, *size, *march), rref.clip_range(vol, pose, k, *size, *march, exact=True)


def _spare(full, k_lo, k_hi):
    """The samples to spare of the hit rays: min over them of (hit_k - 1) - k_lo and of k_hi - hit_k; None without a hit."""
    hit = full["hit"]
    return (int((full["hit_k"] - 1 - k_lo)[hit].min()), int((k_hi - full["hit_k"])[hit].min())) if hit.any() else None


def test_the_clip_keeps_every_sample_the_full_march_visits_in_the_volume():
    """`clip_to_box` is only an optimisation if no sample it drops could have been valid.  The restated clip (rref.clip_range, fp32,
    operation by operation) against the march that visits every sample: for every ray of every CLIP_CASES entry and of every view the
    GPU tests had before them, the first and the last sample at which the ray, still marching, was inside the volume lie in
    [k_lo, k_hi].  The older views never come near: under an exact clip (no slack, no extra sample) every hit of theirs has a sample
    to spare on both sides, under the kernel's clip at least 3 - the whole margin could have been deleted without a test failing.
    In CLIP_CASES the exact clip has 0 to spare on either side (the next test)."""
    old_exact, old_kernel, count = [], [], 0
    for source, views in (("old", _existing_views()), ("new", _clip_views())):
        for what, vol, pose, k, h, w, march, min_weight in views:
            full = rref.render(vol, pose, k, h, w, *march, min_weight)
            k_lo, k_hi = rref.clip_range(vol, pose, k, h, w, *march)
            seen = full["first_in"] >= 0
            assert (k_lo[seen] <= full["first_in"][seen]).all() and (full["last_in"][seen] <= k_hi[seen]).all(), what
            assert (k_lo >= 0).all() and (k_hi >= -1).all() and (k_hi <= rref.sample_count(*march) - 1).all(), what
            count += int(seen.sum())
            if source == "old" and full["hit"].any():
                old_kernel.append(_spare(full, k_lo, k_hi))
                old_exact.append(_spare(full, *rref.clip_range(vol, pose, k, h, w, *march, exact=True)))
    print(f"{count} rays with a sample in the volume; the older views' hits spare at least {np.min(old_kernel, axis=0)} samples under the "
          f"kernel's clip and {np.min(old_exact, axis=0)} under an exact one")
    assert count > 20000 and np.min(old_kernel) >= 3 and np.min(old_exact) >= 1


GROUPS = {g: [c["id"] for c in rref.CLIP_CASES if c["group"] == g] for g in (1, 2)}


@pytest.mark.parametrize("case_id", GROUPS[1] + GROUPS[2])
def test_the_face_cases_leave_an_exact_clip_nothing_to_spare(case_id):
    """Conditions on the inputs of groups 1 and 2, not on the kernel: under the exact clip at least half the hit rays of an entering case
    use the first sample of the range as `prev`, at least half those of a leaving case hit at its last sample, and the exact range
    narrowed by one sample on both sides loses hits.  Measured: every hit ray of every case, 713 to 851 of the 851 rays."""
    (vol, pose, k, march), full, (k_lo, k_hi) = _case(case_id)
    hit = full["hit"]
    assert len(GROUPS[1]) == len(GROUPS[2]) == 6 and hit.sum() > 400
    edge = (full["hit_k"] - 1 == k_lo) if case_id in GROUPS[1] else (full["hit_k"] == k_hi)
    assert 2 * int((edge & hit).sum()) >= int(hit.sum()), (int((edge & hit).sum()), int(hit.sum()))
    same = rref.render(vol, pose, k, rref.CLIP_H, rref.CLIP_W, *march, k_range=(k_lo, k_hi))
    assert np.array_equal(same["depth"].view(np.uint32), full["depth"].view(np.uint32))      # exact is still enough, to the sample
    narrow = rref.render(vol, pose, k, rref.CLIP_H, rref.CLIP_W, *march, k_range=(k_lo + 1, k_hi - 1))
    lost = int((hit & ~narrow["hit"]).sum())
    print(f"{case_id}: {int(hit.sum())} hits, {int((edge & hit).sum())} on the edge of the exact range, {lost} lost one sample in")
    assert 2 * lost >= int(hit.sum())


def test_the_other_cases_are_what_they_say():
    by_id = {c["id"]: c for c in rref.CLIP_CASES}
    assert sorted({str(c["group"]) for c in rref.CLIP_CASES}) == ["1", "2", "3", "4", "5", "6", "7", "8", "noise"]
    for case in rref.CLIP_CASES:                                             # whole blocks wherever the case is not about a thin or fused volume
        if case["group"] in (1, 2, 3, 4, 6, 7):
            assert all(d % 8 == 0 for d in case["volume"]()["dims"]), case["id"]
    # axis-parallel rays: the middle pixel of every entering view has two direction components exactly 0
    for case_id in GROUPS[1]:
        (vol, pose, k, march), _, _ = _case(case_id)
        o, e = rref.rays(vol, pose, k, rref.CLIP_H, rref.CLIP_W)
        middle = 11 * rref.CLIP_W + 18
        assert sorted(float(abs(x[middle])) for x in e) == [0.0, 0.0, 16.0] and all(float(v) == round(float(v)) for v in o)
    # beside the box: the middle column is `empty` by the e == 0 branch, and columns next to it hit through the side
    for name, columns in (("4-beside-xlo", slice(19, 37)), ("4-beside-xhi", slice(0, 18))):
        (vol, pose, k, march), full, _ = _case(name)
        o, e = rref.rays(vol, pose, k, rref.CLIP_H, rref.CLIP_W)
        k_lo, k_hi = rref.clip_range(vol, pose, k, rref.CLIP_H, rref.CLIP_W, *march)
        assert (e[0].reshape(rref.CLIP_H, -1)[:, 18] == 0).all() and not 0 <= float(o[0]) <= 24 and (k_hi[:, 18] == -1).all()
        assert full["hit"][:, columns].any() and not full["hit"][:, 18].any()
    # a centre on the x = 0 face and one on a lattice point: o is exact, the first sample is the centre itself
    for name, zero in (("3-centre-on-face", True), ("3-centre-on-lattice", False)):
        (vol, pose, k, march), full, _ = _case(name)
        o, _ = rref.rays(vol, pose, k, rref.CLIP_H, rref.CLIP_W)
        assert march[0] == 0.0 and (float(o[0]) == 0.0) == zero and full["hit"].sum() > 400
        assert zero or all(float(v) == round(float(v)) for v in o)
    # thin volumes: one cell layer is hit, no cell layer is not
    for case in (c for c in rref.CLIP_CASES if c["group"] == 5):
        _, full, _ = _case(case["id"])
        assert (full["hit"].sum() > 300) if "two" in case["id"] else (not full["hit"].any() and (full["first_in"] < 0).all()), case["id"]
    # far cameras: 1500 samples, hits, and at 60 km an ulp of t above the step
    for name in ("6-far-600m", "6-far-60km"):
        (vol, pose, k, march), full, _ = _case(name)
        assert rref.sample_count(*march) == 1500 and full["hit"].sum() > 700
    assert np.spacing(np.float32(by_id["6-far-60km"]["t_min"])) > np.float32(by_id["6-far-60km"]["step"])
    # t_max: on the hit sample's t_k every ray hits, one ulp below none does
    found, lost = _case("7-t_max-found"), _case("7-t_max-lost")
    assert found[1]["hit"].all() and not lost[1]["hit"].any()
    assert np.nextafter(np.float32(found[0][3][1]), np.float32(0)) == np.float32(lost[0][3][1])
    assert rref.sample_count(*found[0][3]) == rref.sample_count(*lost[0][3]) + 1 == int(found[1]["hit_k"].max()) + 1
    # poses that are no rotation: some of camera_cases' see the volume, the scaled arc poses see the scene
    for kind in ("scaled", "sheared", "wild"):
        for world in ("origin", "far"):
            hits = [int(_case(c["id"])[1]["hit"].sum()) for c in rref.CLIP_CASES if c["id"].startswith(f"8-{kind}-{world}-")]
            assert len(hits) == 9 and hits[-1] > 300 and sum(h > 0 for h in hits[:-1]) >= 1, (kind, world, hits)


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
@pytest.mark.parametrize("case_id", [c["id"] for c in rref.CLIP_CASES if c["group"] == "noise"])
def test_the_brick_rule_on_volumes_that_are_no_scene(case_id, min_weight):
    """Independent voxels, one in 200 negative, a tenth unseen: a brick is empty or not by chance and a ray passes in and out of both
    kinds.  The march that skips equals the full one bit for bit and skips no valid negative sample."""
    vol, pose, k, march = _case(case_id)[0]
    negative = (vol["tsdf"] < 0) & (vol["weight"] > min_weight)
    bricks = rref.brick_flags(vol, min_weight)
    got = rref.render(vol, pose, k, rref.CLIP_H, rref.CLIP_W, *march, min_weight, bricks=bricks)
    print(f"{case_id} min_weight {min_weight}: {int(negative.sum())} of {negative.size} voxels seen and negative, {int(bricks.sum())} of {bricks.size} bricks "
          f"set, {int(got['hit'].sum())} hits, cells {got['evaluations']} -> {got['brick_evaluations']}")
    assert 0 < negative.sum() < negative.size / 100 and 0 < bricks.sum() and (bricks.sum() < bricks.size or bricks.size < 10)
    assert got["skipped_negative"] == 0 and np.array_equal(got["depth"].view(np.uint32), got["brick_depth"].view(np.uint32))
    assert got["brick_evaluations"] <= got["evaluations"] and got["hit"].any()
