"""CPU: the host side of the cross-view consistency filter (monorec_amd.consistency) - the C entry's declaration, binding and argument
checks, the relative poses formed in double, the runners' planning with the config key, and the numpy restatement
(tests/depth_consistency_ref.py) on the two scenes the GPU tests use.  Nothing here launches a kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import depth_consistency_ref as ref
from monorec_amd import _lib, consistency, tsdf_export as tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------------------------------ C entry
def test_entry_is_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    declared = re.search(r"\bint mr_depth_consistency_f32\s*\(([^;]*)\)\s*;", header)
    assert declared and "mr_depth_consistency_f32" in _lib.ABI
    assert len(declared.group(1).split(",")) == len(_lib.ABI["mr_depth_consistency_f32"][1]) == 16
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() == 24
    assert int(re.search(r"#define MR_CONSISTENCY_MAX_VIEWS (\d+)", header).group(1)) == _lib.MR_CONSISTENCY_MAX_VIEWS == consistency.MAX_VIEWS == 8
    # the structure mirrors the header's, field for field: 24 + 4 floats and a pointer
    struct = re.search(r"typedef struct mr_consistency_view \{(.*?)\} mr_consistency_view;", header, re.S).group(1)
    assert [f[0] for f in _lib.ConsistencyView._fields_] == ["m", "back", "fx", "fy", "cx", "cy", "inv_depth"]
    assert re.findall(r"\b(m|back|fx|fy|cx|cy|inv_depth)\b(?=[\[,;])", re.sub(r"/\*.*?\*/", "", struct, flags=re.S)) == [f[0] for f in _lib.ConsistencyView._fields_]
    assert ctypes.sizeof(_lib.ConsistencyView) == 28 * 4 + 8
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    assert any("`mr_depth_consistency_f32`" in line and "consistency.py" in line for line in table)
    from monorec_amd import build
    assert ("depth_consistency.hip", ["-ffp-contract=off"]) in build.SOURCES


def test_entry_rejects_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are host
    memory nothing may touch."""
    h, w = 5, 7
    inv = (ctypes.c_float * (h * w))()
    out = (ctypes.c_float * (h * w))()
    hits = (ctypes.c_uint8 * (h * w))()
    inf, nan = float("inf"), float("nan")

    def views(n, hole=None):
        array = (_lib.ConsistencyView * max(n, 1))()
        for j in range(max(n, 1)):
            array[j].fx = array[j].fy = 1.0
            array[j].inv_depth = None if j == hole else ctypes.addressof(inv)
        return array

    def call(inv_p=ctypes.addressof(inv), views_p=None, n=2, rel_tol=0.01, reproj=1.0, min_views=2, hh=h, ww=w,
             out_p=ctypes.addressof(out), hits_p=ctypes.addressof(hits), null_views=False):
        array = None if null_views else (views(n) if views_p is None else views_p)
        return hip_lib.mr_depth_consistency_f32(inv_p, 1.0, 1.0, 0.0, 0.0, array, n, rel_tol, reproj, min_views, 0, hh, ww, out_p, hits_p, None)

    bad = [dict(inv_p=None), dict(null_views=True), dict(out_p=None, hits_p=None), dict(n=0), dict(n=-1), dict(n=9, views_p=views(9)),
           dict(views_p=views(2, hole=0)), dict(views_p=views(2, hole=1)), dict(n=8, views_p=views(8, hole=7)),
           dict(hh=0), dict(hh=-1), dict(ww=0), dict(ww=-3), dict(hh=1 << 16, ww=1 << 15), dict(hh=2147483647, ww=2), dict(hh=46341, ww=46341),
           dict(rel_tol=nan), dict(rel_tol=-0.01), dict(rel_tol=-inf), dict(reproj=nan), dict(reproj=-1.0), dict(reproj=-inf), dict(min_views=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert b"argument" in hip_lib.mr_error_string(-1).lower()


# ------------------------------------------------------------------------------------------ relative poses
@pytest.mark.parametrize("shift", [ref.ORIGIN, ref.FAR], ids=["origin", "far"])
def test_relative_views_are_the_double_product_rounded_once(shift):
    """m = inv(pose_j) @ pose and back = inv(m) equal the float64 product rounded to fp32, element for element, in both worlds; in the
    far world (coordinates of a kilometre) the fp32 product of the fp32 inverse is wrong by far more than the double one's rounding."""
    frames, ks = ref.camera_cases(ref.SMALL, seed=3, kind="aniso", shift=shift)
    poses = [torch.from_numpy(f[0]) for f in frames]
    k0 = torch.tensor(ref_k(ks[0]))
    k, views = consistency.relative_views(poses[0].reshape(1, 4, 4), k0, [(None, p, torch.tensor(ref_k(kj))) for p, kj in zip(poses[1:], ks[1:])])
    assert k == tuple(float(F(v)) for v in ks[0]) and len(views) == 7
    worst32 = 0.0
    for j, view in enumerate(views):
        want = np.linalg.inv(frames[j + 1][0].astype(np.float64)) @ frames[0][0].astype(np.float64)
        assert np.array_equal(np.array(view.m[:], dtype=F).reshape(3, 4), want[:3].astype(F))
        assert np.array_equal(np.array(view.back[:], dtype=F).reshape(3, 4), np.linalg.inv(want)[:3].astype(F))
        assert (view.fx, view.fy, view.cx, view.cy) == tuple(float(F(v)) for v in ks[j + 1]) and view.inv_depth is None
        # m @ back is the identity to fp32 rounding of its entries (the translation column: metres times 2^-24)
        ident = np.vstack([want[:3].astype(F).astype(np.float64), [0, 0, 0, 1]]) @ np.vstack([np.linalg.inv(want)[:3].astype(F).astype(np.float64), [0, 0, 0, 1]])
        assert np.abs(ident - np.eye(4)).max() < 1e-5
        single = (torch.inverse(poses[j + 1]) @ poses[0]).numpy().astype(np.float64)
        worst32 = max(worst32, np.abs(single[:3, 3] - want[:3, 3]).max())
    if shift == ref.FAR:
        assert worst32 > 1e-4                                        # a tenth of a millimetre and more, lost by the fp32 product
    for bad in ([], [(None, poses[1], k0)] * 9):
        with pytest.raises(ValueError, match="neighbours"):
            consistency.relative_views(poses[0], k0, bad)
    with pytest.raises(ValueError, match="4 x 4"):
        consistency.relative_views(torch.eye(3), k0, [(None, poses[1], k0)])


def ref_k(k):
    fx, fy, cx, cy = k
    return [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]


def test_filter_depth_needs_device_tensors_and_at_most_eight_neighbours():
    d, pose, k = torch.ones(4, 6), torch.eye(4), torch.tensor(ref_k((5.0, 5.0, 3.0, 2.0)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consistency.filter_depth(d, pose, k, [(d, pose, k)])
    with pytest.raises((ValueError, RuntimeError), match="neighbours|no CPU fallback"):
        consistency.filter_depth(d, pose, k, [(d, pose, k)] * 9)
    with pytest.raises(ValueError, match="neighbours"):
        consistency.relative_views(pose, k, [(None, pose, k)] * 9)


# ------------------------------------------------------------------------------------------ config key, planning
def test_settings_of_the_config_key():
    assert consistency.settings(None) is None and consistency.settings(False) is None
    assert consistency.settings(True) == consistency.settings({}) == dict(rel_tol=0.01, max_reproj_px=1.0, min_views=2, average=False)
    assert consistency.settings({"min_views": 3, "average": True}) == dict(rel_tol=0.01, max_reproj_px=1.0, min_views=3, average=True)
    assert consistency.settings({"max_reproj_px": float("inf")})["max_reproj_px"] == float("inf")
    for bad in ({"tolerance": 0.1}, {"rel_tol": -1}, {"rel_tol": float("nan")}, {"max_reproj_px": -0.5}, {"min_views": -1}, {"min_views": 1.5},
                {"average": 1}, "yes", 3):
        with pytest.raises(ValueError, match="consistency"):
            consistency.settings(bad)


class _Model(torch.nn.Module):
    def __init__(self, in_flight):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.hip_in_flight = in_flight


class _Dataset:
    target_image_size = (24, 40)

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_stream_planning_with_the_key_and_without_the_vote():
    """With `consistency` and `use_mask` false the stream plans like the vote - the first and last two keyframes of the window are not
    exported, a rank runs two extra either side - but keeps the model's whole `hip_in_flight` in flight (the buffered depths are its own
    copies); with both, the vote's rule on `hip_in_flight` stands as it is; without the key nothing differs from today."""
    base = {"use_mask": False, "start": 1, "end": 12}
    plain = tx.KeyframeStream(base, model=_Model(4), dataset=_Dataset(20))
    assert plain.consistency is None and not plain.buffered and plain.plan == tx.plan_shard(11, False) and plain.depth_in_flight == 4
    for value in (False, None):
        same = tx.KeyframeStream(dict(base, consistency=value), model=_Model(4), dataset=_Dataset(20))
        assert same.consistency is None and same.plan == plain.plan and same.depth_in_flight == 4 and same.export_items() == plain.export_items()
    on = tx.KeyframeStream(dict(base, consistency={"min_views": 3}), model=_Model(4), dataset=_Dataset(20))
    assert on.consistency == dict(rel_tol=0.01, max_reproj_px=1.0, min_views=3, average=False) and on.buffered and not on.use_mask
    assert on.plan == tx.plan_shard(11, True) == {"total": 7, "exports": (0, 7), "items": (0, 11), "halo": 2}
    assert on.export_items() == list(range(3, 10)) and on.depth_in_flight == 4
    assert tx.KeyframeStream(dict(base, consistency=True), model=_Model(1), dataset=_Dataset(20)).depth_in_flight == 1
    covered = []
    for rank in range(3):
        part = tx.KeyframeStream(dict(base, consistency=True), model=_Model(4), dataset=_Dataset(20), shard=(rank, 3))
        assert part.plan == tx.plan_shard(11, True, rank, 3)
        covered += part.export_items()
    assert covered == on.export_items()
    voted = tx.KeyframeStream(dict(base, use_mask=True, consistency=True), model=_Model(4), dataset=_Dataset(20))
    assert voted.plan == on.plan and voted.depth_in_flight == 2
    with pytest.raises(ValueError, match="hip_in_flight >= 3"):
        tx.KeyframeStream(dict(base, use_mask=True, consistency=True), model=_Model(2), dataset=_Dataset(20))
    with pytest.raises(ValueError, match="unknown consistency key"):
        tx.KeyframeStream(dict(base, consistency={"rel_tolerance": 0.01}), model=_Model(4), dataset=_Dataset(20))
    from monorec_amd.pointcloud import PointcloudBuilder
    assert PointcloudBuilder(None).consistency is None and PointcloudBuilder(None, consistency=True).consistency == consistency.settings(True)
    with pytest.raises(ValueError, match="unknown consistency key"):
        PointcloudBuilder(None, consistency={"views": 2})
    with pytest.raises(ValueError, match="buffer"):
        PointcloudBuilder(None, buffer_length=11, consistency=True)


# ------------------------------------------------------------------------------------------ the restatement on the scenes
def _scene_a():
    a = ref.SCENE_A
    inv, pose, neighbours = ref.scene(a["reference"], a["neighbours"], radius=a["radius"])
    return inv, ref.views_of(pose, neighbours, ref.INTRINSICS_30)


def test_scene_a_reaches_every_outcome():
    """Scene A (the arc of radius 1 m, reference 5, neighbours 3, 4, 6 and 10, which looks away): each of the six outcomes at least 5 times
    over the 4 x 880 valid pixel-neighbour pairs, exactly one outcome per pair, and hits / out as the definition derives them."""
    a = ref.SCENE_A
    inv, views = _scene_a()
    out, hits, traces = ref.filter_depth(inv, ref.INTRINSICS_30, views, a["rel_tol"], a["max_reproj_px"], 2, False)
    valid = ref.valid_depth(inv)[0]
    counts = ref.outcome_counts(traces)
    print("scene A outcomes", counts, "valid", int(valid.sum()), "hit histogram", np.bincount(hits.ravel(), minlength=5).tolist())
    assert all(counts[name] >= 5 for name in ref.OUTCOMES), counts
    assert sum(counts.values()) == 4 * int(valid.sum()) and int(valid.sum()) == 880
    for t in traces:
        assert np.array_equal(sum(t[name].astype(int) for name in ref.OUTCOMES), valid.astype(int))
    assert traces[3]["behind"].sum() == valid.sum()                          # the camera that looks away
    assert np.array_equal(hits, sum(t["hit"] for t in traces).astype(np.uint8)) and not hits[~valid].any()
    assert np.array_equal(out, np.where(hits >= 2, inv, F(0))) and out.dtype == F
    # every count of hits from 0 to 3 occurs: min_views 1 .. 3 each cut between pixels that are there
    assert all((hits[valid] == n).sum() >= 5 for n in range(4))
    # averaging moves kept pixels, by less than the tolerance allows, and leaves zeroed ones zero
    mean, hits2, _ = ref.filter_depth(inv, ref.INTRINSICS_30, views, a["rel_tol"], a["max_reproj_px"], 2, True)
    kept = hits >= 2
    assert np.array_equal(hits2, hits) and not mean[~kept].any() and (mean[kept] != inv[kept]).any()
    assert np.abs(mean[kept] / inv[kept] - 1).max() < 2 * a["rel_tol"]
    # without the reprojection bound the reproj outcome is empty but for p_2 <= 0, and nothing else changes
    _, _, loose = ref.filter_depth(inv, ref.INTRINSICS_30, views, a["rel_tol"], np.inf, 2, False)
    loose_counts = ref.outcome_counts(loose)
    assert loose_counts["reproj"] == 0 and loose_counts["hit"] == counts["hit"] + counts["reproj"]
    assert all(loose_counts[name] == counts[name] for name in ("behind", "outside", "nodepth", "depth"))


def test_scene_b_zeroes_the_spoiled_block_and_keeps_the_rest():
    """Scene B (the default arc, reference 4, neighbours 2, 3, 5, 6): a block of 6 x 10 pixels whose inverse depth is 1.25 times too large
    gets no hit and is zeroed; every other valid pixel is kept, and at least 90 % of them are confirmed by all four neighbours."""
    b = ref.SCENE_B
    inv, pose, neighbours = ref.scene(b["reference"], b["neighbours"], radius=b["radius"])
    assert all(np.array_equal(p, f[0]) for p, f in zip([pose] + [n[1] for n in neighbours],
                                                        [ref.make_frames(ref.INTRINSICS_30)[j] for j in (b["reference"],) + b["neighbours"]]))
    y0, y1, x0, x1 = b["block"]
    spoiled = inv.copy()
    spoiled[y0:y1, x0:x1] *= F(b["factor"])
    block = np.zeros(inv.shape, bool)
    block[y0:y1, x0:x1] = True
    valid = ref.valid_depth(spoiled)[0]
    assert valid[block].all() and block.sum() == 60
    out, hits, _ = ref.filter_depth(spoiled, ref.INTRINSICS_30, ref.views_of(pose, neighbours, ref.INTRINSICS_30), b["rel_tol"], b["max_reproj_px"],
                                    b["min_views"], False)
    histogram = np.bincount(hits[valid], minlength=5)
    print("scene B hit histogram over valid pixels", histogram.tolist())
    assert not hits[block].any() and not out[block].any()
    rest = valid & ~block
    assert rest.sum() == 820 and np.array_equal(out[rest], spoiled[rest]) and (hits[rest] >= b["min_views"]).all()
    assert (hits[rest] == 4).sum() >= 0.9 * rest.sum()
    assert not out[~valid].any() and not hits[~valid].any()
