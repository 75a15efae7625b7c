"""GPU: the cross-view consistency filter - `mr_depth_consistency_f32` against the numpy restatement of tests/depth_consistency_ref.py on
the analytic scene (every launch shape, general cameras in both worlds, inputs placed where each decision sits), and the three runners
with the config key against one-at-a-time loops.  `hits` must be equal and `out` bit-equal everywhere: no pixel is left out, no tolerance."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import depth_consistency_ref as ref
from monorec_amd import _lib, consistency, pointcloud, synth, tsdf_export as tx, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
K30 = ref.INTRINSICS_30
INF = float("inf")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch(inv, k, views, rel_tol, reproj, min_views, average, want_out=True, want_hits=True):
    """One direct call of the C entry on the restatement's inputs.  The outputs start from a pattern the kernel never writes by itself,
    so that a pixel it skipped cannot pass.  Returns (out or None, hits or None) as numpy arrays."""
    lib = _lib.load()
    h, w = inv.shape
    d = _dev(inv)
    maps = [_dev(v[3]) for v in views]
    array = (_lib.ConsistencyView * len(views))()
    for j, (m, back, kj, _) in enumerate(views):
        array[j].m[:] = np.asarray(m, dtype=F).reshape(-1).tolist()
        array[j].back[:] = np.asarray(back, dtype=F).reshape(-1).tolist()
        array[j].fx, array[j].fy, array[j].cx, array[j].cy = (float(F(v)) for v in kj)
        array[j].inv_depth = maps[j].data_ptr()
    out = torch.full((h, w), 7.0, dtype=torch.float32, device=DEV) if want_out else None
    hits = torch.full((h, w), 205, dtype=torch.uint8, device=DEV) if want_hits else None
    fx, fy, cx, cy = (float(F(v)) for v in k)
    _lib.check(lib.mr_depth_consistency_f32(d.data_ptr(), fx, fy, cx, cy, array, len(views), float(rel_tol), float(reproj), int(min_views),
                                            int(average), h, w, out.data_ptr() if want_out else None, hits.data_ptr() if want_hits else None,
                                            torch.cuda.current_stream().cuda_stream), "mr_depth_consistency_f32")
    torch.cuda.synchronize()
    return (out.cpu().numpy() if want_out else None), (hits.cpu().numpy() if want_hits else None)


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype == F and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


def _check(inv, k, views, rel_tol, reproj, min_views, average, what=""):
    """Device against restatement, both outputs.  Returns the restatement's (out, hits, traces)."""
    want_out, want_hits, traces = ref.filter_depth(inv, k, views, rel_tol, reproj, min_views, average)
    out, hits = _launch(inv, k, views, rel_tol, reproj, min_views, average)
    assert np.array_equal(hits, want_hits), what
    _same_bits(out, want_out, what)
    return want_out, want_hits, traces


# ------------------------------------------------------------------------------------------ 1. scene A
EIGHT = (3, 4, 6, 10, 2, 7, 1, 8)              # scene A's four neighbours first; frame 10 looks away


@functools.lru_cache(maxsize=None)
def _scene(height=24, width=40, neighbours=EIGHT):
    """Scene A's arc rendered at one size: (inv_depth of frame 5, views of `neighbours`).  Shared, never modified."""
    a = ref.SCENE_A
    inv, pose, others = ref.scene(a["reference"], neighbours, radius=a["radius"], height=height, width=width)
    return inv, ref.views_of(pose, others, K30)


@pytest.mark.parametrize("reproj", [0.5, INF], ids=["half_px", "unbounded"])
@pytest.mark.parametrize("average", [0, 1], ids=["keep", "average"])
@pytest.mark.parametrize("num_views", [1, 4, 8])
def test_scene_a_equals_the_restatement(hip_lib, num_views, average, reproj):
    inv, views = _scene()
    views = views[:num_views]
    min_views = min(2, num_views)
    want_out, want_hits, traces = _check(inv, K30, views, ref.SCENE_A["rel_tol"], reproj, min_views, average)
    if num_views == 4 and reproj == 0.5:                                     # the inputs are the ones the CPU test pins as non-degenerate
        assert ref.outcome_counts(traces) == dict(behind=880, outside=110, nodepth=18, depth=60, reproj=345, hit=2107)
    assert (want_out != 0).any() and (want_out[ref.valid_depth(inv)[0]] == 0).any()
    out_alone, none = _launch(inv, K30, views, ref.SCENE_A["rel_tol"], reproj, min_views, average, want_hits=False)
    assert none is None
    _same_bits(out_alone, want_out, "out alone")
    none, hits_alone = _launch(inv, K30, views, ref.SCENE_A["rel_tol"], reproj, min_views, average, want_out=False)
    assert none is None and np.array_equal(hits_alone, want_hits)


@pytest.mark.parametrize("average", [0, 1], ids=["keep", "average"])
@pytest.mark.parametrize("size", [(24, 40), (5, 37), (1, 1), (3, 130), (9, 33), (17, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ragged_tiles_and_widths(hip_lib, size, average):
    """The same scene rendered at sizes that end inside a 32 x 8 tile, are narrower than one, one pixel, wider than one tile row, one
    pixel past a tile both ways, and whole tiles."""
    inv, views = _scene(*size, neighbours=EIGHT[:4])
    _, hits, _ = _check(inv, K30, views, ref.SCENE_A["rel_tol"], 0.5, 1, average, what=str(size))
    if size != (1, 1):
        assert hits.any()


# ------------------------------------------------------------------------------------------ 2. hard cameras
def _through_python(inv, pose, k, neighbours, **kw):
    """`consistency.filter_depth` on device copies against the restatement fed the matrices `relative_views` formed."""
    k3 = torch.tensor(ref_k(k))
    given = [(_dev(inv_j), torch.from_numpy(np.asarray(pose_j)), torch.tensor(ref_k(kj))) for inv_j, pose_j, kj in neighbours]
    out, hits = consistency.filter_depth(_dev(inv), torch.from_numpy(np.asarray(pose)), k3, given, **kw)
    _, array = consistency.relative_views(torch.from_numpy(np.asarray(pose)), k3, [(None, p, kj) for _, p, kj in given])
    views = [(np.array(v.m[:], dtype=F).reshape(3, 4), np.array(v.back[:], dtype=F).reshape(3, 4), (v.fx, v.fy, v.cx, v.cy), n[0])
             for v, n in zip(array, neighbours)]
    want_out, want_hits, traces = ref.filter_depth(inv, k, views, kw.get("rel_tol", 0.01), kw.get("max_reproj_px", 1.0), kw.get("min_views", 2),
                                                   kw.get("average", False))
    assert out.shape == inv.shape and hits.shape == inv.shape and hits.dtype == torch.uint8
    assert np.array_equal(hits.cpu().numpy(), want_hits)
    _same_bits(out.cpu().numpy(), want_out)
    return want_out, want_hits, traces


def ref_k(k):
    fx, fy, cx, cy = (float(v) for v in k)
    return [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]


@pytest.mark.parametrize("shift", [ref.ORIGIN, ref.FAR], ids=["origin", "far"])
@pytest.mark.parametrize("kind", ["rigid", "offcentre", "aniso"])
def test_hard_cameras_in_both_worlds(hip_lib, kind, shift):
    """Eight cameras anywhere in and round a box, turned any way, each with its own intrinsics (principal points outside the image,
    fy = 4 fx), random depth: frame 0 against the other seven, through the Python entry."""
    frames, ks = ref.camera_cases(ref.SMALL, seed=11, kind=kind, shift=shift)
    maps = [ref.inverse_depth(f[1]) for f in frames]
    neighbours = [(maps[j], frames[j][0], ks[j]) for j in range(1, 8)]
    for average in (False, True):
        _, _, traces = _through_python(maps[0], frames[0][0], ks[0], neighbours, rel_tol=0.5, max_reproj_px=3.0, min_views=1, average=average)
    counts = ref.outcome_counts(traces)
    assert counts["behind"] > 0 and counts["outside"] > 0, counts


@pytest.mark.parametrize("shift", [ref.ORIGIN, ref.FAR], ids=["origin", "far"])
def test_neighbours_with_their_own_intrinsics_on_the_scene(hip_lib, shift):
    """The arc scene moved into either world, every neighbour rendered with intrinsics of its own: all six outcomes occur, so the
    neighbour's fx fy cx cy are used on the way there and on the way back."""
    poses = ref.arc_poses(11, 1.0)
    moved = []
    for p in poses:
        q = p.astype(np.float64)
        q[:3, 3] += np.array(shift)
        moved.append(q.astype(F))
    own = {3: (28.0, 33.0, 18.0, 12.25), 4: (30.0, 30.0, 19.5, 11.5), 6: (36.0, 31.0, 21.0, 10.0), 10: (30.0, 30.0, 19.5, 11.5), 7: (24.0, 26.0, 17.5, 13.0)}
    inv = ref.inverse_depth(ref.render(poses[5], K30, 24, 40)[0])             # rendered in the scene's own frame; the shift moves every pose alike
    neighbours = [(ref.inverse_depth(ref.render(poses[j], kj, 24, 40)[0]), moved[j], kj) for j, kj in own.items()]
    _, hits, traces = _through_python(inv, moved[5], K30, neighbours, rel_tol=0.02, max_reproj_px=0.75, min_views=2, average=True)
    counts = ref.outcome_counts(traces)
    print("own intrinsics", "far" if shift == ref.FAR else "origin", counts)
    assert all(counts[name] >= 5 for name in ref.OUTCOMES), counts
    assert all(t["hit"].sum() > 100 for j, t in enumerate(traces) if j != 3)  # every neighbour but the one that looks away confirms pixels


# ------------------------------------------------------------------------------------------ 3. where the decisions sit
EYE = np.eye(4, dtype=F)[:3]
K1 = (1.0, 1.0, 0.0, 0.0)                      # with inverse depth 1 a pixel (x, y) is the point (x, y, 1)


def test_projection_landing_on_the_half_pixels_at_the_image_edges(hip_lib):
    """u on -0.5 and on width - 0.5, v on -0.5 and on height - 0.5: roundf takes the halves away from zero, out of the image."""
    h, w = 3, 6
    ones = np.ones((h, w), F)
    views = [(EYE, EYE, (1.0, 1.0, -0.5, 0.0), ones), (EYE, EYE, (1.0, 1.0, 0.5, 0.0), ones),
             (EYE, EYE, (1.0, 1.0, 0.0, -0.5), ones), (EYE, EYE, (1.0, 1.0, 0.0, 0.5), ones)]
    out, hits, traces = _check(ones, K1, views, 0.01, INF, 4, 0)
    assert (traces[0]["u_raw"][:, 0] == F(-0.5)).all() and traces[0]["outside"][:, 0].all() and traces[0]["hit"][:, 1:].all()
    assert (traces[1]["u_raw"][:, w - 1] == F(w - 0.5)).all() and traces[1]["outside"][:, w - 1].all() and traces[1]["hit"][:, :w - 1].all()
    assert (traces[2]["v_raw"][0] == F(-0.5)).all() and traces[2]["outside"][0].all() and traces[2]["hit"][1:].all()
    assert (traces[3]["v_raw"][h - 1] == F(h - 0.5)).all() and traces[3]["outside"][h - 1].all() and traces[3]["hit"][:h - 1].all()
    assert hits[1, 1] == 4 and hits[0, 0] == 2 and hits[1, 0] == 3 and out[1, 1] == 1 and out[0, 0] == 0


def test_a_point_in_the_neighbours_image_plane_is_behind(hip_lib):
    """q_2 == 0 exactly: not in front."""
    inv = np.array([[1.0, 0.5, 1.0, 0.25, 2.0]], F)                            # depths 1, 2, 1, 4, 0.5 against a camera one metre ahead
    m = EYE.copy()
    m[2, 3] = -1.0
    back = EYE.copy()
    back[2, 3] = 1.0
    _, hits, traces = _check(inv, K1, [(m, back, K1, np.ones((1, 5), F))], 10.0, INF, 1, 0)
    assert np.array_equal(traces[0]["q2"], np.array([[0.0, 1.0, 0.0, 3.0, -0.5]], F))
    assert traces[0]["behind"].tolist() == [[True, False, True, False, True]] and hits.tolist() == [[0, 1, 0, 1, 0]]


@pytest.mark.parametrize("step", [-1, 0, 1], ids=["ulp_below", "equal", "ulp_above"])
def test_depth_difference_on_the_tolerance(hip_lib, step):
    """|dn - q_2| = 1 against rel_tol * q_2 with rel_tol one ulp below 1, 1, one ulp above: fails, passes, passes."""
    rel_tol = {-1: np.nextafter(F(1), F(0)), 0: F(1), 1: np.nextafter(F(1), F(2))}[step]
    inv, other = np.ones((1, 3), F), np.full((1, 3), 0.5, F)                  # q_2 = 1, dn = 2
    _, hits, traces = _check(inv, K1, [(EYE, EYE, K1, other)], rel_tol, INF, 1, 1)
    t = traces[0]
    assert (t["diff"] == 1).all() and (t["bound"] == rel_tol).all()
    assert (t["bound"] == [np.nextafter(F(1), F(0)), F(1), np.nextafter(F(1), F(2))][step + 1]).all()
    assert t["depth"].all() if step < 0 else t["hit"].all()
    assert (hits == (0 if step < 0 else 1)).all()


@pytest.mark.parametrize("step", [-1, 0, 1], ids=["ulp_below", "equal", "ulp_above"])
def test_reprojection_error_on_the_bound(hip_lib, step):
    """The way back lands half a pixel to the right: ex * ex + ey * ey = 0.25 against max_reproj_px one ulp below 0.5, 0.5, one above."""
    bound = {-1: np.nextafter(F(0.5), F(0)), 0: F(0.5), 1: np.nextafter(F(0.5), F(1))}[step]
    ones = np.ones((2, 5), F)
    back = EYE.copy()
    back[0, 3] = 0.5
    _, hits, traces = _check(ones, K1, [(EYE, back, K1, ones)], 0.01, bound, 1, 0)
    t = traces[0]
    assert (t["err2"] == F(0.25)).all() and (F(bound) * F(bound) < F(0.25)) == (step < 0)
    assert t["reproj"].all() if step < 0 else t["hit"].all()
    assert (hits == (0 if step < 0 else 1)).all()


@pytest.mark.parametrize("min_views", [0, 1, 2, 3, 4])
def test_min_views_cuts_between_pixels_that_are_there(hip_lib, min_views):
    """Scene A has pixels with 0, 1, 2 and 3 hits: n == min_views is kept, n == min_views - 1 zeroed; min_views 0 keeps every valid
    pixel and still zeroes the invalid ones; 4 keeps none (frame 10 never confirms)."""
    inv, views = _scene()
    out, hits, _ = _check(inv, K30, views[:4], ref.SCENE_A["rel_tol"], 0.5, min_views, 0)
    valid = ref.valid_depth(inv)[0]
    assert (~valid).sum() == 80 and not out[~valid].any()
    for n in range(4):
        at = valid & (hits == n)
        assert at.sum() >= 5 and ((out[at] == inv[at]).all() if n >= min_views else not out[at].any())
    if min_views == 0:
        assert np.array_equal(out[valid], inv[valid])


@pytest.mark.parametrize("average", [0, 1], ids=["keep", "average"])
@pytest.mark.parametrize("min_views", [0, 3])
def test_values_that_are_no_depth(hip_lib, min_views, average):
    """0, -1, NaN, +inf and a subnormal (its reciprocal overflows) in the reference and in the neighbours: invalid wherever they stand."""
    nan, tiny = np.nan, 1e-40
    assert 0 < F(tiny) < np.finfo(F).tiny
    inv = np.array([[1, 0, -1, nan, INF, tiny, 1, 1, 1]], F)
    views = [(EYE, EYE, K1, np.array([[1, 1, 1, 1, 1, 1, 0, -1, 1]], F)),
             (EYE, EYE, K1, np.array([[nan, 1, 1, 1, 1, 1, INF, tiny, 1]], F)),
             (EYE, EYE, K1, np.ones((1, 9), F))]
    out, hits, traces = _check(inv, K1, views, 0.01, 1.0, min_views, average)
    assert hits.tolist() == [[2, 0, 0, 0, 0, 0, 1, 1, 3]]
    assert traces[0]["nodepth"].tolist() == [[False] * 6 + [True, True, False]] and traces[1]["nodepth"].tolist() == [[True] + [False] * 5 + [True, True, False]]
    assert (out != 0).tolist() == [[min_views == 0] + [False] * 5 + [min_views == 0] * 2 + [True]]


def test_eight_views_in_one_launch_and_the_order_is_real(hip_lib):
    """One launch with eight views equals the restatement fed the same eight in order; the hits do not depend on the order, the averaged
    depth does - fp32 sums in another order round differently - so reversing the neighbours changes some bits."""
    inv, views = _scene()
    assert len(views) == 8
    forward, hits, _ = _check(inv, K30, views, ref.SCENE_A["rel_tol"], 0.5, 2, 1)
    backward, hits_back, _ = _check(inv, K30, views[::-1], ref.SCENE_A["rel_tol"], 0.5, 2, 1)
    assert np.array_equal(hits, hits_back) and hits.max() >= 6
    differ = forward.view(np.uint32) != backward.view(np.uint32)
    assert differ.any() and not differ[hits < 2].any()
    assert np.abs(forward - backward).max() < 1e-6


def test_python_entry_shapes_and_refusals(hip_lib):
    inv, views = _scene(neighbours=EIGHT[:4])
    a = ref.SCENE_A
    poses = ref.arc_poses(11, a["radius"])
    k3 = torch.tensor(ref_k(K30))
    neighbours = [(_dev(v[3]).reshape(1, 1, 24, 40), torch.from_numpy(poses[j]).reshape(1, 4, 4), k3.reshape(1, 3, 3)) for v, j in zip(views, EIGHT[:4])]
    want_out, want_hits, _ = ref.filter_depth(inv, K30, views, 0.01, 0.5, 2, False)
    given = _dev(inv).reshape(1, 1, 24, 40)
    own = torch.empty(1, 1, 24, 40, device=DEV)
    out, hits = consistency.filter_depth(given, torch.from_numpy(poses[5]), k3, neighbours, max_reproj_px=0.5, out=own)
    assert out is own and out.shape == (1, 1, 24, 40) and hits.shape == (24, 40)
    _same_bits(out.cpu().numpy().reshape(24, 40), want_out)
    assert np.array_equal(hits.cpu().numpy(), want_hits) and np.array_equal(given.cpu().numpy().reshape(24, 40), inv)
    with pytest.raises(ValueError, match="out"):
        consistency.filter_depth(given, torch.from_numpy(poses[5]), k3, neighbours, out=given)
    with pytest.raises(ValueError, match="out"):
        consistency.filter_depth(given, torch.from_numpy(poses[5]), k3, neighbours, out=neighbours[1][0])
    with pytest.raises(ValueError, match="neighbours"):
        consistency.filter_depth(given, torch.from_numpy(poses[5]), k3, neighbours * 3)
    with pytest.raises(ValueError, match="neighbour 0"):
        consistency.filter_depth(given, torch.from_numpy(poses[5]), k3, [(given[..., :20], neighbours[0][1], k3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consistency.filter_depth(given, torch.from_numpy(poses[5]), k3, [(given.cpu(), neighbours[0][1], k3)])


# ------------------------------------------------------------------------------------------ 4. the runners
STEPS, KEYFRAMES = 16, 9
# the seeded model's depth is no reconstruction (with the default key two pixels in a thousand survive): a tolerance under which about
# half the pixels of a keyframe are confirmed by two neighbours and half are not
KEY = {"rel_tol": 0.5, "max_reproj_px": 64.0, "min_views": 2, "average": True}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return synth.make_kitti_tree(tmp_path_factory.mktemp("kitti"), sequences=(("03", 120, 400),), frames=20)      # 10 samples


@pytest.fixture(scope="module")
def model(hip_lib):
    from monorec_amd import MonoRecModel
    m = MonoRecModel(cv_depth_steps=STEPS, hip_in_flight=4)
    sd = synth.seeded_state_dict(m.state_dict(), seed=0)
    sd["att_module.classifier.0.bias"] = sd["att_module.classifier.0.bias"] - 5.0          # a vote that keeps some pixels
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _config(tree, out_dir, use_mask, **extra):
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    return dict({"name": "consistency", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": KEYFRAMES, "min_d": 3, "max_d": 30,
                 "use_mask": use_mask, "output_dir": str(out_dir), "export_ring": 3, "export_workers": 2, "consistency": dict(KEY),
                 "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": STEPS}},
                 "data_set": {"type": "KittiOdometryDataset", "args": args}}, **extra)


@pytest.fixture(scope="module")
def collected(tree, model):
    """One forward at a time with owned outputs, and per keyframe that has two either side its depth filtered against those four by
    `filter_depth` - what the runners must feed their pack / integrate / add_depthmap.  Shared, never modified."""
    from monorec_amd import kitti
    from monorec_amd.pointcloud import static_mask
    config = _config(tree, "unused", True)
    dataset = kitti.KittiOdometryDataset(**dict(config["data_set"]["args"], device=DEV))
    loader = kitti.DeviceLoader(dataset, batch_size=1, start=config["start"], end=config["end"])
    entries = []
    with torch.no_grad():
        for data, _ in loader:
            out = model(data)
            entries.append(dict(keyframe=data["keyframe"].clone(), depth=out["result"].clone(), pose=data["keyframe_pose"].clone(),
                                intrinsics=data["keyframe_intrinsics"].clone(), mask=static_mask(out["cv_mask"], 32),
                                ids=[int(data["sequence"]), int(data["image_id"])]))
    dataset.close()
    assert len(entries) == KEYFRAMES
    for e in range(2, KEYFRAMES - 2):
        others = [(entries[j]["depth"], entries[j]["pose"], entries[j]["intrinsics"]) for j in (e - 2, e - 1, e + 1, e + 2)]
        entries[e]["filtered"], entries[e]["hits"] = consistency.filter_depth(entries[e]["depth"], entries[e]["pose"], entries[e]["intrinsics"], others, **KEY)
        window = entries[e - 2:e + 3]
        entries[e]["vote"] = (torch.sum(torch.stack([w["mask"] for w in window]), dim=0) > 5 - 1).to(dtype=torch.float32)
    return entries


def test_the_runner_inputs_are_not_degenerate(collected):
    """Per exported keyframe the filter keeps some pixels and zeroes some, moves kept ones (average), and the vote cuts further."""
    for e in range(2, KEYFRAMES - 2):
        entry = collected[e]
        kept = (entry["filtered"] != 0)
        share = float(kept.float().mean())
        print(f"keyframe {e}: {share:.3f} kept, hits {torch.bincount(entry['hits'].reshape(-1).long(), minlength=5).tolist()}")
        assert 0.02 < share < 0.98
        assert (entry["filtered"][kept] != entry["depth"][kept]).any()
        both = float(((entry["filtered"] * entry["vote"]) != 0).float().mean())
        assert 0 < both < share


def _files(directory):
    return {n: open(os.path.join(directory, n), "rb").read() for n in sorted(os.listdir(directory))}


def _serial_export(collected, config, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    crop, lo, hi = config["roi"], config["min_d"], config["max_d"]
    tx.save_intrinsics_for_tsdf(out_dir, collected[0]["intrinsics"][0], crop=crop)
    ids = []
    for number, e in enumerate(range(2, KEYFRAMES - 2)):
        entry = collected[e]
        depth = entry["filtered"] * entry["vote"] if config["use_mask"] else entry["filtered"]
        tx.save_frame_for_tsdf(out_dir, number, entry["keyframe"][0], depth[0, 0], entry["pose"][0], crop, lo, hi)
        ids.append(entry["ids"])
    return ids


@pytest.fixture(scope="module")
def unsharded(tree, model, tmp_path_factory):
    out = tmp_path_factory.mktemp("consistent_whole")
    return str(out), tx.run(_config(tree, out, False), model=model)


@pytest.mark.parametrize("use_mask", [False, True], ids=["plain", "vote"])
def test_export_runner_equals_the_one_at_a_time_loop(tree, model, collected, unsharded, tmp_path, use_mask):
    if use_mask:
        out = str(tmp_path / "pipelined")
        count = tx.run(_config(tree, out, True), model=model)
    else:
        out, count = unsharded
    ids = _serial_export(collected, _config(tree, out, use_mask), str(tmp_path / "serial"))
    assert count == KEYFRAMES - 4 == len(ids)
    got, want = _files(out), _files(str(tmp_path / "serial"))
    assert sorted(got) == sorted(list(want) + ["frames.json"])
    for name, data in want.items():
        assert got[name] == data, name
    assert tx.read_manifest(out) == {i: tuple(v) for i, v in enumerate(ids)}
    assert len({got[f"frame-{i:06d}.depth.png"] for i in range(count)}) == count
    # and the key does something: the same run without it writes other depth files (and, without the vote, four more)
    plain = str(tmp_path / "no_key")
    config = _config(tree, plain, use_mask)
    del config["consistency"]
    assert tx.run(config, model=model) == (KEYFRAMES - 4 if use_mask else KEYFRAMES)
    offset = 0 if use_mask else 2
    assert any(_files(plain)[f"frame-{i + offset:06d}.depth.png"] != got[f"frame-{i:06d}.depth.png"] for i in range(count))
    assert all(_files(plain)[f"frame-{i + offset:06d}.color.jpg"] == got[f"frame-{i:06d}.color.jpg"] for i in range(count))


def test_shards_in_turn_equal_the_unsharded_directory(tree, model, unsharded, tmp_path):
    whole, count = unsharded
    out = str(tmp_path / "shards")
    counts = [tx.run(_config(tree, out, False), model=model, shard=(rank, 2)) for rank in (1, 0)]
    assert sum(counts) == count and all(c > 0 for c in counts)
    got, want = _files(out), _files(whole)
    assert sorted(got) == sorted(want) and "camera-intrinsics.txt" in got and "frames.json" in got
    for name, data in want.items():
        assert got[name] == data, name


@pytest.mark.parametrize("use_mask,fuse_batch", [(False, 3), (True, 1)], ids=["plain_batch3", "vote_batch1"])
def test_fusion_runner_equals_the_one_at_a_time_loop(tree, model, collected, tmp_path, use_mask, fuse_batch):
    config = _config(tree, tmp_path, use_mask, voxel_size=0.5, trunc_voxels=3, fuse_batch=fuse_batch, file_name="surface.ply",
                     save_volume=os.path.join(str(tmp_path), "volume.npz"))
    count = tf.run(config, model=model)
    with np.load(config["save_volume"]) as z:
        got = {k: z[k] for k in z.files}
    assert int(got["frames"]) == KEYFRAMES - 4 and count > 0
    volume = tf.TSDFVolume(origin=got["origin"], dims=got["dims"], voxel_size=config["voxel_size"], trunc=config["voxel_size"] * config["trunc_voxels"],
                           device=DEV)
    crop = config["roi"]
    for e in range(2, KEYFRAMES - 2):
        entry = collected[e]
        depth = entry["filtered"] * entry["vote"] if use_mask else entry["filtered"]
        k = entry["intrinsics"][0].clone()
        k[0, 2] -= crop[2]
        k[1, 2] -= crop[0]
        packed, colour, _ = tx.pack_frames(depth, entry["keyframe"], crop, config["min_d"], config["max_d"])
        volume.integrate(packed[0], colour[0], entry["pose"][0], k)
    tsdf, weight, colour = volume.grids()
    assert weight.max() > 1
    assert np.array_equal(got["weight"], weight) and np.array_equal(got["tsdf"], tsdf) and np.array_equal(got["colour"], colour)


def _ply_records(data):
    head, _, body = data.partition(b"end_header\n")
    return np.frombuffer(body, dtype="<f4")


@pytest.mark.parametrize("use_mask", [False, True], ids=["plain", "vote"])
def test_pointcloud_runner_equals_the_one_at_a_time_loop(tree, model, collected, tmp_path, use_mask):
    config = _config(tree, tmp_path, use_mask)
    buf = io.BytesIO()
    count = pointcloud.run(config, model=model, out=buf, dropout=0)
    got = _ply_records(buf.getvalue())
    saver = pointcloud.PLYSaver(64, 96, min_d=config["min_d"], max_d=config["max_d"], batch_size=1, roi=config["roi"], dropout=0)
    saver.to(DEV)
    for e in range(2, KEYFRAMES - 2):
        entry = collected[e]
        masks = [w["mask"] for w in collected[e - 2:e + 3]] if use_mask else None
        saver.add_depthmap(entry["filtered"], entry["keyframe"], entry["intrinsics"].to(DEV), entry["pose"].to(DEV), static_masks=masks, min_hits=1)
    want = np.frombuffer(np.asarray(saver.data, dtype="<f4").tobytes(), dtype="<f4")
    assert count > 0 and got.size == 6 * count == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    without = dict(config)
    del without["consistency"]
    assert pointcloud.run(without, model=model, out=io.BytesIO(), dropout=0) > count          # the filter removed points


def test_slots_the_runner_needs_with_the_key(tree, tmp_path):
    """The buffered depths are the stream's own copies, so the filter alone asks for no spare slot; with the vote its documented rule stands."""
    from monorec_amd import MonoRecModel
    small = MonoRecModel(cv_depth_steps=STEPS, hip_in_flight=2)
    small.load_state_dict(synth.seeded_state_dict(small.state_dict(), seed=0))
    small = small.to(DEV).eval()
    with pytest.raises(ValueError, match="hip_in_flight >= 3"):
        tx.run(_config(tree, tmp_path / "x", True), model=small)
    with pytest.raises(ValueError, match="hip_in_flight >= 3"):
        tf.run(_config(tree, tmp_path / "y", True, voxel_size=0.5), model=small)
    stream = tx.KeyframeStream(_config(tree, tmp_path / "z", False), model=small)
    assert stream.depth_in_flight == 2 and stream.plan["halo"] == 2
    stream.dataset.close()
