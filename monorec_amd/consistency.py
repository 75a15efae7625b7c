"""Cross-view consistency filter of depth maps on the MI355X: a keyframe's inverse depth against the inverse depth of neighbouring keyframes,
before it goes into a point cloud, an export or a volume.

    from monorec_amd.consistency import filter_depth, relative_views
    filtered, hits = filter_depth(result, pose, intrinsics, [(result_j, pose_j, intrinsics_j), ...])

Every valid pixel is lifted to 3-D with its own depth, projected into each neighbour, compared there with the depth the neighbour predicted
(nearest pixel; relative tolerance `rel_tol`) and brought back with the neighbour's depth; a neighbour that agrees and lands within
`max_reproj_px` of the start is a hit.  Pixels with fewer than `min_views` hits are zeroed - flying pixels at depth edges, sky, reflections:
what no neighbouring keyframe confirms.  With `average` the kept pixels hold the mean depth of the pixel and its hits.  The arithmetic is
defined in include/monorec_hip.h (`mr_depth_consistency_f32`), one launch, no CPU fallback.

The runners take it as the optional config key `consistency` (`settings`): `tsdf_export.run`, `tsdf_fusion.run` and `pointcloud.run` filter
the middle keyframe of their buffer of five against the other four."""
import ctypes
import functools

import numpy as np
import torch

from . import _lib

MAX_VIEWS = _lib.MR_CONSISTENCY_MAX_VIEWS
DEFAULTS = dict(rel_tol=0.01, max_reproj_px=1.0, min_views=2, average=False)

_need_cuda = functools.partial(_lib.need_cuda, "consistency")


def settings(value):
    """The value of the runner key `consistency`, checked: None (absent) or false -> None (no filter); true -> DEFAULTS; a dict with any of
    `rel_tol`, `max_reproj_px`, `min_views`, `average` -> DEFAULTS updated by it.  Unknown sub-keys and values the launch would refuse raise."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"monorec_amd.consistency: consistency {value!r} must be false, true or a dict of {', '.join(DEFAULTS)}")
    unknown = sorted(set(value) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"monorec_amd.consistency: unknown consistency key(s) {', '.join(map(repr, unknown))} (known: {', '.join(DEFAULTS)})")
    out = dict(DEFAULTS, **value)
    out["rel_tol"], out["max_reproj_px"] = float(out["rel_tol"]), float(out["max_reproj_px"])
    if not out["rel_tol"] >= 0 or not out["max_reproj_px"] >= 0:
        raise ValueError("monorec_amd.consistency: rel_tol and max_reproj_px must be >= 0")
    if not isinstance(out["average"], bool) or isinstance(out["min_views"], bool) or int(out["min_views"]) != out["min_views"] or out["min_views"] < 0:
        raise ValueError("monorec_amd.consistency: min_views must be an integer >= 0 and average true or false")
    out["min_views"] = int(out["min_views"])
    return out


def _host(t):
    """A matrix given as a tensor anywhere, or as anything numpy takes, as a numpy array (a device tensor costs a synchronising copy)."""
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _pose64(pose, what):
    p = _host(pose)
    if p.size != 16:
        raise ValueError(f"monorec_amd.consistency: {what} must be one 4 x 4 camera -> world matrix, not {tuple(p.shape)}")
    return p.astype(np.float64).reshape(4, 4)


def _intrinsics(k, what):
    k = _host(k)
    if k.size not in (9, 16):
        raise ValueError(f"monorec_amd.consistency: {what} must be one 3 x 3 or 4 x 4 matrix, not {tuple(k.shape)}")
    k = k.astype(np.float32).reshape(k.shape[-2], k.shape[-1])
    return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])


def relative_views(pose, intrinsics, neighbours):
    """The `mr_consistency_view` array of a reference keyframe (`pose` camera -> world 4 x 4, `intrinsics` 3 x 3 or 4 x 4, anywhere) and
    `neighbours` = [(inv_depth_j or None, pose_j, intrinsics_j)]: per neighbour m = inv(pose_j) @ pose and back = inv(m), formed in
    DOUBLE on the host and rounded once to fp32 - an fp32 product of two poses of a KITTI-scale world loses the millimetres -, the
    neighbour's fx fy cx cy and the data pointer of its inverse depth (None: left NULL for the caller to fill).
    Returns ((fx, fy, cx, cy) of the reference, ctypes array of _lib.ConsistencyView)."""
    if not 1 <= len(neighbours) <= MAX_VIEWS:
        raise ValueError(f"monorec_amd.consistency: {len(neighbours)} neighbours; one launch takes 1 to {MAX_VIEWS}")
    ref = _pose64(pose, "pose")
    views = (_lib.ConsistencyView * len(neighbours))()
    m = np.linalg.inv(np.stack([_pose64(n[1], f"pose of neighbour {j}") for j, n in enumerate(neighbours)])) @ ref      # all neighbours at once
    both = np.concatenate([m[:, :3], np.linalg.inv(m)[:, :3]], axis=1).astype(np.float32)  # m, then back: 24 floats, as the structure starts
    for j, (inv_depth, _, k_j) in enumerate(neighbours):
        view = views[j]
        ctypes.memmove(ctypes.addressof(view), both[j].ctypes.data, 96)
        view.fx, view.fy, view.cx, view.cy = _intrinsics(k_j, f"intrinsics of neighbour {j}")
        view.inv_depth = None if inv_depth is None else inv_depth.data_ptr()
    return _intrinsics(intrinsics, "intrinsics"), views


def filter_depth(inv_depth, pose, intrinsics, neighbours, rel_tol=0.01, max_reproj_px=1.0, min_views=2, average=False, out=None):
    """One `mr_depth_consistency_f32` launch on the current stream.  inv_depth (H, W) or (1, 1, H, W) on the device - the model's
    `result` -, `pose` / `intrinsics` its camera -> world pose and pixel intrinsics (anywhere), `neighbours` a list of 1 to 8
    (inv_depth_j, pose_j, intrinsics_j) of the same size, checked in the order given.  `out`: a contiguous fp32 device tensor of
    inv_depth's size to write into; it must not be an input (the neighbours are read unfiltered).
    Returns (filtered - inv_depth's shape; 0 where fewer than `min_views` neighbours agree -, hits (H, W) uint8)."""
    _need_cuda(inv_depth, "inv_depth")
    if len(neighbours) > MAX_VIEWS or not neighbours:
        raise ValueError(f"monorec_amd.consistency: {len(neighbours)} neighbours; one launch takes 1 to {MAX_VIEWS}")
    h, w = int(inv_depth.shape[-2]), int(inv_depth.shape[-1])
    if inv_depth.numel() != h * w:
        raise ValueError(f"monorec_amd.consistency: inv_depth {tuple(inv_depth.shape)} must be one (H, W) or (1, 1, H, W) map")
    lib = _lib.load()
    d = inv_depth.contiguous().float()
    others = []
    for j, (dj, _, _) in enumerate(neighbours):
        _need_cuda(dj, f"inv_depth of neighbour {j}")
        if dj.numel() != h * w or tuple(dj.shape[-2:]) != (h, w) or dj.device != d.device:
            raise ValueError(f"monorec_amd.consistency: neighbour {j} {tuple(dj.shape)} is not one {h} x {w} map on {d.device}")
        others.append(dj.contiguous().float())
    if out is None:
        out = torch.empty(inv_depth.shape, dtype=torch.float32, device=d.device)
    elif (out.dtype != torch.float32 or out.numel() != h * w or out.device != d.device or not out.is_contiguous()
          or any(out.data_ptr() == t.data_ptr() for t in [d] + others)):
        raise ValueError("monorec_amd.consistency: out must be a contiguous fp32 tensor of inv_depth's size on its device, and none of the inputs")
    hits = torch.empty((h, w), dtype=torch.uint8, device=d.device)
    k, views = relative_views(pose, intrinsics, [(t, p, kj) for t, (_, p, kj) in zip(others, neighbours)])
    with torch.cuda.device(d.device):
        _lib.check(lib.mr_depth_consistency_f32(d.data_ptr(), k[0], k[1], k[2], k[3], views, len(others), float(rel_tol), float(max_reproj_px),
                                                int(min_views), int(bool(average)), h, w, out.data_ptr(), hits.data_ptr(),
                                                torch.cuda.current_stream(d.device).cuda_stream), "mr_depth_consistency_f32")
    # the launch is asynchronous: copies made here (non-contiguous or non-fp32 inputs) must outlive it - the caching allocator hands a
    # freed block only to the same stream, behind the launch, so dropping them now is safe
    return out, hits
