"""Helper of test_tsdf_sparse.py / test_gpu_tsdf_sparse.py: the rules of mr_tsdf_sparse_integrate_f32 / mr_tsdf_sparse_extract_f32 as
include/monorec_hip.h states them, restated in numpy on top of tsdf_fusion_ref.py.  The sparse volume is kept as the dense volume it
stands for (a block without storage holds the empty state tsdf 1, weight 0, colour 0) plus the boolean grid of allocated blocks."""
import numpy as np

import tsdf_fusion_ref as ref

F = np.float32
B = 8                                          # MR_TSDF_BLOCK

# the two volumes of the tests, in whole blocks: 6 x 4 x 6 blocks round the scene; 16 x 4 x 6, wider than any frustum
FIRST = dict(dims=(48, 32, 48), origin=(-1.3, -0.8, 0.9), voxel_size=0.06, trunc=0.18)
SECOND = dict(dims=(128, 32, 48), origin=(-3.81, -0.8, 0.9), voxel_size=0.06, trunc=0.18)
K = ref.INTRINSICS_30


def new_volume(dims, origin, voxel_size, trunc, colour=True, offset=(0, 0, 0)):
    assert all(d % B == 0 for d in dims) and all(o % B == 0 for o in offset), "whole blocks"
    vol = ref.new_volume(dims, origin, voxel_size, trunc, colour=colour, offset=offset)
    vol["allocated"] = np.zeros((dims[2] // B, dims[1] // B, dims[0] // B), bool)
    return vol


def any_per_block(mask):
    """(nz, ny, nx) bool -> (nz / 8, ny / 8, nx / 8) bool: some voxel of the block."""
    nz, ny, nx = mask.shape
    return mask.reshape(nz // B, B, ny // B, B, nx // B, B).any(axis=(1, 3, 5))


def per_voxel(blocks):
    """(nbz, nby, nbx) -> (nz, ny, nx): every block's value at each of its voxels."""
    return blocks.repeat(B, axis=0).repeat(B, axis=1).repeat(B, axis=2)


def intrinsics_of(intrinsics, count):
    """One (fx, fy, cx, cy) for all of `count` frames, or one per frame, as a list of `count`."""
    ks = np.asarray(intrinsics, dtype=np.float64)
    assert ks.shape in ((4,), (count, 4)), ks.shape
    return [tuple(ks)] * count if ks.ndim == 1 else [tuple(k) for k in ks]


def integrate_launch(vol, frames, intrinsics=K, max_depth_m=np.inf):
    """One launch of `frames` = [(cam_to_world, depth_cm, colour)] into `vol`, in place: the frames go into a trial copy with
    `ref.integrate` one by one - for a block without storage that is the empty start state -, the blocks with a voxel in some frame's
    band join the allocated set, and only allocated blocks keep the trial's values.  `intrinsics`: one (fx, fy, cx, cy), or one per
    frame.  Returns the grid of newly allocated blocks."""
    trial = ref.copy_volume(vol)
    band = np.zeros(vol["tsdf"].shape, bool)
    for (pose, depth, colour), k in zip(frames, intrinsics_of(intrinsics, len(frames))):
        band |= ref.integrate(trial, ref.world_to_camera(pose), k, depth, colour if vol["colour"] is not None else None, max_depth_m)["band"]
    new = any_per_block(band) & ~vol["allocated"]
    vol["allocated"] = vol["allocated"] | new
    keep = per_voxel(vol["allocated"])
    for key in ("tsdf", "weight") + (("colour",) if vol["colour"] is not None else ()):
        vol[key] = np.where(keep[..., None] if key == "colour" else keep, trial[key], vol[key])
    return new


def fuse(spec, frames, batch, colour=True, intrinsics=K, max_depth_m=np.inf, changed=None):
    """A new volume of `spec` after `frames` in launches of `batch`.  `changed`: a list that receives, per launch, the mask of the
    voxels whose weight the launch changed."""
    vol = new_volume(colour=colour, **spec)
    ks = intrinsics_of(intrinsics, len(frames))
    for lo in range(0, len(frames), batch):
        before = vol["weight"]
        integrate_launch(vol, frames[lo:lo + batch], ks[lo:lo + batch], max_depth_m)
        if changed is not None:
            changed.append(vol["weight"] != before)
    return vol


def dense(spec, frames, colour=True, intrinsics=K):
    """The dense restatement of the same frames."""
    vol = ref.new_volume(colour=colour, **spec)
    for pose, depth, image in frames:
        ref.integrate(vol, ref.world_to_camera(pose), intrinsics, depth, image if colour else None)
    return vol


def extract(vol, min_weight=0.0):
    """mr_tsdf_sparse_extract_f32: the dense rule on the volume `vol` stands for."""
    return ref.extract(vol, min_weight)


def blocks_of(vol):
    """The allocated blocks in the order of their table index, as `SparseTSDFVolume.blocks_host()` returns them."""
    bz, by, bx = np.nonzero(vol["allocated"])
    coords = np.stack([bx, by, bz], axis=1).astype(np.int32)

    def cut(a):
        return np.stack([a[z * B:z * B + B, y * B:y * B + B, x * B:x * B + B] for x, y, z in coords]) if len(coords) else a[:0]
    return coords, cut(vol["tsdf"]), cut(vol["weight"]), cut(vol["colour"]) if vol["colour"] is not None else None


def sparsify(vol, allocated):
    """A dense restatement volume as a sparse one with the blocks `allocated` (nbz, nby, nbx bool): the others become empty."""
    out = ref.copy_volume(vol)
    keep = per_voxel(allocated)
    out["tsdf"] = np.where(keep, vol["tsdf"], F(1.0)).astype(F)
    out["weight"] = np.where(keep, vol["weight"], F(0.0)).astype(F)
    if vol["colour"] is not None:
        out["colour"] = np.where(keep[..., None], vol["colour"], np.uint8(0)).astype(np.uint8)
    out["allocated"] = allocated.copy()
    return out


# ------------------------------------------------------------------------------------------ culls that cut
# The cases of test_culls_that_cut (GPU) and of the CPU test that proves them sharp: every kind of ref.camera_cases with every depth
# limit in both worlds on SECOND, launches of 1, 3 and 8 and both colour settings dealt round so that every value of every axis meets
# every depth limit, and four more launches of 1 (the launch box is then one frame's own).
SHIFTS = {"origin": ref.ORIGIN, "far": ref.FAR}
CULL_DEPTHS = (None, 2.0, 0.6)
# (kind, max_depth_m, shift name) -> seed where seed 0 misses a precondition (its launches change 352 and 263 voxels, fewer than 500)
CULL_SEEDS = {("offcentre", 0.6, "origin"): 1, ("offcentre", 0.6, "far"): 1, ("aniso", 0.6, "origin"): 3, ("aniso", 0.6, "far"): 3}


def _cull_cases():
    cases = []
    for ki, kind in enumerate(ref.CAMERA_KINDS):
        for di, depth in enumerate(CULL_DEPTHS):
            for si, shift in enumerate(SHIFTS):
                cases.append((kind, depth, shift, (1, 3, 8)[(ki + di + si) % 3], (ki + si) % 2 == 0))
    cases += [("rigid", 0.6, "origin", 1, False), ("scaled", 0.6, "far", 1, True), ("offcentre", 2.0, "origin", 1, False),
              ("aniso", 0.6, "far", 1, True)]
    assert len(set(cases)) == len(cases) == 40
    return cases


CULL_CASES = _cull_cases()


def cull_case_id(case):
    kind, depth, shift, batch, colour = case
    return f"{kind}-{'inf' if depth is None else depth}-{shift}-{batch}-{'colour' if colour else 'plain'}"


def cull_inputs(kind, depth, shift):
    """(spec, frames, ks, limit) of a case: SECOND moved to the case's world and ref.camera_cases' eight frames for it."""
    seed = CULL_SEEDS.get((kind, depth, shift), 0)
    frames, ks = ref.camera_cases(SECOND, seed, kind, depth, SHIFTS[shift])
    return ref.shifted(SECOND, SHIFTS[shift]), frames, ks, np.inf if depth is None else depth


# ------------------------------------------------------------------------------------------ dense restatement volumes as sparse ones
def pad_to_blocks(vol):
    """A copy of a dense restatement volume with its dims rounded up to whole blocks, the new voxels empty (tsdf 1, weight 0, colour 0):
    what `SparseTSDFVolume` makes of those dims."""
    nx, ny, nz = (-(-d // B) * B for d in vol["dims"])
    out = ref.new_volume((nx, ny, nz), vol["origin"], vol["voxel"], vol["trunc"], colour=vol["colour"] is not None)
    z, y, x = vol["tsdf"].shape
    for key in ("tsdf", "weight") + (("colour",) if vol["colour"] is not None else ()):
        out[key][:z, :y, :x] = vol[key]
    return out


def without_positive_blocks(vol):
    """`pad_to_blocks(vol)` as a sparse volume in which only the blocks that hold a seen negative voxel have storage."""
    full = pad_to_blocks(vol)
    return sparsify(full, any_per_block((full["tsdf"] < 0) & (full["weight"] > 0)))
