"""The volumes of the sparse mesh tests (tests/test_tsdf_sparse_mesh.py, tests/test_gpu_tsdf_sparse_mesh.py) as restatement dicts with an
`allocated` grid, and their expected meshes.  Nothing is restated here: the mesh of a sparse volume is `tsdf_mesh_ref.mesh` of the dense
volume it stands for - a block without storage unseen -, which `tsdf_sparse_ref.sparsify` builds.  Everything is computed once and never
modified."""
import functools

import numpy as np

import tsdf_fusion_ref as ref
import tsdf_mesh_ref as mref
import tsdf_sparse_ref as sref

B = sref.B
AXES, SEAMS, BACKGROUNDS = (0, 1, 2), (8, 7), (1, -1)
PATTERNS = [(axis, seam, background) for axis in AXES for seam in SEAMS for background in BACKGROUNDS]
NOISE_DIMS = (24, 24, 24)
NOISE_SEEDS = {3: 5, 4: 6}                     # seed of the voxels -> seed of the 60 % of the 3^3 blocks that keep storage
NOISE_SHARE = 0.6


def all_blocks(vol):
    """A dense restatement volume, padded to whole blocks, as a sparse one in which every block has storage."""
    full = sref.pad_to_blocks(vol)
    nx, ny, nz = full["dims"]
    return sref.sparsify(full, np.ones((nz // B, ny // B, nx // B), bool))


def plain(vol):
    """A copy without the colour volume."""
    out = ref.copy_volume(vol)
    out["colour"] = None
    return out


@functools.lru_cache(maxsize=None)
def pattern(axis, seam, background):
    """`mref.pattern_volume` with the cubes of all 256 sign patterns based at voxel `seam` of `axis`: 8 puts the cube's base in the next
    block and its owners one and two voxels into it, 7 puts the base in the last voxel of a block and every other corner across the face."""
    return all_blocks(mref.pattern_volume(axis, seam, background))


@functools.lru_cache(maxsize=None)
def positive_dropped(axis, colour=True):
    vol = sref.without_positive_blocks(mref.pattern_volume(axis, 8, 1))
    return vol if colour else plain(vol)


def noise_blocks(seed):
    return np.random.default_rng(NOISE_SEEDS[seed]).random((3, 3, 3)) < NOISE_SHARE


@functools.lru_cache(maxsize=None)
def noise(seed, colour=True):
    return sref.sparsify(sref.pad_to_blocks(mref.noise_volume(NOISE_DIMS, seed, colour=colour)), noise_blocks(seed))


@functools.lru_cache(maxsize=None)
def sphere():
    return all_blocks(mref.sphere_volume(**mref.SPHERE_VOLUME))


def without_blocks(vol, coords):
    """A copy of a sparse restatement volume in which the blocks `coords` (n, 3: bx by bz) have lost their storage."""
    allocated = vol["allocated"].copy()
    for bx, by, bz in np.asarray(coords).reshape(-1, 3):
        allocated[bz, by, bx] = False
    return sref.sparsify(vol, allocated)


def surface_block(vol):
    """(bx, by, bz) of the first allocated block, in table order, that holds seen voxels of both signs."""
    seen = vol["weight"] > 0
    both = sref.any_per_block(seen & (vol["tsdf"] < 0)) & sref.any_per_block(seen & ~(vol["tsdf"] < 0)) & vol["allocated"]
    bz, by, bx = (int(v[0]) for v in np.nonzero(both))
    return bx, by, bz


def cube_touches_block(cubes, block):
    """(m,) bool: the cube of base voxel cubes[i] (its corners reach one voxel further) has a corner in `block`."""
    lo = np.asarray(block) * B
    return np.all((cubes + 1 >= lo) & (cubes <= lo + B - 1), axis=1)


_mesh_cache = {}


def mesh(vol, min_weight=0.0):
    """(`mref.mesh(vol, min_weight)`, its canonical form), cached per volume object - the volumes above are shared and never modified."""
    key = (id(vol), float(min_weight))
    if key not in _mesh_cache:
        got = mref.mesh(vol, min_weight)
        _mesh_cache[key] = (vol, got, mref.canonical(got["vertices"], got["triangles"]))
    return _mesh_cache[key][1:]
