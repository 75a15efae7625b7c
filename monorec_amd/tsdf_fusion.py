"""TSDF fusion on the MI355X: the keyframes `tsdf_export` packs, integrated into a dense voxel volume in device memory, and the
surface at its zero crossings, as points or as a welded triangle mesh - the step the export's files were written for, without the files.

    from monorec_amd.tsdf_fusion import TSDFVolume, bounds_from_frusta, fuse_directory, run
    python -m monorec_amd.tsdf_fusion --config configs/test/pointcloud_monorec.json

`TSDFVolume` owns three device arrays, x fastest (`idx = (z * ny + y) * nx + x`): `tsdf` fp32 (1 = far in front of any surface),
`weight` fp32 (number of keyframes that saw the voxel) and optionally `colour` (r, g, b, 0 bytes).  `integrate()` is one launch
(`mr_tsdf_integrate_f32`) per up to 8 keyframes: int16 centimetre depth and interleaved byte colour exactly as `mr_tsdf_frame_f32` /
`tsdf_export.pack_frames` leave them, a camera -> world pose (inverted on the host in fp32) and the pixel intrinsics.  The
arithmetic - a running average of the truncated signed distance along the camera's z axis - is written out operation by operation in
include/monorec_hip.h and restated in numpy by tests/tsdf_fusion_ref.py; the device result equals it bit for bit.  `extract()` returns
the points where an edge of the grid crosses zero between two seen voxels (`mr_tsdf_extract_f32`: count, then fill), as the x y z r g b
records `pointcloud.PLYSaver` writes.  `mesh()` returns the same surface as an indexed triangle mesh (`mr_tsdf_mesh_vertices_f32`,
`mr_tsdf_mesh_triangles_f32`: marching tetrahedra over the Kuhn split of every cube of eight voxels - six tetrahedra per cube, a
16-case table instead of marching cubes' 256, no ambiguous cases, so the mesh is a closed 2-manifold wherever the voxels are seen,
at the price of about twice the triangles of marching cubes).  Every vertex lies on one of seven edges its voxel owns, so the mesh
comes out welded by construction, with no hashing and no sort; the vertices on the three axis edges are `extract()`'s records.  The
rules are in include/monorec_hip.h, restated in numpy by tests/tsdf_mesh_ref.py.  `render()` casts the volume back into one camera or a
batch (`mr_tsdf_render_f32`: a thread per pixel marches its ray in camera-z steps to the first crossing from non-negative to negative
trilinear tsdf) and returns depth, the unit surface normal (the interpolant's gradient, in world axes) and colour per pixel;
`render_result()` is that depth as the model's inverse-depth `result`, 0 where nothing was hit, for `metrics.*_sparse_onlyvalid_metric`.
`skip_grid()` (`mr_tsdf_skip_grid_u8`) is a byte per brick of 4^3 voxels that lets the march pass empty space with one load per sample
and changes no bit of the result; header and tests/tsdf_render_ref.py as above.  There is no CPU fallback: CPU tensors raise.

`SparseTSDFVolume` is the same volume for scenes whose dense grid does not fit (200 m x 200 m x 40 m of road at 0.1 m are 19 GB): a
direct-indexed table of blocks of 8^3 voxels and a pool that holds only the blocks some keyframe put within the truncation band of a
surface (`mr_tsdf_sparse_integrate_f32`, the dense kernel's arithmetic through csrc/tsdf_common.h).  It has the integrate methods and
`extract` / `count` / `save_ply` (`mr_tsdf_sparse_extract_f32`) and `render` / `render_result` (`mr_tsdf_sparse_render_f32`: the dense
march through the table, bit for bit the render of the gathered volume) and `mesh` / `mesh_counts` / `save_mesh_ply`
(`mr_tsdf_sparse_mesh_vertices_f32`, `mr_tsdf_sparse_mesh_triangles_f32`: the dense mesh of the gathered volume as a canonical mesh, from
the blocks themselves, with 4 bytes of workspace per pool voxel) of `TSDFVolume`; `to_dense()` (`mr_tsdf_sparse_gather_f32`) hands any
region that fits to the dense class, which nothing needs any more.  The runner key `sparse_volume` selects it, `sparse_render` renders
and scores it and `sparse_mesh` meshes it without the dense copy.

`run(config)` takes the configs of `pointcloud.run` / `tsdf_export.run` and drives the same pipelined loop
(`tsdf_export.KeyframeStream`): per keyframe one pack launch into a staging slot on the device, per `fuse_batch` keyframes one
integrate launch on the same stream; nothing is copied to the host before the surface is written.  With `fused_metrics` in the config,
`Fusion.score()` renders the fused volume into every exported keyframe again and scores it against the dataset's targets; with
`render_dir`, `write()` also writes those views as 16-bit centimetre PNGs and JPEGs.

`mesh(normals=True)` adds a unit normal per vertex (the gradient of the tsdf at the two ends of the vertex's edge, interpolated like
its position), `mesh(cell=2 | 4 | 8)` returns a clustered level of detail: one vertex per cluster of cell^3 voxels that owns a vertex
of the full mesh, and the full mesh's triangles between three different clusters (`mr_tsdf_mesh_cluster_vertices_f32`,
`mr_tsdf_mesh_cluster_triangles_f32` and their `mr_tsdf_sparse_` twins; a cluster is summed as a tree of a fixed shape, so there are no
float atomics and tests/tsdf_mesh_lod_ref.py pins the result bit for bit).  The runner keys `mesh_cell` and `mesh_normals` pass them to the
mesh file.

Not here: quadric or edge-collapse decimation, marching cubes; repeated triangles of a clustered mesh are kept (removing one would
leave a directed edge without its reverse); a mesh of a region of the sparse volume (it meshes the whole of it), growth of its pool,
eviction or hashing; a cap on the weight; fusing across ranks (`run` is single-process)."""
import contextlib
import ctypes
import functools
import math
import os
import re

import numpy as np
import torch

from . import _lib
from . import tsdf_export as tx
from .pointcloud import write_mesh_ply, write_ply

MAX_FRAMES = _lib.MR_TSDF_MAX_FRAMES          # keyframes per integrate launch
TILE = _lib.MR_TSDF_TILE                      # (x, y, z) voxels of one workgroup of the integrate kernel: the unit of its frustum culling
BLOCK = _lib.MR_TSDF_BLOCK                    # edge of one block of `SparseTSDFVolume` in voxels
BRICK = _lib.MR_TSDF_BRICK                    # edge of one brick of `TSDFVolume.skip_grid` in voxels
MESH_CELLS = _lib.MR_TSDF_MESH_CELLS          # the `cell` of `mesh`: 1 (the full mesh) or the cluster edge of a level of detail, in voxels
CLUSTER_TILE = _lib.MR_TSDF_CLUSTER_TILE      # (x, y, z) voxels of one workgroup of the dense volume's clustered vertex kernel
MAX_RENDER_SAMPLES = 1 << 20                  # samples per ray of one render launch


_need_cuda = functools.partial(_lib.need_cuda, "tsdf_fusion")


def _matrix(m, what):
    """A 4 x 4 (or 3 x 3 / 3 x 4) matrix from anywhere as fp32 on the host."""
    m = torch.as_tensor(m).detach().to("cpu", torch.float32)
    if m.dim() != 2:
        raise ValueError(f"{what}: expected one matrix, got shape {tuple(m.shape)}")
    return m


def _host_batches(cam_to_world, intrinsics):
    """Poses (B, 4, 4), intrinsics (n, 3 x 3 / 4 x 4) from anywhere as fp32 on the host, and B; whether n is 1 or B the caller checks."""
    poses = torch.as_tensor(cam_to_world).detach().to("cpu", torch.float32).reshape(-1, 4, 4)
    ks = torch.as_tensor(intrinsics).detach().to("cpu", torch.float32)
    return poses, ks.reshape(-1, ks.shape[-2], ks.shape[-1]), poses.shape[0]


def _set_intrinsics(view, k):
    view.fx, view.fy, view.cx, view.cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])


def _write(file, writer, *arrays):
    """writer(f, *arrays) into `file`: a binary file object, or a path."""
    with (contextlib.nullcontext(file) if hasattr(file, "write") else open(file, "wb")) as f:
        writer(f, *arrays)


# ------------------------------------------------------------------------------------------ geometry on the host
def bounds_from_frusta(cam_to_world_list, intrinsics, height, width, max_depth_m, voxel_size=0.1):
    """The axis-aligned box, in double on the host, of every camera centre and of the four image-corner rays at depth `max_depth_m`
    (corners of the pixel grid's outline, (-.5, -.5) .. (width - .5, height - .5): what rounds into the image) - it contains every
    point a keyframe can see within `max_depth_m`.  `intrinsics`: one matrix, or one per pose (a list or a stacked array).  Rounded
    outwards to whole multiples of `voxel_size`.
    Returns ((x0, y0, z0), (x1, y1, z1))."""
    if isinstance(intrinsics, (list, tuple)):
        intrinsics = np.stack([np.asarray(torch.as_tensor(k).detach().cpu().numpy(), dtype=np.float64) for k in intrinsics])
    ks = np.asarray(torch.as_tensor(intrinsics).detach().cpu().numpy(), dtype=np.float64)
    ks = ks.reshape(-1, ks.shape[-2], ks.shape[-1])
    poses = list(cam_to_world_list)
    if not poses:
        raise ValueError("bounds_from_frusta: no poses")
    if ks.shape[0] not in (1, len(poses)):
        raise ValueError(f"bounds_from_frusta: {len(poses)} poses but {ks.shape[0]} intrinsics (one, or one per pose)")
    depth, voxel = float(max_depth_m), float(voxel_size)
    if not (depth > 0 and math.isfinite(depth)) or not voxel > 0:
        raise ValueError("bounds_from_frusta: max_depth_m must be positive and finite, voxel_size positive")
    points = []
    for i, pose in enumerate(poses):
        k = ks[i if ks.shape[0] > 1 else 0]
        fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
        corners = np.array([[(u - cx) / fx * depth, (v - cy) / fy * depth, depth, 1.0]
                            for u in (-0.5, width - 0.5) for v in (-0.5, height - 0.5)] + [[0.0, 0.0, 0.0, 1.0]])
        t = np.asarray(torch.as_tensor(pose).detach().cpu().numpy(), dtype=np.float64).reshape(4, 4)
        points.append((corners @ t.T)[:, :3])
    points = np.concatenate(points)
    lo = np.floor(points.min(axis=0) / voxel) * voxel
    hi = np.ceil(points.max(axis=0) / voxel) * voxel
    return tuple(float(v) for v in lo), tuple(float(v) for v in hi)


def dims_of_bounds(bounds, voxel_size):
    """Voxels per axis whose points `lo + i * voxel_size` cover [lo, hi]: `round-up((hi - lo) / voxel_size) + 1`."""
    lo, hi = (np.asarray(b, dtype=np.float64) for b in bounds)
    if lo.shape != (3,) or hi.shape != (3,) or not np.all(hi >= lo):
        raise ValueError(f"bounds {bounds}: expected ((x0, y0, z0), (x1, y1, z1)) with hi >= lo")
    return tuple(int(math.ceil(float(d) / float(voxel_size) - 1e-9)) + 1 for d in hi - lo)


def _mesh_options(cell, normals):
    """`cell` checked, and the keywords of `mesh` that differ from its defaults: none for the full mesh without normals."""
    if isinstance(cell, bool) or cell not in MESH_CELLS:
        raise ValueError(f"monorec_amd.tsdf_fusion: cell {cell!r} must be one of {', '.join(str(c) for c in MESH_CELLS)} "
                         f"(1: the full mesh; the others divide the block of {BLOCK} voxels)")
    more = {} if cell == 1 else {"cell": int(cell)}
    if normals:
        more["normals"] = True
    return more


def volume_bytes(dims, colour=True):
    return int(dims[0]) * int(dims[1]) * int(dims[2]) * (12 if colour else 8)


# ------------------------------------------------------------------------------------------ the volume
class _Volume:
    """What `TSDFVolume` and `SparseTSDFVolume` share: the geometry of the constructor, the host half of the integration (checks, pose
    inverse, `mr_tsdf_view` arrays), the count-then-fill protocol and the launches of the surface points and of the mesh, and the host
    half of the ray-cast (poses, intrinsics, `mr_tsdf_ray_view` arrays, outputs, the defaults of the range).  A subclass has
    `_integrate_launch` (one launch of its integrate entry), `_SURFACE_ENTRIES` (the names of its extract, mesh-vertex and mesh-triangle
    entries), `_surface_args` (what those entries take ahead of the origin: the volume, or the table, the pool, `block_of_slot` and the
    slots - with the colour, and without it for the triangle entry), `_mesh_voxels`, `_render_shared` (what the launches of one `render`
    call share, made before the first) and `_render_launch` (one launch of its render entry)."""

    def _geometry(self, bounds, voxel_size, trunc, origin, dims):
        """Sets dims, origin, voxel_size and trunc as the entries will see them (fp32); returns voxel_size as given."""
        voxel_size = float(voxel_size)
        if not voxel_size > 0:
            raise ValueError(f"voxel_size {voxel_size}: must be positive")
        if (bounds is None) == (origin is None or dims is None):
            raise ValueError(f"{type(self).__name__}: give either bounds or origin and dims")
        if bounds is not None:
            origin, dims = bounds[0], dims_of_bounds(bounds, voxel_size)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f"dims {dims}: expected three sizes of at least 1")
        self.origin = tuple(float(np.float32(v)) for v in origin)
        self.voxel_size = float(np.float32(voxel_size))
        self.trunc = float(np.float32(5 * voxel_size if trunc is None else trunc))
        if not self.trunc > 0:
            raise ValueError(f"trunc {trunc}: must be positive")
        return voxel_size

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def drop_skip_grids(self):
        pass

    # -- integrate
    def integrate(self, depth_cm, colour, cam_to_world, intrinsics, max_depth_m=None):
        """Integrate one keyframe or a batch, in order: depth_cm (h, w) / (B, h, w) int16 centimetres (0: no depth), colour (h, w, 3) /
        (B, h, w, 3) uint8 (None for a volume without colour) - the two outputs of `tsdf_export.pack_frames` -, cam_to_world (4, 4) /
        (B, 4, 4) anywhere, intrinsics one 3 x 3 / 4 x 4 matrix of the packed image or one per keyframe.  `max_depth_m`: depths beyond
        it are ignored.  Launches of at most 8 keyframes on the current stream."""
        _need_cuda(depth_cm, "depth_cm")
        if depth_cm.dim() == 2:
            depth_cm = depth_cm.unsqueeze(0)
            colour = None if colour is None else colour.unsqueeze(0)
        b = depth_cm.shape[0]
        poses, ks, count = _host_batches(cam_to_world, intrinsics)
        if count != b or ks.shape[0] not in (1, b) or (colour is not None and colour.shape[0] != b):
            raise ValueError(f"integrate: {b} depth maps, {count} poses, {ks.shape[0]} intrinsics"
                             + ("" if colour is None else f", {colour.shape[0]} colour images"))
        self.integrate_views([(depth_cm[i], None if colour is None else colour[i], poses[i], ks[i if ks.shape[0] == b else 0])
                              for i in range(b)], max_depth_m)

    def integrate_views(self, views, max_depth_m=None):
        """The same for a list of (depth_cm (h, w), colour (h, w, 3) | None, cam_to_world, intrinsics) whose arrays need not be slices
        of one tensor (the runner's staging slots)."""
        self.integrate_prepared(self.prepare_views(views), max_depth_m)

    def prepare_views(self, views):
        """The host half of `integrate_views`: checks, the fp32 inverse of every pose and the `mr_tsdf_view` arrays of the launches (at
        most 8 views each).  Returns what `integrate_prepared` launches; it keeps the images alive."""
        keep, frames, size = [], [], None
        for depth, colour, pose, k in views:
            _need_cuda(depth, "depth_cm")
            if depth.dtype != torch.int16 or depth.dim() != 2:
                raise ValueError(f"depth_cm: expected (h, w) int16, got {tuple(depth.shape)} {depth.dtype}")
            if size is None:
                size = tuple(depth.shape)
            if tuple(depth.shape) != size:
                raise ValueError("integrate: the keyframes of one call must have one size")
            depth = depth.contiguous()
            if self.has_colour:
                if colour is None:
                    raise ValueError("integrate: this volume has colour; pass the packed colour image (or build it with colour=False)")
                _need_cuda(colour, "colour")
                if colour.dtype != torch.uint8 or tuple(colour.shape) != size + (3,):
                    raise ValueError(f"colour: expected {size + (3,)} uint8, got {tuple(colour.shape)} {colour.dtype}")
                colour = colour.contiguous()
            else:
                colour = None
            view = _lib.TsdfView()
            _set_intrinsics(view, _matrix(k, "intrinsics"))
            m = torch.inverse(_matrix(pose, "cam_to_world").reshape(4, 4))          # world -> camera, fp32 on the host
            view.m[:] = [float(v) for v in m[:3, :4].reshape(-1)]
            view.depth_cm = depth.data_ptr()
            view.colour = colour.data_ptr() if colour is not None else None
            frames.append(view)
            keep.append((depth, colour))
        arrays = [(_lib.TsdfView * len(frames[lo:lo + MAX_FRAMES]))(*frames[lo:lo + MAX_FRAMES]) for lo in range(0, len(frames), MAX_FRAMES)]
        return dict(arrays=arrays, size=size, count=len(frames), keep=keep)

    def integrate_prepared(self, prepared, max_depth_m=None):
        """The launches of `prepare_views`' result, on the current stream."""
        lib = _lib.load()
        limit = float("inf") if max_depth_m is None else float(max_depth_m)
        with torch.cuda.device(self.device):
            for array in prepared["arrays"]:
                self._integrate_launch(lib, array, limit, prepared["size"])
        self._keep = prepared["keep"]                          # alive until the launches have run (same stream: the next call may drop them)
        self.drop_skip_grids()
        self.frames += prepared["count"]

    # -- surface points
    def extract(self, min_weight=0):
        """(n, 6) fp32 on the device: x y z red green blue of every edge crossing between two voxels of weight > min_weight.  Two
        launches (count, fill) and one read of the count.  The order of the records is unspecified."""
        count = self.count(min_weight)
        records = torch.empty(count, 6, dtype=torch.float32, device=self.device)
        if count and self._extract_launch(min_weight, records) != count:
            raise RuntimeError("monorec_amd.tsdf_fusion: the volume changed between the count and the fill launch")
        return records

    def count(self, min_weight=0):
        """Number of records `extract(min_weight)` would return (the count launch alone)."""
        return self._extract_launch(min_weight)

    def _extract_launch(self, min_weight, records=None):
        """One launch of the extract entry on the current stream - counting, or filling `records` - and the read of its cursor."""
        cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        out = (None, 0) if records is None else (records.data_ptr(), records.shape[0])
        name = self._SURFACE_ENTRIES[0]
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), name)(*self._surface_args()[0], self._origin, self.voxel_size, float(min_weight), *out,
                                                  cursor.data_ptr(), self._stream()), name)
        return int(cursor.item())

    def save_ply(self, file, min_weight=0):
        """The surface points as a binary .ply (pointcloud.PLYSaver's header and records) to a path or a binary file object.  Returns
        the number of vertices."""
        records = self.extract(min_weight).cpu().numpy()
        _write(file, write_ply, records.reshape(-1))
        return records.shape[0]

    # -- the surface as a mesh
    def mesh_counts(self, min_weight=0, cell=1):
        """(vertices, triangles) `mesh(min_weight, cell)` would return: the two count launches and one read."""
        more = _mesh_options(cell, False)
        cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self._mesh_launches(min_weight, cursor, **more)
        n, m = cursor.tolist()
        return int(n), int(m)

    def mesh(self, min_weight=0, cell=1, normals=False):
        """The zero-crossing surface between voxels of weight > min_weight as a welded triangle mesh on the device: vertices (n, 6) fp32
        x y z red green blue - those on the grid's axis edges are `extract(min_weight)`'s records - and triangles (m, 3) int32 indices
        into them, wound so that (b - a) x (c - a) points from inside (tsdf < 0) to outside.  Marching tetrahedra: closed wherever the
        voxels are seen, about twice the triangles of marching cubes.  A count launch per array, one read of both counts, a fill launch per
        array; 4 bytes per voxel of workspace for the time of the call - per voxel of the grid for `TSDFVolume`, per voxel of the allocated
        blocks for `SparseTSDFVolume`, which meshes its blocks as they are (`mr_tsdf_sparse_mesh_vertices_f32`,
        `mr_tsdf_sparse_mesh_triangles_f32`).  The order of both arrays is unspecified.

        `normals=True` returns (vertices, triangles, vertex_normals): (n, 3) fp32, unit length or exactly 0 - the gradient of the tsdf
        (central differences, one-sided where a neighbour is outside the grid, unseen or without storage) at the two ends of the
        vertex's edge, interpolated like its position; it points where the winding does.  `cell` = 2, 4 or 8 returns a level of
        detail: the voxels are grouped into clusters of cell^3, every cluster that owns a vertex of the full mesh emits one vertex -
        the mean position and colour of those it owns, the normalised sum of their normals - and every triangle of the full mesh
        between three different clusters is kept, with its winding; the others are dropped.  Every directed edge is still matched by
        its reverse wherever the full mesh is closed; triangles that repeat are kept, or that would break.  The sums run in one fixed
        order (include/monorec_hip.h; tests/tsdf_mesh_lod_ref.py restates them), so the result is deterministic.  The workspace is 4
        bytes per cluster.  `cell=1, normals=False` is exactly the call without them.  Another cell raises a ValueError."""
        more = _mesh_options(cell, normals)
        n, m = self.mesh_counts(min_weight, cell)
        if n >= 2 ** 31:
            raise ValueError(f"monorec_amd.tsdf_fusion: a mesh of {n} vertices does not fit int32 indices; raise min_weight or mesh a part")
        vertices = torch.empty(n, 6, dtype=torch.float32, device=self.device)
        triangles = torch.empty(m, 3, dtype=torch.int32, device=self.device)
        if normals:
            more["normals"] = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        if n:
            cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
            vertex_base = torch.empty(self._mesh_voxels() if cell == 1 else self._mesh_clusters(cell), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                self._mesh_launches(min_weight, cursor, vertices, triangles, vertex_base, **more)
            if cursor.tolist() != [n, m]:
                raise RuntimeError("monorec_amd.tsdf_fusion: the volume changed between the count and the fill launches")
        return (vertices, triangles, more["normals"]) if normals else (vertices, triangles)

    def _mesh_launches(self, min_weight, cursor, vertices=None, triangles=None, vertex_base=None, cell=1, normals=None):
        """The two mesh entries on the current stream, the vertex one first: counting (no outputs) or filling.  `cell` > 1: the cluster
        entries, with `vertex_base` their cluster_base; `normals`: the tensor the vertex entry fills beside `vertices`."""
        lib, nothing = _lib.load(), (None, 0)
        _, vertex_entry, triangle_entry = self._SURFACE_ENTRIES
        with_colour, without_colour = self._surface_args(vertex_base, cell)
        base = vertex_base.data_ptr() if vertex_base is not None else None
        out = nothing if vertices is None else (vertices.data_ptr(), vertices.shape[0])
        cells, beside = (), ()
        if cell != 1:
            vertex_entry, triangle_entry = (name.replace("_mesh_", "_mesh_cluster_") for name in (vertex_entry, triangle_entry))
            cells, beside = (int(cell),), (normals.data_ptr() if normals is not None else None,)
        elif normals is not None:
            vertex_entry, beside = vertex_entry.replace("_vertices_", "_vertices_normals_"), (normals.data_ptr(),)
        if vertices is None or vertices.shape[0]:
            _lib.check(getattr(lib, vertex_entry)(*with_colour, self._origin, self.voxel_size, float(min_weight), *cells, out[0], out[1], *beside,
                                                  base, cursor.data_ptr(), self._stream()), vertex_entry)
        out = nothing if triangles is None else (triangles.data_ptr(), triangles.shape[0])
        if triangles is None or triangles.shape[0]:
            _lib.check(getattr(lib, triangle_entry)(*without_colour, float(min_weight), *cells, base, out[0], out[1], cursor.data_ptr() + 8,
                                                    self._stream()), triangle_entry)

    def save_mesh_ply(self, file, min_weight=0, cell=1, normals=False):
        """The mesh as a binary .ply (`pointcloud.write_mesh_ply`) to a path or a binary file object; `cell` and `normals` as for `mesh`,
        the normals as the properties nx ny nz.  Returns (vertices, triangles)."""
        arrays = [t.cpu().numpy() for t in self.mesh(min_weight, **_mesh_options(cell, normals))]
        _write(file, write_mesh_ply, *arrays)
        return arrays[0].shape[0], arrays[1].shape[0]

    # -- the volume seen from a camera
    def render(self, cam_to_world, intrinsics, height, width, t_min=0.0, t_max=None, step=None, min_weight=0, normals=True, colour=True,
               skip=True):
        """Ray-cast the volume into one camera or a batch: cam_to_world (4, 4) / (B, 4, 4) anywhere, intrinsics one 3 x 3 / 4 x 4 matrix
        or one per pose, images of height x width.  Every ray is sampled at camera-z depths t_min, t_min + step, ... <= t_max metres
        (`step` defaults to the voxel size, `t_max` to t_min plus the volume's diagonal) and ends at the first crossing from
        non-negative to negative tsdf between two samples whose 8 corners all have weight > min_weight (`mr_tsdf_render_f32`,
        `mr_tsdf_sparse_render_f32`; the arithmetic is in include/monorec_hip.h).  Launches of at most 8 views on the current stream.
        Returns dict(depth (B, h, w) fp32 metres, 0 where nothing was hit, normal (B, h, w, 3) fp32 unit vectors in world axes pointing
        out of the surface | None, colour (B, h, w, 3) uint8 | None) on the device.  `skip`: `TSDFVolume` marches with
        `skip_grid(min_weight)`, which changes no bit of the result; `SparseTSDFVolume` accepts and ignores it (a sample in a block
        without storage costs one table entry as it is)."""
        poses, ks, b = _host_batches(cam_to_world, intrinsics)
        height, width = int(height), int(width)
        if b < 1 or ks.shape[0] not in (1, b):
            raise ValueError(f"render: {b} poses, {ks.shape[0]} intrinsics (one, or one per pose)")
        if height < 1 or width < 1:
            raise ValueError(f"render: an image of {height} x {width}")
        t_min = float(t_min)
        step = self.voxel_size if step is None else float(step)
        if t_max is None:
            t_max = t_min + self.voxel_size * math.sqrt(sum(d * d for d in self.dims))
        march = (t_min, float(t_max), step)
        shared = self._render_shared(march, min_weight, skip)
        depth = torch.empty(b, height, width, dtype=torch.float32, device=self.device)
        normal = torch.empty(b, height, width, 3, dtype=torch.float32, device=self.device) if normals else None
        image = torch.empty(b, height, width, 3, dtype=torch.uint8, device=self.device) if colour else None
        views = []
        for i in range(b):
            view = _lib.TsdfRayView()
            view.m[:] = [float(v) for v in poses[i][:3, :4].reshape(-1)]
            _set_intrinsics(view, ks[i if ks.shape[0] == b else 0])
            view.depth = depth[i].data_ptr()
            view.normal = normal[i].data_ptr() if normals else None
            view.colour = image[i].data_ptr() if colour else None
            views.append(view)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            for lo in range(0, b, MAX_FRAMES):
                chunk = views[lo:lo + MAX_FRAMES]
                self._render_launch(lib, (_lib.TsdfRayView * len(chunk))(*chunk), (height, width), march, float(min_weight), shared)
        return dict(depth=depth, normal=normal, colour=image)

    def render_result(self, cam_to_world, intrinsics, height, width, **kwargs):
        """The rendered depth in the model's `result` convention: (B, 1, h, w) inverse depth, 0 where nothing was hit - what
        `metrics.*_sparse_onlyvalid_metric` (`pred_all_valid=False`) scores.  Keywords as `render` (normals and colour are not rendered)."""
        depth = self.render(cam_to_world, intrinsics, height, width, **dict(kwargs, normals=False, colour=False))["depth"]
        return torch.where(depth > 0, 1.0 / depth, torch.zeros_like(depth)).unsqueeze(1)


class TSDFVolume(_Volume):
    """A dense TSDF volume on the device.  Give `bounds` = ((x0, y0, z0), (x1, y1, z1)) - e.g. from `bounds_from_frusta` - or `origin`
    and `dims` = (nx, ny, nz); `voxel_size` in metres; `trunc` (default 5 voxels) the truncation distance.  A volume above `max_bytes`
    raises a ValueError that names the voxel size that would fit.  `storage` = (tsdf, weight, colour | None): use these device tensors
    (flat, of nx * ny * nz elements / x 4 bytes) instead of allocating - they are reset too."""

    def __init__(self, bounds=None, voxel_size=0.1, trunc=None, colour=True, device="cuda:0", max_bytes=8 << 30, origin=None, dims=None,
                 storage=None):
        voxel_size = self._geometry(bounds, voxel_size, trunc, origin, dims)
        self.has_colour = bool(colour)
        need = volume_bytes(self.dims, self.has_colour)
        if need > int(max_bytes):
            extent = [(d - 1) * voxel_size for d in self.dims]
            box, fits = ((0.0, 0.0, 0.0), tuple(extent)), voxel_size
            while volume_bytes(dims_of_bounds(box, float(f"{fits:.3g}")), self.has_colour) > int(max_bytes):
                fits *= 1.01
            raise ValueError(f"TSDFVolume: {self.dims[0]} x {self.dims[1]} x {self.dims[2]} voxels of {voxel_size:g} m need {need / 2 ** 30:.2f} GiB, "
                             f"more than max_bytes = {int(max_bytes) / 2 ** 30:.2f} GiB; a voxel size of {float(f'{fits:.3g}'):g} m would fit")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("monorec_amd.tsdf_fusion: the volume lives on a CUDA (HIP) device - there is no CPU fallback")
        n = self.dims[0] * self.dims[1] * self.dims[2]
        if storage is None:
            self.tsdf = torch.empty(n, dtype=torch.float32, device=self.device)
            self.weight = torch.empty(n, dtype=torch.float32, device=self.device)
            self.colour = torch.empty(n, 4, dtype=torch.uint8, device=self.device) if self.has_colour else None
        else:
            self.tsdf, self.weight, self.colour = storage
            for t, what in ((self.tsdf, "tsdf"), (self.weight, "weight")) + (((self.colour, "colour"),) if self.has_colour else ()):
                _need_cuda(t, what)
                if not t.is_contiguous() or t.numel() != (n * 4 if what == "colour" else n) or \
                        t.dtype != (torch.uint8 if what == "colour" else torch.float32):
                    raise ValueError(f"storage: {what} must be a contiguous tensor of the volume's size and type")
            if not self.has_colour:
                self.colour = None
        self._origin = (ctypes.c_float * 3)(*self.origin)
        self._keep = None
        self._skip = {}                                        # min_weight -> skip_grid(min_weight), dropped by whatever writes the volume
        self.frames = 0                                        # keyframes integrated so far
        self.reset()

    def _volume_args(self):
        return (self.tsdf.data_ptr(), self.weight.data_ptr(), self.colour.data_ptr() if self.colour is not None else None, *self.dims)

    def reset(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mr_tsdf_volume_reset_f32(*self._volume_args(), self._stream()), "mr_tsdf_volume_reset_f32")
        self.frames = 0
        self.drop_skip_grids()

    def _integrate_launch(self, lib, array, limit, size):
        _lib.check(lib.mr_tsdf_integrate_f32(*self._volume_args(), self._origin, self.voxel_size, self.trunc, limit, array, len(array),
                                             size[0], size[1], self._stream()), "mr_tsdf_integrate_f32")

    # -- surface
    _SURFACE_ENTRIES = ("mr_tsdf_extract_f32", "mr_tsdf_mesh_vertices_f32", "mr_tsdf_mesh_triangles_f32")

    def _surface_args(self, vertex_base=None, cell=1):
        args = self._volume_args()
        return args, args[:2] + args[3:]

    def _mesh_voxels(self):
        """Elements of `mesh()`'s vertex_base: one per voxel of the grid."""
        return self.tsdf.numel()

    def _mesh_clusters(self, cell):
        """Elements of `mesh(cell=...)`'s cluster_base: one per cluster of the grid, partial ones on the high side included."""
        return math.prod((d + cell - 1) // cell for d in self.dims)

    # -- the volume seen from a camera
    def skip_grid(self, min_weight=0):
        """(bz, by, bx) uint8 on the device, one byte per brick of `BRICK`^3 voxels: 1 where a voxel of weight > min_weight and negative
        tsdf lies in the brick or on its + faces (`mr_tsdf_skip_grid_u8`: one sweep of the volume).  Cached per `min_weight` until the
        volume is written through this object (`integrate*`, `reset`, `load`); call `drop_skip_grids()` after writing the arrays directly."""
        key = float(np.float32(min_weight))
        if key != key:
            raise ValueError("skip_grid: min_weight is NaN")
        grid = self._skip.get(key)
        if grid is None:
            shape = tuple((d + BRICK - 1) // BRICK for d in reversed(self.dims))
            grid = torch.empty(shape, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().mr_tsdf_skip_grid_u8(self.tsdf.data_ptr(), self.weight.data_ptr(), *self.dims, key, grid.data_ptr(),
                                                            self._stream()), "mr_tsdf_skip_grid_u8")
            self._skip[key] = grid
        return grid

    def drop_skip_grids(self):
        self._skip = {}

    def _render_shared(self, march, min_weight, skip):
        return self.skip_grid(min_weight).data_ptr() if skip else None            # the bricks

    def _render_launch(self, lib, array, size, march, min_weight, bricks):
        _lib.check(lib.mr_tsdf_render_f32(*self._volume_args(), self._origin, self.voxel_size, min_weight, bricks, array, len(array), *size,
                                          *march, self._stream()), "mr_tsdf_render_f32")

    # -- the volume itself
    def grids(self):
        """Host copies shaped (nz, ny, nx): tsdf, weight, colour (nz, ny, nx, 4) or None."""
        nx, ny, nz = self.dims
        colour = self.colour.cpu().numpy().reshape(nz, ny, nx, 4) if self.colour is not None else None
        return self.tsdf.cpu().numpy().reshape(nz, ny, nx), self.weight.cpu().numpy().reshape(nz, ny, nx), colour

    def save(self, file):
        """.npz: tsdf, weight (nz, ny, nx) fp32, colour (nz, ny, nx, 4) uint8 if any, origin, dims (nx, ny, nz), voxel_size, trunc."""
        tsdf, weight, colour = self.grids()
        arrays = dict(tsdf=tsdf, weight=weight, origin=np.asarray(self.origin, dtype=np.float32), dims=np.asarray(self.dims, dtype=np.int64),
                      voxel_size=np.float32(self.voxel_size), trunc=np.float32(self.trunc), frames=np.int64(self.frames))
        if colour is not None:
            arrays["colour"] = colour
        np.savez(file, **arrays)

    @classmethod
    def load(cls, file, device="cuda:0", max_bytes=8 << 30):
        with np.load(file) as z:
            volume = cls(origin=z["origin"], dims=z["dims"], voxel_size=float(z["voxel_size"]), trunc=float(z["trunc"]),
                         colour="colour" in z.files, device=device, max_bytes=max_bytes)
            volume.tsdf.copy_(torch.from_numpy(z["tsdf"].reshape(-1)))
            volume.weight.copy_(torch.from_numpy(z["weight"].reshape(-1)))
            if volume.colour is not None:
                volume.colour.copy_(torch.from_numpy(z["colour"].reshape(-1, 4)))
            volume.frames = int(z["frames"]) if "frames" in z.files else 0
            volume.drop_skip_grids()
        return volume


# ------------------------------------------------------------------------------------------ the block-sparse volume
def sparse_bytes(blocks, capacity, colour=True):
    """Device bytes of a sparse volume of `blocks` = (nbx, nby, nbz) blocks with a pool of `capacity` slots: 4 per table entry, and per
    slot 512 voxels of 12 (8 without colour) bytes plus its 4 bytes of `block_of_slot`."""
    return 4 * int(blocks[0]) * int(blocks[1]) * int(blocks[2]) + int(capacity) * (BLOCK ** 3 * (12 if colour else 8) + 4)


class SparseTSDFVolume(_Volume):
    """A block-sparse TSDF volume on the device: storage only for the blocks of `BLOCK`^3 = 8 x 8 x 8 voxels that some keyframe puts
    within the truncation band of a surface - for scenes whose dense grid `TSDFVolume` refuses.  A direct-indexed `table` of one int32
    per block (-1: no storage, else a slot; no hashing) and a pool of `capacity_blocks` slots (`tsdf`, `weight`, `colour` of 512 voxels
    each, `block_of_slot`), handed out on the device by one fetch-add per new block on `cursor` (include/monorec_hip.h has the rules,
    tests/tsdf_sparse_ref.py restates them).  The constructor is `TSDFVolume`'s; the dims are ROUNDED UP to whole blocks (`dims` holds
    the voxels, a multiple of 8 per axis, `blocks` the blocks: the volume may reach up to 7 voxels beyond the bounds asked for on the
    high side).  `max_bytes` is the budget for table plus pool; `capacity_blocks` defaults to what fits in it (at most every block) and
    raises above it; a table that alone exceeds the budget raises a ValueError that names its size.

    A block gets its slot in the first integrate launch that brings one of its voxels into the band; from then on it equals the same
    block of a dense volume that was empty at the start of that launch.  Free space seen only by EARLIER launches is lost for it (those
    voxels have a lower weight than in a dense volume, and a crossing into a block that was never in a band is gone), that of earlier
    frames of the same launch is kept; which slot a block gets is unspecified, everything else is deterministic.  A pool that runs out
    drops the blocks that found no room: `overflowed()` tells, nothing is written out of bounds.
    `extract` / `count` / `save_ply` (`mr_tsdf_sparse_extract_f32`) and `render` / `render_result` (`mr_tsdf_sparse_render_f32`) work on
    the sparse volume itself.  `render` has `TSDFVolume.render`'s signature and returns, bit for bit, what `to_dense(bounds).render` would:
    a block without storage is unseen (tsdf 1, weight 0, colour 0), which costs a ray one table entry per sample; `skip` is accepted and
    ignored.  It reads the cursor once per call, and a range of more than 2^20 samples per ray raises a ValueError.
    `mesh` / `mesh_counts` / `save_mesh_ply` (`mr_tsdf_sparse_mesh_vertices_f32`, `mr_tsdf_sparse_mesh_triangles_f32`) have `TSDFVolume`'s
    signatures and return, as a canonical mesh (the order of both arrays is unspecified), what `to_dense(bounds).mesh` would for
    min_weight >= 0: a workgroup per allocated block, vertices welded across block faces through the table, and a workspace of 4 bytes per
    voxel of the ALLOCATED blocks, not of the grid.  A block without storage is unseen whatever min_weight is (with min_weight < 0 the
    gathered volume's empty blocks would count as seen).
    `to_dense()` gathers any region that fits into a `TSDFVolume`; nothing here needs it any more."""

    def __init__(self, bounds=None, voxel_size=0.1, trunc=None, colour=True, device="cuda:0", max_bytes=8 << 30, origin=None, dims=None,
                 capacity_blocks=None):
        voxel_size = self._geometry(bounds, voxel_size, trunc, origin, dims)
        self.blocks = tuple((d + BLOCK - 1) // BLOCK for d in self.dims)
        self.dims = tuple(b * BLOCK for b in self.blocks)
        self.has_colour = bool(colour)
        count, budget = self.blocks[0] * self.blocks[1] * self.blocks[2], int(max_bytes)
        what = f"SparseTSDFVolume: {self.blocks[0]} x {self.blocks[1]} x {self.blocks[2]} blocks of {BLOCK}^3 voxels of {voxel_size:g} m"
        if count >= 2 ** 31:
            raise ValueError(f"{what} are {count} blocks; the table holds fewer than 2^31 - use a coarser voxel or a smaller box")
        if sparse_bytes(self.blocks, 0) > budget:
            raise ValueError(f"{what}: the table alone needs {4 * count / 2 ** 20:.1f} MiB, more than max_bytes = {budget / 2 ** 20:.1f} MiB")
        fits = (budget - sparse_bytes(self.blocks, 0)) // sparse_bytes((0, 0, 0), 1, self.has_colour)
        self.capacity = min(fits, count) if capacity_blocks is None else int(capacity_blocks)
        if self.capacity < 1 or self.capacity > fits:
            raise ValueError(f"{what}: a pool of {self.capacity} blocks and the table need {sparse_bytes(self.blocks, self.capacity, self.has_colour) / 2 ** 20:.1f} MiB; "
                             f"max_bytes = {budget / 2 ** 20:.1f} MiB has room for {fits} blocks (at least 1 is needed)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("monorec_amd.tsdf_fusion: the volume lives on a CUDA (HIP) device - there is no CPU fallback")
        n = self.capacity * BLOCK ** 3
        self.table = torch.empty(count, dtype=torch.int32, device=self.device)
        self.tsdf = torch.empty(n, dtype=torch.float32, device=self.device)
        self.weight = torch.empty(n, dtype=torch.float32, device=self.device)
        self.colour = torch.empty(n, 4, dtype=torch.uint8, device=self.device) if self.has_colour else None
        self.block_of_slot = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
        self.cursor = torch.empty(1, dtype=torch.int64, device=self.device)
        self._origin = (ctypes.c_float * 3)(*self.origin)
        self._keep = None
        self.frames = 0                                        # keyframes integrated so far
        self.reset()

    @property
    def bounds(self):
        """((x0, y0, z0), (x1, y1, z1)) of the first and the last voxel (after the rounding to whole blocks)."""
        return self.origin, tuple(o + (d - 1) * self.voxel_size for o, d in zip(self.origin, self.dims))

    def _table_args(self):
        return (self.table.data_ptr(), *self.blocks, self.tsdf.data_ptr(), self.weight.data_ptr(),
                self.colour.data_ptr() if self.colour is not None else None)

    def reset(self):
        """The table to -1, the cursor to 0, on the current stream; the pool needs no clearing (a block is written in full when it gets
        a slot)."""
        self.table.fill_(-1)
        self.cursor.zero_()
        self.frames = 0

    def _integrate_launch(self, lib, array, limit, size):
        _lib.check(lib.mr_tsdf_sparse_integrate_f32(*self._table_args(), self.block_of_slot.data_ptr(), self.capacity, self.cursor.data_ptr(),
                                                    self._origin, self.voxel_size, self.trunc, limit, array, len(array), size[0], size[1],
                                                    self._stream()), "mr_tsdf_sparse_integrate_f32")

    # -- state
    def allocated_blocks(self):
        """Blocks that have storage (one read of the cursor)."""
        return min(int(self.cursor.item()), self.capacity)

    def overflowed(self):
        """True when some block found no room in the pool (one read of the cursor): those blocks are missing from the volume."""
        return int(self.cursor.item()) > self.capacity

    def bytes_in_use(self):
        """The table (4 bytes per block) plus the pool bytes of the allocated blocks: exactly `allocated_blocks()` x 512 x 12 (x 8 without colour)."""
        return sparse_bytes(self.blocks, 0) + self.allocated_blocks() * BLOCK ** 3 * (12 if self.has_colour else 8)

    # -- surface
    _SURFACE_ENTRIES = ("mr_tsdf_sparse_extract_f32", "mr_tsdf_sparse_mesh_vertices_f32", "mr_tsdf_sparse_mesh_triangles_f32")

    def _surface_args(self, vertex_base=None, cell=1):
        """Over the allocated slots (one read of the cursor), or over those a mesh's `vertex_base` (with `cell` > 1: its cluster_base)
        was sized for."""
        slots = self.allocated_blocks() if vertex_base is None else vertex_base.numel() // (BLOCK // cell) ** 3
        args = self._table_args()
        return args + (self.block_of_slot.data_ptr(), slots), args[:6] + (self.block_of_slot.data_ptr(), slots)

    def _mesh_voxels(self):
        """Elements of `mesh()`'s vertex_base: one per pool voxel of the allocated blocks (one read of the cursor)."""
        return self.allocated_blocks() * BLOCK ** 3

    def _mesh_clusters(self, cell):
        """Elements of `mesh(cell=...)`'s cluster_base: (8 / cell)^3 per allocated block (one read of the cursor)."""
        return self.allocated_blocks() * (BLOCK // cell) ** 3

    # -- the volume seen from a camera
    def _render_shared(self, march, min_weight, skip):
        """The range checked here, where the message can name its keywords, and the slots in use: one read of the cursor per call."""
        t_min, t_max, step = march
        if step > 0 and np.float32(t_min) + np.float32(MAX_RENDER_SAMPLES) * np.float32(step) <= np.float32(t_max):     # sample 2^20 exists
            raise ValueError(f"SparseTSDFVolume.render: t_max = {t_max:g} and step = {step:g} from t_min = {t_min:g} are more than 2^20 samples "
                             f"per ray; lower t_max or raise step")
        return self.allocated_blocks()                                            # `skip`: accepted and ignored, the table is the skip grid

    def _render_launch(self, lib, array, size, march, min_weight, num_slots):
        _lib.check(lib.mr_tsdf_sparse_render_f32(*self._table_args(), num_slots, self._origin, self.voxel_size, min_weight, array, len(array), *size,
                                                 *march, self._stream()), "mr_tsdf_sparse_render_f32")

    # -- dense views of it
    def allocated_box(self):
        """(offset, dims) in voxels of the bounding box of the allocated blocks, or None when there is none."""
        n = self.allocated_blocks()
        if not n:
            return None
        coords = self._block_coords(self.block_of_slot[:n].cpu().numpy())
        lo, hi = coords.min(axis=0), coords.max(axis=0) + 1
        return tuple(int(v) * BLOCK for v in lo), tuple(int(v) * BLOCK for v in hi - lo)

    def _block_coords(self, index):
        index = np.asarray(index, dtype=np.int64)
        return np.stack([index % self.blocks[0], index // self.blocks[0] % self.blocks[1], index // (self.blocks[0] * self.blocks[1])], axis=1)

    def to_dense(self, bounds=None, max_bytes=8 << 30, offset=None, dims=None):
        """A `TSDFVolume` holding a copy of a region (`mr_tsdf_sparse_gather_f32`; blocks without storage read as tsdf 1, weight 0,
        colour 0): of `bounds` = ((x0, y0, z0), (x1, y1, z1)) in metres, clipped to the volume, or of `offset` and `dims` in voxels (need
        not be block-aligned), or - the default - of the bounding box of the allocated blocks.  Above `max_bytes` the usual ValueError.
        The dense volume's origin is the fp32 position of the region's first voxel, so with an offset other than 0 its voxel positions
        (origin + i * voxel_size) may differ from this volume's in the last bit; the whole volume (`to_dense(volume.bounds)`) has
        the same positions."""
        if bounds is not None:
            lo, hi = (np.asarray(b, dtype=np.float64) for b in bounds)
            first = np.clip(np.floor((lo - self.origin) / self.voxel_size + 1e-6), 0, np.asarray(self.dims) - 1).astype(np.int64)
            last = np.clip(np.ceil((hi - self.origin) / self.voxel_size - 1e-6), first, np.asarray(self.dims) - 1).astype(np.int64)
            offset, dims = tuple(int(v) for v in first), tuple(int(v) for v in last - first + 1)
        elif offset is None or dims is None:
            box = self.allocated_box()
            if box is None:
                raise ValueError("SparseTSDFVolume.to_dense: no block is allocated; give bounds")
            offset, dims = box
        offset, dims = tuple(int(v) for v in offset), tuple(int(v) for v in dims)
        if len(offset) != 3 or len(dims) != 3 or min(offset) < 0 or min(dims) < 1 or any(o + d > n for o, d, n in zip(offset, dims, self.dims)):
            raise ValueError(f"SparseTSDFVolume.to_dense: the box of {dims} voxels at {offset} leaves the volume of {self.dims}")
        origin = tuple(float(np.float32(o) + np.float32(i) * np.float32(self.voxel_size)) for o, i in zip(self.origin, offset))
        dense = TSDFVolume(origin=origin, dims=dims, voxel_size=self.voxel_size, trunc=self.trunc, colour=self.has_colour, device=self.device,
                           max_bytes=max_bytes)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mr_tsdf_sparse_gather_f32(*self._table_args(), *offset, *dims, *dense._volume_args()[:3], self._stream()),
                       "mr_tsdf_sparse_gather_f32")
        dense.frames = self.frames
        return dense

    # -- the volume itself
    def blocks_host(self):
        """Host copies of the allocated blocks in the order of their table index (not of their slots): coordinates (n, 3) int32
        (bx, by, bz), tsdf and weight (n, 8, 8, 8) fp32 indexed [z][y][x], colour (n, 8, 8, 8, 4) uint8 or None."""
        n = self.allocated_blocks()
        index = self.block_of_slot[:n].cpu().numpy().astype(np.int64)
        order = np.argsort(index, kind="stable")
        tsdf = self.tsdf[:n * BLOCK ** 3].cpu().numpy().reshape(n, BLOCK, BLOCK, BLOCK)[order]
        weight = self.weight[:n * BLOCK ** 3].cpu().numpy().reshape(n, BLOCK, BLOCK, BLOCK)[order]
        colour = self.colour[:n * BLOCK ** 3].cpu().numpy().reshape(n, BLOCK, BLOCK, BLOCK, 4)[order] if self.colour is not None else None
        return self._block_coords(index[order]).astype(np.int32), tsdf, weight, colour

    def save(self, file):
        """.npz: blocks (n, 3) int32 block coordinates, tsdf, weight (n, 8, 8, 8) fp32, colour (n, 8, 8, 8, 4) uint8 if any - in the order of
        the table, whatever the slots were -, origin, dims (nx, ny, nz voxels), voxel_size, trunc, frames."""
        blocks, tsdf, weight, colour = self.blocks_host()
        arrays = dict(blocks=blocks, tsdf=tsdf, weight=weight, origin=np.asarray(self.origin, dtype=np.float32),
                      dims=np.asarray(self.dims, dtype=np.int64), voxel_size=np.float32(self.voxel_size), trunc=np.float32(self.trunc),
                      frames=np.int64(self.frames))
        if colour is not None:
            arrays["colour"] = colour
        np.savez(file, **arrays)

    def set_blocks(self, blocks, tsdf, weight, colour=None):
        """Replace the volume's content by these blocks (`blocks_host()`'s arrays, in any order, no block twice): slot i holds block i."""
        blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
        n = blocks.shape[0]
        index = (blocks[:, 2] * self.blocks[1] + blocks[:, 1]) * self.blocks[0] + blocks[:, 0]
        if n > self.capacity or (n and (blocks.min() < 0 or np.any(blocks >= np.asarray(self.blocks)))) or len(np.unique(index)) != n:
            raise ValueError(f"SparseTSDFVolume: {n} blocks for a pool of {self.capacity}, a block outside {self.blocks}, or one given twice")
        if (colour is None) != (self.colour is None):
            raise ValueError("SparseTSDFVolume: the blocks and the volume must both have colour, or neither")
        self.reset()
        if n:
            self.table[torch.from_numpy(index).to(self.device)] = torch.arange(n, dtype=torch.int32, device=self.device)
            self.block_of_slot[:n].copy_(torch.from_numpy(index.astype(np.int32)))
            self.tsdf[:n * BLOCK ** 3].copy_(torch.from_numpy(np.ascontiguousarray(tsdf, dtype=np.float32).reshape(-1)))
            self.weight[:n * BLOCK ** 3].copy_(torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32).reshape(-1)))
            if self.colour is not None:
                self.colour[:n * BLOCK ** 3].copy_(torch.from_numpy(np.ascontiguousarray(colour, dtype=np.uint8).reshape(-1, 4)))
        self.cursor.fill_(n)

    @classmethod
    def load(cls, file, device="cuda:0", max_bytes=8 << 30, capacity_blocks=None):
        """The volume of a `save`d .npz; `capacity_blocks` defaults to what fits in `max_bytes`."""
        with np.load(file) as z:
            volume = cls(origin=z["origin"], dims=z["dims"], voxel_size=float(z["voxel_size"]), trunc=float(z["trunc"]),
                         colour="colour" in z.files, device=device, max_bytes=max_bytes, capacity_blocks=capacity_blocks)
            volume.set_blocks(z["blocks"], z["tsdf"], z["weight"], z["colour"] if "colour" in z.files else None)
            volume.frames = int(z["frames"]) if "frames" in z.files else 0
        return volume


# ------------------------------------------------------------------------------------------ a directory of tsdf_export
_FRAME = re.compile(r"^frame-(\d+)\.pose\.txt$")


def list_export_directory(directory):
    """[(number, base path)] of the `frame-%06d.*` triples of a directory written by tsdf_export, in numeric order."""
    frames = []
    for name in os.listdir(str(directory)):
        m = _FRAME.match(name)
        if m:
            frames.append((int(m.group(1)), os.path.join(str(directory), name[:-len(".pose.txt")])))
    return sorted(frames)


def read_export_pose(base):
    """Camera -> world (4, 4) fp32 of one triple.  The pose file holds `inverse(pose)` (utils/util.py:91): it is inverted again, in fp32."""
    world_to_cam = torch.from_numpy(np.loadtxt(base + ".pose.txt").astype(np.float32)).reshape(4, 4)
    return torch.inverse(world_to_cam)


def read_export_frame(base):
    """One triple from the files: depth (h, w) int16 centimetres, colour (h, w, 3) uint8 (the decoded JPEG), camera -> world (4, 4)
    fp32 (`read_export_pose`)."""
    from PIL import Image
    with Image.open(base + ".depth.png") as img:
        depth = np.array(img)
    with Image.open(base + ".color.jpg") as img:
        colour = np.array(img.convert("RGB"))
    return depth.astype(np.uint16).view(np.int16), colour, read_export_pose(base)


def fuse_directory(directory, volume=None, voxel_size=0.1, trunc=None, colour=True, max_depth_m=None, bounds=None, device="cuda:0",
                   max_bytes=8 << 30):
    """Fuse a directory written by `tsdf_export` (`camera-intrinsics.txt` and the `frame-*` triples in numeric order, read with Pillow)
    into `volume`, or into a new one over `bounds`, or over `bounds_from_frusta` of the poses and `max_depth_m`.  Only the pose files
    are read ahead (to size the volume); the images are decoded eight keyframes at a time, one integrate launch each.  The colour
    comes from the JPEGs, so it differs from that of a live fusion; the depth does not.  Returns the volume."""
    frames = list_export_directory(directory)
    if not frames:
        raise ValueError(f"{directory}: no frame-*.pose.txt files")
    k = torch.from_numpy(np.loadtxt(os.path.join(str(directory), "camera-intrinsics.txt")).astype(np.float32)).reshape(3, 3)
    if volume is None:
        if bounds is None:
            if max_depth_m is None:
                raise ValueError("fuse_directory: without a volume and without bounds, max_depth_m is needed to size one")
            from PIL import Image
            with Image.open(frames[0][1] + ".depth.png") as img:
                w, h = img.size
            bounds = bounds_from_frusta([read_export_pose(base) for _, base in frames], k, h, w, max_depth_m, voxel_size)
        volume = TSDFVolume(bounds, voxel_size, trunc=trunc, colour=colour, device=device, max_bytes=max_bytes)
    for lo in range(0, len(frames), MAX_FRAMES):
        chunk = [read_export_frame(base) for _, base in frames[lo:lo + MAX_FRAMES]]
        depth = torch.from_numpy(np.stack([f[0] for f in chunk])).to(volume.device)
        image = torch.from_numpy(np.stack([f[1] for f in chunk])).to(volume.device) if volume.has_colour else None
        volume.integrate(depth, image, torch.stack([f[2] for f in chunk]), k, max_depth_m)
    return volume


# ------------------------------------------------------------------------------------------ the runner
# the metrics `Fusion.score()` can report, in metrics.metrics_from_sums' order: the onlyvalid variants leave out what a render did not hit
FUSED_METRICS = tuple(f"{base}_sparse_onlyvalid_metric" for base in ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))


def fusion_settings(config):
    """The fusion keys of a runner config, checked: dict(voxel_size, trunc, bounds, max_bytes, fuse_batch, file_name, mesh_file_name,
    save_volume, fused_metrics, render_dir).  `mesh_cell` and `mesh_normals` are checked here too; `mesh_settings` returns them."""
    voxel = float(config.get("voxel_size", 0.1))
    trunc_voxels = float(config.get("trunc_voxels", 5))
    batch = int(config.get("fuse_batch", 4))
    if not voxel > 0:
        raise ValueError(f"monorec_amd.tsdf_fusion: voxel_size {voxel} must be positive")
    if not trunc_voxels > 0:
        raise ValueError(f"monorec_amd.tsdf_fusion: trunc_voxels {trunc_voxels} must be positive")
    if not 1 <= batch <= MAX_FRAMES:
        raise ValueError(f"monorec_amd.tsdf_fusion: fuse_batch {batch} must be 1 .. {MAX_FRAMES}")
    bounds = config.get("bounds", None)
    if bounds is None and config.get("max_d", None) is None:
        raise ValueError("monorec_amd.tsdf_fusion: the config has neither `bounds` nor `max_d`; one of them is needed to size the volume")
    if bounds is not None:
        dims_of_bounds(bounds, voxel)
    fused_metrics = config.get("fused_metrics", None)
    fused_metrics = [] if fused_metrics is None else fused_metrics
    if not isinstance(fused_metrics, (list, tuple)) or any(name not in FUSED_METRICS for name in fused_metrics):
        raise ValueError(f"monorec_amd.tsdf_fusion: fused_metrics {fused_metrics!r} must be a list of *_sparse_onlyvalid_metric names "
                         f"({', '.join(FUSED_METRICS)}): a render is 0 where no surface was hit, which only they leave out")
    mesh_settings(config)                                      # checked here, with the other keys; `Fusion` keeps what it returns
    return dict(voxel_size=voxel, trunc=trunc_voxels * voxel, bounds=bounds, max_bytes=int(config.get("tsdf_max_bytes", 8 << 30)),
                fuse_batch=batch, file_name=config.get("file_name", "tsdf.ply"), mesh_file_name=config.get("mesh_file_name", None),
                save_volume=config.get("save_volume", None), fused_metrics=list(fused_metrics), render_dir=config.get("render_dir", None))


def mesh_settings(config):
    """The runner keys `mesh_cell` (default 1) and `mesh_normals` (default false), checked, as the keywords of `save_mesh_ply` that
    differ from its defaults: what `Fusion.write()` passes on for `mesh_file_name`, with and without `sparse_mesh`."""
    mesh_cell, mesh_normals = config.get("mesh_cell", 1), config.get("mesh_normals", False)
    if isinstance(mesh_cell, bool) or mesh_cell not in MESH_CELLS:
        raise ValueError(f"monorec_amd.tsdf_fusion: mesh_cell {mesh_cell!r} must be one of {', '.join(str(c) for c in MESH_CELLS)} "
                         f"(1: the full mesh; a larger cell: one vertex per cluster of cell^3 voxels)")
    if not isinstance(mesh_normals, bool):
        raise ValueError(f"monorec_amd.tsdf_fusion: mesh_normals {mesh_normals!r} must be true or false")
    return _mesh_options(int(mesh_cell), mesh_normals)


def sparse_setting(config):
    """The runner key `sparse_volume` (default false), checked: fuse into a `SparseTSDFVolume` over the same bounds, with
    `tsdf_max_bytes` as the budget of its table and pool."""
    sparse = config.get("sparse_volume", False)
    if not isinstance(sparse, bool):
        raise ValueError(f"monorec_amd.tsdf_fusion: sparse_volume {sparse!r} must be true or false")
    return sparse


def sparse_mesh_setting(config):
    """The runner key `sparse_mesh` (default false), checked: with `sparse_volume`, mesh the sparse volume itself
    (`SparseTSDFVolume.save_mesh_ply`) and not the whole of it gathered into a dense one."""
    native = config.get("sparse_mesh", False)
    if not isinstance(native, bool):
        raise ValueError(f"monorec_amd.tsdf_fusion: sparse_mesh {native!r} must be true or false")
    if native and not sparse_setting(config):
        raise ValueError("monorec_amd.tsdf_fusion: sparse_mesh needs sparse_volume: true (a dense volume is meshed as it is)")
    return native


def sparse_render_setting(config):
    """The runner key `sparse_render` (default false), checked: with `sparse_volume`, render and score the sparse volume itself
    (`SparseTSDFVolume.render`) and not the whole of it gathered into a dense one."""
    native = config.get("sparse_render", False)
    if not isinstance(native, bool):
        raise ValueError(f"monorec_amd.tsdf_fusion: sparse_render {native!r} must be true or false")
    if native and not sparse_setting(config):
        raise ValueError("monorec_amd.tsdf_fusion: sparse_render needs sparse_volume: true (a dense volume is rendered as it is)")
    return native


class Fusion:
    """The stages of `run`, for callers that want them apart (tools/bench_tsdf_fusion.py times them): the constructor builds model,
    dataset and volume, `fuse()` drives the keyframe loop, `write()` extracts and saves."""

    def __init__(self, config, model=None, dataset=None, device="cuda:0"):
        self.config, self.settings, self.sparse = config, fusion_settings(config), sparse_setting(config)
        self.sparse_render, self.sparse_mesh = sparse_render_setting(config), sparse_mesh_setting(config)
        self.mesh_options = mesh_settings(config)              # cell and normals of the mesh file, where they are not the defaults
        settings = self.settings
        if settings["bounds"] is not None:
            self._check_dense_outputs(settings["bounds"])         # before the model is built
        self.stream = stream = tx.KeyframeStream(config, model, dataset, (0, 1), device, who="monorec_amd.tsdf_fusion")
        y0, y1, x0, x1 = tx.crop_box(stream.crop, stream.height, stream.width)
        self.offset = (y0, x0)
        ch, cw = y1 - y0, x1 - x0
        bounds = settings["bounds"]
        if bounds is None:
            items = stream.export_items()
            if not hasattr(stream.dataset, "keyframe_geometry"):
                raise ValueError("monorec_amd.tsdf_fusion: this dataset cannot hand out its poses ahead of the run; give `bounds` in the config")
            if not items:
                raise ValueError("monorec_amd.tsdf_fusion: the window exports no keyframe, nothing to size the volume from; give `bounds`")
            geometry = [stream.dataset.keyframe_geometry(i) for i in items]
            bounds = bounds_from_frusta([g[0] for g in geometry], [self.shifted(g[1]) for g in geometry], ch, cw, config["max_d"],
                                        settings["voxel_size"])
            self._check_dense_outputs(bounds)
        self.volume = (SparseTSDFVolume if self.sparse else TSDFVolume)(bounds, settings["voxel_size"], trunc=settings["trunc"], colour=True,
                                                                        device=stream.device, max_bytes=settings["max_bytes"])
        self._dense = None                                     # the sparse volume gathered for the mesh (renders and score), once asked for
        depth_bytes, colour_bytes = tx.packed_sizes(1, ch, cw)
        self._slots = [torch.empty(depth_bytes + colour_bytes, dtype=torch.uint8, device=stream.device) for _ in range(settings["fuse_batch"])]
        self.mesh_counts = None                                # (vertices, triangles) of the mesh file, once `write()` has written one

    def _check_dense_outputs(self, bounds):
        """With `sparse_volume`, the mesh without `sparse_mesh` - and the renders and the score without `sparse_render` - work on the whole
        volume gathered into a dense one, which must fit `tsdf_max_bytes` too: a ValueError that names the keys before anything is fused."""
        settings = self.settings
        dense = (() if self.sparse_mesh else ("mesh_file_name",)) + (() if self.sparse_render else ("render_dir", "fused_metrics"))
        asked = [key for key in dense if settings[key]]
        if not self.sparse or not asked:
            return
        dims = tuple((d + BLOCK - 1) // BLOCK * BLOCK for d in dims_of_bounds(bounds, settings["voxel_size"]))
        if volume_bytes(dims) > settings["max_bytes"]:
            raise ValueError(f"monorec_amd.tsdf_fusion: {', '.join(asked)} with sparse_volume need the volume gathered into a dense one of "
                             f"{dims[0]} x {dims[1]} x {dims[2]} voxels, {volume_bytes(dims) / 2 ** 30:.2f} GiB, more than tsdf_max_bytes = "
                             f"{settings['max_bytes'] / 2 ** 30:.2f} GiB; raise tsdf_max_bytes, or write the points alone (file_name)")

    def meshed(self):
        """The volume `write()` meshes: `dense()`, or with `sparse_mesh` the sparse volume itself."""
        return self.volume if self.sparse_mesh else self.dense()

    def dense(self):
        """The volume `mesh()` works on without `sparse_mesh`: the volume itself, or the whole sparse one gathered (`to_dense`, once)."""
        if not self.sparse:
            return self.volume
        if self._dense is None:
            self._check_dense_outputs(self.volume.bounds)
            self._dense = self.volume.to_dense(self.volume.bounds, max_bytes=self.settings["max_bytes"])
        return self._dense

    def rendered(self):
        """The volume `score()` and `write_renders()` render: `dense()`, or with `sparse_render` the sparse volume itself."""
        return self.volume if self.sparse_render else self.dense()

    def shifted(self, k):
        """The intrinsics of the cropped image, as `save_intrinsics_for_tsdf` shifts them, on a copy."""
        k = torch.as_tensor(k).detach().to("cpu", torch.float32)
        k = k.reshape(k.shape[-2], k.shape[-1]).clone()
        k[0, 2] -= self.offset[1]
        k[1, 2] -= self.offset[0]
        return k

    def fuse(self):
        config, stream, volume, slots = self.config, self.stream, self.volume, self._slots
        staged, keep = [], []

        def flush():
            if staged:
                volume.integrate_views(staged)
                del staged[:]
                del keep[:]

        def emit(number, entry, masks):
            depth, colour, alive = tx.pack_frames(entry["depth"], entry["keyframe"], stream.crop, config.get("min_d", None),
                                                  config.get("max_d", None), static_masks=masks, min_hits=1, out=slots[len(staged)])
            keep.append(alive)
            staged.append((depth[0], colour[0], _matrix(torch.as_tensor(entry["pose"]).reshape(4, 4), "keyframe_pose"),
                           self.shifted(entry["intrinsics"])))            # each keyframe's own calibration
            if len(staged) == len(slots):
                flush()

        stream.run(emit)
        flush()
        if self.sparse and volume.overflowed():
            raise RuntimeError(f"monorec_amd.tsdf_fusion: the pool of {volume.capacity} blocks ({sparse_bytes((0, 0, 0), volume.capacity) / 2 ** 20:.1f} MiB) "
                               f"of the sparse volume ran out, blocks of the surface are missing; raise tsdf_max_bytes (or the voxel size)")
        return self

    def write(self):
        out_dir = self.config.get("output_dir", "saved")
        os.makedirs(out_dir, exist_ok=True)
        count = self.volume.save_ply(os.path.join(out_dir, self.settings["file_name"]))
        if self.settings["mesh_file_name"] is not None:
            self.mesh_counts = self.meshed().save_mesh_ply(os.path.join(out_dir, self.settings["mesh_file_name"]),
                                                           **self.mesh_options)
        if self.settings["save_volume"] is not None:
            self.volume.save(self.settings["save_volume"])
        if self.settings["render_dir"] is not None:
            self.write_renders(self.settings["render_dir"])
        return count

    # -- the fused volume seen from the keyframes again
    def _render_range(self):
        max_d = self.config.get("max_d", None)
        return dict(t_min=0.0, t_max=None if max_d is None else float(max_d))

    def score(self, roi=None, max_distance=None):
        """A second pass over the exported keyframes, without the model: the volume rendered into every keyframe's camera
        (`keyframe_pose`, the uncropped `keyframe_intrinsics`, the dataset's `target_image_size`; eight views per launch) and scored
        against the sample's target with the config's `fused_metrics`.  The metric sums stay on the device until the end.  `roi` /
        `max_distance`: as the metric functions take them.  Returns dict(metrics {name: value} - each what the metric function of that
        name returns for all samples as one batch -, coverage: the share of target pixels the render hit, samples)."""
        from . import metrics
        stream, volume = self.stream, self.rendered()
        items = stream.export_items()
        height, width = stream.height, stream.width
        sums, hit, have = [], torch.zeros((), dtype=torch.int64, device=volume.device), torch.zeros((), dtype=torch.int64, device=volume.device)
        for lo in range(0, len(items), MAX_FRAMES):
            samples = [stream.dataset[i] for i in items[lo:lo + MAX_FRAMES]]
            target = torch.stack([torch.as_tensor(t).to(volume.device).reshape(1, height, width) for _, t in samples])
            result = volume.render_result(torch.stack([_matrix(d["keyframe_pose"], "keyframe_pose") for d, _ in samples]),
                                          torch.stack([_matrix(d["keyframe_intrinsics"], "keyframe_intrinsics") for d, _ in samples]),
                                          height, width, **self._render_range())
            sums.append(metrics.sparse_metric_sums_device(dict(result=result, target=target), roi, max_distance, pred_all_valid=False))
            have += (target > 0).sum()
            hit += ((target > 0) & (result != 0)).sum()
        if not sums:
            return dict(metrics={name: float("nan") for name in self.settings["fused_metrics"]}, coverage=float("nan"), samples=0)
        values = metrics.metrics_from_sums(torch.cat(sums).cpu())
        have = int(have.item())
        return dict(metrics={name: float(values[FUSED_METRICS.index(name)]) for name in self.settings["fused_metrics"]},
                    coverage=int(hit.item()) / have if have else float("nan"), samples=len(items))

    def write_renders(self, directory):
        """Per exported keyframe the fused depth and colour as the export would have written them - the crop's size and shifted
        intrinsics, `frame-%06d.fused.depth.png` (16 bit, centimetres, 0: nothing) and `frame-%06d.fused.color.jpg`, names that sort
        next to the export's.  After the fusion and synchronous: not a stage of the loop.  Returns the number of keyframes."""
        from PIL import Image
        stream, volume = self.stream, self.rendered()
        os.makedirs(str(directory), exist_ok=True)
        items = stream.export_items()
        y0, y1, x0, x1 = tx.crop_box(stream.crop, stream.height, stream.width)
        first = stream.plan["exports"][0]
        for lo in range(0, len(items), MAX_FRAMES):
            chunk = items[lo:lo + MAX_FRAMES]
            if hasattr(stream.dataset, "keyframe_geometry"):
                geometry = [stream.dataset.keyframe_geometry(i) for i in chunk]
            else:
                geometry = [(d["keyframe_pose"], d["keyframe_intrinsics"]) for d, _ in (stream.dataset[i] for i in chunk)]
            views = volume.render(torch.stack([_matrix(g[0], "keyframe_pose") for g in geometry]), torch.stack([self.shifted(g[1]) for g in geometry]),
                                  y1 - y0, x1 - x0, normals=False, **self._render_range())
            depth_cm = (views["depth"] * 100.0).clamp_(0.0, 65535.0).to(torch.int32).cpu().numpy().astype(np.uint16)
            colour = views["colour"].cpu().numpy()
            for j in range(len(chunk)):
                base = os.path.join(str(directory), f"frame-{first + lo + j:06d}.fused")
                Image.fromarray(depth_cm[j]).save(base + ".depth.png")
                Image.fromarray(colour[j]).save(base + ".color.jpg")
        return len(items)


def run(config, model=None, dataset=None, device="cuda:0"):
    """Fuse the keyframes of a config of `tsdf_export.run`'s shape (same `data_set`, `arch`, `start` / `end`, `roi`, `min_d` / `max_d`,
    `use_mask`) and write the surface points to `output_dir/file_name` (default `tsdf.ply`).  Optional keys: `voxel_size` (0.1),
    `trunc_voxels` (5), `mesh_file_name` (None; a name: the surface is also written as a triangle mesh, `TSDFVolume.save_mesh_ply`, next to
    the points), `mesh_cell` (1; 2, 4 or 8: that file holds the clustered level of detail `mesh(cell=...)`), `mesh_normals` (false; true:
    it carries a unit normal per vertex), `bounds` (else `bounds_from_frusta` over the window's exported keyframe poses and `max_d`; without both it
    raises), `tsdf_max_bytes`, `fuse_batch` (keyframes per integrate launch, default 4), `save_volume` (a path for `TSDFVolume.save`),
    `render_dir` (a directory for `Fusion.write_renders`), `fused_metrics` (names for `Fusion.score()`; `main` prints its result),
    `sparse_volume` (false; true: fuse into a `SparseTSDFVolume` over the same bounds with `tsdf_max_bytes` as the budget of table and pool -
    points and `save_volume` come from it, mesh, renders and score from the whole of it gathered into a dense volume, which must fit
    `tsdf_max_bytes` as well; a pool that ran out raises after the loop), `sparse_render` (false; true, with `sparse_volume` only: renders and
    score come from the sparse volume itself, `SparseTSDFVolume.render` - the same bits without the dense copy), `sparse_mesh` (false; true,
    with `sparse_volume` only: `mesh_file_name` is written from the sparse volume itself, `SparseTSDFVolume.save_mesh_ply` - the same mesh
    without the dense copy; with both keys nothing asks for room for one), `consistency` (absent or false: nothing; as for
    `tsdf_export.run`: every keyframe's depth is filtered against the two keyframes before and after it before it is packed,
    monorec_amd.consistency, and the first and last two keyframes of the window are not fused, with or without `use_mask`).

    Per keyframe `pack_frames` (vote, crop, thresholds: the depths are exactly the ones the export writes to the PNG) fills a staging slot
    on the device; after `fuse_batch` keyframes, or at the end, one integrate launch follows on the same stream.  Every keyframe is
    integrated with its own intrinsics, shifted by the crop on a copy.  Single-process.  Returns the number of surface points written."""
    return Fusion(config, model, dataset, device).fuse().write()


def main(argv=None):
    config, device = tx.load_config(argv, prog="python -m monorec_amd.tsdf_fusion",
                                    description="MonoRec keyframes fused into a TSDF volume on the device; the surface points as a .ply")
    fusion = Fusion(config, device=device).fuse()
    count = fusion.write()
    print(f"{count} surface points written to {os.path.join(config.get('output_dir', 'saved'), config.get('file_name', 'tsdf.ply'))}")
    if fusion.sparse:
        print(f"{fusion.volume.allocated_blocks()} of {fusion.volume.table.numel()} blocks allocated, {fusion.volume.bytes_in_use() / 2 ** 20:.1f} MiB in use "
              f"(dense: {volume_bytes(fusion.volume.dims) / 2 ** 20:.1f} MiB)")
    if fusion.mesh_counts is not None:
        print(f"{fusion.mesh_counts[0]} vertices and {fusion.mesh_counts[1]} triangles written to "
              f"{os.path.join(config.get('output_dir', 'saved'), config['mesh_file_name'])}")
    if fusion.settings["render_dir"] is not None:
        print(f"fused depth and colour of every exported keyframe written to {fusion.settings['render_dir']}")
    if fusion.settings["fused_metrics"]:
        scored = fusion.score()
        for name, value in scored["metrics"].items():
            print(f"{name}: {value:.6f}")
        print(f"fused coverage: {scored['coverage']:.4f} of the target pixels of {scored['samples']} keyframes")


if __name__ == "__main__":
    main()
