"""Point-cloud path on the MI355X: drop-in for the reference's `utils.PLYSaver`
(utils/ply_utils.py:8-53) and the mask logic of `create_pointcloud.py:57-102`.

    from monorec_amd.pointcloud import PLYSaver, static_mask, PointcloudBuilder

`PLYSaver` keeps the reference's constructor, `add_depthmap(depth, image, intrinsics, extrinsics)`, `save(file)`,
`.to(device)` and `.data` (an `array('f')` of x y z r g b records).  Differences that matter on the device:
  * the records stay in HBM behind a device-side cursor: `add_depthmap` is one asynchronous launch, the host copy
    happens once, in `save()` / on first access of `.data` (the reference does `.cpu().tolist()` per keyframe);
  * the 1/depth, range / roi / dropout tests, back-projection, pose multiply, colours and the ordered boolean-mask
    compaction are one kernel (`mr_pointcloud_append_f32`), optionally with the 5-mask vote and `depth *= mask`
    of create_pointcloud.py:90-92 fused in (`static_masks=`).
There is no CPU fallback: CPU tensors raise.

`run(config)` is the whole of `create_pointcloud.py` for a config of that script's shape (configs/test/pointcloud_monorec.json,
pointcloud_monorec_tmvo.json) with the data source on the device too:

    python -m monorec_amd.pointcloud --config configs/test/pointcloud_monorec_tmvo.json"""
import ctypes
import functools
from array import array

import numpy as np
import torch

from . import _lib


_need_cuda = functools.partial(_lib.need_cuda, "pointcloud")


def static_mask(cv_mask, mask_fill=32, threshold=0.1):
    """create_pointcloud.py:76-77: `(F.conv2d((cv_mask >= .1).float(), ones(33, 33), padding=16) < 1).float()`."""
    _need_cuda(cv_mask, "cv_mask")
    lib = _lib.load()
    x = cv_mask.contiguous().float()
    b, c, h, w = x.shape
    assert c == 1
    out = torch.empty_like(x)
    _lib.check(lib.mr_static_mask_f32(x.data_ptr(), out.data_ptr(), b, h, w, float(threshold), int(mask_fill),
                                      torch.cuda.current_stream().cuda_stream), "mr_static_mask_f32")
    return out


def write_ply(file, data):
    """utils/ply_utils.py:18-32: the header and the binary little-endian float records x y z red green blue.  `data`: a flat
    `array('f')` or fp32 numpy array of six floats per vertex (also what monorec_amd.tsdf_fusion writes its surface points with)."""
    fields = ("x", "y", "z", "red", "green", "blue")
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(data) // 6}"]
    lines += [f"property float {name}" for name in fields] + ["end_header"]
    file.write(("\n".join(lines) + "\n").encode("ascii"))
    if isinstance(data, array):
        data.tofile(file)
    else:
        file.write(data.tobytes())


def write_mesh_ply(file, vertices, triangles, normals=None):
    """A triangle mesh as a binary little-endian .ply: `write_ply`'s six float vertex properties, then `element face M` with
    `property list uchar int vertex_indices` (13 bytes per triangle).  `vertices`: (n, 6) fp32 numpy array x y z red green blue,
    `triangles`: (m, 3) integer numpy array of indices into it (what monorec_amd.tsdf_fusion.TSDFVolume.mesh returns, on the host).
    `normals`: None, or (n, 3) fp32 - the vertex records then are 9 floats, with the properties nx ny nz after blue."""
    vertices = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 6)
    triangles = np.asarray(triangles).reshape(-1, 3)
    if len(triangles) and (triangles.min() < 0 or triangles.max() >= len(vertices)):
        raise ValueError(f"write_mesh_ply: triangle indices outside the {len(vertices)} vertices")
    names = ("x", "y", "z", "red", "green", "blue")
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype="<f4").reshape(-1, 3)
        if len(normals) != len(vertices):
            raise ValueError(f"write_mesh_ply: {len(normals)} normals for {len(vertices)} vertices")
        vertices, names = np.concatenate([vertices, normals], axis=1), names + ("nx", "ny", "nz")
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vertices)}"]
    lines += [f"property float {name}" for name in names]
    lines += [f"element face {len(triangles)}", "property list uchar int vertex_indices", "end_header"]
    file.write(("\n".join(lines) + "\n").encode("ascii"))
    file.write(vertices.tobytes())
    faces = np.empty(len(triangles), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"] = 3
    faces["v"] = triangles
    file.write(faces.tobytes())


class PLYSaver(torch.nn.Module):
    """utils/ply_utils.py:8-53 with device-resident records."""

    def __init__(self, height, width, min_d=3, max_d=400, batch_size=1, roi=None, dropout=0, capacity=1 << 22):
        super().__init__()
        if int(capacity) < 1:                       # 0 would never grow (`_ensure` doubles it)
            raise ValueError(f"PLYSaver: capacity must be at least 1 record, not {capacity}")
        self.height, self.width = height, width
        self.min_d, self.max_d = min_d, max_d
        self.roi = roi
        self.dropout = dropout
        self.batch_size = batch_size
        self._capacity = int(capacity)              # records; grows by doubling
        self._records = None                        # (capacity, 6) fp32 on the device
        self._cursor = None                         # int64[1] on the device
        self._host = array('f')                     # records already copied out (after save / .data)
        self._device = None
        self._pending = 0                           # upper bound of records appended since the last host sync

    # -- torch.nn.Module plumbing the reference script uses: plysaver.to(device)
    def _apply(self, fn):
        super()._apply(fn)
        probe = fn(torch.empty(0))
        self._device = probe.device
        return self

    def _ensure(self, device, incoming):
        if self._records is None:
            self._device = device
            self._records = torch.empty(self._capacity, 6, dtype=torch.float32, device=device)
            self._cursor = torch.zeros(1, dtype=torch.int64, device=device)
        if self._pending + incoming > self._capacity:           # could overflow: find out how full it really is
            used = int(self._cursor.item())
            self._pending = used
            while used + incoming > self._capacity:
                self._capacity *= 2
            if self._capacity > self._records.shape[0]:
                grown = torch.empty(self._capacity, 6, dtype=torch.float32, device=device)
                grown[:used] = self._records[:used]
                self._records = grown

    def add_depthmap(self, depth, image, intrinsics, extrinsics, static_masks=None, min_hits=1, uniform=None):
        """`depth` is the predicted inverse depth (B,1,H,W) like in the reference.  Extras: `static_masks` (list of the
        buffered static_mask() outputs) fuses the vote + `depth *= mask` of create_pointcloud.py:90-92; `uniform`
        replaces the `torch.rand_like(depth)` of ply_utils.py:45 (given: deterministic; None with dropout > 0: drawn
        here on the device).  Like the reference (:44) it thins only with dropout > 0: with dropout 0 a `uniform` is
        not handed to the kernel, whose `uniform > dropout` would drop the entries that are exactly 0."""
        for t, n in ((depth, "depth"), (image, "image"), (intrinsics, "intrinsics"), (extrinsics, "extrinsics")):
            _need_cuda(t, n)
        lib = _lib.load()
        b, _, h, w = depth.shape
        self._ensure(depth.device, b * h * w)
        depth = depth.contiguous().float()
        image = image.contiguous().float()
        kinv = torch.inverse(intrinsics.float().cpu())[:, :3, :3].contiguous().to(depth.device)     # ply_utils.py:47, host LAPACK
        pose = extrinsics.float().contiguous()
        if not self.dropout > 0:
            uniform = None
        elif uniform is None:
            uniform = torch.rand_like(depth)
        if uniform is not None:
            uniform = uniform.contiguous().float()
        # the contiguous fp32 copies are held in `masks` (and in _keep): the pointer of a temporary copy would be handed out
        # again by the allocator for the next mask's copy
        masks = [m.contiguous().float() for m in static_masks] if static_masks else []
        ptrs = (ctypes.c_void_p * max(len(masks), 1))(*[m.data_ptr() for m in masks])
        roi = (ctypes.c_int32 * 4)(*self.roi) if self.roi is not None else None
        _lib.check(lib.mr_pointcloud_append_f32(
            depth.data_ptr(), ptrs, len(masks), float(len(masks) - min_hits), image.data_ptr(), kinv.data_ptr(),
            pose.data_ptr(), uniform.data_ptr() if uniform is not None else None, float(self.dropout),
            float(self.min_d), float(self.max_d), roi, b, h, w, self._records.data_ptr(), self._records.shape[0],
            self._cursor.data_ptr(), torch.cuda.current_stream().cuda_stream), "mr_pointcloud_append_f32")
        self._keep = (depth, image, kinv, pose, uniform, masks)          # alive until the launch has run
        self._pending += b * h * w

    def _drain(self):
        if self._records is None:
            return
        used = int(self._cursor.item())
        if used > self._records.shape[0]:
            raise RuntimeError("PLYSaver: device record buffer overflowed (internal capacity accounting)")
        if used:
            self._host.frombytes(self._records[:used].cpu().numpy().tobytes())
        self._cursor.zero_()
        self._pending = 0

    @property
    def data(self):
        self._drain()
        return self._host

    def save(self, file):
        """utils/ply_utils.py:18-32 (same header, binary little-endian float records)."""
        write_ply(file, self.data)


class PointcloudBuilder:
    """The keyframe loop body of create_pointcloud.py:66-102: static mask per keyframe, buffers of `buffer_length`,
    vote + masked depth of the middle keyframe into the PLYSaver.  Feed it the model's input/output dicts.
    `consistency` (None: nothing; else what monorec_amd.consistency.settings accepts): the middle keyframe's depth is first filtered
    against the other buffered keyframes, at most 8 of them, oldest first (`consistency.filter_depth`)."""

    def __init__(self, plysaver, mask_fill=32, buffer_length=5, min_hits=1, use_mask=True, consistency=None):
        from .consistency import MAX_VIEWS, settings
        self.ply = plysaver
        self.mask_fill, self.buffer_length, self.min_hits, self.use_mask = mask_fill, buffer_length, min_hits, use_mask
        self.key_index = buffer_length // 2
        self.consistency = settings(consistency)
        if self.consistency is not None and not 2 <= buffer_length <= MAX_VIEWS + 1:
            raise ValueError(f"PointcloudBuilder: consistency needs a buffer of 2 to {MAX_VIEWS + 1} keyframes, not {buffer_length}")
        self._buf = []

    def add(self, data, result):
        output = result["result"]
        cv_mask = result["cv_mask"] if "cv_mask" in result else output.new_zeros(output.shape)
        # clones: `result` may come from submit() (views of resident buffers that later forwards overwrite), and the buffered
        # depth is multiplied in place by the vote below
        self._buf.append(dict(pose=data["keyframe_pose"].clone(), intrinsics=data["keyframe_intrinsics"].clone(),
                              mask=static_mask(cv_mask, self.mask_fill), keyframe=data["keyframe"].clone(),
                              depth=output.clone()))
        if self.consistency is not None:           # the relative poses are formed on the host: one copy per keyframe, not one per use
            self._buf[-1]["host"] = (data["keyframe_pose"].cpu(), data["keyframe_intrinsics"].cpu())
        if len(self._buf) >= self.buffer_length:
            k = self._buf[self.key_index]
            masks = [e["mask"] for e in self._buf] if self.use_mask else None
            depth = k["depth"]
            if self.consistency is not None:
                from .consistency import filter_depth
                others = [(e["depth"],) + e["host"] for e in self._buf if e is not k]
                depth, _ = filter_depth(depth, k["host"][0], k["host"][1], others, **self.consistency)
            self.ply.add_depthmap(depth, k["keyframe"], k["intrinsics"], k["pose"], static_masks=masks,
                                  min_hits=self.min_hits)
            del self._buf[0]


DEVICE_DATASETS = ("KittiOdometryDataset", "TUMMonoVODataset", "TUMMonoVOMultiDataset")


def _dataset_class(name):
    """`config.initialize('data_set', module_data)` (create_pointcloud.py:32) resolved to the device-side classes."""
    if name not in DEVICE_DATASETS:
        raise ValueError(f"monorec_amd.pointcloud: no device data source for data_set.type {name!r} (available: {', '.join(DEVICE_DATASETS)})")
    if name == "KittiOdometryDataset":
        from .kitti import KittiOdometryDataset
        return KittiOdometryDataset
    from . import tum_mono_vo
    return getattr(tum_mono_vo, name)


def run(config, model=None, dataset=None, out=None, dropout=.75, device="cuda:0"):
    """create_pointcloud.py:16-105 for a config dict of that script's shape: `data_set.type/args` -> device dataset, windowed by
    `start` / `end` (DS_Wrapper), batch size 1 -> `arch.args` -> MonoRecModel -> PointcloudBuilder (static masks, 5-keyframe vote)
    -> PLYSaver(`min_d`, `max_d`, `roi`, dropout) -> `output_dir/file_name`.  `model` / `dataset`: use these instead of building them
    from the config; `out`: a path or a binary file object instead of `output_dir/file_name`; `dropout`: the random thinning the
    script hard-wires to .75 (:52).  Optional key `consistency` (absent or false: nothing; else monorec_amd.consistency.settings): the
    middle keyframe's depth is filtered against the other four buffered ones before it goes to the saver.  Returns the number of
    records written."""
    import os
    from .kitti import DeviceLoader
    if dataset is None:
        dataset_class = _dataset_class(config["data_set"]["type"])
    if model is None and config["arch"]["type"] != "MonoRecModel":
        raise ValueError(f"monorec_amd.pointcloud: arch.type {config['arch']['type']!r} is not MonoRecModel")
    if model is None:
        from .model import MonoRecModel
        model = MonoRecModel(**config["arch"]["args"]).to(device)
    device = next(model.parameters()).device
    if dataset is None:
        dataset = dataset_class(**dict(config["data_set"]["args"], device=device))
    model.eval()
    loader = DeviceLoader(dataset, batch_size=1, start=config.get("start", 0), end=config.get("end", -1))
    height, width = dataset.target_image_size
    saver = PLYSaver(height, width, min_d=config.get("min_d", 3), max_d=config.get("max_d", 30), batch_size=loader.batch_size,
                     roi=config.get("roi", None), dropout=dropout)
    saver.to(device)
    builder = PointcloudBuilder(saver, mask_fill=32, buffer_length=5, min_hits=1, use_mask=config.get("use_mask", True),
                                consistency=config.get("consistency", None))
    with torch.no_grad():
        for data, _ in loader:
            result = model(data)
            # the datasets keep the 4x4 matrices on the host for the model's pose algebra; the saver multiplies on the device
            builder.add(dict(data, keyframe_pose=data["keyframe_pose"].to(device),
                             keyframe_intrinsics=data["keyframe_intrinsics"].to(device)), result)
    if out is None:
        output_dir = config.get("output_dir", "saved")
        os.makedirs(output_dir, exist_ok=True)
        out = os.path.join(output_dir, config.get("file_name", "pc.ply"))
    if hasattr(out, "write"):
        saver.save(out)
    else:
        with open(out, "wb") as f:
            saver.save(f)
    return len(saver.data) // 6


def main(argv=None):
    """The command line of create_pointcloud.py:108-119 (utils/parse_config.py:21-32: with --resume the config.json beside the
    checkpoint is read first and --config updates it)."""
    import argparse
    import json
    import os
    parser = argparse.ArgumentParser(description="MonoRec point cloud on the device (create_pointcloud.py)")
    parser.add_argument("-c", "--config", default=None, type=str, help="config file path")
    parser.add_argument("-r", "--resume", default=None, type=str, help="checkpoint; its folder's config.json is the base config")
    parser.add_argument("-d", "--device", default="cuda:0", type=str, help="torch device (default: cuda:0)")
    args = parser.parse_args(argv)
    if args.resume is None and args.config is None:
        parser.error("a configuration file is needed: --config FILE")
    config = {}
    if args.resume is not None:
        with open(os.path.join(os.path.dirname(os.path.abspath(args.resume)), "config.json")) as f:
            config = json.load(f)
    if args.config is not None:
        with open(args.config) as f:
            config.update(json.load(f))
    print(f"{run(config, device=args.device)} points written")


if __name__ == "__main__":
    main()
