"""TSDF-fusion export on the MI355X: the reference's `save_frame_for_tsdf` / `save_intrinsics_for_tsdf` (utils/util.py:78-98) and a
pipelined runner that writes one `frame-%06d.color.jpg` / `.depth.png` (16 bit, centimetres) / `.pose.txt` triple per keyframe plus
`camera-intrinsics.txt` - the layout the usual volumetric-fusion tools read.

    from monorec_amd.tsdf_export import save_frame_for_tsdf, save_intrinsics_for_tsdf, TSDFExporter, run
    python -m monorec_amd.tsdf_export --config configs/test/pointcloud_monorec.json

Everything the reference does to a keyframe before it calls Pillow - crop, `1 / depth * 100` to int16 with its wrap-around, the
`< 0` / `< min` / `> max` zeroing, `(keyframe + .5) * 255` to interleaved bytes, optionally the static-mask vote and `depth *= mask` of
create_pointcloud.py:90-92 - is one launch (`mr_tsdf_frame_f32`, bit for bit the x86 torch result).  There is no CPU fallback for it.

The encoders are the slow part (a 16-bit PNG costs tens of milliseconds, the model delivers a keyframe in little more than one), so
`TSDFExporter` never makes the device wait for them: `add()` enqueues the pack launch and an asynchronous copy into a slot of a pinned
ring on the caller's stream and returns; a pool of threads (Pillow's encoders release the GIL, like the decoders of
input_pipeline.FrameCache's pool) waits for the slot's event and writes the files.  `add()` blocks only when every slot is taken."""
import ctypes
import functools
import json
import os
import queue
import threading

import numpy as np
import torch

from . import _lib

BUFFER_LENGTH = 5            # create_pointcloud.py:57: keyframes voted over; the middle one is exported


# ------------------------------------------------------------------------------------------ host helpers
def threshold_cm(distance, none):
    """`depth < min_distance * 100` (utils/util.py:86,88) compares an int16 tensor with a Python float: torch does that in fp32, with
    the product formed in double first (.07 * 100 = 7.000000000000001 becomes 7.0: a depth of exactly 7 cm is kept).  Returns the
    fp32 threshold in centimetres as a Python float; `none` (-inf / +inf) when there is no threshold."""
    if distance is None:
        return float(none)
    return float(np.float32(float(distance) * 100))


def crop_box(crop, height, width):
    """The reference's crop `[y0, y1, x0, x1]` (slices `[crop[0]:crop[1], crop[2]:crop[3]]`) as checked non-negative bounds."""
    if crop is None:
        return 0, int(height), 0, int(width)
    y0, y1, x0, x1 = (int(v) for v in crop)
    if not (0 <= y0 < y1 <= height and 0 <= x0 < x1 <= width):
        raise ValueError(f"crop {list(crop)} is empty or outside the {height} x {width} image (y0, y1, x0, x1)")
    return y0, y1, x0, x1


def plan_shard(window, use_mask, rank=0, world=1, buffer_length=BUFFER_LENGTH):
    """Which keyframes of a window of `window` items rank `rank` of `world` runs and writes.  With `use_mask` the rule is
    create_pointcloud.py:66-102: a buffer of `buffer_length`, the middle keyframe is exported once the buffer is full, so the first and
    last `buffer_length // 2` keyframes of the window are never exported.  Exported frames are numbered 0 .. total-1 in export order and
    split into contiguous ranges; a rank also runs the `buffer_length // 2` keyframes either side that its votes need.
    Returns dict(total, exports=(lo, hi), items=(first, last)) - export numbers [lo, hi), window items [first, last)."""
    rank, world, window = int(rank), int(world), int(window)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"shard ({rank}, {world}): need 0 <= rank < world")
    halo = buffer_length // 2 if use_mask else 0
    total = max(0, window - 2 * halo)
    lo, hi = total * rank // world, total * (rank + 1) // world
    items = (lo, hi + 2 * halo) if hi > lo else (lo, lo)          # export e is window item e + halo and needs items e .. e + 2 halo
    return {"total": total, "exports": (lo, hi), "items": items, "halo": halo}


def write_manifest(out_dir, frames, merge=False):
    """`frames.json`: export number -> [sequence, image_id].  `merge`: add to the entries another shard has written (the directory is
    locked meanwhile), so that the shards of one run leave the file an unsharded run leaves."""
    path = os.path.join(str(out_dir), "frames.json")
    fd = os.open(str(out_dir), os.O_RDONLY)
    try:
        import fcntl
        fcntl.flock(fd, fcntl.LOCK_EX)
        entries = {}
        if merge and os.path.exists(path):
            with open(path) as f:
                entries = {int(k): v for k, v in json.load(f)["frames"].items()}
        entries.update({int(k): [int(v[0]), int(v[1])] for k, v in frames.items()})
        tmp = path + f".{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump({"version": 1, "frames": {str(k): entries[k] for k in sorted(entries)}}, f, indent=1)
            f.write("\n")
        os.replace(tmp, path)
    finally:
        os.close(fd)
    return path


def read_manifest(out_dir):
    with open(os.path.join(str(out_dir), "frames.json")) as f:
        return {int(k): tuple(v) for k, v in json.load(f)["frames"].items()}


def write_frame_files(out_dir, index, depth, colour, inverse_pose, png_compress_level=None):
    """What utils/util.py:89-91 writes, from the packed arrays: `depth` (h, w) int16 or uint16 (never negative), `colour` (h, w, 3)
    uint8, `inverse_pose` (4, 4).  The PNG is written as unsigned 16 bit (`I;16`): the pixel values of the reference's int16 image,
    without the mode-`I` save Pillow has deprecated.  `png_compress_level=None` is Pillow's default, as in the reference."""
    from PIL import Image
    base = os.path.join(str(out_dir), f"frame-{int(index):06d}")
    Image.fromarray(np.ascontiguousarray(colour)).save(base + ".color.jpg")
    png = Image.fromarray(np.ascontiguousarray(depth).view(np.uint16))
    if png_compress_level is None:
        png.save(base + ".depth.png")
    else:
        png.save(base + ".depth.png", compress_level=int(png_compress_level))
    np.savetxt(base + ".pose.txt", np.asarray(inverse_pose))


def _inverse_pose(pose):
    """`torch.inverse(pose)` (utils/util.py:91) on the host in fp32, like the rest of the project's 4 x 4 algebra."""
    return torch.inverse(pose.detach().to("cpu", torch.float32).reshape(4, 4)).numpy()


# ------------------------------------------------------------------------------------------ the launch
_need_cuda = functools.partial(_lib.need_cuda, "tsdf_export")


def packed_sizes(batch, ch, cw):
    """Bytes of the depth block (rounded up to 16, so that the colour block behind it stays aligned) and of the colour block."""
    depth_bytes = batch * ch * cw * 2
    return (depth_bytes + 15) // 16 * 16, batch * ch * cw * 3


def pack_frames(inv_depth, keyframe, crop=None, min_distance=None, max_distance=None, static_masks=None, min_hits=1, out=None):
    """One `mr_tsdf_frame_f32` launch on the current stream.  inv_depth (B,1,H,W) or (H,W); keyframe (B,3,H,W) or (3,H,W) in
    [-.5, .5]; `static_masks`: the buffered static_mask() outputs whose vote (`sum > len - min_hits`) multiplies the inverse depth first.
    Returns (depth (B, ch, cw) int16, colour (B, ch, cw, 3) uint8, keep-alive tuple); with `out` (a uint8 device buffer of
    sum(packed_sizes) bytes) the two are views of it."""
    _need_cuda(inv_depth, "depth")
    _need_cuda(keyframe, "keyframe")
    lib = _lib.load()
    h, w = int(inv_depth.shape[-2]), int(inv_depth.shape[-1])
    d = inv_depth.reshape(-1, h, w).contiguous().float()
    k = keyframe.reshape(-1, 3, h, w).contiguous().float()
    b = d.shape[0]
    if k.shape[0] != b:
        raise ValueError(f"keyframe {tuple(keyframe.shape)} and depth {tuple(inv_depth.shape)} disagree on the batch")
    y0, y1, x0, x1 = crop_box(crop, h, w)
    ch, cw = y1 - y0, x1 - x0
    depth_bytes, colour_bytes = packed_sizes(b, ch, cw)
    if out is None:
        out = torch.empty(depth_bytes + colour_bytes, dtype=torch.uint8, device=d.device)
    elif out.numel() < depth_bytes + colour_bytes or out.device != d.device or out.dtype != torch.uint8:
        raise ValueError("out: too small, on another device or not uint8")
    depth = out[:b * ch * cw * 2].view(torch.int16).view(b, ch, cw)
    colour = out[depth_bytes:depth_bytes + colour_bytes].view(b, ch, cw, 3)
    masks = [m.reshape(-1, h, w).contiguous().float() for m in (static_masks or [])]
    for m in masks:
        _need_cuda(m, "static mask")
        if m.shape[0] != b:
            raise ValueError("static masks and depth disagree on the batch")
    ptrs = (ctypes.c_void_p * max(len(masks), 1))(*[m.data_ptr() for m in masks])
    box = (ctypes.c_int32 * 4)(y0, y1, x0, x1)
    with torch.cuda.device(d.device):
        _lib.check(lib.mr_tsdf_frame_f32(d.data_ptr(), k.data_ptr(), ptrs, len(masks), float(len(masks) - min_hits), box,
                                         threshold_cm(min_distance, "-inf"), threshold_cm(max_distance, "inf"), b, h, w,
                                         depth.data_ptr(), colour.data_ptr(), torch.cuda.current_stream(d.device).cuda_stream),
                   "mr_tsdf_frame_f32")
    return depth, colour, (d, k, masks)


# ------------------------------------------------------------------------------------------ drop-in functions
def save_frame_for_tsdf(dir, index, keyframe, depth, pose, crop=None, min_distance=None, max_distance=None):
    """utils/util.py:78-91 with the reference's signature and file names, for DEVICE tensors: keyframe (3,H,W) in [-.5, .5], depth
    (H,W) - the predicted inverse depth -, pose (4,4).  One launch, one copy, then Pillow.  (A leading batch dimension of one is accepted.)"""
    packed_depth, packed_colour, _ = pack_frames(depth, keyframe, crop, min_distance, max_distance)
    if packed_depth.shape[0] != 1:
        raise ValueError("save_frame_for_tsdf writes one keyframe; use TSDFExporter for a stream of them")
    write_frame_files(dir, index, packed_depth[0].cpu().numpy(), packed_colour[0].cpu().numpy(), _inverse_pose(pose))


def save_intrinsics_for_tsdf(dir, intrinsics, crop=None):
    """utils/util.py:94-98: `camera-intrinsics.txt`, the 3 x 3 pixel intrinsics with the principal point moved into the crop.
    Unlike the reference, which shifts `intrinsics[0, 2]` / `[1, 2]` of the CALLER's tensor in place (a second call shifts twice),
    this works on a copy: the argument is left as it was."""
    k = intrinsics.detach().to("cpu").reshape(intrinsics.shape[-2], intrinsics.shape[-1]).clone()
    if crop is not None:
        k[0, 2] -= crop[2]
        k[1, 2] -= crop[0]
    np.savetxt(os.path.join(str(dir), "camera-intrinsics.txt"), k[:3, :3].numpy())


# ------------------------------------------------------------------------------------------ the exporter
class _Slot:
    def __init__(self, nbytes, pin):
        self.host = torch.empty(nbytes, dtype=torch.uint8)
        self.ids = torch.zeros(2, dtype=torch.int32)
        if pin:
            self.host, self.ids = self.host.pin_memory(), self.ids.pin_memory()
        self.device = None          # staging buffer on the device, allocated by the first add()
        self.event = None
        self.keep = None            # inputs of the launch, alive until the slot is reused


class TSDFExporter:
    """Writer of one export directory.  `add()` is asynchronous (pack launch + copy into a pinned ring slot + event on the current
    stream); `workers` threads wait for the events and encode.  `ring` slots bound what is in flight: `add()` blocks when all are taken -
    the back-pressure.  `close()` drains, writes `frames.json` (export number -> [sequence, image_id] of the frames that were given
    ids) and re-raises the first error of a worker.  Usable as a context manager."""

    def __init__(self, out_dir, height, width, crop=None, min_distance=None, max_distance=None, ring=8, workers=8,
                 png_compress_level=None, merge_manifest=False, pin=None):
        if ring < 1 or workers < 1:
            raise ValueError("ring and workers must be at least 1")
        self.out_dir = str(out_dir)
        os.makedirs(self.out_dir, exist_ok=True)
        self.height, self.width = int(height), int(width)
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        self.box = crop_box(crop, self.height, self.width)
        self.ch, self.cw = self.box[1] - self.box[0], self.box[3] - self.box[2]
        self.min_distance, self.max_distance = min_distance, max_distance
        self.png_compress_level = png_compress_level
        self.merge_manifest = bool(merge_manifest)
        self._depth_bytes, self._colour_bytes = packed_sizes(1, self.ch, self.cw)
        pin = torch.cuda.is_available() if pin is None else bool(pin)
        self._free = queue.Queue()
        for _ in range(int(ring)):
            self._free.put(_Slot(self._depth_bytes + self._colour_bytes, pin))
        self._jobs = queue.Queue()
        self._write = write_frame_files          # (out_dir, index, depth, colour, inverse_pose, png_compress_level); tests wrap it
        self._error = None
        self._lock = threading.Lock()
        self._frames = {}
        self.written = 0
        self._closed = False
        self._threads = [threading.Thread(target=self._work, name=f"tsdf-export-{i}", daemon=True) for i in range(int(workers))]
        for t in self._threads:
            t.start()

    # -- producers
    def _views(self, slot):
        host = slot.host.numpy()
        depth = host[:self.ch * self.cw * 2].view(np.int16).reshape(self.ch, self.cw)
        colour = host[self._depth_bytes:self._depth_bytes + self._colour_bytes].reshape(self.ch, self.cw, 3)
        return depth, colour

    def _check_open(self):
        if self._closed:
            raise RuntimeError("TSDFExporter: closed")
        if self._error is not None:
            raise RuntimeError(f"TSDFExporter: a writer failed: {self._error!r}") from self._error

    def add(self, index, keyframe, inv_depth, pose, static_masks=None, min_hits=1, sequence=None, image_id=None):
        """Enqueue keyframe number `index` of the export: keyframe (1,3,H,W) / (3,H,W), inv_depth (1,1,H,W) / (H,W) on the device,
        pose (4,4) anywhere (inverted on the host).  `static_masks` / `min_hits`: the vote of create_pointcloud.py:90-92 fused into the
        launch.  `sequence` / `image_id` (ints or one-element tensors) go to `frames.json`.  The launch and the copy are enqueued on the
        CURRENT stream - the one that produced (or was ordered behind) the tensors; the tensors may be overwritten by anything
        enqueued on that stream afterwards."""
        self._check_open()
        _need_cuda(inv_depth, "inv_depth")
        if tuple(inv_depth.shape[-2:]) != (self.height, self.width) or inv_depth.numel() != self.height * self.width:
            raise ValueError(f"inv_depth {tuple(inv_depth.shape)}: expected one {self.height} x {self.width} map")
        inverse_pose = _inverse_pose(pose)
        slot = self._free.get()                                   # blocks while every slot is being copied or encoded
        try:
            device = inv_depth.device
            if slot.device is None or slot.device.device != device:
                slot.device = torch.empty(slot.host.numel(), dtype=torch.uint8, device=device)
                slot.event = torch.cuda.Event()
            _, _, slot.keep = pack_frames(inv_depth, keyframe, self.crop, self.min_distance, self.max_distance, static_masks,
                                          min_hits, out=slot.device)
            with torch.cuda.device(device):
                slot.host.copy_(slot.device, non_blocking=True)
                ids = None
                if sequence is not None and image_id is not None:
                    if torch.is_tensor(sequence) or torch.is_tensor(image_id):
                        slot.ids[0:1].copy_(torch.as_tensor(sequence).reshape(-1)[:1], non_blocking=True)
                        slot.ids[1:2].copy_(torch.as_tensor(image_id).reshape(-1)[:1], non_blocking=True)
                        ids = "slot"
                    else:
                        ids = (int(sequence), int(image_id))
                slot.event.record(torch.cuda.current_stream(device))
        except BaseException:
            self._free.put(slot)
            raise
        self._jobs.put((slot, int(index), inverse_pose, ids, slot.event))

    def add_packed(self, index, depth, colour, pose, sequence=None, image_id=None):
        """The same hand-over for arrays that are on the host already (depth (ch, cw) int16, colour (ch, cw, 3) uint8): through the
        ring and the pool, without launch, copy or event."""
        self._check_open()
        depth, colour = np.asarray(depth), np.asarray(colour)
        if depth.shape != (self.ch, self.cw) or colour.shape != (self.ch, self.cw, 3) or depth.dtype != np.int16 or colour.dtype != np.uint8:
            raise ValueError(f"add_packed: expected int16 {(self.ch, self.cw)} and uint8 {(self.ch, self.cw, 3)}")
        inverse_pose = _inverse_pose(torch.as_tensor(pose))
        slot = self._free.get()
        d, c = self._views(slot)
        d[...] = depth
        c[...] = colour
        ids = None if sequence is None or image_id is None else (int(sequence), int(image_id))
        self._jobs.put((slot, int(index), inverse_pose, ids, None))

    # -- consumers
    def _work(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            slot, index, inverse_pose, ids, event = job
            try:
                if event is not None:
                    event.synchronize()
                if ids == "slot":
                    ids = (int(slot.ids[0]), int(slot.ids[1]))
                depth, colour = self._views(slot)
                self._write(self.out_dir, index, depth, colour, inverse_pose, self.png_compress_level)
                with self._lock:
                    self.written += 1
                    if ids is not None:
                        self._frames[index] = ids
            except BaseException as e:       # kept for close(); the slot goes back so that the producer cannot hang
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                self._free.put(slot)

    def close(self):
        """Wait for every enqueued frame, stop the pool, write `frames.json`, re-raise the first worker error."""
        if self._closed:
            return
        self._closed = True
        for _ in self._threads:
            self._jobs.put(None)
        for t in self._threads:
            t.join()
        if self._error is not None:
            raise self._error
        write_manifest(self.out_dir, self._frames, merge=self.merge_manifest)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                # do not mask the caller's exception with a writer's
            try:
                self.close()
            except BaseException:
                pass
        return False


# ------------------------------------------------------------------------------------------ the runner
class KeyframeStream:
    """The keyframe loop of `run`, shared with monorec_amd.tsdf_fusion.run: builds model and dataset from a config of
    create_pointcloud.py's shape unless they are handed in, plans the window (`plan_shard`), checks that the model keeps enough slots
    in flight for the vote, and `run(emit)` drives the pipelined loop (prepare / submit / synchronize), calling
    `emit(number, entry, masks)` once per exported keyframe in export order: `entry` holds keyframe, depth (views of the model's
    resident buffers, valid until the next submit), pose, intrinsics, sequence, image_id; `masks` the static masks to vote over, or None.

    With the config key `consistency` (monorec_amd.consistency.settings) the stream buffers BUFFER_LENGTH keyframes whether or not
    `use_mask` is set - the window is planned as `plan_shard(window, use_mask or consistency)`, so the first and last two keyframes of
    the window are not exported, as with the vote - and `entry["depth"]` is the middle keyframe's depth filtered against the other four
    buffered ones (`consistency.filter_depth`, the two older ones first): a buffer of the stream's own, valid until the next emit.  The
    vote multiplies afterwards; zeroing commutes with it.  The buffered depths are then not views of the model's slots: every collected
    depth is copied, device to device on the caller's stream, into a ring of BUFFER_LENGTH maps that the stream owns, like the static
    masks an output of its own - a buffered keyframe needs no slot after its collect, and without `use_mask` the model's whole
    `hip_in_flight` stays in flight."""

    def __init__(self, config, model=None, dataset=None, shard=(0, 1), device="cuda:0", who="monorec_amd.tsdf_export"):
        from . import consistency
        from .pointcloud import _dataset_class
        self.who = who
        rank, world = int(shard[0]), int(shard[1])
        self.rank, self.world = rank, world
        self.use_mask = use_mask = bool(config.get("use_mask", True))
        self.consistency = consistency.settings(config.get("consistency", None))                 # None: no filter, nothing below differs from a run without the key
        self.buffered = buffered = use_mask or self.consistency is not None
        plan_shard(0, buffered, rank, world)                                # a bad shard is reported before anything is built
        if model is None and config["arch"]["type"] != "MonoRecModel":
            raise ValueError(f"{who}: arch.type {config['arch']['type']!r} is not MonoRecModel")
        if dataset is None:
            dataset_class = _dataset_class(config["data_set"]["type"])
        if model is None:
            from .model import MonoRecModel
            args = dict(config["arch"].get("args", {}))
            if use_mask:
                args.setdefault("hip_in_flight", 6)
            model = MonoRecModel(**args).to(device)
        device = next(model.parameters()).device
        if dataset is None:
            dataset = dataset_class(**dict(config["data_set"]["args"], device=device))
        model.eval()
        self.model, self.dataset, self.device = model, dataset, device
        self.start, end = int(config.get("start", 0)), int(config.get("end", -1))
        self.window = max(0, (len(dataset) if end == -1 else end) - self.start)
        self.plan = plan_shard(self.window, buffered, rank, world)
        halo = self.plan["halo"] if use_mask else 0                         # (the vote's rule is kept as it is, with or without the filter)
        self.slots = int(getattr(model, "hip_in_flight", 1))
        # keyframe e is packed when keyframe e + halo has been collected, and that must come before submit number e + slots, which reuses its
        # slot: with P forwards pending the collect of e + halo precedes submit e + halo + P, so P <= slots - halo
        self.depth_in_flight = self.slots - halo
        if self.depth_in_flight < 1:
            raise ValueError(f"{who}: use_mask keeps a keyframe's outputs for {halo} more keyframes; the model needs "
                             f"hip_in_flight >= {halo + 1} (has {self.slots})")
        self.height, self.width = dataset.target_image_size
        self.crop = config.get("roi", None)
        self.intrinsics = None                                              # keyframe_intrinsics of the first item run() has loaded

    def export_items(self):
        """Dataset indices of the keyframes this rank exports, in export order."""
        lo, hi = self.plan["exports"]
        return [self.start + e + self.plan["halo"] for e in range(lo, hi)]

    def run(self, emit):
        import collections
        from .consistency import filter_depth
        from .kitti import DeviceLoader
        from .pointcloud import static_mask
        model, plan, slots, use_mask = self.model, self.plan, self.slots, self.use_mask
        first, last = plan["items"]
        loader = DeviceLoader(self.dataset, batch_size=1, start=self.start + first, end=self.start + last) if last > first else ()
        pending, buffer = collections.deque(), []
        state = {"submitted": 0, "exported": 0, "collected": 0}
        settings, ring = self.consistency, None
        middle = BUFFER_LENGTH // 2

        def export(entry, masks):
            # the submit that overwrites this keyframe's resident outputs is number entry.item + slots: it must not have happened yet
            if state["submitted"] > entry["item"] + slots:
                raise RuntimeError(f"{self.who}: a buffered keyframe's slot was reused before its pack launch (internal)")
            number = plan["exports"][0] + state["exported"]
            state["exported"] += 1
            emit(number, entry, masks)

        def export_filtered(masks):
            # the buffered depths are ring copies: the collect that overwrites the oldest one's is number oldest.item + BUFFER_LENGTH
            if state["collected"] > buffer[0]["item"] + BUFFER_LENGTH or [e["item"] for e in buffer] != list(range(buffer[0]["item"], buffer[0]["item"] + BUFFER_LENGTH)):
                raise RuntimeError(f"{self.who}: a buffered keyframe's depth copy was overwritten before the consistency filter read it (internal)")
            entry = buffer[middle]
            others = [(e["depth"], e["pose"], e["intrinsics"]) for k, e in enumerate(buffer) if k != middle]
            filtered, _ = filter_depth(entry["depth"], entry["pose"], entry["intrinsics"], others, out=ring[BUFFER_LENGTH], **settings)
            number = plan["exports"][0] + state["exported"]
            state["exported"] += 1
            emit(number, dict(entry, depth=filtered), masks)

        def collect():
            nonlocal ring
            item, data, handle = pending.popleft()
            out = handle.synchronize()                                  # the host waits: no blocked wait packet on the stream
            entry = dict(item=item, keyframe=data["keyframe"], depth=out["result"], pose=data["keyframe_pose"],
                         intrinsics=data["keyframe_intrinsics"], sequence=data.get("sequence"), image_id=data.get("image_id"))
            if not self.buffered:
                export(entry, None)
                return
            if settings is not None:
                # the copy reads the slot's resident output: the submit that overwrites it, number item + slots, must not have happened yet
                if state["submitted"] > item + slots:
                    raise RuntimeError(f"{self.who}: a collected keyframe's slot was reused before its depth was copied (internal)")
                if ring is None:                                        # BUFFER_LENGTH buffered depths and the filtered map
                    ring = torch.empty((BUFFER_LENGTH + 1,) + tuple(out["result"].shape), dtype=torch.float32, device=out["result"].device)
                entry["depth"] = ring[item % BUFFER_LENGTH]
                entry["depth"].copy_(out["result"])                     # device to device, on the caller's stream
                state["collected"] += 1
            if use_mask:
                cv_mask = out["cv_mask"] if "cv_mask" in out else out["result"].new_zeros(out["result"].shape)
                entry["mask"] = static_mask(cv_mask, 32)                # create_pointcloud.py:76-77; an output of its own, not a view
            buffer.append(entry)
            if len(buffer) >= BUFFER_LENGTH:
                masks = [e["mask"] for e in buffer] if use_mask else None
                if settings is not None:
                    export_filtered(masks)
                else:
                    export(buffer[middle], masks)
                del buffer[0]

        with torch.no_grad():
            for item, (data, _) in enumerate(loader):
                if self.intrinsics is None:
                    self.intrinsics = data["keyframe_intrinsics"][0]
                token = model.prepare(data)                             # pose algebra while the device is busy
                while len(pending) >= self.depth_in_flight:
                    collect()
                pending.append((item, data, model.submit(data, token)))
                state["submitted"] += 1
            while pending:
                collect()
        assert state["exported"] == plan["exports"][1] - plan["exports"][0]
        return state["exported"]


def run(config, model=None, dataset=None, shard=(0, 1), device="cuda:0", export=True):
    """Export the keyframes of a config of create_pointcloud.py's shape (configs/test/pointcloud_monorec*.json): `data_set` -> device
    dataset windowed by `start` / `end`, `arch` -> MonoRecModel, `roi` -> the crop, `min_d` / `max_d` -> the thresholds (absent: none),
    `use_mask` -> the 5-keyframe vote, `output_dir` -> the directory.  Optional keys: `export_ring`, `export_workers`,
    `png_compress_level`, `consistency` (absent or false: nothing; true or a dict of `rel_tol` .01, `max_reproj_px` 1, `min_views` 2,
    `average` false: every exported depth is first filtered against the two keyframes before and the two after it,
    monorec_amd.consistency - the first and last two keyframes of the window are then not exported, with or without `use_mask`).
    `model` / `dataset`: use these instead of building them.

    The loop (KeyframeStream) is pipelined (prepare / submit / synchronize with the model's `hip_in_flight`).  The outputs of submit() are
    views of the slot's resident buffers; nothing is cloned but the static masks (outputs of their own launch): the pack launch of a
    keyframe is enqueued before the submit that reuses its slot.  With `use_mask` a keyframe is exported two collects after its own, so
    two slots fewer are kept in flight (a model built here gets `hip_in_flight` 6 for that reason, unless `arch.args` says otherwise; a
    model handed in needs at least 3).

    `shard=(rank, world)`: the exported frames 0 .. N-1 are split into contiguous ranges; a rank runs the two extra keyframes either side
    its votes need and writes only its own files, rank 0 also `camera-intrinsics.txt`; `frames.json` is merged.  The union of the shards
    is the unsharded directory, byte for byte.  `export=False` runs the same loop without `add()` (the measurement of DESIGN.md section 7).
    Returns the number of frames this rank wrote."""
    stream = KeyframeStream(config, model, dataset, shard, device)
    crop = stream.crop
    out_dir = config.get("output_dir", "saved")
    os.makedirs(out_dir, exist_ok=True)
    exporter = None
    if export:
        exporter = TSDFExporter(out_dir, stream.height, stream.width, crop=crop, min_distance=config.get("min_d", None),
                                max_distance=config.get("max_d", None), ring=int(config.get("export_ring", 8)),
                                workers=int(config.get("export_workers", 8)), png_compress_level=config.get("png_compress_level", None),
                                merge_manifest=stream.world > 1)

    def emit(number, entry, masks):
        if exporter is not None:
            exporter.add(number, entry["keyframe"], entry["depth"], entry["pose"], static_masks=masks, min_hits=1,
                         sequence=entry["sequence"], image_id=entry["image_id"])

    try:
        exported = stream.run(emit)
        if stream.rank == 0 and stream.window > 0 and export:
            k = stream.intrinsics
            if k is None:                                           # rank 0 ran nothing (fewer exports than ranks, or none at all)
                k = stream.dataset[stream.start][0]["keyframe_intrinsics"]
            save_intrinsics_for_tsdf(out_dir, k, crop=crop)
    except BaseException:
        if exporter is not None:
            try:
                exporter.close()
            except BaseException:
                pass
        raise
    if exporter is not None:
        exporter.close()
    return exported


def load_config(argv=None, prog="python -m monorec_amd.tsdf_export",
                description="MonoRec keyframes as TSDF-fusion input (frame-%%06d.color.jpg / .depth.png / .pose.txt)"):
    """The command line of create_pointcloud.py:108-119 (utils/parse_config.py:21-32: with --resume the config.json beside the
    checkpoint is read first and --config updates it).  Returns (config, device)."""
    import argparse
    parser = argparse.ArgumentParser(prog=prog, description=description)
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
    for key in ("data_set", "arch"):
        if key not in config:
            parser.error(f"the configuration has no `{key}` section")
    return config, args.device


def main(argv=None):
    config, device = load_config(argv)
    from . import distributed
    shard = distributed.world_info()
    print(f"{run(config, shard=shard, device=device)} frames written to {config.get('output_dir', 'saved')}")


if __name__ == "__main__":
    main()
