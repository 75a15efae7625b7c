"""Pre-decoded frame store: the 8-bit result of the Pillow-exact crop and resize (and the sparse depth targets) of a dataset, packed
once by the device pipeline and read back through `mmap` -> pinned buffer -> one small unpack launch instead of a PNG / JPEG decode
and a resize per frame.

    python -m monorec_amd.frame_store pack --config configs/evaluate/eval_monorec.json --out data/kitti_store [--device cuda:0]
    dataset = KittiOdometryDataset("data/kitti", ..., frame_store="data/kitti_store")      # samples bit-equal to those without it

One file per stream under the store directory: `<key>_cam<k>.mrfs` (frames) and `<key>_target.mrfs` (targets), `<key>` = the KITTI
sequence name or the TUM-MonoVO sequence folder name.  Layout (little endian):

    0   8 bytes   magic "MRFSTORE"
    8   uint32    version                      12  uint32  header bytes
    16  uint64    length of the whole file
    24  header    JSON: everything a record depends on (see `frame_header` / `target_header`)
    ..  index     (uint64 offset, uint64 nbytes) per record, 8-byte aligned; nbytes == 0: the record is absent
    ..  records   each at a multiple of 4096 bytes

    frame record    `channels` planes of h * w bytes, each padded to a multiple of 16: the value of the resize BEFORE the response
                    table, the division and the grey stacking (kitti_odometry_dataset.py:120-134, tum_mono_vo_dataset.py:92-94) - the
                    table is applied at unpack, so it is not part of the header
    target record   uint32 n, n uint32 cell indices (ascending), n float32 values: the non-zero cells of the final target
                    (kitti_odometry_dataset.py:226-246).  Both target paths only ever write non-zero values, so the round trip is exact.

A store is tied to the geometry it was packed for: source image size, crop box and `target_image_size` (for targets also the depth
options) are in the header and checked when a dataset opens the file.  `FrameStoreWriter` / `FrameStoreReader` never touch the
device; `pack` needs a HIP device like the rest of the pipeline."""
import json
import os
import struct

import numpy as np

MAGIC = b"MRFSTORE"
VERSION = 1
RECORD_ALIGN = 4096
PLANE_ALIGN = 16
_PREFIX = struct.Struct("<8sIIQ")
PACK_HINT = "write it with `python -m monorec_amd.frame_store pack --config FILE --out DIR`"


def _round_up(n, m):
    return (n + m - 1) // m * m


def plane_stride(height, width):
    return _round_up(int(height) * int(width), PLANE_ALIGN)


def frames_path(store_dir, key, camera):
    return os.path.join(str(store_dir), f"{key}_cam{camera}.mrfs")


def targets_path(store_dir, key):
    return os.path.join(str(store_dir), f"{key}_target.mrfs")


def _plain(value):
    """What JSON makes of a header value: tuples become lists, numpy scalars Python numbers."""
    return json.loads(json.dumps(value, default=lambda v: v.item() if hasattr(v, "item") else list(v)))


def frame_header(dataset_class, sequence, camera, source_image_size, crop_box, target_image_size, channels, records):
    """Header of a frame stream.  `crop_box`: as `Image.crop` rounds it."""
    return _plain({"store_version": VERSION, "kind": "frames", "dataset": dataset_class, "sequence": sequence, "camera": camera,
                   "source_image_size": [int(v) for v in source_image_size], "crop_box": [int(round(v)) for v in crop_box],
                   "target_image_size": [int(v) for v in target_image_size], "channels": int(channels), "records": int(records)})


def target_header(dataset_class, sequence, camera, source_image_size, crop_box, target_image_size, records, depth_folder, lidar_depth,
                  annotated_lidar, dso_depth, dso_depth_parameters):
    """Header of a target stream: the frame geometry and every option the target depends on."""
    return _plain({"store_version": VERSION, "kind": "targets", "dataset": dataset_class, "sequence": sequence, "camera": camera,
                   "source_image_size": [int(v) for v in source_image_size], "crop_box": [int(round(v)) for v in crop_box],
                   "target_image_size": [int(v) for v in target_image_size], "channels": 1, "records": int(records),
                   "depth_folder": depth_folder, "lidar_depth": bool(lidar_depth), "annotated_lidar": bool(annotated_lidar),
                   "dso_depth": bool(dso_depth),
                   "dso_depth_parameters": None if dso_depth_parameters is None else [float(v) for v in dso_depth_parameters]})


def encode_target(target):
    """(.., H, W) float32 numpy target -> (ascending uint32 cell indices, float32 values) of its non-zero cells."""
    flat = np.ascontiguousarray(target, dtype=np.float32).reshape(-1)
    index = np.flatnonzero(flat)
    return index.astype(np.uint32), flat[index]


def decode_target(index, value, cells):
    """numpy mirror of mr_scatter_sparse_f32: zero-filled (cells,) float32 with value[i] at index[i]."""
    out = np.zeros(int(cells), dtype=np.float32)
    out[np.asarray(index, dtype=np.int64)] = value
    return out


class FrameStoreWriter:
    """Writes one stream: `header` (with its `records` count) first, records in any order, index table on `close()`."""

    def __init__(self, path, header):
        self.path, self.header = str(path), _plain(header)
        self.count = int(self.header["records"])
        blob = json.dumps(self.header, sort_keys=True).encode()
        self._table_at = _round_up(_PREFIX.size + len(blob), 8)
        self._table = np.zeros((self.count, 2), dtype="<u8")
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        self._f = open(self.path, "wb")
        self._f.write(_PREFIX.pack(MAGIC, VERSION, len(blob), 0))
        self._f.write(blob)
        self._end = self._table_at + self._table.nbytes
        self._f.write(b"\0" * (self._end - self._f.tell()))

    def _append(self, index, payload):
        if not 0 <= index < self.count:
            raise IndexError(f"record {index} outside the {self.count} records of {self.path}")
        if self._table[index, 1]:
            raise ValueError(f"record {index} of {self.path} is already written")
        at = _round_up(self._end, RECORD_ALIGN)
        self._f.write(b"\0" * (at - self._end))
        self._f.write(payload)
        self._table[index] = (at, len(payload))
        self._end = at + len(payload)

    def add_frame(self, index, planes):
        """planes: uint8 (channels, h, w) or (channels, >= h * w) - the planes of one resized frame."""
        h, w = self.header["target_image_size"]
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        planes = planes.reshape(planes.shape[0], -1)[:, :h * w]
        if planes.shape != (self.header["channels"], h * w):
            raise ValueError(f"frame of shape {planes.shape} in a store of {self.header['channels']} x {h * w}")
        padded = np.zeros((planes.shape[0], plane_stride(h, w)), dtype=np.uint8)
        padded[:, :h * w] = planes
        self._append(index, padded.tobytes())

    def add_target(self, index, cell_index, value):
        cell_index, value = np.ascontiguousarray(cell_index, dtype="<u4"), np.ascontiguousarray(value, dtype="<f4")
        if cell_index.shape != value.shape or cell_index.ndim != 1:
            raise ValueError("a target record needs as many values as indices")
        self._append(index, struct.pack("<I", cell_index.size) + cell_index.tobytes() + value.tobytes())

    def close(self):
        if self._f is None:
            return
        self._f.seek(self._table_at)
        self._f.write(self._table.tobytes())
        self._f.seek(0)
        self._f.write(_PREFIX.pack(MAGIC, VERSION, len(json.dumps(self.header, sort_keys=True).encode()), self._end))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FrameStoreReader:
    """Read-only view of one stream through `np.memmap`.  Raises FileNotFoundError when the file is missing, ValueError (naming the
    offending field) when it is not a store of this version, is truncated or its index table points outside the file."""

    def __init__(self, path):
        self.path = str(path)
        if not os.path.isfile(self.path):
            raise FileNotFoundError(f"frame store {self.path} not found - {PACK_HINT}")
        size = os.path.getsize(self.path)
        if size < _PREFIX.size:
            raise ValueError(f"{self.path}: file length {size} is shorter than the fixed prefix: truncated")
        self._map = np.memmap(self.path, dtype=np.uint8, mode="r")
        magic, version, header_bytes, length = _PREFIX.unpack(self._map[:_PREFIX.size].tobytes())
        if magic != MAGIC:
            raise ValueError(f"{self.path}: magic {magic!r} is not {MAGIC!r}: not a frame store")
        if version != VERSION:
            raise ValueError(f"{self.path}: version {version} is not the version {VERSION} this reader knows")
        if length != size:
            raise ValueError(f"{self.path}: file length {size} differs from the {length} bytes it was written with: truncated")
        if _PREFIX.size + header_bytes > size:
            raise ValueError(f"{self.path}: header of {header_bytes} bytes does not fit the file length {size}")
        self.header = json.loads(self._map[_PREFIX.size:_PREFIX.size + header_bytes].tobytes().decode())
        self.count = int(self.header["records"])
        table_at = _round_up(_PREFIX.size + header_bytes, 8)
        if table_at + 16 * self.count > size:
            raise ValueError(f"{self.path}: index table of {self.count} records does not fit the file length {size}")
        self._table = np.frombuffer(self._map[table_at:table_at + 16 * self.count].tobytes(), dtype="<u8").reshape(self.count, 2)
        present = self._table[:, 1] > 0
        bad = present & ((self._table[:, 0] + self._table[:, 1] > size) | (self._table[:, 0] % RECORD_ALIGN != 0) |
                         (self._table[:, 0] < table_at + 16 * self.count))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{self.path}: index table entry {i} (offset {int(self._table[i, 0])}, {int(self._table[i, 1])} bytes) "
                             f"points outside the records of a file of {size} bytes")
        h, w = self.header["target_image_size"]
        self.cells, self.plane_stride = int(h) * int(w), plane_stride(h, w)
        self.channels = int(self.header["channels"])
        if self.header["kind"] == "frames":
            wrong = present & (self._table[:, 1] != self.channels * self.plane_stride)
            if wrong.any():
                raise ValueError(f"{self.path}: index table entry {int(np.flatnonzero(wrong)[0])} is not a frame record of "
                                 f"{self.channels} x {self.plane_stride} bytes")

    def matches(self, expected_header):
        """None when every field of `expected_header` equals this file's, else the name of the first field that differs."""
        for name, value in _plain(expected_header).items():
            if name not in self.header or self.header[name] != value:
                return name
        return None

    def require(self, expected_header):
        name = self.matches(expected_header)
        if name is not None:
            raise ValueError(f"frame store {self.path} was packed for another {name}: {self.header.get(name)!r}, this dataset needs "
                             f"{_plain(expected_header)[name]!r} - a store is tied to its geometry; {PACK_HINT}")
        return self

    def has(self, index):
        return 0 <= index < self.count and bool(self._table[index, 1])

    def offset(self, index):
        return int(self._table[index, 0])

    def _bytes(self, index):
        if not self.has(index):
            return None
        at, n = int(self._table[index, 0]), int(self._table[index, 1])
        return self._map[at:at + n]

    def frame(self, index):
        """uint8 (channels, plane_stride) view of the mapped file, or None when the frame is absent."""
        raw = self._bytes(index)
        return None if raw is None else raw.reshape(self.channels, self.plane_stride)

    def target(self, index):
        """(n, raw bytes of n uint32 indices + n float32 values) or None when absent; validated against the record and the grid."""
        raw = self._bytes(index)
        if raw is None:
            return None
        n = int(np.frombuffer(raw[:4].tobytes(), dtype="<u4")[0])
        if raw.size != 4 + 8 * n or n > self.cells:
            raise ValueError(f"{self.path}: target record {index} says n = {n} but holds {raw.size} bytes (grid of {self.cells} cells)")
        body = raw[4:]
        if n and int(np.frombuffer(body[:4 * n], dtype="<u4").max()) >= self.cells:
            raise ValueError(f"{self.path}: target record {index} has a cell index outside the grid of {self.cells} cells")
        return n, body

    def target_arrays(self, index):
        """(uint32 indices, float32 values) of a target record, or None."""
        rec = self.target(index)
        if rec is None:
            return None
        n, body = rec
        body = np.array(body)
        return body[:4 * n].view("<u4"), body[4 * n:].view("<f4")

    def close(self):
        self._map = None


def open_frames(store_dir, expected_header):
    """The frame stream of `expected_header`'s sequence and camera under `store_dir`, checked against it."""
    return FrameStoreReader(frames_path(store_dir, expected_header["sequence"], expected_header["camera"])).require(expected_header)


def open_targets(store_dir, expected_header):
    return FrameStoreReader(targets_path(store_dir, expected_header["sequence"])).require(expected_header)


# ------------------------------------------------------------------------------------------------ packing (needs a HIP device)
def _decode_ahead(load, indices, workers):
    """(index, decoded image) in order, the decodes running up to 2 * workers ahead on `workers` threads."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers, thread_name_prefix="monorec-pack") as pool:
        pending, todo = deque(), iter(indices)
        for j in todo:
            pending.append((j, pool.submit(load, j)))
            if len(pending) >= 2 * workers:
                break
        while pending:
            j, fut = pending.popleft()
            nxt = next(todo, None)
            if nxt is not None:
                pending.append((nxt, pool.submit(load, nxt)))
            yield j, np.ascontiguousarray(np.asarray(fut.result()))


def _pack_frames(cache, header, store_dir, indices, workers):
    with FrameStoreWriter(frames_path(store_dir, header["sequence"], header["camera"]), header) as writer:
        for j, image in _decode_ahead(cache.load, sorted(indices), workers):
            writer.add_frame(j, cache.pre.resize_u8(image).cpu().numpy())
    return len(indices)


def pack(dataset, store_dir, indices=None):
    """Write the store of `dataset` (KittiOdometryDataset, TUMMonoVODataset or TUMMonoVOMultiDataset, opened WITHOUT `frame_store`)
    under `store_dir`: every frame and target its samples `indices` (default: all) reach - keyframes, neighbours, `offset_d`, the
    stereo camera; for a masked dataset that is exactly what its index set touches.  Everything else stays absent and is decoded
    when asked for.  Every stream file of the dataset is written, also one without records.  Returns the number of records."""
    if hasattr(dataset, "datasets"):                                    # TUMMonoVOMultiDataset
        keys = [d._store_key for d in dataset.datasets]
        if len(set(keys)) != len(keys):
            raise ValueError(f"frame store: the sequence folders {keys} do not have distinct names")
        wanted, written, base = (None if indices is None else sorted(indices)), 0, 0
        for d in dataset.datasets:
            local = None if wanted is None else [i - base for i in wanted if base <= i < base + len(d)]
            written += pack(d, store_dir, local)
            base += len(d)
        return written
    if getattr(dataset, "frame_store", None) is not None:
        raise ValueError("frame store: pack a dataset opened without frame_store (its samples are what gets stored)")
    workers = min(16, max(1, int(dataset._decode_workers)))
    frames, targets = dataset._store_reach(range(len(dataset)) if indices is None else indices)
    written = 0
    for (stream, camera), touched in sorted(frames.items()):
        written += _pack_frames(dataset._cache(stream, camera), dataset._frame_header(stream, camera), store_dir, touched, workers)
    for stream, touched in sorted(targets.items()):
        header = dataset._target_header(stream)
        with FrameStoreWriter(targets_path(store_dir, header["sequence"]), header) as writer:
            for key in sorted(touched):
                flat = dataset._target(stream, key).reshape(-1)
                cell = flat.nonzero().flatten()
                writer.add_target(key, cell.cpu().numpy(), flat[cell].cpu().numpy())
                written += 1
    return written


def dataset_from_config(config, device="cuda:0"):
    """The device dataset of an eval config (`data_loader.type/args`, configs/evaluate/*.json) or a point-cloud config
    (`data_set.type/args`, configs/test/pointcloud_*.json), opened without a store."""
    if "data_set" in config:
        from .pointcloud import _dataset_class
        args = dict(config["data_set"]["args"])
        args.pop("frame_store", None)
        return _dataset_class(config["data_set"]["type"])(**dict(args, device=device))
    if "data_loader" not in config:
        raise ValueError("frame store: the config has neither data_loader nor data_set")
    if config["data_loader"]["type"] != "KittiOdometryDataloader":
        raise ValueError(f"frame store: no device data source for data_loader.type {config['data_loader']['type']!r}")
    from .kitti import KittiOdometryDataset
    args = dict(config["data_loader"]["args"])
    workers = max(1, int(args.pop("num_workers", 4)))
    for name in ("batch_size", "shuffle", "validation_split", "frame_store"):
        args.pop(name, None)
    return KittiOdometryDataset(**dict(args, decode_workers=workers, device=device))


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m monorec_amd.frame_store", description="pre-decoded frame store")
    sub = parser.add_subparsers(dest="command", required=True)
    p = sub.add_parser("pack", help="write the store of the dataset a config describes")
    p.add_argument("-c", "--config", required=True, help="eval config (data_loader) or point-cloud config (data_set)")
    p.add_argument("-o", "--out", required=True, help="store directory")
    p.add_argument("-d", "--device", default="cuda:0")
    args = parser.parse_args(argv)
    with open(args.config) as f:
        config = json.load(f)
    dataset = dataset_from_config(config, device=args.device)
    count = pack(dataset, args.out)
    dataset.close()
    print(f"{count} records written to {args.out}")


if __name__ == "__main__":
    main()
