"""Pre-decoded frame store (monorec_amd.frame_store), host side: the container round trip, its error cases, the sparse target
encoding, dataset construction with `frame_store=` and the three C-ABI entries behind it.  No GPU; the device side is
tests/test_gpu_frame_store.py."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

from monorec_amd import _lib, frame_store, kitti, synth, tum_mono_vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mr_preprocess_image_u8_u8", "mr_unpack_frame_u8_f32", "mr_scatter_sparse_f32")


def _frame_header(h, w, channels, records=4, **changes):
    head = frame_store.frame_header("KittiOdometryDataset", "03", 2, (40, 56), (3.0, 2.0, 51.0, 34.0), (h, w), channels, records)
    return dict(head, **changes)


def _target_header(h, w, records=3, **changes):
    head = frame_store.target_header("KittiOdometryDataset", "03", 2, (40, 56), (3, 2, 51, 34), (h, w), records, "image_depth_annotated",
                                     True, True, False, None)
    return dict(head, **changes)


def _planes(h, w, channels, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(channels, h, w)).astype(np.uint8)


# ------------------------------------------------------------------------------------------ container
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("h,w", [(5, 7), (16, 24)])
def test_frame_records_round_trip(tmp_path, h, w, channels):
    path = tmp_path / "03_cam2.mrfs"
    frames = {0: _planes(h, w, channels, 1), 3: _planes(h, w, channels, 2), 1: _planes(h, w, channels, 3)}      # record 2 stays absent
    with frame_store.FrameStoreWriter(path, _frame_header(h, w, channels)) as writer:
        for i, planes in frames.items():                                                                          # any order
            writer.add_frame(i, planes)
    reader = frame_store.FrameStoreReader(path)
    assert reader.count == 4 and reader.channels == channels and reader.header == _frame_header(h, w, channels)
    assert reader.plane_stride % 16 == 0 and reader.plane_stride >= h * w and reader.plane_stride - h * w < 16
    assert reader.plane_stride == frame_store.plane_stride(h, w)
    for i, planes in frames.items():
        rec = reader.frame(i)
        assert reader.has(i) and rec.dtype == np.uint8 and rec.shape == (channels, reader.plane_stride)
        assert np.array_equal(rec[:, :h * w].reshape(channels, h, w), planes) and not rec[:, h * w:].any()
        assert reader.offset(i) % 4096 == 0 and reader.offset(i) > 0
        with pytest.raises(ValueError):
            rec[0, 0] = 1                                                                                         # mapped read-only
    assert not reader.has(2) and reader.frame(2) is None and not reader.has(4) and not reader.has(-1)
    assert reader.matches(_frame_header(h, w, channels)) is None
    with pytest.raises(ValueError, match="already written"):
        w2 = frame_store.FrameStoreWriter(tmp_path / "again.mrfs", _frame_header(h, w, channels))
        w2.add_frame(0, frames[0])
        w2.add_frame(0, frames[0])


def test_target_records_round_trip(tmp_path):
    h, w = 5, 7
    path = tmp_path / "03_target.mrfs"
    full = np.random.RandomState(4).rand(h * w).astype(np.float32) + 0.5
    some_index, some_value = np.array([0, 9, 34], dtype=np.uint32), np.array([0.25, 3.5, 1e-3], dtype=np.float32)
    with frame_store.FrameStoreWriter(path, _target_header(h, w, records=4)) as writer:
        writer.add_target(0, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))            # an empty target is a record
        writer.add_target(2, np.arange(h * w, dtype=np.uint32), full)
        writer.add_target(3, some_index, some_value)
    reader = frame_store.FrameStoreReader(path)
    assert reader.has(0) and not reader.has(1) and reader.target(1) is None and reader.target_arrays(1) is None
    n, raw = reader.target(0)
    assert n == 0 and raw.size == 0
    index, value = reader.target_arrays(2)
    assert index.dtype == np.uint32 and value.dtype == np.float32
    assert np.array_equal(index, np.arange(h * w)) and np.array_equal(value.view(np.uint32), full.view(np.uint32))
    n, raw = reader.target(3)
    assert n == 3 and bytes(raw) == some_index.tobytes() + some_value.tobytes()
    assert all(reader.offset(i) % 4096 == 0 for i in (0, 2, 3))
    assert np.array_equal(frame_store.decode_target(*reader.target_arrays(3), h * w).nonzero()[0], some_index)


def _written(tmp_path, name="s.mrfs"):
    path = tmp_path / name
    with frame_store.FrameStoreWriter(path, _frame_header(16, 24, 3, records=2)) as writer:
        writer.add_frame(0, _planes(16, 24, 3, 5))
        writer.add_frame(1, _planes(16, 24, 3, 6))
    return path


def test_missing_store_is_a_file_not_found_error_with_the_command(tmp_path):
    with pytest.raises(FileNotFoundError, match="monorec_amd.frame_store pack"):
        frame_store.FrameStoreReader(tmp_path / "nothing.mrfs")


def test_wrong_magic_version_and_length_raise(tmp_path):
    path = _written(tmp_path)
    good = path.read_bytes()
    frame_store.FrameStoreReader(path)
    path.write_bytes(b"PNGSTORE" + good[8:])
    with pytest.raises(ValueError, match="magic"):
        frame_store.FrameStoreReader(path)
    path.write_bytes(good[:8] + struct.pack("<I", frame_store.VERSION + 1) + good[12:])
    with pytest.raises(ValueError, match="version"):
        frame_store.FrameStoreReader(path)
    path.write_bytes(good[:-1])
    with pytest.raises(ValueError, match="file length"):
        frame_store.FrameStoreReader(path)
    path.write_bytes(good[:10])
    with pytest.raises(ValueError, match="file length"):
        frame_store.FrameStoreReader(path)


def test_index_table_pointing_past_the_end_raises(tmp_path):
    path = _written(tmp_path)
    good = bytearray(path.read_bytes())
    header_bytes = struct.unpack_from("<I", good, 12)[0]
    table_at = (24 + header_bytes + 7) // 8 * 8
    offset, nbytes = struct.unpack_from("<QQ", good, table_at + 16)
    assert offset % 4096 == 0 and offset + nbytes == len(good)                   # the last record ends the file
    for entry in ((offset + 4096, nbytes), (offset, nbytes + 16)):
        bad = bytearray(good)
        struct.pack_into("<QQ", bad, table_at + 16, *entry)
        path.write_bytes(bytes(bad))
        with pytest.raises(ValueError, match="index table"):
            frame_store.FrameStoreReader(path)


@pytest.mark.parametrize("field,value", [("target_image_size", [8, 48]), ("crop_box", [3, 2, 51, 35]), ("channels", 1), ("dso_depth", True)])
def test_header_mismatch_names_the_field(tmp_path, field, value):
    if field == "dso_depth":
        path, mine = tmp_path / "03_target.mrfs", _target_header(16, 24)
        with frame_store.FrameStoreWriter(path, mine) as writer:
            writer.add_target(0, np.array([1], dtype=np.uint32), np.array([2.0], dtype=np.float32))
    else:
        path, mine = _written(tmp_path), _frame_header(16, 24, 3, records=2)
    reader = frame_store.FrameStoreReader(path)
    assert reader.matches(mine) is None and reader.require(mine) is reader
    other = dict(mine, **{field: value})
    assert reader.matches(other) == field
    with pytest.raises(ValueError, match=field):
        reader.require(other)


def test_crop_box_is_stored_as_pillow_rounds_it():
    assert _frame_header(16, 24, 3)["crop_box"] == [3, 2, 51, 34]
    head = frame_store.frame_header("TUMMonoVODataset", "sequence_50", 0, (1024, 1280), (0, 32.0, 1280, 992.0), (480, 640), 1, 10)
    assert head["crop_box"] == [0, 32, 1280, 992] and json.loads(json.dumps(head)) == head


# ------------------------------------------------------------------------------------------ sparse targets
def test_sparse_target_encoding_is_exact():
    _, targets = synth.make_depth_pair(batch=2, height=64, width=96)
    targets = [t.numpy() for t in targets] + [np.zeros((1, 64, 96), dtype=np.float32)]
    assert 0 < np.count_nonzero(targets[0]) < targets[0].size
    for t in targets:
        index, value = frame_store.encode_target(t)
        assert index.dtype == np.uint32 and value.dtype == np.float32 and index.size == np.count_nonzero(t)
        assert np.all(np.diff(index.astype(np.int64)) > 0)                       # ascending, unique
        back = frame_store.decode_target(index, value, t.size).reshape(t.shape)
        assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), t.view(np.uint32))


# ------------------------------------------------------------------------------------------ datasets
def test_kitti_dataset_with_a_missing_store(tmp_path):
    tree = synth.make_kitti_tree(tmp_path / "kitti", sequences=(("03", 40, 120),), frames=12)
    kw = dict(sequences=["03"], depth_folder="image_depth_annotated", target_image_size=(16, 32), lidar_depth=True, dso_depth=False)
    plain = kitti.KittiOdometryDataset(tree, device="cpu", **kw)
    ds = kitti.KittiOdometryDataset(tree, device="cpu", frame_store=str(tmp_path / "no_store"), **kw)      # host bookkeeping unchanged
    assert len(ds) == len(plain) > 0 and ds._crop_boxes == plain._crop_boxes and plain.frame_store is None
    with pytest.raises(FileNotFoundError, match="monorec_amd.frame_store pack"):
        ds[0]
    public = {k: v for k, v in ds.__dict__.items() if not k.startswith("_")}                           # evaluate.py dumps these
    assert json.loads(json.dumps(public))["frame_store"] == str(tmp_path / "no_store")
    loader = kitti.KittiOdometryDataloader(dataset_dir=tree, batch_size=2, shuffle=False, num_workers=2, device="cpu",
                                           frame_store=str(tmp_path / "no_store"), **kw)
    assert loader.dataset.frame_store == str(tmp_path / "no_store")
    head = ds._frame_header(0, 2)
    assert head["sequence"] == "03" and head["camera"] == 2 and head["channels"] == 3 and head["records"] == 12
    assert head["target_image_size"] == [16, 32] and ds._frame_header(0, 0)["channels"] == 1
    assert ds._target_header(0)["lidar_depth"] is True and ds._target_header(0)["dso_depth_parameters"] is None


def test_kitti_store_reach_of_a_masked_stereo_dataset(tmp_path):
    tree = synth.make_kitti_tree(tmp_path / "kitti", sequences=(("03", 40, 120),), frames=16)
    ds = kitti.KittiOdometryDataset(tree, device="cpu", sequences=["03"], depth_folder="image_depth_annotated", target_image_size=(16, 32),
                                    **synth.KITTI_OPTION_CASES["masked_grey_stereo"])
    frames, targets = ds._store_reach(range(len(ds)))
    keys = ds._indices[0]
    assert sorted(frames) == [(0, 0), (0, 1)] and frames[(0, 1)] == set(keys) == targets[0]
    assert frames[(0, 0)] == {k + o for k in keys for o in (-2, -1, 0, 1, 2)}
    assert len(frames[(0, 0)]) < 16                                               # not everything: the rest stays absent
    assert ds._store_reach([])[0] == {(0, 0): set(), (0, 1): set()}              # every stream has an entry


def test_tum_dataset_with_a_missing_store(tmp_path):
    tree = synth.make_tmvo_tree(tmp_path / "sequence_xx")
    kw = dict(frame_count=2, target_image_size=(24, 32), color_augmentation=False, device="cpu")
    ds = tum_mono_vo.TUMMonoVODataset(tree, frame_store=str(tmp_path / "no_store"), **kw)
    assert len(ds) == len(tum_mono_vo.TUMMonoVODataset(tree, **kw)) > 0
    with pytest.raises(FileNotFoundError, match="monorec_amd.frame_store pack"):
        ds[0]
    public = {k: v for k, v in ds.__dict__.items() if not k.startswith("_")}
    assert json.loads(json.dumps(public))["frame_store"] == str(tmp_path / "no_store")
    head = ds._frame_header()
    assert head["sequence"] == "sequence_xx" and head["channels"] == 1 and head["records"] == 9 and "lut" not in head
    multi = tum_mono_vo.TUMMonoVOMultiDataset([tree], frame_store=str(tmp_path / "no_store"), **kw)
    assert multi.datasets[0].frame_store == str(tmp_path / "no_store")
    assert ds._store_reach([0]) == ({(0, 0): {0, 1, 2}}, {})


def test_config_forms_of_the_command_line(tmp_path):
    tree = synth.make_kitti_tree(tmp_path / "kitti", sequences=(("03", 40, 120),), frames=12)
    args = dict(dataset_dir=tree, depth_folder="image_depth_annotated", sequences=["03"], target_image_size=[16, 32], lidar_depth=True,
                dso_depth=False)
    ds = frame_store.dataset_from_config({"data_loader": {"type": "KittiOdometryDataloader", "args": dict(
        args, batch_size=2, shuffle=False, validation_split=0, num_workers=3, frame_store="ignored")}}, device="cpu")
    assert isinstance(ds, kitti.KittiOdometryDataset) and ds._decode_workers == 3 and ds.frame_store is None
    ds = frame_store.dataset_from_config({"data_set": {"type": "KittiOdometryDataset", "args": args}}, device="cpu")
    assert isinstance(ds, kitti.KittiOdometryDataset)
    with pytest.raises(ValueError):
        frame_store.dataset_from_config({"arch": {}})
    with pytest.raises(ValueError, match="without frame_store"):
        frame_store.pack(kitti.KittiOdometryDataset(device="cpu", frame_store=str(tmp_path / "s"), **args), tmp_path / "s")


# ------------------------------------------------------------------------------------------ ABI
def test_entries_are_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.ABI and getattr(hip_lib, name) is not None
        assert re.search(r"^\| `" + name + r"` \|", table, flags=re.M), name
    for line in ("kitti_odometry_dataset.py:120-134", "kitti_odometry_dataset.py:226-246", "tum_mono_vo_dataset.py:92-94"):
        assert line in header
    assert hip_lib.mr_abi_version() >= 22


def test_bad_arguments_are_reported_not_launched(hip_lib):
    src, dst = ctypes.create_string_buffer(256), ctypes.create_string_buffer(1024)
    s, d = ctypes.addressof(src), ctypes.addressof(dst)
    unpack = hip_lib.mr_unpack_frame_u8_f32
    assert unpack(s, 3, 35, 5, 7, None, d, None) == -1                          # plane_stride % 16 != 0
    assert unpack(s, 3, 32, 5, 7, None, d, None) == -1                          # plane_stride < h * w
    assert unpack(s, 2, 48, 5, 7, None, d, None) == -1                          # channels
    assert unpack(s, 3, 48, 5, 7, None, None, None) == -1                       # null dst
    assert unpack(None, 3, 48, 5, 7, None, d, None) == -1
    assert unpack(s, 3, 48, 0, 7, None, d, None) == -1 and unpack(s, 3, 48, 5, 0, None, d, None) == -1
    scatter = hip_lib.mr_scatter_sparse_f32
    assert scatter(s, s, 1, None, 35, None) == -1 and scatter(s, s, 1, d, 0, None) == -1 and scatter(None, s, 1, d, 35, None) == -1
    assert scatter(s, None, 1, d, 35, None) == -1 and scatter(s, s, -1, d, 35, None) == -1
    box = (ctypes.c_int32 * 4)(0, 0, 8, 8)
    resize = lambda channels=3, dst=d, stride=64, out_h=4: hip_lib.mr_preprocess_image_u8_u8(s, 8, 8, channels, 8 * channels, box, out_h, 4, s, s, 3,
                                                                                          s, s, 3, 8, dst, stride, None)
    assert resize(channels=2) == -1 and resize(dst=None) == -1 and resize(stride=15) == -1 and resize(out_h=0) == -1
