"""TUM-MonoVO data source on the device: mr_preprocess_image_u8_lut_f32 behind ImagePreprocessor(lut=) against Pillow,
monorec_amd.tum_mono_vo.TUMMonoVODataset sample by sample against the tensors the unmodified reference class produced
(tests/golden/tmvo_tree.*), pointcloud.run end to end, and one sample at the real 480x640 / four-source-frame shape."""
import hashlib
import io
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from monorec_amd import input_pipeline, kitti, pointcloud, synth, tum_mono_vo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
META = json.load(open(os.path.join(GOLDEN, "tmvo_tree.json")))
Z = np.load(os.path.join(GOLDEN, "tmvo_tree.npz"))

IDENTITY = np.arange(256, dtype=np.float32)
INVERSE_RESPONSE = tum_mono_vo.invert_pcalib(255.0 * (np.arange(256) / 255.0) ** 0.6).numpy()      # synth.make_tmvo_tree's pcalib.txt
FRACTIONAL = (255.0 * (np.arange(256) / 255.0) ** 1.7).astype(np.float32)                           # non-integer entries


def _pillow_statement(img_u8, box, out_h, out_w, table):
    """tum_mono_vo_dataset.py:84-100 with the Pillow of this machine."""
    from PIL import Image
    resized = np.asarray(Image.fromarray(img_u8).convert("RGB").crop(box).resize((out_w, out_h), Image.BILINEAR))
    t = torch.from_numpy(np.asarray(table, dtype=np.float32))[torch.from_numpy(resized.astype(np.int64))]
    return (t / 255 - .5).permute(2, 0, 1).contiguous()


def _dataset_box(h, w, oh, ow):
    return input_pipeline.compute_target_intrinsics(np.identity(4), (h, w), (oh, ow))[1]


PREPROCESS_CASES = {
    # name: (source h, w, channels, target h, w, crop box or None for the box the dataset computes)
    "tum_1024x1280_grey_2x": (1024, 1280, 1, 480, 640, None),            # box (0, 32, 1280, 992): the real geometry
    "grey_97x131_odd_ratio": (97, 131, 1, 40, 56, None),
    "rgb_97x131_odd_ratio": (97, 131, 3, 40, 56, None),
    "grey_20x30_upscaled": (20, 30, 1, 48, 64, None),
    "rgb_20x30_upscaled": (20, 30, 3, 48, 64, None),
    "grey_origin_not_multiple_of_4": (97, 131, 1, 40, 56, (3, 2, 128, 95)),
    "grey_origin_1_odd_row_length": (61, 83, 1, 24, 32, (1, 1, 82, 60)),
    "rgb_origin_not_multiple_of_4": (97, 131, 3, 40, 56, (5.0, 3, 126.0, 93)),
    "grey_700x900_down_28x": (700, 900, 1, 24, 32, None),                 # 504 source rows per tile: 32 KiB of LDS intermediate
}


@pytest.mark.parametrize("table", ["identity", "inverse_response", "fractional"])
@pytest.mark.parametrize("name", sorted(PREPROCESS_CASES))
def test_lut_preprocess_is_bit_equal_to_pillow(hip_lib, name, table):
    h, w, c, oh, ow, box = PREPROCESS_CASES[name]
    lut = {"identity": IDENTITY, "inverse_response": INVERSE_RESPONSE, "fractional": FRACTIONAL}[table]
    img = synth.make_u8_image(h, w, c, seed=17)
    box = box if box is not None else _dataset_box(h, w, oh, ow)
    if name.startswith("tum_"):
        assert tuple(box) == (0, 32.0, 1280, 992.0)
    pre = input_pipeline.ImagePreprocessor((h, w), (oh, ow), crop_box=box, device=DEV, lut=lut)
    got = pre(img).cpu()
    want = _pillow_statement(img, box, oh, ow, lut)
    assert got.dtype == torch.float32 and got.shape == (3, oh, ow)
    assert torch.equal(got, want), int((got != want).sum())
    if table == "identity":       # without a table: the existing entry, the same bits
        plain = input_pipeline.ImagePreprocessor((h, w), (oh, ow), crop_box=box, device=DEV)
        assert plain.lut is None and torch.equal(plain(img).cpu(), got)
    # a device-resident source at an odd address gives the same bits
    flat = torch.zeros(1 + img.size, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(img).to(DEV).flatten()
    out = torch.full((3, oh, ow), float("nan"), device=DEV)
    pre(flat[1:].view(img.shape), out=out)
    assert torch.equal(out.cpu(), want)


def test_lut_argument_checks(hip_lib):
    with pytest.raises(ValueError):
        input_pipeline.ImagePreprocessor((8, 8), (4, 4), device=DEV, lut=np.zeros(255))
    pre = input_pipeline.ImagePreprocessor((8, 8), (4, 4), device=DEV, lut=[float(i) for i in range(256)])      # any array-like
    assert pre.lut.is_cuda and pre.lut.dtype == torch.float32 and pre.lut.shape == (256,)
    assert torch.equal(pre(np.full((8, 8), 255, dtype=np.uint8)).cpu(), torch.full((3, 4, 4), 0.5))


def _check_sample_layout(data, target, ds, index):
    assert sorted(data) == ["frames", "image_id", "intrinsics", "keyframe", "keyframe_intrinsics", "keyframe_pose", "poses", "sequence"]
    h, w = ds.target_image_size
    for t in [data["keyframe"]] + data["frames"]:
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (3, h, w)
    for m in [data["keyframe_pose"], data["keyframe_intrinsics"]] + data["poses"] + data["intrinsics"]:
        assert not m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (4, 4)          # the matrices stay on the host
    assert len(data["frames"]) == len(data["poses"]) == len(data["intrinsics"]) == ds.frame_count
    for key, value in (("sequence", 0), ("image_id", index + ds._offset)):
        assert data[key].dtype == torch.int64 and tuple(data[key].shape) == (1,) and int(data[key]) == value
    assert target.is_cuda and target.dtype == torch.float32 and tuple(target.shape) == (1, h, w) and not bool(target.any())


@pytest.mark.parametrize("case", sorted(synth.TMVO_CASES))
def test_dataset_samples_are_bit_equal_to_the_reference_fixture(hip_lib, tmp_path, case):
    tree_kw, ds_kw = synth.TMVO_CASES[case]
    tree = synth.make_tmvo_tree(tmp_path / "sequence_xx", **tree_kw)
    want = META["cases"][case]
    from PIL import Image
    first = np.asarray(Image.open(os.path.join(tree, "images", "00000.jpg")))
    assert list(first.shape) == want["first_image_shape"] and hashlib.sha1(first.tobytes()).hexdigest() == want["first_image_sha1"]
    ds = tum_mono_vo.TUMMonoVODataset(tree, color_augmentation=False, device=DEV, decode_workers=3, **ds_kw)
    assert len(ds) == want["length"] > 0
    touched = set()
    for i in range(len(ds)):
        data, target = ds[i]
        _check_sample_layout(data, target, ds, i)
        assert want["samples"][i]["image_id"] == int(data["image_id"]) and want["samples"][i]["id_dtype"] == str(data["image_id"].dtype)
        assert want["samples"][i]["id_shape"] == list(data["image_id"].shape) and want["samples"][i]["sequence_dtype"] == str(data["sequence"].dtype)
        assert torch.equal(data["keyframe"].cpu(), torch.from_numpy(Z[f"{case}.{i}.keyframe"])), (case, i)
        frames = torch.from_numpy(Z[f"{case}.{i}.frames"])
        assert len(data["frames"]) == frames.shape[0]
        for j, f in enumerate(data["frames"]):
            assert torch.equal(f.cpu(), frames[j]), (case, i, j)
        assert np.array_equal(data["keyframe_intrinsics"].numpy().view(np.uint32), Z[f"{case}.intrinsics"].view(np.uint32))
        assert np.array_equal(torch.stack(data["poses"]).numpy()[:, :3, 3].view(np.uint32), Z[f"{case}.{i}.poses"][:, :3, 3].view(np.uint32))
        assert np.allclose(torch.stack(data["poses"]).numpy(), Z[f"{case}.{i}.poses"], rtol=0, atol=2e-7)     # rotations: 1 ulp, tests/test_tum_mono_vo.py
        touched |= {i + ds._offset, *ds._source_rows(i)}
    assert ds.cache.decoded == len(touched), "every image is decoded and resized once per sweep"       # the reference: 1 + frame_count times
    ds.close()


def test_dataset_on_a_jpeg_encoded_tree(hip_lib, tmp_path):
    """The decode path real sequences take: JPEG files (written by Pillow here), against the Pillow statement on the same decode."""
    from PIL import Image
    tree_kw, ds_kw = synth.TMVO_CASES["tall_dilated"]
    tree = synth.make_tmvo_tree(tmp_path / "sequence_xx", **tree_kw)
    folder = os.path.join(tree, "images")
    for name in sorted(os.listdir(folder)):
        pixels = np.asarray(Image.open(os.path.join(folder, name)))
        Image.fromarray(pixels).save(os.path.join(folder, name), format="JPEG", quality=92)
    with Image.open(os.path.join(folder, "00000.jpg")) as img:
        assert img.format == "JPEG" and img.mode == "L"
    ds = tum_mono_vo.TUMMonoVODataset(tree, color_augmentation=False, device=DEV, decode_workers=2, **ds_kw)
    statement = lambda row: _pillow_statement(np.asarray(Image.open(os.path.join(folder, f"{ds._image_index[row]:05d}.jpg"))),
                                              ds._crop_box, *ds.target_image_size, ds._pcalib.numpy())
    for i in range(len(ds)):
        data, target = ds[i]
        _check_sample_layout(data, target, ds, i)
        assert torch.equal(data["keyframe"].cpu(), statement(i + ds._offset))
        for f, row in zip(data["frames"], ds._source_rows(i)):
            assert torch.equal(f.cpu(), statement(row))
    ds.close()


def _seeded_model(depth_steps):
    from monorec_amd import MonoRecModel
    model = MonoRecModel(cv_depth_steps=depth_steps)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    return model.to(DEV).eval()


def _ply_records(buf):
    head, _, body = buf.getvalue().partition(b"end_header\n")
    count = int([line for line in head.decode().split("\n") if line.startswith("element vertex")][0].split()[-1])
    records = np.frombuffer(body, dtype="<f4")
    assert records.size == 6 * count
    return head, records


# Depth window of the end-to-end case: the network's inverse depths lie in [0.0025, 0.33], i.e. 3 m .. 400 m; with this window part
# of the pixels inside the roi passes and part does not
E2E_MIN_D, E2E_MAX_D = 3, 8

E2E_WINDOWS = {
    # name: (start, end, use_mask) -> the samples that go through the model; the buffer of five hands keyframes 2 .. n-3 to the saver
    "whole_sequence": (0, -1, False),                # 1925 records from keyframes 2, 3, 4 (3 x 4480 pixels inside the roi)
    "window_1_to_6": (1, 6, False),                  # samples 1 .. 5: keyframe 3 alone
    # the random-init mask head calls every pixel moving, so the vote empties the depth maps: 0 records on both sides - which still
    # tells a run() that dropped `use_mask` (1925 records) from one that passed it on
    "whole_sequence_masked": (0, -1, True),
}


@pytest.mark.parametrize("name", sorted(E2E_WINDOWS))
def test_pointcloud_run_equals_the_loop_over_its_pieces(hip_lib, tmp_path, name):
    """pointcloud.run on a 140x200 grey sequence -> 64x96, nine pose rows, frame_count 2 (seven samples): the records of the PLY it
    writes equal, bit for bit, the loop dataset -> model(data) -> PointcloudBuilder.add written out here.  Wiring only; the model's
    numbers belong to the parity tests."""
    from monorec_amd.pointcloud import PLYSaver, PointcloudBuilder
    start, end, use_mask = E2E_WINDOWS[name]
    tree = synth.make_tmvo_tree(tmp_path / "sequence_xx", height=140, width=200, seed=9)
    args = dict(dataset_dir=tree, frame_count=2, scale_factor=3, target_image_size=[64, 96], color_augmentation=False)
    roi, min_d, max_d = [4, 60, 8, 88], E2E_MIN_D, E2E_MAX_D
    config = {"name": "Pointcloud Creation", "n_gpu": 1, "output_dir": str(tmp_path / "out"), "file_name": "tmvo.ply", "roi": roi,
              "start": start, "end": end, "min_d": min_d, "max_d": max_d, "use_mask": use_mask,
              "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": 8}},
              "data_set": {"type": "TUMMonoVODataset", "args": args}}
    model = _seeded_model(8)
    count = pointcloud.run(config, model=model, dropout=0)
    with open(tmp_path / "out" / "tmvo.ply", "rb") as f:
        head, got = _ply_records(io.BytesIO(f.read()))
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and got.size == 6 * count

    ds = tum_mono_vo.TUMMonoVODataset(device=DEV, **args)
    assert len(ds) == 7
    saver = PLYSaver(64, 96, min_d=min_d, max_d=max_d, batch_size=1, roi=roi, dropout=0)
    saver.to(DEV)
    builder = PointcloudBuilder(saver, mask_fill=32, buffer_length=5, min_hits=1, use_mask=use_mask)
    samples = list(range(start, len(ds) if end == -1 else end))
    with torch.no_grad():
        for i in samples:
            data, _ = kitti.collate([ds[i]])
            result = model(data)
            builder.add(dict(data, keyframe_pose=data["keyframe_pose"].to(DEV), keyframe_intrinsics=data["keyframe_intrinsics"].to(DEV)), result)
    want = np.frombuffer(np.asarray(saver.data, dtype="<f4").tobytes(), dtype="<f4")
    added = len(samples) - 4
    print(f"{name}: {count} records from {added} keyframes of {64 * 96} pixels")
    assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if not use_mask:
        # neither filter degenerate: the roi alone leaves 56 * 80 = 4480 of the 6144 pixels of a keyframe, the depth range drops more
        assert 0 < count < added * 56 * 80, count
    # the same run into a file object, through a dataset built by the caller
    buf = io.BytesIO()
    assert pointcloud.run(config, model=model, dataset=ds, out=buf, dropout=0) == count
    assert np.array_equal(_ply_records(buf)[1].view(np.uint32), got.view(np.uint32))
    ds.close()


def test_real_shape_sample_goes_through_the_model(hip_lib, tmp_path):
    """configs/test/pointcloud_monorec_tmvo.json's shape: 1024x1280 grey images -> 480x640, frame_count 4, scale_factor 3."""
    tree = synth.make_tmvo_tree(tmp_path / "sequence_xx", height=1024, width=1280, images=6, dropped=(), seed=3)
    ds = tum_mono_vo.TUMMonoVODataset(tree, frame_count=4, scale_factor=3, target_image_size=(480, 640), color_augmentation=False, device=DEV)
    assert len(ds) == 2 and tuple(ds._crop_box) == (0, 32.0, 1280, 992.0)
    data, target = kitti.collate([ds[0]])
    assert tuple(data["keyframe"].shape) == (1, 3, 480, 640) and len(data["frames"]) == 4 and tuple(target.shape) == (1, 1, 480, 640)
    model = _seeded_model(32)
    with torch.no_grad():
        out = model(data)
    torch.cuda.synchronize()
    for key in ("result", "cv_mask"):
        assert tuple(out[key].shape) == (1, 1, 480, 640) and bool(torch.isfinite(out[key]).all()), key
    ds.close()
