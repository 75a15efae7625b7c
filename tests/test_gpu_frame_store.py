"""Pre-decoded frame store on the device: mr_unpack_frame_u8_f32 against the torch expression, mr_preprocess_image_u8_u8 against
Pillow, mr_scatter_sparse_f32 against numpy, and the identity the feature rests on - a dataset opened with `frame_store=` yields the
samples of the same dataset without it, bit for bit, without decoding an image (KITTI option matrix, TUM-MonoVO, pointcloud.run)."""
import io
import os

import numpy as np
import pytest
import torch

from monorec_amd import frame_store, input_pipeline, kitti, pointcloud, synth, tum_mono_vo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVERSE_RESPONSE = tum_mono_vo.invert_pcalib(255.0 * (np.arange(256) / 255.0) ** 0.6).numpy()      # synth.make_tmvo_tree's pcalib.txt
COMMON = dict(sequences=["03", "07"], depth_folder="image_depth_annotated", target_image_size=(64, 128))


# ------------------------------------------------------------------------------------------ kernels
def _record(h, w, channels, seed):
    """uint8 (channels, plane_stride): every byte value where the plane has room for it, 0xAB in the padding."""
    rng = np.random.RandomState(seed)
    n, stride = h * w, frame_store.plane_stride(h, w)
    rec = np.full((channels, stride), 0xAB, dtype=np.uint8)
    for c in range(channels):
        values = np.concatenate([rng.permutation(256), rng.randint(0, 256, size=max(n - 256, 0))])[:n]
        rec[c, :n] = rng.permutation(values).astype(np.uint8)
    return rec


@pytest.mark.parametrize("with_lut", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("h,w", [(5, 7), (16, 64), (33, 130)])          # under one wave: 2 chunks + 3 tail bytes; no tail; h*w % 16 == 2
def test_unpack_equals_the_torch_expression(hip_lib, h, w, channels, with_lut):
    rec = _record(h, w, channels, seed=h + channels)
    if h * w >= 256:
        assert all(np.unique(rec[c, :h * w]).size == 256 for c in range(channels))
    pre = input_pipeline.ImagePreprocessor((h, w), (h, w), device=DEV, lut=INVERSE_RESPONSE if with_lut else None)
    u = torch.from_numpy(rec[:, :h * w].reshape(channels, h, w).copy())
    if with_lut:
        want = torch.from_numpy(INVERSE_RESPONSE)[u.long()] / 255 - .5
    else:
        want = u.float() / 255 - .5
    want = want.expand(3, h, w) if channels == 1 else want
    got = pre.unpack(rec)                                               # host record: pinned ring, upload, launch
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, h, w)
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    # a device-resident record into a destination with guard floats on both sides: nothing outside (3, h, w) is written
    guard = torch.full((8 + 3 * h * w + 8,), float("nan"), device=DEV)
    out = guard[8:8 + 3 * h * w].view(3, h, w)
    pre.unpack(torch.from_numpy(rec).to(DEV), out=out)
    assert torch.equal(out.cpu(), want)
    assert bool(torch.isnan(guard[:8]).all()) and bool(torch.isnan(guard[-8:]).all())


RESIZE_CASES = {
    # name: (source h, w, channels, crop box or None, target h, w)
    "rgb_37x53_box": (37, 53, 3, (3, 2, 51, 34), 16, 24),
    "grey_40x56": (40, 56, 1, None, 20, 28),
}


@pytest.mark.parametrize("name", sorted(RESIZE_CASES))
def test_u8_resize_equals_pillow_and_unpacks_to_the_preprocessor_output(hip_lib, name):
    from PIL import Image
    h, w, c, box, oh, ow = RESIZE_CASES[name]
    img = synth.make_u8_image(h, w, c)
    pil = Image.fromarray(img)
    want = np.asarray((pil.crop(box) if box is not None else pil).resize((ow, oh), Image.BILINEAR))
    want = want.reshape(oh, ow, c).transpose(2, 0, 1)
    for lut in (None, INVERSE_RESPONSE):
        pre = input_pipeline.ImagePreprocessor((h, w), (oh, ow), crop_box=box, device=DEV, lut=lut)
        rec = pre.resize_u8(img)
        assert rec.dtype == torch.uint8 and tuple(rec.shape) == (c, pre.plane_stride) and pre.plane_stride % 16 == 0
        got = rec.cpu().numpy()
        assert np.array_equal(got[:, :oh * ow].reshape(c, oh, ow), want) and not got[:, oh * ow:].any()
        full = pre(img)
        assert torch.equal(pre.unpack(rec), full)                       # device record
        assert torch.equal(pre.unpack(got), full)                       # the bytes as the store hands them over


@pytest.mark.parametrize("n", [0, 1, 35])
def test_scatter_equals_numpy(hip_lib, n):
    cells = 35
    index = {0: np.zeros(0, np.uint32), 1: np.array([cells - 1], np.uint32), 35: np.arange(cells, dtype=np.uint32)}[n]
    value = (np.random.RandomState(n).rand(n).astype(np.float32) + 0.25)
    raw = np.frombuffer(index.tobytes() + value.tobytes(), dtype=np.uint8)
    got = input_pipeline.scatter_sparse(raw, n, cells, device=DEV)
    want = frame_store.decode_target(index, value, cells)
    assert got.dtype == torch.float32 and tuple(got.shape) == (cells,)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------ datasets
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return synth.make_kitti_tree(tmp_path_factory.mktemp("kitti"))


def _to_host(value):
    if torch.is_tensor(value):
        return value.cpu().clone()
    if isinstance(value, list):
        return [_to_host(v) for v in value]
    return value


def _samples(ds):
    return [(_to_host(dict(data)), _to_host(target)) for data, target in (ds[i] for i in range(len(ds)))]


def _same(a, b, what):
    assert torch.is_tensor(a) and torch.is_tensor(b), what
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), what


def _assert_same_samples(got, want, what):
    assert len(got) == len(want) > 0
    for i, ((data, target), (wdata, wtarget)) in enumerate(zip(got, want)):
        assert sorted(data) == sorted(wdata), (what, i)
        for key, value in wdata.items():
            if isinstance(value, list):
                assert len(data[key]) == len(value)
                for j, v in enumerate(value):
                    _same(data[key][j], v, (what, i, key, j))
            else:
                _same(data[key], value, (what, i, key))
        _same(target, wtarget, (what, i, "target"))


@pytest.mark.parametrize("case", sorted(synth.KITTI_OPTION_CASES))
def test_kitti_samples_from_the_store_are_bit_equal(hip_lib, tree, tmp_path, case):
    kw = dict(COMMON, **synth.KITTI_OPTION_CASES[case])
    plain = kitti.KittiOdometryDataset(tree, device=DEV, decode_workers=3, **kw)
    want = _samples(plain)
    frames, targets = plain._store_reach(range(len(plain)))
    assert frame_store.pack(plain, tmp_path / "store") == sum(map(len, frames.values())) + sum(map(len, targets.values()))
    plain.close()
    stored = kitti.KittiOdometryDataset(tree, device=DEV, decode_workers=3, frame_store=str(tmp_path / "store"), **kw)
    _assert_same_samples(_samples(stored), want, case)
    assert len(stored._caches) == (2 if kw.get("return_stereo") else 1) * 2          # two sequences
    for key, cache in stored._caches.items():
        assert cache.decoded == 0 and cache.unpacked == len(frames[key]) > 0, (key, cache.decoded, cache.unpacked)
        assert cache.pre._ring is not None and len(cache.pre._ring) == 4             # the one pinned ring of the camera
        reader = cache.store
        assert all(reader.has(j) == (j in frames[key]) for j in range(reader.count))  # everything else stays absent
    stored.close()


def test_kitti_partial_store_falls_back_to_the_decode(hip_lib, tree, tmp_path):
    kw = dict(COMMON, **synth.KITTI_OPTION_CASES["eval_config"])
    plain = kitti.KittiOdometryDataset(tree, device=DEV, decode_workers=2, **kw)
    want = _samples(plain)
    frame_store.pack(plain, tmp_path / "store", indices=[0, 1, len(plain) - 1])
    plain.close()
    stored = kitti.KittiOdometryDataset(tree, device=DEV, decode_workers=2, frame_store=str(tmp_path / "store"), **kw)
    _assert_same_samples(_samples(stored), want, "partial")
    first, last = stored._caches[(0, 2)], stored._caches[(1, 2)]
    assert first.unpacked == 4 and first.decoded > 0 and last.unpacked == 3 and last.decoded > 0
    assert len(first.pre._ring) == 4                                                 # decoded images and records share the ring
    stored.close()


def test_kitti_store_of_another_target_size_is_refused(hip_lib, tree, tmp_path):
    kw = dict(COMMON, **synth.KITTI_OPTION_CASES["eval_config"])
    plain = kitti.KittiOdometryDataset(tree, device=DEV, decode_workers=2, **kw)
    frame_store.pack(plain, tmp_path / "store", indices=[0])
    plain.close()
    other = kitti.KittiOdometryDataset(tree, device=DEV, frame_store=str(tmp_path / "store"), **dict(kw, target_image_size=(32, 64)))
    with pytest.raises(ValueError, match="target_image_size"):
        other[0]
    other.close()


@pytest.mark.parametrize("case", sorted(synth.TMVO_CASES))
def test_tum_samples_from_the_store_are_bit_equal(hip_lib, tmp_path, case):
    tree_kw, ds_kw = synth.TMVO_CASES[case]
    folder = synth.make_tmvo_tree(tmp_path / "sequence_xx", **tree_kw)
    plain = tum_mono_vo.TUMMonoVODataset(folder, color_augmentation=False, device=DEV, decode_workers=3, **ds_kw)
    want = _samples(plain)
    rows = plain._store_reach(range(len(plain)))[0][(0, 0)]
    assert frame_store.pack(plain, tmp_path / "store") == len(rows)
    plain.close()
    reader = frame_store.FrameStoreReader(frame_store.frames_path(tmp_path / "store", "sequence_xx", 0))
    assert reader.channels == tree_kw.get("channels", 1) and reader.count == len(plain._image_index)
    multi = tum_mono_vo.TUMMonoVOMultiDataset([folder], color_augmentation=False, device=DEV, decode_workers=3,
                                              frame_store=str(tmp_path / "store"), **ds_kw)
    _assert_same_samples(_samples(multi), want, case)                   # the response table is applied at unpack
    cache = multi.datasets[0].cache
    assert cache.decoded == 0 and cache.unpacked == len(rows) > 0
    multi.close()


def test_pointcloud_run_writes_the_same_bytes_from_the_store(hip_lib, tree, tmp_path):
    """pointcloud.run on sequence 03 of the small tree (120x400 -> 64x128, six samples, two keyframes reach the saver) with and without
    the store, the same seeded model, dropout 0."""
    from monorec_amd import MonoRecModel
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 128], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    config = {"name": "Pointcloud Creation", "n_gpu": 1, "roi": [4, 60, 8, 120], "start": 0, "end": -1, "min_d": 3, "max_d": 80,
              "use_mask": False, "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": 8}},
              "data_set": {"type": "KittiOdometryDataset", "args": args}}
    model = MonoRecModel(cv_depth_steps=8)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    plain = kitti.KittiOdometryDataset(device=DEV, **args)
    assert len(plain) == 6
    frame_store.pack(plain, tmp_path / "store")
    plain.close()
    a, b = io.BytesIO(), io.BytesIO()
    count = pointcloud.run(config, model=model, out=a, dropout=0)
    stored = kitti.KittiOdometryDataset(device=DEV, frame_store=str(tmp_path / "store"), **args)
    assert pointcloud.run(config, model=model, dataset=stored, out=b, dropout=0) == count > 0
    assert a.getvalue() == b.getvalue()
    assert all(c.decoded == 0 and c.unpacked > 0 for c in stored._caches.values())
    stored.close()
