"""TUM-MonoVO samples assembled on the MI355X: the sample dict of the reference's `TUMMonoVODataset` /
`TUMMonoVOMultiDataset` (data_loader/tum_mono_vo_dataset.py:14-254) with every per-pixel step on the device.

    from monorec_amd.tum_mono_vo import TUMMonoVODataset
    dataset = TUMMonoVODataset("data/tummonovo/sequence_50_rect", frame_count=4, scale_factor=3, color_augmentation=False)
    data, target = dataset[0]                    # configs/test/pointcloud_monorec_tmvo.json:25-37

Same constructor keywords, `len()`, `__getitem__` -> `(data, keyframe_depth)` and the same keys / shapes / dtypes as the
reference.  A sequence folder holds

    images/NNNNN.jpg   rectified grey images          result.txt   DSO poses, one row `time tx ty tz qx qy qz qw` per tracked frame
    times.txt          `id time [exposure]` per image  camera.txt   relative intrinsics fx fy cx cy, optionally after a model name
    pcalib.txt         256 values of the photometric response

  * everything read from the text files (image index, poses, crop box, intrinsics, inverse response table) is formed once on
    the host, in the reference's float64 expressions; the quaternion -> matrix step is written out (scipy is not a dependency);
  * images: decode on host threads ahead of the sweep (`input_pipeline.FrameCache`), then ONE device launch per *new* image
    (crop, Pillow-exact bilinear resize, inverse response table, /255 - .5, CHW).  The reference decodes, resizes and maps
    every image 1 + frame_count times; here consecutive samples share the preprocessed frames in HBM;
  * `frame_store=DIR` (monorec_amd.frame_store): the resized 8-bit frames come from a packed store instead of the image files - no
    decode, one unpack launch that applies the response table, the same bits.

Not provided (raise NotImplementedError): colour augmentation (training), `only_keyframes` and EXR depth maps (both need
`images_depth/*.exr`, read through OpenCV; "WIP" in the reference).  There is no CPU fallback: the first `__getitem__` needs a
HIP device."""
import os

import numpy as np
import torch

from . import input_pipeline


def invert_pcalib(pcalib):
    """tum_mono_vo_dataset.py:247-254: for every 8-bit value the first index of the response whose value reaches it."""
    inv = np.zeros(256, dtype=np.float32)
    j = 0
    for i in range(256):
        while j < 255 and i + .5 > pcalib[j]:
            j += 1
        inv[i] = j
    return torch.from_numpy(inv)


def build_image_index(result_times, image_times, eps=1e-5):
    """tum_mono_vo_dataset.py:153-162: row of times.txt (= image file number) of every row of result.txt."""
    index = np.zeros(len(result_times), dtype=np.int64)
    current = 0
    for i, timestamp in enumerate(result_times):
        while not timestamp <= image_times[current] + eps:
            current += 1
        index[i] = current
    return index


def load_orig_intrinsics(camera_file):
    """tum_mono_vo_dataset.py:176-189: relative (f_x, f_y, c_x, c_y) of the first line of camera.txt, which starts either with
    the numbers or with the name of the camera model."""
    with open(camera_file) as f:
        fields = f.readline().split()
    if not "0" <= fields[0][0] <= "9":
        fields = fields[1:]
    p_cam = np.identity(4, dtype=np.float64)
    p_cam[0, 0], p_cam[1, 1], p_cam[0, 2], p_cam[1, 2] = (float(v) for v in fields[:4])
    return p_cam


def quaternions_to_matrices(q):
    """(N, 4) quaternions x, y, z, w (scalar last, any norm) -> (N, 3, 3) float64 rotations: what
    `scipy.spatial.transform.Rotation.from_quat(q).as_matrix()` computes (tum_mono_vo_dataset.py:232)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    q = q / np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.empty((q.shape[0], 3, 3), dtype=np.float64)
    m[:, 0, 0] = x2 - y2 - z2 + w2
    m[:, 1, 0] = 2 * (xy + zw)
    m[:, 2, 0] = 2 * (xz - yw)
    m[:, 0, 1] = 2 * (xy - zw)
    m[:, 1, 1] = -x2 + y2 - z2 + w2
    m[:, 2, 1] = 2 * (yz + xw)
    m[:, 0, 2] = 2 * (xz + yw)
    m[:, 1, 2] = 2 * (yz - xw)
    m[:, 2, 2] = -x2 - y2 + z2 + w2
    return m


class TUMMonoVODataset:
    """Drop-in for `data_loader.tum_mono_vo_dataset.TUMMonoVODataset` with device-resident samples."""

    def __init__(self, dataset_dir, frame_count=2, target_image_size=(480, 640), max_length=None, dilation=1, only_keyframes=False,
                 color_augmentation=True, scale_factor=1, device="cuda:0", decode_workers=8, cache_frames=None, frame_store=None):
        if color_augmentation:
            raise NotImplementedError("monorec_amd.tum_mono_vo: colour augmentation is a training feature - pass "
                                      "color_augmentation=False, as configs/test/pointcloud_monorec_tmvo.json does")
        if only_keyframes:
            raise NotImplementedError("monorec_amd.tum_mono_vo: only_keyframes needs the EXR depth maps of images_depth/ (OpenCV)")
        self.dataset_dir = str(dataset_dir)
        depth_dir = os.path.join(self.dataset_dir, "images_depth")
        if os.path.isdir(depth_dir) and any(n.endswith(".exr") for n in os.listdir(depth_dir)):
            raise NotImplementedError("monorec_amd.tum_mono_vo: EXR depth maps (images_depth/) need OpenCV and are not supported")
        self.frame_count, self.only_keyframes, self.dilation = frame_count, only_keyframes, dilation
        self.target_image_size = tuple(target_image_size)
        self.color_augmentation, self.scale_factor = color_augmentation, scale_factor
        self._device = torch.device(device)         # private: the scripts dump the public attributes as JSON

        # ---- the text files (:60-73)
        path = lambda *names: os.path.join(self.dataset_dir, *names)
        self._result = np.loadtxt(path("result.txt"), ndmin=2)
        self._times = np.loadtxt(path("times.txt"), ndmin=2)
        self._pcalib = invert_pcalib(np.loadtxt(path("pcalib.txt")).reshape(-1))
        self._image_index = build_image_index(self._result[:, 0], self._times[:, 1])
        self.length = self._result.shape[0] - frame_count * dilation
        if max_length is not None:
            self.length = min(self.length, max_length)
        self._offset = (frame_count // 2) * dilation

        # ---- geometry of the cropped / resized images (:191-226, :257-265): relative intrinsics times the image size, then the rule
        # KITTI uses
        from PIL import Image
        with Image.open(path("images", "00000.jpg")) as img:
            self._orig_size = (img.size[1], img.size[0])
            self._channels = 1 if img.mode == "L" else 3
        p_cam = load_orig_intrinsics(path("camera.txt"))
        p_cam[0, 0] *= self._orig_size[1]
        p_cam[1, 1] *= self._orig_size[0]
        p_cam[0, 2] *= self._orig_size[1]
        p_cam[1, 2] *= self._orig_size[0]
        fractions, self._crop_box = input_pipeline.compute_target_intrinsics(p_cam, self._orig_size, self.target_image_size)
        self._intrinsics = input_pipeline.format_intrinsics(fractions, self.target_image_size)

        # ---- poses (:228-235): float64 rotation and t * scale_factor, one rounding to float32
        poses = torch.eye(4).unsqueeze(0).repeat(self._result.shape[0], 1, 1)
        poses[:, :3, :3] = torch.tensor(quaternions_to_matrices(self._result[:, 4:8]))
        poses[:, :3, 3] = torch.tensor(self._result[:, 1:4]) * scale_factor
        self._poses = poses.to(torch.float32)

        # ---- device side, created on first use so that the bookkeeping above works without a GPU
        self._decode_workers = int(decode_workers)
        self._cache_frames = int(cache_frames) if cache_frames is not None else 2 * ((frame_count + 1) * dilation + 1)
        self._frames = None              # FrameCache, keyed by the row of result.txt
        self._depth = None               # the constant (1, H, W) zero target (:79,129-130)
        # pre-decoded store (monorec_amd.frame_store): a directory, kept as a plain string (the scripts dump the public attributes); the
        # file of this sequence is opened on first use and checked against the geometry above.  It holds the bytes BEFORE the response
        # table, which is applied at unpack.
        self.frame_store = None if frame_store is None else str(frame_store)
        self._store_key = os.path.basename(os.path.normpath(self.dataset_dir))

    def __len__(self):
        return self.length

    def _source_rows(self, index):
        """Rows of result.txt of the source frames (:134-136): index, index + dilation, ... without the keyframe's - the TUM
        class's own order, not KITTI's symmetric one."""
        return [index + i for i in range(0, (self.frame_count + 1) * self.dilation, self.dilation) if i != self._offset]

    # ------------------------------------------------------------------ pre-decoded store (monorec_amd.frame_store)
    def _frame_header(self, stream=0, cam=0):
        from . import frame_store
        return frame_store.frame_header("TUMMonoVODataset", self._store_key, 0, self._orig_size, self._crop_box, self.target_image_size,
                                        self._channels, len(self._image_index))

    def _store_reach(self, indices):
        """What the samples `indices` read: ({(0, 0): rows of result.txt}, {}) - the target is the constant zero map."""
        rows = set()
        for i in indices:
            if not 0 <= i < self.length:
                raise IndexError()
            rows.update([i + self._offset] + self._source_rows(i))
        return {(0, 0): rows}, {}

    def _cache(self, stream=0, cam=0):
        return self.cache

    # ------------------------------------------------------------------ device side
    @property
    def cache(self):
        if self._frames is None:
            from PIL import Image
            store = None
            if self.frame_store is not None:
                from . import frame_store
                store = frame_store.open_frames(self.frame_store, self._frame_header())
            folder, image_index = os.path.join(self.dataset_dir, "images"), self._image_index

            def load(row):
                with Image.open(os.path.join(folder, f"{image_index[row]:05d}.jpg")) as img:
                    # a grey image goes through the resize once (one channel, three equal output planes): `convert('RGB')` before a
                    # per-channel resize (:85-89) gives the same bytes
                    return np.asarray(img if img.mode == "L" else img.convert("RGB"))
            pre = input_pipeline.ImagePreprocessor(self._orig_size, self.target_image_size, crop_box=self._crop_box,
                                                   device=self._device, lut=self._pcalib)
            self._frames = input_pipeline.FrameCache(load, pre, capacity=self._cache_frames, workers=self._decode_workers,
                                                     index_range=(0, len(image_index)), store=store)
            self._depth = torch.zeros((1, *self.target_image_size), dtype=torch.float32, device=self._device)
        return self._frames

    def __getitem__(self, index):
        if not 0 <= index < self.length:
            raise IndexError()
        key = index + self._offset
        sources = self._source_rows(index)
        cache = self.cache
        # the 4x4 pose / intrinsics matrices stay on the HOST, like kitti.KittiOdometryDataset's: MonoRecModel forms its projection
        # matrices with the reference's CPU operators (model.host_geometry)
        data = {
            "keyframe": cache.frame(key),
            "keyframe_pose": self._poses[key],
            "keyframe_intrinsics": self._intrinsics,
            "frames": [cache.frame(j) for j in sources],
            "poses": [self._poses[j] for j in sources],
            "intrinsics": [self._intrinsics for _ in range(self.frame_count)],
            "sequence": torch.tensor([0], device=self._device),                    # int64, as the reference's (:145-146)
            "image_id": torch.tensor([int(key)], device=self._device),
        }
        return data, self._depth

    def keyframe_geometry(self, index):
        """(keyframe_pose, keyframe_intrinsics) of sample `index` as `__getitem__` hands them out, without decoding a frame."""
        if not 0 <= index < self.length:
            raise IndexError()
        return self._poses[index + self._offset], self._intrinsics

    def close(self):
        if self._frames is not None:
            self._frames.close()
            self._frames = None


class TUMMonoVOMultiDataset:
    """`data_loader.tum_mono_vo_dataset.TUMMonoVOMultiDataset` (:14-35): several sequence folders one after the other."""

    def __init__(self, dataset_dirs, **kwargs):
        if not isinstance(dataset_dirs, (list, tuple)):
            dataset_dirs = [dataset_dirs]
        self.datasets = [TUMMonoVODataset(d, **kwargs) for d in dataset_dirs]

    @property
    def target_image_size(self):
        return self.datasets[0].target_image_size

    def __len__(self):
        return sum(len(d) for d in self.datasets)

    def __getitem__(self, index):
        for dataset in self.datasets:
            if index < len(dataset):
                return dataset[index]
            index -= len(dataset)
        raise IndexError()

    def keyframe_geometry(self, index):
        for dataset in self.datasets:
            if index < len(dataset):
                return dataset.keyframe_geometry(index)
            index -= len(dataset)
        raise IndexError()

    def close(self):
        for dataset in self.datasets:
            dataset.close()
