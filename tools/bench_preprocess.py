"""Times the per-frame image preprocessing (csrc/preprocess.hip) at a user's sizes, on the GPU:

  * the launch alone (device-resident source, device events over many launches): mr_preprocess_image_u8_f32 and
    mr_preprocess_image_u8_lut_f32, and the two launches of the pre-decoded frame store (monorec_amd.frame_store) beside them, to be
    compared with the f32 resize launch of the same session: mr_preprocess_image_u8_u8 (the packer's resize) and
    mr_unpack_frame_u8_f32 (stored bytes -> frame, with and without the table);
  * a frame end to end on the device path: decoded uint8 image on the host -> pinned staging -> upload -> launch (host clock, synchronised);
  * a stored frame end to end: record on the host -> pinned staging -> upload -> unpack launch (host clock, synchronised);
  * the reference-style host path for the same frame: Pillow convert / crop / resize, response table, /255 - .5, CHW on the CPU, then
    the upload of the float32 result (host clock, synchronised) - what a TUM-MonoVO sample cost per frame before the device path.

`--compare-lib PATH`: another build of the library (e.g. the parent commit's) whose mr_preprocess_image_u8_f32 is timed
alternately with this tree's on the same inputs, outputs compared bit for bit.

    python tools/bench_preprocess.py [--compare-lib other/libmonorec_hip.so] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monorec_amd import _lib, input_pipeline, synth, tum_mono_vo  # noqa: E402

DEV = "cuda:0"
SHAPES = {"tum_1024x1280_to_480x640_grey": (1024, 1280, 1, 480, 640), "kitti_370x1226_to_256x512_rgb": (370, 1226, 3, 256, 512),
          "kitti_370x1226_to_256x512_grey": (370, 1226, 1, 256, 512)}


def event_ms(fn, launches, repeats=5):
    """Median over `repeats` windows of the device time per call of `fn` (`launches` calls per window)."""
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / launches)
    return float(np.median(times)), float(min(times)), float(max(times))


def host_ms(fn, calls, repeats=5):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(times)), float(min(times)), float(max(times))


def raw_launch(lib, pre, image, channels, out, with_lut=False):
    """The C-ABI call itself (no Python around it but ctypes), so that the windows below are not bound by the host."""
    name = "mr_preprocess_image_u8_lut_f32" if with_lut else "mr_preprocess_image_u8_f32"
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.ABI[name]
    args = (image.data_ptr(), pre.orig_h, pre.orig_w, channels, pre.orig_w * channels, pre._box_c, pre.out_h, pre.out_w, pre.hb.data_ptr(),
            pre.hk.data_ptr(), pre.hks, pre.vb.data_ptr(), pre.vk.data_ptr(), pre.vks, pre.max_rows) + ((pre.lut.data_ptr(),) if with_lut else ())
    stream = torch.cuda.current_stream().cuda_stream
    return lambda: fn(*args, out.data_ptr(), stream)


def raw_store_launches(lib, pre, image, channels, out):
    """The frame store's launches as raw C-ABI calls: (u8 resize of `image` into a record, unpack of that record, unpack with the table)."""
    record = torch.zeros(channels, pre.plane_stride, dtype=torch.uint8, device=image.device)
    stream = torch.cuda.current_stream().cuda_stream
    resize_args = (image.data_ptr(), pre.orig_h, pre.orig_w, channels, pre.orig_w * channels, pre._box_c, pre.out_h, pre.out_w, pre.hb.data_ptr(),
                   pre.hk.data_ptr(), pre.hks, pre.vb.data_ptr(), pre.vk.data_ptr(), pre.vks, pre.max_rows, record.data_ptr(), pre.plane_stride, stream)
    unpack_args = lambda lut: (record.data_ptr(), channels, pre.plane_stride, pre.out_h, pre.out_w, lut, out.data_ptr(), stream)
    plain_args, lut_args = unpack_args(None), unpack_args(pre.lut.data_ptr())
    return (record, lambda: lib.mr_preprocess_image_u8_u8(*resize_args), lambda: lib.mr_unpack_frame_u8_f32(*plain_args),
            lambda: lib.mr_unpack_frame_u8_f32(*lut_args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare-lib", default=None)
    ap.add_argument("--launches", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from PIL import Image
    other = ctypes.CDLL(a.compare_lib) if a.compare_lib else None
    table = tum_mono_vo.invert_pcalib(255.0 * (np.arange(256) / 255.0) ** 0.6)
    res = {"device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "shapes": {}}
    for name, (h, w, c, oh, ow) in SHAPES.items():
        img = synth.make_u8_image(h, w, c, seed=17)
        _, box = input_pipeline.compute_target_intrinsics(np.identity(4), (h, w), (oh, ow))
        plain = input_pipeline.ImagePreprocessor((h, w), (oh, ow), crop_box=box, device=DEV)
        lut = input_pipeline.ImagePreprocessor((h, w), (oh, ow), crop_box=box, device=DEV, lut=table)
        dev_img = torch.from_numpy(img).to(DEV)
        out = torch.empty(3, oh, ow, device=DEV)
        row = {}
        this = raw_launch(plain.lib, plain, dev_img, c, out)
        this_lut = raw_launch(lut.lib, lut, dev_img, c, out, with_lut=True)
        for _ in range(50):
            this(), this_lut()
        torch.cuda.synchronize()
        if other is not None:
            out_other = torch.empty_like(out)
            that = raw_launch(other, plain, dev_img, c, out_other)
            for _ in range(50):
                that()
            torch.cuda.synchronize()
            this()
            row["bit_equal_to_compare_lib"] = bool(torch.equal(out, out_other))
            # alternating windows: A B A B ...
            ta, tb = [], []
            for _ in range(5):
                ta.append(event_ms(this, a.launches, 1)[0])
                tb.append(event_ms(that, a.launches, 1)[0])
            row["launch_us_this_tree"] = [round(1e3 * float(np.median(ta)), 3), round(1e3 * min(ta), 3), round(1e3 * max(ta), 3)]
            row["launch_us_compare_lib"] = [round(1e3 * float(np.median(tb)), 3), round(1e3 * min(tb), 3), round(1e3 * max(tb), 3)]
        else:
            row["launch_us_this_tree"] = [round(1e3 * v, 3) for v in event_ms(this, a.launches)]
        row["launch_us_lut_entry"] = [round(1e3 * v, 3) for v in event_ms(this_lut, a.launches)]
        # the frame store's launches on the same image: the record the packer writes, and its way back
        record, resize_u8, unpack, unpack_lut = raw_store_launches(lut.lib, lut, dev_img, c, out)
        for _ in range(50):
            resize_u8(), unpack(), unpack_lut()
        this()
        want = out.clone()
        resize_u8(), unpack()
        torch.cuda.synchronize()
        row["unpack_bit_equal_to_f32_resize"] = bool(torch.equal(out, want))
        row["launch_us_u8_resize"] = [round(1e3 * v, 3) for v in event_ms(resize_u8, a.launches)]
        row["launch_us_unpack"] = [round(1e3 * v, 3) for v in event_ms(unpack, a.launches)]
        row["launch_us_unpack_lut"] = [round(1e3 * v, 3) for v in event_ms(unpack_lut, a.launches)]
        row["record_bytes"] = int(record.numel())
        host_record = record.cpu().numpy()
        row["frame_ms_store_path_lut"] = [round(v, 4) for v in host_ms(lambda: lut.unpack(host_record, out=out), 200)]
        # a frame end to end, device path (host image -> pinned ring -> upload -> launch) against the host path
        row["frame_ms_device_path_lut"] = [round(v, 4) for v in host_ms(lambda: lut(img, out=out), 200)]
        pil = Image.fromarray(img)
        lut_cpu = table.clone()

        def host_path():
            t = torch.tensor(np.array(pil.convert("RGB").crop(box).resize((ow, oh), resample=Image.BILINEAR))).to(dtype=torch.float32)
            t = lut_cpu[t.to(dtype=torch.long)]
            return (t / 255 - .5).permute(2, 0, 1).to(DEV)
        assert torch.equal(host_path(), lut(img))
        row["frame_ms_host_path_lut"] = [round(v, 4) for v in host_ms(host_path, 50)]
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
