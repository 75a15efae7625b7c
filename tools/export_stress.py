#!/usr/bin/env python
"""CPU-only stress of the writer side of the TSDF-fusion export (monorec_amd.tsdf_export.TSDFExporter) - the counterpart of
tools/store_stress.py on the output side:

    python tools/export_stress.py [--frames 64] [--workers 1,2,4,8,16] [--levels none,1,3] [--json profiles/tsdf_export_stress.json]

No device is touched: 256 x 512 frames that are on the host already go through `add_packed` - the ring, the pool of encoder threads,
Pillow, the file system (a temporary directory) - exactly as a frame does once its copy has landed.  Two kinds of depth map:

    scene   what a depth map looks like: a smooth ground plane and background with a few objects at their own depth (hard edges)
            and half a centimetre of noise, some pixels dropped to zero
    noise   incompressible 15-bit noise: the encoder's worst case

and the PNG compression levels None (Pillow's default, what the reference writes), 1 and 3; the colour image is one textured frame
throughout.  Reported per (kind, level): the time of one PNG and one JPEG encode on one thread, the PNG's size, and frames/s of the
whole pool for each worker count (at most 16, and never more than the CPUs this process may use)."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH = 256, 512


def scene_depth(seed):
    """Centimetres, int16: ground plane + far background + boxes at their own depth, +-0.5 cm noise, 3 % of the pixels dropped."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH].astype(np.float32)
    horizon = HEIGHT * 0.45
    ground = 160.0 * HEIGHT / np.maximum(yy - horizon, 1.0)                      # cm, 1 / (row below the horizon)
    depth = np.where(yy > horizon + 4, np.minimum(ground, 3000.0), 2500.0 + 2.0 * xx)
    for _ in range(6):
        cy, cx = rng.randint(HEIGHT // 3, HEIGHT - 20), rng.randint(20, WIDTH - 60)
        hh, ww = rng.randint(15, 60), rng.randint(20, 90)
        depth[cy - hh:cy, cx:cx + ww] = rng.randint(400, 2500)
    depth = depth + rng.uniform(-0.5, 0.5, depth.shape)
    depth[rng.rand(HEIGHT, WIDTH) < 0.03] = 0
    return depth.astype(np.int16)


def noise_depth(seed):
    return np.random.RandomState(seed).randint(0, 32768, size=(HEIGHT, WIDTH)).astype(np.int16)


def one_encode_ms(depth, colour, level, repeats=5):
    from PIL import Image
    png_ms, jpg_ms, size = [], [], 0
    for _ in range(repeats):
        buf = io.BytesIO()
        t = time.perf_counter()
        img = Image.fromarray(depth.view(np.uint16))
        img.save(buf, format="PNG") if level is None else img.save(buf, format="PNG", compress_level=level)
        png_ms.append((time.perf_counter() - t) * 1e3)
        size = buf.tell()
        buf = io.BytesIO()
        t = time.perf_counter()
        Image.fromarray(colour).save(buf, format="JPEG")
        jpg_ms.append((time.perf_counter() - t) * 1e3)
    return min(png_ms), min(jpg_ms), size


def pool_rate(frames, colour, level, workers, count):
    import torch
    from monorec_amd import tsdf_export
    pose = torch.eye(4)
    with tempfile.TemporaryDirectory() as tmp:
        ex = tsdf_export.TSDFExporter(tmp, HEIGHT, WIDTH, ring=max(8, 2 * workers), workers=workers, png_compress_level=level, pin=False)
        t = time.perf_counter()
        for i in range(count):
            ex.add_packed(i, frames[i % len(frames)], colour, pose)
        ex.close()
        dt = time.perf_counter() - t
        assert ex.written == count
    return count / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames per measurement")
    ap.add_argument("--workers", default="1,2,4,8,16")
    ap.add_argument("--levels", default="none,1,3")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import PIL
    import torch
    from monorec_amd import synth
    torch.set_num_threads(1)
    cpus = len(os.sched_getaffinity(0))
    workers = sorted({min(int(w), 16, max(cpus, 1)) for w in a.workers.split(",")})
    levels = [None if v == "none" else int(v) for v in a.levels.split(",")]
    colour = synth.make_u8_image(HEIGHT, WIDTH, 3, seed=21)
    kinds = {"scene": [scene_depth(s) for s in range(8)], "noise": [noise_depth(s) for s in range(8)]}
    out = {"host_cpus": cpus, "pillow": PIL.__version__, "frame": [HEIGHT, WIDTH], "frames_per_measurement": a.frames, "pool": "threads", "rows": []}
    for kind, frames in kinds.items():
        for level in levels:
            png_ms, jpg_ms, size = one_encode_ms(frames[0], colour, level)
            row = {"kind": kind, "png_compress_level": level, "png_ms_one_thread": round(png_ms, 3), "jpeg_ms_one_thread": round(jpg_ms, 3),
                   "png_bytes": size, "frames_per_s": {}}
            for w in workers:
                row["frames_per_s"][str(w)] = round(pool_rate(frames, colour, level, w, a.frames), 1)
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
