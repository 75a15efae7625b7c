#!/usr/bin/env python
"""What the cross-view consistency filter costs on one MI355X:

    python tools/bench_depth_consistency.py [--json FILE]                       # the launch alone
    python tools/bench_depth_consistency.py --runner [--key on|off|both] [--root CHECKOUT] [--json FILE]

launch   `mr_depth_consistency_f32` at 256 x 512 with 4 and with 8 neighbours, `out` and `hits` both written, on a plane seen by cameras
         0.3 m apart (nearly every pixel goes all the way to a hit: the longest path through the kernel).  The `mr_consistency_view`
         array is prepared beforehand and the C entry is called directly, so no host work of `filter_depth` lies inside a timing.
         call_us: device events round N back-to-back launches, over N, after a warm-up; N is chosen from a first window so that a timed
         window lasts at least `--window-ms` (300); median and range of `--repeats` windows.  This is the kernel plus the gap to the next
         launch, not a kernel time from a trace.  Bytes per launch are a FORMULA, not a counter: the reference map read, every
         neighbour map read once, `out` and `hits` written; `fraction_of_hbm` is that over call_us against 6.29 TB/s - the maps of a
         loop like this one stay in the caches, so it says how far from a bandwidth problem the launch is, not what HBM delivered.
runner   keyframes/s of `tsdf_fusion.Fusion(...).fuse()` at c2 (B1 256 x 512 F2 D32, seeded weights, `fuse_batch` 4) over the resident
         keyframes of tools/bench_tsdf_fusion.py, without and with the config key `consistency`, without and with `use_mask`, the rows
         interleaved, `--repeats` timed runs of `--keyframes` each after a warm-up run of 24; host clock, ended by a device
         synchronise; keyframes counted are the ones fused (with the key or the vote: four fewer than the window).  `--root CHECKOUT`
         runs the same loop on the package of another checkout (a parent commit, which knows no key: `--key off`)."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

HBM_BYTES_PER_S = 6.29e12
HEIGHT, WIDTH = 256, 512
DEV = "cuda:0"


def launch_rows(repeats, window_ms):
    import torch
    from monorec_amd import _lib, consistency
    lib = _lib.load()
    k = torch.tensor([[300.0, 0, 255.5], [0, 300.0, 127.5], [0, 0, 1]])
    gen = torch.Generator().manual_seed(0)
    rows = []
    for num_views in (4, 8):
        offsets = [0.3 * s for s in (-2, -1, 1, 2, -4, -3, 3, 4)][:num_views]
        poses = []
        for dx in [0.0] + offsets:
            pose = torch.eye(4)
            pose[0, 3] = dx
            poses.append(pose)
        # a fronto-parallel plane 10 m ahead: every camera sees inverse depth 0.1 (a thousandth of noise, inside the tolerance)
        maps = [(0.1 * (1 + 1e-3 * (torch.rand(HEIGHT, WIDTH, generator=gen) - 0.5))).to(DEV) for _ in poses]
        (fx, fy, cx, cy), views = consistency.relative_views(poses[0], k, [(m, p, k) for m, p in zip(maps[1:], poses[1:])])
        out = torch.empty(HEIGHT, WIDTH, device=DEV)
        hits = torch.empty(HEIGHT, WIDTH, dtype=torch.uint8, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        args = (maps[0].data_ptr(), fx, fy, cx, cy, views, num_views, 0.01, 1.0, 2, 0, HEIGHT, WIDTH, out.data_ptr(), hits.data_ptr(), stream)

        def window(n):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            lib.mr_depth_consistency_f32(*args)                           # the device is busy when the first event is recorded
            start.record()
            for _ in range(n):
                lib.mr_depth_consistency_f32(*args)
            end.record()
            end.synchronize()
            return start.elapsed_time(end)                                # ms

        _lib.check(lib.mr_depth_consistency_f32(*args), "mr_depth_consistency_f32")
        window(200)                                                       # warm-up: code object, clocks
        first = window(2000)
        n = max(2000, int(2000 * window_ms / first) + 1)
        times = [window(n) for _ in range(repeats)]
        per_call = [t * 1e3 / n for t in times]
        histogram = torch.bincount(hits.reshape(-1).long(), minlength=num_views + 1).tolist()
        moved = HEIGHT * WIDTH * (4 + 4 * num_views + 4 + 1)
        median = statistics.median(per_call)
        row = {"neighbours": num_views, "launches_per_window": n, "window_ms_median": round(statistics.median(times), 1),
               "call_us_median": round(median, 2), "call_us_min": round(min(per_call), 2), "call_us_max": round(max(per_call), 2),
               "bytes_per_launch": moved, "fraction_of_hbm": round(moved / (median * 1e-6) / HBM_BYTES_PER_S, 3),
               "pixels_with_every_neighbour_a_hit": round(histogram[num_views] / (HEIGHT * WIDTH), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"frame": [HEIGHT, WIDTH], "hbm_tb_per_s": HBM_BYTES_PER_S / 1e12,
            "call_us": "device events round N back-to-back direct calls (views prepared beforehand), over N: kernel plus launch gap",
            "bytes": "formula: 4 bytes read per pixel of the reference and of every neighbour, 4 + 1 written; not a counter", "rows": rows}


def runner_rows(root, key, keyframes, repeats):
    import torch
    spec = importlib.util.spec_from_file_location("bench_tsdf_fusion", os.path.join(root, "tools", "bench_tsdf_fusion.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)                                        # puts `root` at the head of sys.path and imports its package
    from monorec_amd import MonoRecModel, synth, tsdf_fusion
    assert os.path.samefile(os.path.dirname(os.path.dirname(tsdf_fusion.__file__)), root), "the package of another checkout was imported"
    model = MonoRecModel(cv_depth_steps=32, hip_in_flight=4)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    base = {"min_d": 3, "max_d": 30, "fuse_batch": 4, "arch": {"type": "MonoRecModel"}, "data_set": {"type": "resident"}}
    datasets = {n: bench.ResidentDataset(n) for n in (24, keyframes)}

    def fuse(n, use_mask, with_key):
        config = dict(base, use_mask=use_mask, end=n)
        if with_key:
            config["consistency"] = True
        with tempfile.TemporaryDirectory() as tmp:
            fusion = tsdf_fusion.Fusion(dict(config, output_dir=tmp), model=model, dataset=datasets[n])
            torch.cuda.synchronize()
            t = time.perf_counter()
            fusion.fuse()
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t
            return int(fusion.volume.frames), seconds

    keys = {"off": [False], "on": [True], "both": [False, True]}[key]
    variants = [(use_mask, with_key) for use_mask in (False, True) for with_key in keys]
    for v in variants:
        fuse(24, *v)
    rates = {v: [] for v in variants}
    for _ in range(repeats):
        for v in variants:                                                # interleaved: drift hits every row alike
            done, seconds = fuse(keyframes, *v)
            rates[v].append(done / seconds)
    rows = []
    for (use_mask, with_key), values in rates.items():
        row = {"use_mask": use_mask, "consistency": with_key, "keyframes_per_s_median": round(statistics.median(values), 1),
               "keyframes_per_s_min": round(min(values), 1), "keyframes_per_s_max": round(max(values), 1), "runs": len(values)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"shape": "c2: B1 256x512 F2 D32", "keyframes": keyframes, "fuse_batch": 4, "hip_in_flight": 4, "package": root, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--runner", action="store_true")
    ap.add_argument("--key", choices=["on", "off", "both"], default="both")
    ap.add_argument("--keyframes", type=int, default=400)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_consistency: no device - a time is measured on the GPU or not at all")
    out = {"device": torch.cuda.get_device_name(0)}
    if a.runner:
        out["runner"] = runner_rows(root, a.key, a.keyframes, a.repeats)
    else:
        out["launch"] = launch_rows(a.repeats, a.window_ms)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
