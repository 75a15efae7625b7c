#!/usr/bin/env python
"""Rates of the TSDF fusion on one MI355X (profiles/tsdf_fusion_rate.json):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/bench_tsdf_fusion.py --trace-schedule DIR/schedule.json
    python tools/bench_tsdf_fusion.py --kernel-trace DIR/.../t_kernel_trace.csv --trace-schedule DIR/schedule.json --json profiles/tsdf_fusion_rate.json

integrate   `mr_tsdf_integrate_f32` alone: 256 x 512 frames into a 512 x 512 x 128 volume of 0.1 m voxels, 1 / 4 / 8 frames per launch.
            `inside`: the volume lies wholly inside every frustum and in front of every surface, so no tile is culled and every voxel
            is updated - a launch reads and writes the whole volume once.  `culled`: the camera stands in the middle of the volume
            and looks along x.  The `mr_tsdf_view` arrays are prepared beforehand and the C entry is called directly, so no host work
            of `TSDFVolume.integrate` (pose inverses, conversions) lies inside a timing.  Two figures per row, named for what they are:
              kernel_us  the KERNEL's time: median End - Start of its dispatches in a `rocprofv3 --kernel-trace` run of its own (first
                         command above; 3 warm-up and 10 traced launches per row).  The share of the HBM rate is taken over this.
              call_us    device events round 10 back-to-back direct launches, over 10 (profiler off): kernel plus launch gaps.
            Bytes per launch are a FORMULA, not a counter: voxels x (8 + 4 colour) read + the same written for `inside`; the images
            (0.66 MB per frame, served by the caches) are left out.  6.29 TB/s is the achievable HBM rate the fraction refers to.
loop        `tsdf_fusion.Fusion` (the stages of `tsdf_fusion.run`) at c2 (B1 256 x 512 F2 D32, seeded weights) over keyframes
            resident on the device (eight samples, the poses advancing 0.1 m per keyframe), next to `tsdf_export.run(export=False)`
            and the file-writing runner, interleaved, `--repeats` timed runs each after one warm-up run of 24 keyframes; host clock,
            every stage ended by a device synchronise; median and range of keyframes/s.  `seconds_last_run` holds the stages of the last
            run: setup, loop, extract (points to a file) and mesh (`TSDFVolume.mesh()`, on the device).
mesh        `--mesh-json FILE` alone (profiles/tsdf_mesh_rate.json): the 512 x 512 x 128 volume after eight keyframes of the `culled` camera
            with the wide intrinsics (a plane across the volume), `extract()` next to `mesh()`: host clock round the whole call, and
            device events round each launch (direct calls of the C entries), median of `--repeats` after a warm-up."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from monorec_amd import MonoRecModel, synth, tsdf_export, tsdf_fusion

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.29e12
HEIGHT, WIDTH = 256, 512


# ------------------------------------------------------------------------------------------ integrate alone
DIMS, VOXEL = (512, 512, 128), 0.1
TRACE_WARMUP, TRACE_LAUNCHES = 3, 10
KERNEL = "tsdf_integrate_kernel"


def integrate_cases():
    """Yields (row, volume, launch): `launch()` enqueues ONE mr_tsdf_integrate_f32 of the row's prepared views, nothing else."""
    inside_pose = torch.eye(4)
    inside_pose[:3, 3] = torch.tensor([25.6, 25.6, -25.0])                 # 25 m in front of the z = 0 face, looking along z
    culled_pose = torch.tensor([[0.0, 0, 1, 25.6], [0, 1, 0, 25.6], [-1, 0, 0, 6.4], [0, 0, 0, 1]])     # at the centre, looking along x
    cases = {"inside": (inside_pose, torch.tensor([[100.0, 0, 255.5], [0, 100.0, 127.5], [0, 0, 1]]), 6000),
             "culled": (culled_pose, torch.tensor([[300.0, 0, 255.5], [0, 300.0, 127.5], [0, 0, 1]]), 2000)}
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (8, HEIGHT, WIDTH, 3), generator=gen, dtype=torch.uint8).to(DEV)
    for colour in (True, False):
        volume = tsdf_fusion.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=DIMS, voxel_size=VOXEL, colour=colour, device=DEV)
        for case, (pose, k, depth_cm) in cases.items():
            if case == "culled" and not colour:
                continue
            depth = torch.full((8, HEIGHT, WIDTH), depth_cm, dtype=torch.int16, device=DEV)
            poses = pose.repeat(8, 1, 1)
            poses[:, 1, 3] += 0.01 * torch.arange(8)
            volume.reset()
            volume.integrate(depth[:1], images[:1] if colour else None, poses[:1], k)
            updated = float((volume.weight > 0).float().mean())
            for frames in (1, 4, 8):
                prepared = volume.prepare_views([(depth[i], images[i] if colour else None, poses[i], k) for i in range(frames)])
                row = {"case": case, "colour": colour, "frames_per_launch": frames, "voxels_updated_by_one_frame": round(updated, 4)}
                yield row, volume, (lambda v=volume, p=prepared: v.integrate_prepared(p))
        del volume


def trace_schedule(path):
    """The launches a kernel-trace run makes, in order; written to `path` for the summary."""
    schedule = []
    for row, volume, launch in integrate_cases():
        for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
            launch()
        torch.cuda.synchronize()
        schedule.append(row)
    with open(path, "w") as f:
        json.dump({"kernel": KERNEL, "warmup": TRACE_WARMUP, "launches": TRACE_LAUNCHES, "rows": schedule}, f, indent=1)


def kernel_times(trace_csv, schedule_json):
    """{row index: [kernel ns of the traced launches]} from a rocprofv3 kernel-trace csv and the schedule of that run."""
    import csv
    schedule = json.load(open(schedule_json))
    spans = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(trace_csv)) if schedule["kernel"] in r["Kernel_Name"]]
    spans.sort()
    out, at = {}, 0
    for i, row in enumerate(schedule["rows"]):
        if row["frames_per_launch"] == 1:
            at += 1                                   # integrate_cases() launches once per case to measure `voxels_updated_by_one_frame`
        durations = [e - b for b, e in spans[at:at + schedule["warmup"] + schedule["launches"]]]
        at += schedule["warmup"] + schedule["launches"]
        out[i] = durations[schedule["warmup"]:]
    if at != len(spans):
        raise SystemExit(f"kernel trace holds {len(spans)} {schedule['kernel']} dispatches, the schedule accounts for {at}")
    return schedule["rows"], out


def integrate_rows(trace_csv=None, schedule_json=None):
    rows = []
    traced = kernel_times(trace_csv, schedule_json) if trace_csv else None
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    for index, (row, volume, launch) in enumerate(integrate_cases()):
        for _ in range(3):
            launch()
        calls = []
        for _ in range(5):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            launch()                                                       # the device is busy when the first event is recorded
            start.record()
            for _ in range(10):
                launch()
            end.record()
            end.synchronize()
            calls.append(start.elapsed_time(end) * 1e3 / 10)
        frames = row["frames_per_launch"]
        row.update(call_us_median=round(statistics.median(calls), 1), call_us_min=round(min(calls), 1), call_us_max=round(max(calls), 1))
        if traced:
            assert traced[0][index] == {k: row[k] for k in traced[0][index]}, "the trace was taken with another schedule"
            kernel = [ns / 1e3 for ns in traced[1][index]]
            median = statistics.median(kernel)
            row.update(kernel_us_median=round(median, 1), kernel_us_min=round(min(kernel), 1), kernel_us_max=round(max(kernel), 1),
                       kernel_us_per_frame=round(median / frames, 1))
            if row["case"] == "inside":
                moved = 2 * voxels * (12 if row["colour"] else 8)
                row.update(bytes_per_launch=moved, bytes_per_frame=moved // frames, tb_per_s_over_kernel_time=round(moved / median / 1e6, 3),
                           fraction_of_hbm_over_kernel_time=round(moved / (median * 1e-6) / HBM_BYTES_PER_S, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"volume": list(DIMS), "voxel_size": VOXEL, "frame": [HEIGHT, WIDTH], "hbm_tb_per_s": HBM_BYTES_PER_S / 1e12,
            "kernel_us": "rocprofv3 --kernel-trace, a run of its own: End - Start of the kernel's dispatches, 3 warm-up + 10 traced per row" if traced else "not measured",
            "call_us": "device events round 10 back-to-back direct mr_tsdf_integrate_f32 calls (views prepared beforehand), over 10; 5 repeats",
            "bytes": "formula: voxels x (4 tsdf + 4 weight + 4 colour) read + the same written per launch; images not counted", "rows": rows}


# ------------------------------------------------------------------------------------------ the loop
class ResidentDataset:
    """`count` keyframes from eight c2 samples that stay on the device; the poses advance `step` metres along z per keyframe."""
    target_image_size = (HEIGHT, WIDTH)

    def __init__(self, count, step=0.1, samples=8):
        self.count, self.step = count, step
        self.samples = []
        for s in range(samples):
            b = synth.make_batch(1, HEIGHT, WIDTH, 2, seed=1 + s)
            self.samples.append({"keyframe": b["keyframe"][0].to(DEV), "frames": [f[0].to(DEV) for f in b["frames"]],
                                 "keyframe_pose": b["keyframe_pose"][0], "poses": [p[0] for p in b["poses"]],
                                 "keyframe_intrinsics": b["keyframe_intrinsics"][0], "intrinsics": [k[0] for k in b["intrinsics"]]})
        self.zero = torch.zeros(1, HEIGHT, WIDTH, device=DEV)

    def __len__(self):
        return self.count

    def _advance(self, index):
        g = torch.eye(4)
        g[2, 3] = self.step * index
        return g

    def keyframe_geometry(self, index):
        s = self.samples[index % len(self.samples)]
        return self._advance(index) @ s["keyframe_pose"], s["keyframe_intrinsics"]

    def __getitem__(self, index):
        if not 0 <= index < self.count:
            raise IndexError()
        s, g = self.samples[index % len(self.samples)], self._advance(index)
        data = dict(s, keyframe_pose=g @ s["keyframe_pose"], poses=[g @ p for p in s["poses"]],
                    sequence=torch.tensor([0], dtype=torch.int32, device=DEV), image_id=torch.tensor([index], dtype=torch.int32, device=DEV))
        return data, self.zero


def loop_rows(keyframes, repeats):
    model = MonoRecModel(cv_depth_steps=32, hip_in_flight=4)
    model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV).eval()
    base = {"use_mask": False, "min_d": 3, "max_d": 30, "arch": {"type": "MonoRecModel"}, "data_set": {"type": "resident"}}
    info, datasets = {}, {n: ResidentDataset(n) for n in (24, keyframes)}

    def export(n, write):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t = time.perf_counter()
            done = tsdf_export.run(dict(base, output_dir=tmp, end=n), model=model, dataset=datasets[n], export=write)
            torch.cuda.synchronize()
            return done, time.perf_counter() - t, {}

    def fuse(n, batch):
        with tempfile.TemporaryDirectory() as tmp:
            laps, clock = {}, time.perf_counter()

            def lap(name):
                nonlocal clock
                torch.cuda.synchronize()
                laps[name], clock = time.perf_counter() - clock, time.perf_counter()

            fusion = tsdf_fusion.Fusion(dict(base, output_dir=tmp, end=n, fuse_batch=batch), model=model, dataset=datasets[n])
            lap("setup")
            fusion.fuse()
            lap("loop")
            info["surface_points"] = fusion.write()
            lap("extract")
            info["mesh"] = [int(t.shape[0]) for t in fusion.volume.mesh()]
            lap("mesh")
            return n, laps["loop"], laps

    runners = {"export_skipped": lambda n: export(n, False), "export_files": lambda n: export(n, True),
               "fuse_batch_1": lambda n: fuse(n, 1), "fuse_batch_4": lambda n: fuse(n, 4), "fuse_batch_8": lambda n: fuse(n, 8)}
    for name, runner in runners.items():
        runner(24)                                                         # warm-up: plans, allocator, the pool's threads
    rates, extras = {name: [] for name in runners}, {}
    for _ in range(repeats):
        for name, runner in runners.items():                              # interleaved: drift hits every row alike
            done, seconds, timings = runner(keyframes)
            rates[name].append(done / seconds)
            if timings:
                extras[name] = {k: round(v, 4) for k, v in timings.items()}
    rows = []
    for name, values in rates.items():
        row = {"runner": name, "keyframes_per_s_median": round(statistics.median(values), 1), "keyframes_per_s_min": round(min(values), 1),
               "keyframes_per_s_max": round(max(values), 1), "runs": len(values)}
        if name in extras:
            row["seconds_last_run"] = extras[name]
        rows.append(row)
        print(json.dumps(row), flush=True)
    geometry = tsdf_fusion.bounds_from_frusta([datasets[keyframes].keyframe_geometry(i)[0] for i in range(keyframes)],
                                              datasets[keyframes].keyframe_geometry(0)[1], HEIGHT, WIDTH, 30, 0.1)
    return {"shape": "c2: B1 256x512 F2 D32", "keyframes": keyframes, "voxel_size": 0.1, "volume": list(tsdf_fusion.dims_of_bounds(geometry, 0.1)),
            "surface_points": info.get("surface_points"), "mesh_vertices_triangles": info.get("mesh"),
            "note": "fuse rows: keyframes / seconds of the loop alone (setup and extraction are in seconds_last_run); export rows: the whole run()",
            "rows": rows}


# ------------------------------------------------------------------------------------------ extract and mesh
def mesh_rows(repeats):
    from monorec_amd import _lib
    lib = _lib.load()
    volume = tsdf_fusion.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=DIMS, voxel_size=VOXEL, colour=True, device=DEV)
    pose = torch.tensor([[0.0, 0, 1, 25.6], [0, 1, 0, 25.6], [-1, 0, 0, 6.4], [0, 0, 0, 1]])      # at the centre, looking along x
    k = torch.tensor([[100.0, 0, 255.5], [0, 100.0, 127.5], [0, 0, 1]])
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (8, HEIGHT, WIDTH, 3), generator=gen, dtype=torch.uint8).to(DEV)
    depth = torch.full((8, HEIGHT, WIDTH), 2000, dtype=torch.int16, device=DEV)
    poses = pose.repeat(8, 1, 1)
    poses[:, 1, 3] += 0.01 * torch.arange(8)
    volume.integrate(depth, images, poses, k)
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    points, (n, m) = volume.count(), volume.mesh_counts()
    stream = torch.cuda.current_stream().cuda_stream
    cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
    records = torch.empty(max(points, n), 6, device=DEV)
    triangles = torch.empty(m, 3, dtype=torch.int32, device=DEV)
    base = torch.empty(voxels, dtype=torch.int32, device=DEV)
    common = (*volume._volume_args(), volume._origin, volume.voxel_size, 0.0)
    plain = (volume.tsdf.data_ptr(), volume.weight.data_ptr(), *DIMS, 0.0)
    launches = {
        "extract_count": lambda: lib.mr_tsdf_extract_f32(*common, None, 0, cursor.data_ptr(), stream),
        "extract_fill": lambda: lib.mr_tsdf_extract_f32(*common, records.data_ptr(), points, cursor.data_ptr(), stream),
        "mesh_vertices_count": lambda: lib.mr_tsdf_mesh_vertices_f32(*common, None, 0, None, cursor.data_ptr(), stream),
        "mesh_vertices_fill": lambda: lib.mr_tsdf_mesh_vertices_f32(*common, records.data_ptr(), n, base.data_ptr(), cursor.data_ptr(), stream),
        "mesh_triangles_count": lambda: lib.mr_tsdf_mesh_triangles_f32(*plain, None, None, 0, cursor.data_ptr(), stream),
        "mesh_triangles_fill": lambda: lib.mr_tsdf_mesh_triangles_f32(*plain, base.data_ptr(), triangles.data_ptr(), m, cursor.data_ptr(), stream),
    }
    tile = tsdf_fusion.TILE
    staged = {"mesh_vertices": (tile[0] + 1) * (tile[1] + 1) * (tile[2] + 1), "mesh_triangles": (tile[0] + 2) * (tile[1] + 2) * (tile[2] + 2)}
    rows = []
    for name, launch in launches.items():
        times = []
        for i in range(repeats + 1):                                       # the first is the warm-up
            cursor.zero_()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            _lib.check(launch(), name)
            end.record()
            end.synchronize()
            if i:
                times.append(start.elapsed_time(end) * 1e3)
        row = {"launch": name, "us_median": round(statistics.median(times), 1), "us_min": round(min(times), 1), "us_max": round(max(times), 1)}
        kind = name.rsplit("_", 1)[0]
        if kind in staged:                                                 # formula: tsdf + weight of the tile and its halo, once per workgroup
            row["bytes_read_per_voxel_formula"] = round(8 * staged[kind] / (tile[0] * tile[1] * tile[2]), 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    calls = {"extract": lambda: volume.extract(), "mesh": lambda: volume.mesh()}
    whole = {}
    for name, call in calls.items():
        times = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t) * 1e6)
        whole[name] = {"us_median": round(statistics.median(times), 1), "us_min": round(min(times), 1), "us_max": round(max(times), 1)}
        print(json.dumps({name: whole[name]}), flush=True)
    return {"volume": list(DIMS), "voxel_size": VOXEL, "surface_points": points, "mesh_vertices": n, "mesh_triangles": m,
            "volume_bytes": voxels * 12, "vertex_base_bytes": voxels * 4, "repeats": repeats,
            "launch_us": "device events round one direct call of the C entry, the stream idle before it", "launches": rows,
            "call_us": "host clock round the whole Python call (count launches, one read, allocation, fill launches), device synchronised",
            "calls": whole, "mesh_over_extract": round(whole["mesh"]["us_median"] / whole["extract"]["us_median"], 2),
            "bytes": "formula, not a counter: 8 bytes (tsdf, weight) per staged voxel; written vertex_base entries, colour reads and the records are not counted"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--keyframes", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--trace-schedule", default=None, help="a path; alone: make the kernel-trace run's launches and write their schedule there")
    ap.add_argument("--kernel-trace", default=None, help="the *_kernel_trace.csv of that run: kernel times go into the rows")
    ap.add_argument("--mesh-json", default=None, help="a path; alone: time extract() and mesh() on the 512 x 512 x 128 volume and write the figures there")
    a = ap.parse_args()
    if a.mesh_json:
        out = {"device": torch.cuda.get_device_name(0), "mesh": mesh_rows(max(a.repeats, 5))}
        with open(a.mesh_json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    if a.trace_schedule and not a.kernel_trace:
        trace_schedule(a.trace_schedule)
        return
    out = {"device": torch.cuda.get_device_name(0), "integrate": integrate_rows(a.kernel_trace, a.trace_schedule)}
    if not a.skip_loop:
        out["loop"] = loop_rows(a.keyframes, a.repeats)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
