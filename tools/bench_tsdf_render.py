#!/usr/bin/env python
"""Kernel times of the TSDF ray-cast on one MI355X (profiles/tsdf_render_rate.json):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/bench_tsdf_render.py --trace-schedule DIR/schedule.json
    python tools/bench_tsdf_render.py --kernel-trace DIR/.../t_kernel_trace.csv --trace-schedule DIR/schedule.json --json profiles/tsdf_render_rate.json

The volume is the 512 x 512 x 128 one of tools/bench_tsdf_fusion.py's mesh rows: eight keyframes of a camera at the centre that looks
along x at a plane 20 m away.  The views are those keyframes' own cameras, 256 x 512, sampled every voxel (0.1 m) from 0 to 30 m.
Rows: the skip-grid launch; one view and eight views per launch, each with the bricks and with `bricks` NULL.  The C entries are
called directly with prepared arguments.  The first command makes 3 warm-up and 10 traced launches per row under the profiler and
writes their order; the second (no device needed) takes median and range of End - Start of the kernel's dispatches from the trace.
A second pair of commands with `MR_HIP_LIBRARY=<a build with -DMR_TSDF_BRICK=8> ... --brick 8` measures the other brick edge.
Bytes are a FORMULA, not a counter: the skip grid reads 8 bytes per voxel once; a render's gathers are served by the caches and are
not counted - only its outputs (19 bytes per pixel) are given."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
HEIGHT, WIDTH = 256, 512
DIMS, VOXEL = (512, 512, 128), 0.1
T_MIN, T_MAX = 0.0, 30.0
TRACE_WARMUP, TRACE_LAUNCHES = 3, 10
KERNELS = {"skip_grid": "tsdf_skip_grid_kernel", "render": "tsdf_render_kernel"}
INTEGRATE_US_PER_FURTHER_FRAME = 129          # profiles/tsdf_fusion_rate.json, with colour: beside the result for scale, not a bar


def cases(brick=None):
    """Yields (row, launch): `launch()` enqueues ONE call of the row's C entry, nothing else.  `brick`: the edge the library named by
    MR_HIP_LIBRARY was built with (-DMR_TSDF_BRICK=8), when it is not the header's."""
    import torch
    from monorec_amd import _lib, tsdf_fusion
    if brick:
        tsdf_fusion.BRICK = int(brick)
    dev = "cuda:0"
    lib = _lib.load()
    volume = tsdf_fusion.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=DIMS, voxel_size=VOXEL, colour=True, device=dev)
    pose = torch.tensor([[0.0, 0, 1, 25.6], [0, 1, 0, 25.6], [-1, 0, 0, 6.4], [0, 0, 0, 1]])      # at the centre, looking along x
    k = torch.tensor([[100.0, 0, 255.5], [0, 100.0, 127.5], [0, 0, 1]])
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (8, HEIGHT, WIDTH, 3), generator=gen, dtype=torch.uint8).to(dev)
    depth_cm = torch.full((8, HEIGHT, WIDTH), 2000, dtype=torch.int16, device=dev)
    poses = pose.repeat(8, 1, 1)
    poses[:, 1, 3] += 0.01 * torch.arange(8)
    volume.integrate(depth_cm, images, poses, k)
    stream = torch.cuda.current_stream().cuda_stream
    bricks = volume.skip_grid(0)
    flagged = float(bricks.float().mean())
    yield ({"launch": "skip_grid", "brick": tsdf_fusion.BRICK, "brick_count": int(bricks.numel()), "bricks_flagged": round(flagged, 4)},
           lambda: _lib.check(lib.mr_tsdf_skip_grid_u8(volume.tsdf.data_ptr(), volume.weight.data_ptr(), *DIMS, 0.0, bricks.data_ptr(), stream), "skip"))
    depth = torch.empty(8, HEIGHT, WIDTH, dtype=torch.float32, device=dev)
    normal = torch.empty(8, HEIGHT, WIDTH, 3, dtype=torch.float32, device=dev)
    colour = torch.empty(8, HEIGHT, WIDTH, 3, dtype=torch.uint8, device=dev)
    views = []
    for i in range(8):
        view = _lib.TsdfRayView()
        view.m[:] = [float(v) for v in poses[i][:3, :4].reshape(-1)]
        view.fx, view.fy, view.cx, view.cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
        view.depth, view.normal, view.colour = depth[i].data_ptr(), normal[i].data_ptr(), colour[i].data_ptr()
        views.append(view)
    hit = None
    for count in (1, 8):
        array = (_lib.TsdfRayView * count)(*views[:count])
        for skip in (True, False):
            def launch(array=array, count=count, skip=skip):
                _lib.check(lib.mr_tsdf_render_f32(*volume._volume_args(), volume._origin, volume.voxel_size, 0.0, bricks.data_ptr() if skip else None,
                                                  array, count, HEIGHT, WIDTH, T_MIN, T_MAX, VOXEL, stream), "render")
            if hit is None:
                launch()
                hit = round(float((depth[0] > 0).float().mean()), 4)
            yield {"launch": "render", "views_per_launch": count, "bricks": skip, "pixels_hit_view_0": hit}, launch


def trace_schedule(path, brick=None):
    """The launches a kernel-trace run makes, in order; written to `path` for the summary."""
    import torch
    schedule = []
    for row, launch in cases(brick):
        for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
            launch()
        torch.cuda.synchronize()
        schedule.append(row)
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "warmup": TRACE_WARMUP, "launches": TRACE_LAUNCHES, "rows": schedule}, f, indent=1)


def summarise(trace_csv, schedule_json):
    import csv
    schedule = json.load(open(schedule_json))
    spans = {name: [] for name in KERNELS}
    for r in csv.DictReader(open(trace_csv)):
        for name, kernel in KERNELS.items():
            if kernel in r["Kernel_Name"]:
                spans[name].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    at = {"skip_grid": 1, "render": 1}            # cases() builds the grid once and renders once (pixels_hit_view_0) ahead of the rows
    rows, per = [], schedule["warmup"] + schedule["launches"]
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    for row in schedule["rows"]:
        name = row["launch"]
        mine = sorted(spans[name])[at[name]:at[name] + per]
        at[name] += per
        if len(mine) != per:
            raise SystemExit(f"the kernel trace holds too few {KERNELS[name]} dispatches for the schedule")
        us = [(e - b) / 1e3 for b, e in mine[schedule["warmup"]:]]
        median = statistics.median(us)
        row = dict(row, kernel_us_median=round(median, 1), kernel_us_min=round(min(us), 1), kernel_us_max=round(max(us), 1))
        if name == "skip_grid":
            row.update(bytes_read_formula=voxels * 8, fraction_of_hbm_over_kernel_time=round(voxels * 8 / (median * 1e-6) / HBM_BYTES_PER_S, 3))
        else:
            views = row["views_per_launch"]
            row.update(kernel_us_per_view=round(median / views, 1), mrays_per_s=round(views * HEIGHT * WIDTH / median, 1),
                       bytes_written_formula=views * HEIGHT * WIDTH * 19)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if any(at[name] != len(spans[name]) for name in KERNELS):
        raise SystemExit(f"the kernel trace holds { {n: len(s) for n, s in spans.items()} } dispatches, the schedule accounts for {at}")
    by = {(r.get("views_per_launch"), r.get("bricks")): r["kernel_us_median"] for r in rows if r["launch"] == "render"}
    return {"device": schedule.get("device"), "volume": list(DIMS), "voxel_size": VOXEL, "view": [HEIGHT, WIDTH], "t_range_m": [T_MIN, T_MAX], "step_m": VOXEL,
            "hbm_tb_per_s": HBM_BYTES_PER_S / 1e12,
            "kernel_us": "rocprofv3 --kernel-trace, a run of its own: End - Start of the kernel's dispatches, 3 warm-up + 10 traced per row",
            "bytes": "formula, not a counter: the skip grid reads tsdf and weight (8 bytes per voxel) once; a render's gathers are not counted, "
                     "its outputs are 19 bytes per pixel (depth 4, normal 12, colour 3)",
            "skip_over_no_skip_8_views": round(by[(8, True)] / by[(8, False)], 3),
            "integrate_us_per_further_frame_for_scale": INTEGRATE_US_PER_FURTHER_FRAME, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-schedule", default=None, help="a path; alone: make the kernel-trace run's launches and write their schedule there")
    ap.add_argument("--kernel-trace", default=None, help="the *_kernel_trace.csv of that run: summarise it (no device needed)")
    ap.add_argument("--brick", type=int, default=None, help="with --trace-schedule alone: MR_HIP_LIBRARY names a build with this -DMR_TSDF_BRICK")
    a = ap.parse_args()
    if not a.trace_schedule:
        ap.error("--trace-schedule PATH is needed (alone under rocprofv3, or with --kernel-trace to summarise)")
    if not a.kernel_trace:
        trace_schedule(a.trace_schedule, a.brick)
        return
    out = summarise(a.kernel_trace, a.trace_schedule)
    if a.json:
        merged = {}
        if os.path.exists(a.json):                                         # one key per brick edge: a second summary joins the first
            with open(a.json) as f:
                merged = json.load(f)
        merged[f"brick_{out['rows'][0]['brick']}"] = out
        with open(a.json, "w") as f:
            json.dump(dict(sorted(merged.items())), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
