#!/usr/bin/env python
"""Kernel times of the ray-cast of the block-sparse TSDF volume beside the dense route it replaces, on one MI355X (DESIGN.md section 7,
profiles/tsdf_sparse_render_rate.json):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/bench_tsdf_sparse_render.py --trace-schedule DIR/schedule.json
    python tools/bench_tsdf_sparse_render.py --kernel-trace DIR/.../t_kernel_trace.csv --trace-schedule DIR/schedule.json \
        --json profiles/tsdf_sparse_render_rate.json

The setup is that of tools/bench_tsdf_render.py: 512 x 512 x 128 voxels of 0.1 m, eight keyframes of a camera at the centre that looks
along x at a plane 20 m away, fused into a `SparseTSDFVolume`; the views are those keyframes' own cameras, 256 x 512, sampled every
0.1 m from 0 to 30 m.  Rows, all in one run: the dense route - `mr_tsdf_sparse_gather_f32` of the whole volume (`to_dense`),
`mr_tsdf_skip_grid_u8` on the result, `mr_tsdf_render_f32` with the bricks at 1 and 8 views per launch - and
`mr_tsdf_sparse_render_f32` at 1 and 8 views per launch.  The C entries are called directly with prepared arguments.  The first command
makes 3 warm-up and 10 traced launches per row under the profiler and writes their order; the second (no device needed) takes median
and range of End - Start of the kernels' dispatches from the trace.  A summary keeps the key `block_jump_variant` of an existing
--json file: the rows of a kernel variant that jumped over blocks without storage, measured once beside the others with this tool and
then removed because it was slower (DESIGN.md has the numbers)."""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH = 256, 512
DIMS, VOXEL = (512, 512, 128), 0.1
T_MIN, T_MAX = 0.0, 30.0
TRACE_WARMUP, TRACE_LAUNCHES = 3, 10
KERNELS = {"gather": "tsdf_sparse_gather_kernel", "skip_grid": "tsdf_skip_grid_kernel", "dense_render": "tsdf_render_kernel",
           "sparse_render": "tsdf_sparse_render_kernel"}


def cases():
    """Yields (row, launch): `launch()` enqueues ONE call of the row's C entry, nothing else.  row["ahead"]: the launches of the row's
    kernel the setup made since the last row of that kernel, which the summary skips."""
    import torch
    from monorec_amd import _lib, tsdf_fusion
    dev = "cuda:0"
    lib = _lib.load()
    pose = torch.tensor([[0.0, 0, 1, 25.6], [0, 1, 0, 25.6], [-1, 0, 0, 6.4], [0, 0, 0, 1]])      # at the centre, looking along x
    k = torch.tensor([[100.0, 0, 255.5], [0, 100.0, 127.5], [0, 0, 1]])
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (8, HEIGHT, WIDTH, 3), generator=gen, dtype=torch.uint8).to(dev)
    depth_cm = torch.full((8, HEIGHT, WIDTH), 2000, dtype=torch.int16, device=dev)
    poses = pose.repeat(8, 1, 1)
    poses[:, 1, 3] += 0.01 * torch.arange(8)
    sparse = tsdf_fusion.SparseTSDFVolume(origin=(0.0, 0.0, 0.0), dims=DIMS, voxel_size=VOXEL, colour=True, device=dev)
    sparse.integrate(depth_cm, images, poses, k)
    slots = sparse.allocated_blocks()
    dense = sparse.to_dense(sparse.bounds)
    bricks = dense.skip_grid(0)
    stream = torch.cuda.current_stream().cuda_stream
    made = collections.Counter({"gather": 1, "skip_grid": 1})                 # launches per kernel so far, setup included
    told = collections.Counter()                                              # ... of which the rows so far account for

    def row_of(kind, **row):
        ahead = made[kind] - told[kind]
        made[kind] += TRACE_WARMUP + TRACE_LAUNCHES
        told[kind] = made[kind]
        return dict(row, launch=kind, ahead=ahead)

    yield (row_of("gather", voxels=DIMS[0] * DIMS[1] * DIMS[2], allocated_blocks=slots, blocks=list(sparse.blocks)),
           lambda: _lib.check(lib.mr_tsdf_sparse_gather_f32(*sparse._table_args(), 0, 0, 0, *DIMS, *dense._volume_args()[:3], stream), "gather"))
    yield (row_of("skip_grid", brick=tsdf_fusion.BRICK, bricks_flagged=round(float(bricks.float().mean()), 4)),
           lambda: _lib.check(lib.mr_tsdf_skip_grid_u8(dense.tsdf.data_ptr(), dense.weight.data_ptr(), *DIMS, 0.0, bricks.data_ptr(), stream), "skip"))
    outputs = {}
    for name in ("dense", "sparse"):
        outputs[name] = (torch.empty(8, HEIGHT, WIDTH, dtype=torch.float32, device=dev), torch.empty(8, HEIGHT, WIDTH, 3, dtype=torch.float32, device=dev),
                         torch.empty(8, HEIGHT, WIDTH, 3, dtype=torch.uint8, device=dev))

    def views_of(name, count):
        views = []
        for i in range(count):
            view = _lib.TsdfRayView()
            view.m[:] = [float(v) for v in poses[i][:3, :4].reshape(-1)]
            view.fx, view.fy, view.cx, view.cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
            view.depth, view.normal, view.colour = (t[i].data_ptr() for t in outputs[name])
            views.append(view)
        return (_lib.TsdfRayView * count)(*views)

    march = (HEIGHT, WIDTH, T_MIN, T_MAX, VOXEL, stream)
    for count in (1, 8):
        def launch(array=views_of("dense", count), count=count):
            _lib.check(lib.mr_tsdf_render_f32(*dense._volume_args(), dense._origin, dense.voxel_size, 0.0, bricks.data_ptr(), array, count, *march), "render")
        yield row_of("dense_render", views_per_launch=count, bricks=True), launch
    for count in (1, 8):
        def launch(array=views_of("sparse", count), count=count):
            _lib.check(lib.mr_tsdf_sparse_render_f32(*sparse._table_args(), slots, sparse._origin, sparse.voxel_size, 0.0, array, count, *march),
                       "sparse render")
        row = row_of("sparse_render", views_per_launch=count)
        if count == 8:                                                         # the eight views of both routes: the same bits?
            launch()
            made["sparse_render"] += 1
            told["sparse_render"] += 1
            row["ahead"] += 1
            equal = all(bool(torch.equal(a, b)) for a, b in zip(outputs["dense"], outputs["sparse"]))
            row.update(equals_dense_render=equal, pixels_hit=round(float((outputs["sparse"][0] > 0).float().mean()), 4))
        yield row, launch


def trace_schedule(path):
    """The launches a kernel-trace run makes, in order; written to `path` for the summary."""
    import torch
    schedule = []
    for row, launch in cases():
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
    at, rows, per = collections.Counter(), [], schedule["warmup"] + schedule["launches"]
    for row in schedule["rows"]:
        name = row["launch"]
        at[name] += row.pop("ahead")
        mine = sorted(spans[name])[at[name]:at[name] + per]
        at[name] += per
        if len(mine) != per:
            raise SystemExit(f"the kernel trace holds too few {KERNELS[name]} dispatches for the schedule")
        us = [(e - b) / 1e3 for b, e in mine[schedule["warmup"]:]]
        row = dict(row, kernel_us_median=round(statistics.median(us), 1), kernel_us_min=round(min(us), 1), kernel_us_max=round(max(us), 1))
        if "views_per_launch" in row:
            row["kernel_us_per_view"] = round(row["kernel_us_median"] / row["views_per_launch"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if any(at[name] != len(spans[name]) for name in KERNELS):
        raise SystemExit(f"the kernel trace holds { {n: len(s) for n, s in spans.items()} } dispatches, the schedule accounts for {dict(at)}")
    by = {(r["launch"], r.get("views_per_launch")): r for r in rows}
    setup = by[("gather", None)]["kernel_us_median"] + by[("skip_grid", None)]["kernel_us_median"]
    return {"device": schedule.get("device"), "volume": list(DIMS), "voxel_size": VOXEL, "view": [HEIGHT, WIDTH], "t_range_m": [T_MIN, T_MAX], "step_m": VOXEL,
            "kernel_us": "rocprofv3 --kernel-trace, a run of its own: End - Start of the kernel's dispatches, 3 warm-up + 10 traced per row",
            "dense_route_us": {f"{n}_views": round(setup + by[("dense_render", n)]["kernel_us_median"], 1) for n in (1, 8)},
            "sparse_route_us": {f"{n}_views": by[("sparse_render", n)]["kernel_us_median"] for n in (1, 8)},
            "not_measured": ["a fused real scene", "a table of millions of blocks", "score() end to end"],
            "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-schedule", default=None, help="a path; alone: make the kernel-trace run's launches and write their schedule there")
    ap.add_argument("--kernel-trace", default=None, help="the *_kernel_trace.csv of that run: summarise it (no device needed)")
    a = ap.parse_args()
    if not a.trace_schedule:
        ap.error("--trace-schedule PATH is needed (alone under rocprofv3, or with --kernel-trace to summarise)")
    if not a.kernel_trace:
        trace_schedule(a.trace_schedule)
        return
    out = summarise(a.kernel_trace, a.trace_schedule)
    if a.json:
        if os.path.exists(a.json):
            with open(a.json) as f:
                kept = json.load(f).get("block_jump_variant")
            if kept is not None:
                out["block_jump_variant"] = kept
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
