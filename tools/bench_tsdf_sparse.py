#!/usr/bin/env python
"""Kernel times and memory of the block-sparse TSDF volume beside the dense one on one MI355X (DESIGN.md section 7,
profiles/tsdf_sparse_rate.json):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/bench_tsdf_sparse.py --trace-schedule DIR/schedule.json
    python tools/bench_tsdf_sparse.py --kernel-trace DIR/.../t_kernel_trace.csv --trace-schedule DIR/schedule.json --json profiles/tsdf_sparse_rate.json

The setup is the `culled` one of tools/bench_tsdf_fusion.py: 512 x 512 x 128 voxels of 0.1 m, the camera in the middle of the volume
looking along x at a plane 20 m away, 256 x 512 frames.  Rows: `mr_tsdf_integrate_f32` and `mr_tsdf_sparse_integrate_f32` at 1, 4 and 8
frames per launch, into volumes that hold those frames already (the sparse launches find their blocks allocated: the steady state of
a fusion), and the count and fill launches of `mr_tsdf_extract_f32` and `mr_tsdf_sparse_extract_f32` after eight keyframes.  Both
volumes are measured in the same run.  The first command makes 3 warm-up and 10 traced launches per row under the profiler and writes
their order; the second (no device needed) takes median and range of End - Start of the kernels' dispatches from the trace.
Memory is not measured but derived: the table is 4 bytes per block, the pool in use `allocated_blocks` x 512 x 12 bytes."""
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
TRACE_WARMUP, TRACE_LAUNCHES = 3, 10
KERNELS = {"dense_integrate": "tsdf_integrate_kernel", "sparse_integrate": "tsdf_sparse_integrate_kernel",
           "dense_extract": "tsdf_mesh_vertices_kernel", "sparse_extract": "tsdf_sparse_extract_kernel"}


def cases():
    """Yields (row, launch): `launch()` enqueues ONE call of the row's C entry, nothing else.  row["ahead"]: the launches of the row's
    kernel the setup made since the last row of that kernel, which the summary skips."""
    import torch
    from monorec_amd import _lib, tsdf_fusion
    dev = "cuda:0"
    lib = _lib.load()
    pose = torch.tensor([[0.0, 0, 1, 25.6], [0, 1, 0, 25.6], [-1, 0, 0, 6.4], [0, 0, 0, 1]])      # at the centre, looking along x
    k = torch.tensor([[300.0, 0, 255.5], [0, 300.0, 127.5], [0, 0, 1]])
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (8, HEIGHT, WIDTH, 3), generator=gen, dtype=torch.uint8).to(dev)
    depth = torch.full((8, HEIGHT, WIDTH), 2000, dtype=torch.int16, device=dev)
    poses = pose.repeat(8, 1, 1)
    poses[:, 1, 3] += 0.01 * torch.arange(8)
    dense = tsdf_fusion.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=DIMS, voxel_size=VOXEL, colour=True, device=dev)
    sparse = tsdf_fusion.SparseTSDFVolume(origin=(0.0, 0.0, 0.0), dims=DIMS, voxel_size=VOXEL, colour=True, device=dev)
    volumes = {"dense": dense, "sparse": sparse}
    made = collections.Counter()                                              # launches per kernel so far, setup included
    told = collections.Counter()                                              # ... of which the rows so far account for

    def row_of(kind, **row):
        ahead = made[kind] - told[kind]
        told[kind] = made[kind] + TRACE_WARMUP + TRACE_LAUNCHES
        made[kind] += TRACE_WARMUP + TRACE_LAUNCHES
        return dict(row, launch=kind, ahead=ahead)

    for name, volume in volumes.items():                                      # the eight keyframes, one launch: what the rows start from
        volume.integrate(depth, images, poses, k)
        made[f"{name}_integrate"] += 1
    allocated = sparse.allocated_blocks()
    memory = {"blocks": list(sparse.blocks), "allocated_blocks": allocated, "overflowed": sparse.overflowed(),
              "sparse_bytes_in_use": sparse.bytes_in_use(), "sparse_table_bytes": 4 * sparse.table.numel(),
              "sparse_pool_bytes_in_use": allocated * 512 * 12, "dense_bytes": tsdf_fusion.volume_bytes(DIMS),
              "voxels_seen_dense": float((dense.weight > 0).float().mean())}
    for name, volume in volumes.items():
        for frames in (1, 4, 8):
            prepared = volume.prepare_views([(depth[i], images[i], poses[i], k) for i in range(frames)])
            yield (row_of(f"{name}_integrate", frames_per_launch=frames, **(memory if name == "sparse" and frames == 1 else {})),
                   lambda v=volume, p=prepared: v.integrate_prepared(p))
    stream = torch.cuda.current_stream().cuda_stream
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    for name, volume in volumes.items():
        count = volume.count()
        made[f"{name}_extract"] += 1
        records = torch.empty(count, 6, dtype=torch.float32, device=dev)
        for fill in (False, True):
            out = (records.data_ptr(), count) if fill else (None, 0)
            if name == "dense":
                def launch(v=volume, out=out):
                    cursor.zero_()
                    _lib.check(lib.mr_tsdf_extract_f32(*v._volume_args(), v._origin, v.voxel_size, 0.0, *out, cursor.data_ptr(), stream), "extract")
            else:
                def launch(v=volume, out=out, used=allocated):
                    cursor.zero_()
                    _lib.check(lib.mr_tsdf_sparse_extract_f32(*v._table_args(), v.block_of_slot.data_ptr(), used, v._origin, v.voxel_size, 0.0, *out,
                                                              cursor.data_ptr(), stream), "sparse extract")
            yield row_of(f"{name}_extract", fill=fill, points=count), launch


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
        if "frames_per_launch" in row:
            row["kernel_us_per_frame"] = round(row["kernel_us_median"] / row["frames_per_launch"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if any(at[name] != len(spans[name]) for name in KERNELS):
        raise SystemExit(f"the kernel trace holds { {n: len(s) for n, s in spans.items()} } dispatches, the schedule accounts for {dict(at)}")
    by = {(r["launch"], r.get("frames_per_launch", r.get("fill"))): r["kernel_us_median"] for r in rows}
    ratios = {f"sparse_over_dense_integrate_{n}_frames": round(by[("sparse_integrate", n)] / by[("dense_integrate", n)], 3) for n in (1, 4, 8)}
    ratios.update({f"sparse_over_dense_extract_{'fill' if fill else 'count'}": round(by[("sparse_extract", fill)] / by[("dense_extract", fill)], 3)
                   for fill in (False, True)})
    return dict({"device": schedule.get("device"), "volume": list(DIMS), "voxel_size": VOXEL, "frame": [HEIGHT, WIDTH],
                 "kernel_us": "rocprofv3 --kernel-trace, a run of its own: End - Start of the kernel's dispatches, 3 warm-up + 10 traced per row",
                 "memory": "derived, not measured: 4 bytes per block of table, allocated_blocks x 512 x 12 bytes of pool in use"}, **ratios, rows=rows)


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
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
