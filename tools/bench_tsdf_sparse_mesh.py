#!/usr/bin/env python
"""Kernel times of the mesh of the block-sparse TSDF volume beside the dense route it replaces, on one MI355X (DESIGN.md section 7,
profiles/tsdf_sparse_mesh_rate.json):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/bench_tsdf_sparse_mesh.py --trace-schedule DIR/schedule.json
    python tools/bench_tsdf_sparse_mesh.py --kernel-trace DIR/.../t_kernel_trace.csv --trace-schedule DIR/schedule.json \
        --json profiles/tsdf_sparse_mesh_rate.json

The setup is that of tools/bench_tsdf_sparse_render.py: 512 x 512 x 128 voxels of 0.1 m, eight keyframes of a camera at the centre that
looks along x at a plane 20 m away, fused into a `SparseTSDFVolume`.  Rows, all in one run: the dense route - `mr_tsdf_sparse_gather_f32`
of the whole volume (`to_dense`), then the count and the fill launch of `mr_tsdf_mesh_vertices_f32` and of `mr_tsdf_mesh_triangles_f32`
on the result - and the native route: the count and the fill launch of `mr_tsdf_sparse_mesh_vertices_f32` and of
`mr_tsdf_sparse_mesh_triangles_f32` on the blocks themselves.  The C entries are called directly with prepared arguments, the cursor
zeroed ahead of every launch.  The first command makes 3 warm-up and 10 traced launches per row under the profiler and writes their
order; the second (no device needed) takes median and range of End - Start of the kernels' dispatches from the trace.  The memory
figures of the summary are derived, not measured: 4 bytes of `vertex_base` per pool voxel of the allocated blocks against 12 bytes of
gathered copy plus 4 of `vertex_base` per voxel of the grid."""
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
KERNELS = {"gather": "tsdf_sparse_gather_kernel", "dense_vertices": "tsdf_mesh_vertices_kernel", "dense_triangles": "tsdf_mesh_triangles_kernel",
           "sparse_vertices": "tsdf_sparse_extract_kernel", "sparse_triangles": "tsdf_sparse_mesh_triangles_kernel"}
BIG_TEST_VOLUME = dict(dims=(4096, 4096, 512), allocated_blocks=30)          # tests/test_gpu_tsdf_sparse_mesh.py


def memory(dims, allocated_blocks):
    """Derived bytes of workspace: the native mesh's vertex_base per pool voxel; the dense route's gathered copy plus vertex_base."""
    voxels = dims[0] * dims[1] * dims[2]
    return {"native_vertex_base_bytes": allocated_blocks * 512 * 4, "dense_gathered_copy_bytes": voxels * 12, "dense_vertex_base_bytes": voxels * 4}


def cases():
    """Yields (row, launch): `launch()` enqueues ONE call of the row's C entry behind a clear of the cursor, nothing else of these
    kernels.  row["ahead"]: the launches of the row's kernel the setup made since the last row of that kernel, which the summary skips."""
    import numpy as np
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
    (n, m), native = dense.mesh_counts(), sparse.mesh_counts()
    stream = torch.cuda.current_stream().cuda_stream
    made = collections.Counter({name: 1 for name in KERNELS})                 # launches per kernel so far: to_dense and the two mesh_counts
    told = collections.Counter()                                              # ... of which the rows so far account for
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    out = {name: (torch.empty(n, 6, dtype=torch.float32, device=dev), torch.empty(m, 3, dtype=torch.int32, device=dev)) for name in ("dense", "sparse")}
    base = {"dense": torch.empty(DIMS[0] * DIMS[1] * DIMS[2], dtype=torch.int32, device=dev),
            "sparse": torch.empty(slots * 512, dtype=torch.int32, device=dev)}

    def row_of(kind, **row):
        ahead = made[kind] - told[kind]
        made[kind] += TRACE_WARMUP + TRACE_LAUNCHES
        told[kind] = made[kind]
        return dict(row, launch=kind, ahead=ahead)

    def checked(call, what):
        def launch():
            cursor.zero_()
            _lib.check(call(), what)
        return launch

    yield (row_of("gather", voxels=DIMS[0] * DIMS[1] * DIMS[2], allocated_blocks=slots, blocks=list(sparse.blocks)),
           checked(lambda: lib.mr_tsdf_sparse_gather_f32(*sparse._table_args(), 0, 0, 0, *DIMS, *dense._volume_args()[:3], stream), "gather"))
    common = (*dense._volume_args(), dense._origin, dense.voxel_size, 0.0)
    plain = (dense.tsdf.data_ptr(), dense.weight.data_ptr(), *DIMS, 0.0)
    vertices, triangles = out["dense"]
    yield (row_of("dense_vertices", mode="count"),
           checked(lambda: lib.mr_tsdf_mesh_vertices_f32(*common, None, 0, None, cursor.data_ptr(), stream), "dense vertices"))
    yield (row_of("dense_vertices", mode="fill", vertices=n),
           checked(lambda: lib.mr_tsdf_mesh_vertices_f32(*common, vertices.data_ptr(), n, base["dense"].data_ptr(), cursor.data_ptr(), stream), "dense vertices"))
    yield (row_of("dense_triangles", mode="count"),
           checked(lambda: lib.mr_tsdf_mesh_triangles_f32(*plain, None, None, 0, cursor.data_ptr(), stream), "dense triangles"))
    yield (row_of("dense_triangles", mode="fill", triangles=m),
           checked(lambda: lib.mr_tsdf_mesh_triangles_f32(*plain, base["dense"].data_ptr(), triangles.data_ptr(), m, cursor.data_ptr(), stream), "dense triangles"))
    table, pool_slots = sparse._table_args(), sparse.block_of_slot.data_ptr()
    shared = (*table, pool_slots, slots, sparse._origin, sparse.voxel_size, 0.0)
    bare = (*table[:6], pool_slots, slots, 0.0)
    s_vertices, s_triangles = out["sparse"]
    yield (row_of("sparse_vertices", mode="count"),
           checked(lambda: lib.mr_tsdf_sparse_mesh_vertices_f32(*shared, None, 0, None, cursor.data_ptr(), stream), "sparse vertices"))
    yield (row_of("sparse_vertices", mode="fill", vertices=native[0]),
           checked(lambda: lib.mr_tsdf_sparse_mesh_vertices_f32(*shared, s_vertices.data_ptr(), n, base["sparse"].data_ptr(), cursor.data_ptr(), stream),
                   "sparse vertices"))
    yield (row_of("sparse_triangles", mode="count"),
           checked(lambda: lib.mr_tsdf_sparse_mesh_triangles_f32(*bare, None, None, 0, cursor.data_ptr(), stream), "sparse triangles"))
    row = row_of("sparse_triangles", mode="fill", triangles=native[1])
    yield (row, checked(lambda: lib.mr_tsdf_sparse_mesh_triangles_f32(*bare, base["sparse"].data_ptr(), s_triangles.data_ptr(), m, cursor.data_ptr(), stream),
                        "sparse triangles"))
    # behind the last row's launches both routes' arrays are filled: the same mesh?  Every triangle as its three vertex records, rotated
    # to the rotation that sorts first, the triangles sorted (tests/tsdf_mesh_ref.py: canonical).
    def canonical(vertices, triangles):
        recs = vertices.cpu().numpy()[triangles.cpu().numpy().astype(np.int64)]
        count = len(recs)
        rotations = np.stack([np.roll(recs, -r, axis=1).reshape(count, 18) for r in range(3)], axis=1).reshape(3 * count, 18)
        order = np.lexsort(tuple(rotations[:, c] for c in range(17, -1, -1)) + (np.repeat(np.arange(count), 3),))
        best = rotations[order[::3]]
        return best[np.lexsort(tuple(best[:, c] for c in range(17, -1, -1)))]
    torch.cuda.synchronize()
    row.update(equals_dense_mesh=bool(native == (n, m) and np.array_equal(canonical(*out["dense"]), canonical(*out["sparse"]))))


def trace_schedule(path):
    """The launches a kernel-trace run makes, in order; written to `path` for the summary."""
    import torch
    schedule = []
    runs = cases()
    for row, launch in runs:
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
        rows.append(row)
        print(json.dumps(row), flush=True)
    if any(at[name] != len(spans[name]) for name in KERNELS):
        raise SystemExit(f"the kernel trace holds { {n: len(s) for n, s in spans.items()} } dispatches, the schedule accounts for {dict(at)}")
    by = {(r["launch"], r.get("mode")): r for r in rows}
    four = [(kind, mode) for kind in ("vertices", "triangles") for mode in ("count", "fill")]

    def route(prefix, key):
        return round(sum(by[(f"{prefix}_{kind}", mode)][key] for kind, mode in four), 1)
    gather = by[("gather", None)]
    allocated = gather["allocated_blocks"]
    return {"device": schedule.get("device"), "volume": list(DIMS), "voxel_size": VOXEL,
            "kernel_us": "rocprofv3 --kernel-trace, a run of its own: End - Start of the kernel's dispatches, 3 warm-up + 10 traced per row",
            "native_route_us": {"median": route("sparse", "kernel_us_median"), "sum_of_min": route("sparse", "kernel_us_min"),
                                "sum_of_max": route("sparse", "kernel_us_max")},
            "dense_route_us": {"median": round(gather["kernel_us_median"] + route("dense", "kernel_us_median"), 1),
                               "sum_of_min": round(gather["kernel_us_min"] + route("dense", "kernel_us_min"), 1),
                               "sum_of_max": round(gather["kernel_us_max"] + route("dense", "kernel_us_max"), 1)},
            "memory_derived": {"this_scene": memory(DIMS, allocated), "test_volume_4096x4096x512": memory(**BIG_TEST_VOLUME)},
            "not_measured": ["a fused real scene", "a table of millions of blocks", "mesh() end to end with its allocations and reads"],
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
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
