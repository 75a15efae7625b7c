#!/usr/bin/env python
"""Counts, bytes and device time of the TSDF mesh per level of detail, on one MI355X (DESIGN.md section 7,
profiles/tsdf_mesh_lod_rate.json):

    python tools/bench_tsdf_mesh_lod.py --json profiles/tsdf_mesh_lod_rate.json

The volume is that of tools/bench_tsdf_sparse_mesh.py: 512 x 512 x 128 voxels of 0.1 m, eight keyframes of a camera at the centre that
looks along x at a plane 20 m away, fused into a `SparseTSDFVolume`; the dense rows run on `to_dense` of it.  For both volume classes,
`cell` 1 (the full mesh: the entries and arguments of `mesh()` as it was before it took `cell`), 2, 4 and 8, with and without normals, a
row has the vertex and triangle counts, the bytes `mesh()` returns - what crosses to the host when it is saved: 24 per vertex, 12 per
triangle, 12 per normal - and the device time of one call's four launches (count and fill of the vertex and of the triangle entry,
`_Volume._mesh_launches`) between two device events, outputs and workspace allocated ahead.  `--warmup` rounds, then `--rounds` timed
ones; a round visits every row once, so the rows share whatever else the machine does.  The spread of the cell 1 row (min .. max over
the rounds) is the margin a clustered row is held against."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH = 256, 512
DIMS, VOXEL = (512, 512, 128), 0.1


def fused(dims=DIMS):
    import torch
    from monorec_amd import tsdf_fusion
    dev = "cuda:0"
    pose = torch.tensor([[0.0, 0, 1, dims[0] * VOXEL / 2], [0, 1, 0, dims[1] * VOXEL / 2], [-1, 0, 0, dims[2] * VOXEL / 2], [0, 0, 0, 1]])
    k = torch.tensor([[100.0, 0, 255.5], [0, 100.0, 127.5], [0, 0, 1]])
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (8, HEIGHT, WIDTH, 3), generator=gen, dtype=torch.uint8).to(dev)
    depth_cm = torch.full((8, HEIGHT, WIDTH), 2000, dtype=torch.int16, device=dev)
    poses = pose.repeat(8, 1, 1)
    poses[:, 1, 3] += 0.01 * torch.arange(8)
    sparse = tsdf_fusion.SparseTSDFVolume(origin=(0.0, 0.0, 0.0), dims=dims, voxel_size=VOXEL, colour=True, device=dev)
    sparse.integrate(depth_cm, images, poses, k)
    return sparse, sparse.to_dense(sparse.bounds)


def rows_of(volumes):
    """[(row, call)]: `call()` enqueues the four launches of one `mesh(cell=..., normals=...)` into buffers made here."""
    import torch
    rows = []
    for name, volume in volumes:
        for normals in (False, True):
            for cell in (1, 2, 4, 8):
                n, m = volume.mesh_counts(0, cell)
                vertices = torch.empty(n, 6, dtype=torch.float32, device=volume.device)
                triangles = torch.empty(m, 3, dtype=torch.int32, device=volume.device)
                base = torch.empty(volume._mesh_voxels() if cell == 1 else volume._mesh_clusters(cell), dtype=torch.int32, device=volume.device)
                cursor = torch.zeros(2, dtype=torch.int64, device=volume.device)
                more = {} if cell == 1 else {"cell": cell}
                fill = dict(more, normals=torch.empty(n, 3, dtype=torch.float32, device=volume.device)) if normals else more

                def call(volume=volume, cursor=cursor, vertices=vertices, triangles=triangles, base=base, more=more, fill=fill):
                    cursor.zero_()
                    volume._mesh_launches(0.0, cursor, **more)
                    cursor.zero_()
                    volume._mesh_launches(0.0, cursor, vertices, triangles, base, **fill)
                row = dict(volume=name, cell=cell, normals=normals, vertices=n, triangles=m,
                           bytes_to_host=24 * n + 12 * m + (12 * n if normals else 0), workspace_bytes=4 * base.numel())
                rows.append((row, call, cursor))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=list(DIMS), help="voxels of the volume (multiples of 8)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_mesh_lod: no GPU - device times are measured, never estimated")
    sparse, dense = fused(tuple(a.dims))
    rows = rows_of((("dense", dense), ("sparse", sparse)))
    times = [[] for _ in rows]
    for r in range(a.warmup + a.rounds):
        for i, (row, call, cursor) in enumerate(rows):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            call()
            end.record()
            end.synchronize()
            if cursor.tolist() != [row["vertices"], row["triangles"]]:
                raise SystemExit(f"the fill launches of {row} counted {cursor.tolist()}")
            if r >= a.warmup:
                times[i].append(begin.elapsed_time(end) * 1e3)
    out = []
    for (row, _, _), us in zip(rows, times):
        full = next(r for r, _, _ in rows if r["volume"] == row["volume"] and r["cell"] == 1 and not r["normals"])
        row.update(device_us_median=round(statistics.median(us), 1), device_us_min=round(min(us), 1), device_us_max=round(max(us), 1),
                   triangles_of_full=round(row["triangles"] / max(full["triangles"], 1), 4))
        out.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "volume": list(a.dims), "voxel_size": VOXEL, "allocated_blocks": sparse.allocated_blocks(),
              "device_us": f"two device events round the four launches of one call, {a.warmup} warm-up + {a.rounds} timed rounds over all rows",
              "not_measured": ["a fused real scene", "mesh() end to end with its allocations and reads", "the copy to the host"], "rows": out}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
