#!/usr/bin/env python
"""CPU-only stress of the input side of an N-rank job on ONE host when the frames come from a pre-decoded store
(monorec_amd.frame_store) - the counterpart of tools/decode_stress.py, to be run back to back with it on the same host:

    python tools/store_stress.py [--ranks 8] [--keyframes 200] [--records 256] [--pace-kfps 0] [--no-pin] [--json out.json]

The parent writes one frame stream through `FrameStoreWriter`: `--records` synthetic 256 x 512 x 3 records (393216 bytes each, the
resized frame of the KITTI configs; 256 records = 96 MiB, a window of one sequence) and reads it once, so that it is in the page cache.
Then `--ranks` processes start.  Each places itself exactly like a rank of `torchrun --nproc-per-node N bench.py`
(monorec_amd.distributed.place_rank), opens the file with `FrameStoreReader` and sweeps `--keyframes` keyframes through
`input_pipeline.FrameCache(store=)`, starting at its own record.  The device step is a no-op: the "preprocessor" copies the record
from the mapped file into one of four host buffers of the pinned ring's size - the host work of a store hit.  Two walks per rank:

    sequential   consecutive keyframes, cache of 8 frames: one new record per keyframe
    no_hits      a cache that keeps nothing (what `use_index_mask`, dilation with a small cache or `return_stereo` do to the
                 walk): three records per keyframe with frame_count = 2

Reported per rank and walk: wall ms per keyframe, the keyframes/s the host side alone sustains, records per keyframe, the longest
wait for a sample; plus the aggregate and the slowest rank.  `--pace-kfps K`: the consumer takes a keyframe every 1 / K s."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH, CHANNELS = 256, 512, 3


class HostCopy:
    """Stands where the ImagePreprocessor stands: `unpack` is the copy into the staging ring, without upload and launch."""

    def __init__(self, nbytes):
        import numpy as np
        self.ring = [np.empty(nbytes, dtype=np.uint8) for _ in range(4)]
        self.pos = 0
        self.bytes = 0

    def unpack(self, record):
        slot = self.ring[self.pos % 4]
        self.pos += 1
        slot.reshape(record.shape)[...] = record
        self.bytes += record.size
        return slot


def write_store(path, records):
    import numpy as np
    from monorec_amd import frame_store, synth
    header = frame_store.frame_header("KittiOdometryDataset", "00", 2, (370, 1226), (0, 0, 1226, 370), (HEIGHT, WIDTH), CHANNELS, records)
    base = [synth.make_u8_image(HEIGHT, WIDTH, CHANNELS, seed=200 + i).transpose(2, 0, 1) for i in range(8)]
    with frame_store.FrameStoreWriter(path, header) as writer:
        for i in range(records):
            writer.add_frame(i, np.roll(base[i % 8], i, axis=2))
    with open(path, "rb") as f:                          # once through: the file is in the page cache when the ranks start
        while f.read(1 << 24):
            pass
    return os.path.getsize(path)


def worker(rank, ranks, keyframes, pace, pin, path, q, go):
    os.environ.update(LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(ranks), WORLD_SIZE=str(ranks), RANK=str(rank))
    import torch
    from monorec_amd import distributed as mrd, frame_store, input_pipeline
    info = mrd.place_rank(rank, ranks) if pin else {"cpus": len(os.sched_getaffinity(0)), "pinned": False}
    threads, _ = mrd.host_thread_budget(info["cpus"])
    torch.set_num_threads(1)
    reader = frame_store.FrameStoreReader(path)
    nbytes = reader.channels * reader.plane_stride
    first = 1 + rank * (reader.count // ranks)           # every rank its own part of the file

    def never(i):
        raise AssertionError(f"record {i} is in the store: nothing may be decoded")
    q.put(("ready", rank))
    go.wait()
    row = {"rank": rank, "cpus": info["cpus"], "pinned": bool(info.get("pinned")), "decode_threads": threads}
    for walk, capacity in (("sequential", 8), ("no_hits", 0)):
        pre = HostCopy(nbytes)
        cache = input_pipeline.FrameCache(never, pre, capacity=capacity, workers=threads, index_range=(0, reader.count), store=reader)
        waits = []
        t0 = time.perf_counter()
        for k in range(keyframes):
            if pace > 0:
                target = t0 + k / pace
                while time.perf_counter() < target:
                    time.sleep(0.0002)
            tw = time.perf_counter()
            cache.sample(1 + (first + k - 1) % (reader.count - 2), frame_count=2)
            waits.append(time.perf_counter() - tw)
        dt = time.perf_counter() - t0
        cache.close()
        assert cache.decoded == 0
        row[walk] = {"wall_ms_per_keyframe": dt / keyframes * 1e3, "host_keyframes_per_s": keyframes / dt, "max_wait_ms": max(waits) * 1e3,
                     "records_per_keyframe": cache.unpacked / keyframes, "copied_GB_per_s": pre.bytes / dt / 1e9}
    q.put(("done", rank, row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--pace-kfps", type=float, default=0.0)
    ap.add_argument("--no-pin", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "00_cam2.mrfs")
        size = write_store(path, a.records)
        ctx = mp.get_context("spawn")
        q, go = ctx.Queue(), ctx.Event()
        procs = [ctx.Process(target=worker, args=(r, a.ranks, a.keyframes, a.pace_kfps, not a.no_pin, path, q, go)) for r in range(a.ranks)]
        for p in procs:
            p.start()
        for _ in procs:
            assert q.get(timeout=300)[0] == "ready"
        go.set()                                         # every rank sweeps at the same time
        rows = sorted((q.get(timeout=900)[2] for _ in procs), key=lambda r: r["rank"])
        for p in procs:
            p.join(timeout=60)
    out = {"host_cpus": len(os.sched_getaffinity(0)), "ranks": a.ranks, "keyframes_per_rank": a.keyframes, "pace_kfps": a.pace_kfps,
           "store_file_bytes": size, "record_bytes": CHANNELS * HEIGHT * WIDTH, "records": a.records, "per_rank": rows}
    for walk in ("sequential", "no_hits"):
        out[walk] = {"aggregate_host_keyframes_per_s": sum(r[walk]["host_keyframes_per_s"] for r in rows),
                     "slowest_rank_keyframes_per_s": min(r[walk]["host_keyframes_per_s"] for r in rows),
                     "fastest_rank_keyframes_per_s": max(r[walk]["host_keyframes_per_s"] for r in rows)}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
