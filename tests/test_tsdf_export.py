"""CPU: the host side of the TSDF-fusion export (monorec_amd.tsdf_export) - the committed fixture of the reference's
save_frame_for_tsdf / save_intrinsics_for_tsdf (tools/make_golden_tsdf.py), shard planning, the manifest, the threshold conversion,
the writer pool on host frames, the C entry's argument checks and the command line.  Nothing here launches a kernel."""
import ctypes
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from monorec_amd import _lib, synth, tsdf_export as tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = np.load(os.path.join(GOLDEN, "tsdf_export.npz"))
META = json.load(open(os.path.join(GOLDEN, "tsdf_export.json")))


def _cases():
    for size in synth.TSDF_SIZES:
        for which in synth.TSDF_SETS:
            for crop_name, crop in synth.TSDF_CROPS[size].items():
                for thr_name, thr in synth.TSDF_THRESHOLDS.items():
                    yield size, which, crop_name, crop, thr_name, thr


# ------------------------------------------------------------------------------------------ fixture
def test_fixture_holds_every_case_and_reaches_every_class():
    """What tools/make_golden_tsdf.py asserted when it wrote the file, re-asserted on the committed arrays: per case the inputs reach
    kept / below the minimum / above the maximum / zero input / wrapped negative and both exact boundary values."""
    seen = 0
    for size, which, crop_name, crop, thr_name, (lo, hi) in _cases():
        name = f"{size[0]}x{size[1]}.{which}"
        case = f"{name}.{crop_name}.{thr_name}"
        y0, y1, x0, x1 = crop if crop is not None else (0, size[0], 0, size[1])
        depth, colour = FIXTURE[case + ".depth"], FIXTURE[case + ".colour"]
        assert depth.dtype == np.int16 and depth.shape == (y1 - y0, x1 - x0) and colour.dtype == np.uint8 and colour.shape == (y1 - y0, x1 - x0, 3)
        assert depth.min() >= 0
        d = FIXTURE[name + ".inv_depth"][y0:y1, x0:x1].astype(np.float64)
        with np.errstate(all="ignore"):
            cm = (1.0 / d) * 100.0
        finite = np.isfinite(cm)
        lo_cm = -1.0 if lo is None else lo * 100
        hi_cm = np.inf if hi is None else hi * 100
        classes = {"kept": (depth > 0).sum(),
                   "zero_input": ((d == 0) & (depth == 0)).sum(),
                   "wrapped_negative": (finite & (cm >= 32768) & (cm < 65536) & (depth == 0)).sum(),
                   "boundary_32767": (FIXTURE[name + ".inv_depth"][y0:y1, x0:x1] == np.float32(synth.TSDF_BOUNDARY_32767)).sum(),
                   "boundary_32768": (FIXTURE[name + ".inv_depth"][y0:y1, x0:x1] == np.float32(synth.TSDF_BOUNDARY_32768)).sum()}
        if lo is not None:
            classes["below_min"] = (finite & (cm >= 1) & (cm < lo_cm) & (depth == 0)).sum()
        if hi is not None:
            classes["above_max"] = (finite & (cm > hi_cm) & (cm < 32767) & (depth == 0)).sum()
        assert all(v > 0 for v in classes.values()), (case, classes)
        assert {k: int(v) for k, v in classes.items()} == {k: v for k, v in META["cases"][case]["classes"].items() if k in classes}
        if thr_name == "3_30":
            assert 2 * np.count_nonzero(depth) >= depth.size, case
        seen += 1
    assert seen == 32 == len(META["cases"])


def test_fixture_boundaries_and_planted_values():
    """1 / 327.67 is the last depth that survives (32767), 1 / 327.68 wraps to -32768 and is dropped; the special inputs sit where
    synth.make_tsdf_case says and give what the issue derives for them."""
    for size in synth.TSDF_SIZES:
        for which in synth.TSDF_SETS:
            name = f"{size[0]}x{size[1]}.{which}"
            planted = synth.make_tsdf_case(size, which)["planted"]
            d, out = FIXTURE[name + ".inv_depth"], FIXTURE[name + ".full.none.depth"]
            assert d[planted["boundary_32767"]] == np.float32(1 / 327.67) and out[planted["boundary_32767"]] == 32767
            assert d[planted["boundary_32768"]] == np.float32(1 / 327.68) and out[planted["boundary_32768"]] == 0
            assert np.isnan(d[planted["nan"]]) and np.isinf(d[planted["inf"]]) and d[planted["zero"]] == 0
            for key in ("zero", "minus_zero", "wrapped", "wrapped_far", "negative", "tiny", "minus_tiny", "subnormal", "nan", "inf", "past_int32"):
                assert out[planted[key]] == 0, (name, key)
            assert out[planted["twice_wrapped"]] == 70000 - 65536          # the low half of the 32-bit conversion, not a saturation
            assert (out[planted["two_metres"]], out[planted["five_cm"]], out[planted["seven_cm"]], out[planted["twentynine_cm"]]) == (200, 5, 7, 29)
            assert (out[planted["three_metres"]], out[planted["thirty_metres"]], out[planted["fifty_metres"]]) == (300, 3000, 5000)
            # 3 / 30 keeps exactly 300 and 3000 cm, 3.005 / 29.995 drops both: the threshold that is not a whole number of centimetres
            assert (FIXTURE[name + ".full.3_30.depth"][planted["three_metres"]], FIXTURE[name + ".full.3_30.depth"][planted["thirty_metres"]]) == (300, 3000)
            assert (FIXTURE[name + ".full.frac.depth"][planted["three_metres"]], FIXTURE[name + ".full.frac.depth"][planted["thirty_metres"]]) == (0, 0)
            # .07 * 100 and .29 * 100 are 7.000000000000001 and 28.999999999999996 in double: the reference keeps 7 and 29 cm, so it compares in fp32
            assert (FIXTURE[name + ".full.ulp.depth"][planted["seven_cm"]], FIXTURE[name + ".full.ulp.depth"][planted["twentynine_cm"]]) == (7, 29)
    assert META["threshold_comparison"]["arithmetic"] == "fp32"


def test_fixture_colour_is_not_the_source_byte():
    """The keyframes hold all 256 byte values u as u / 255 - .5; (k + .5) * 255 truncated gives some of them back one lower."""
    for size in synth.TSDF_SIZES:
        for which in synth.TSDF_SETS:
            name = f"{size[0]}x{size[1]}.{which}"
            k = FIXTURE[name + ".keyframe"]
            source = np.rint((k.astype(np.float64) + .5) * 255).astype(np.int64)
            assert np.array_equal(np.unique(source), np.arange(256))
            assert np.array_equal((source.astype(np.float32) / np.float32(255) - np.float32(.5)), k)
            colour = FIXTURE[name + ".full.none.colour"].astype(np.int64)
            diff = source.transpose(1, 2, 0) - colour
            assert diff.max() == 1 and diff.min() == 0 and (diff == 1).any()
            lower = np.unique(source.transpose(1, 2, 0)[diff == 1])
            assert len(lower) == 63                                   # of the 256 byte values (measured with torch 2.10 on x86)
    assert all(v["depth_mode"] == "I" and v["colour_mode"] == "RGB" for v in META["cases"].values())


def test_threshold_conversion():
    assert tx.threshold_cm(None, "-inf") == float("-inf") and tx.threshold_cm(None, "inf") == float("inf")
    assert tx.threshold_cm(3, "-inf") == 300.0 and tx.threshold_cm(30, "inf") == 3000.0
    assert .07 * 100 != 7 and tx.threshold_cm(.07, "-inf") == 7.0            # product in double, comparison in fp32
    assert .29 * 100 != 29 and tx.threshold_cm(.29, "inf") == 29.0
    assert tx.threshold_cm(3.005, "-inf") == 300.5 and tx.threshold_cm(29.995, "inf") == float(np.float32(2999.5))
    assert tx.threshold_cm(0.123, "inf") == float(np.float32(0.123 * 100))
    assert tx.crop_box(None, 13, 21) == (0, 13, 0, 21) and tx.crop_box([2, 11, 3, 20], 13, 21) == (2, 11, 3, 20)
    for bad in ([2, 2, 3, 20], [2, 14, 3, 20], [-1, 11, 3, 20], [2, 11, 20, 3], [2, 11, 3, 22]):
        with pytest.raises(ValueError):
            tx.crop_box(bad, 13, 21)
    assert tx.packed_sizes(1, 9, 17) == (320, 459) and tx.packed_sizes(2, 24, 32) == (3072, 4608)


# ------------------------------------------------------------------------------------------ shard planning
@pytest.mark.parametrize("use_mask", [True, False])
def test_shard_planning(use_mask):
    """Windows of 0-12 keyframes over 1-4 ranks: the exports are contiguous ranges in rank order that together are 0 .. N-1, every rank
    runs its keyframes plus two either side with the vote, and replaying create_pointcloud.py's buffer over a rank's items exports
    exactly its range - the window items an unsharded run gives the same numbers."""
    def replay(first, last):
        buf, out = [], []
        for item in range(first, last):
            if not use_mask:
                out.append(item)
                continue
            buf.append(item)
            if len(buf) >= 5:
                out.append(buf[2])
                del buf[0]
        return out

    for window in range(13):
        whole = replay(0, window)                                   # export number e is window item whole[e]
        assert len(whole) == (max(0, window - 4) if use_mask else window)
        for world in range(1, 5):
            covered = []
            for rank in range(world):
                plan = tx.plan_shard(window, use_mask, rank, world)
                lo, hi = plan["exports"]
                first, last = plan["items"]
                assert plan["total"] == len(whole) and 0 <= lo <= hi <= plan["total"] and 0 <= first <= last <= window
                assert replay(first, last) == whole[lo:hi]
                if hi > lo and use_mask:
                    assert (first, last) == (whole[lo] - 2, whole[hi - 1] + 3)
                if hi == lo:
                    assert first == last                                # nothing to write: nothing is run
                covered += list(range(lo, hi))
            assert covered == list(range(len(whole)))
    assert tx.plan_shard(12, True, 1, 2) == {"total": 8, "exports": (4, 8), "items": (4, 12), "halo": 2}
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            tx.plan_shard(9, use_mask, rank, world)


# ------------------------------------------------------------------------------------------ writer pool
def _host_frames(n, ch=9, cw=17, seed=3):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, 32768, size=(ch, cw)).astype(np.int16), rng.randint(0, 256, size=(ch, cw, 3)).astype(np.uint8),
             torch.tensor(np.linalg.qr(rng.randn(4, 4))[0], dtype=torch.float32)) for _ in range(n)]


def _read_frame(out_dir, index):
    from PIL import Image
    base = os.path.join(str(out_dir), f"frame-{index:06d}")
    with Image.open(base + ".depth.png") as img:
        mode, depth = img.mode, np.array(img)
    with Image.open(base + ".color.jpg") as img:
        colour = np.array(img)
    return mode, depth, colour, np.loadtxt(base + ".pose.txt")


def test_writer_pool_files_decode_to_what_was_fed(tmp_path):
    import io
    from PIL import Image
    frames = _host_frames(7)
    with tx.TSDFExporter(tmp_path, 13, 21, crop=(2, 11, 3, 20), ring=3, workers=2) as ex:
        for i, (depth, colour, pose) in enumerate(frames):
            ex.add_packed(i, depth, colour, pose, sequence=7, image_id=100 + i)
    assert ex.written == 7
    assert sorted(os.listdir(tmp_path)) == sorted([f"frame-{i:06d}.{ext}" for i in range(7) for ext in ("color.jpg", "depth.png", "pose.txt")] + ["frames.json"])
    for i, (depth, colour, pose) in enumerate(frames):
        mode, got_depth, got_colour, got_pose = _read_frame(tmp_path, i)
        assert mode in ("I;16", "I") and np.array_equal(got_depth.astype(np.int64), depth.astype(np.int64))
        buf = io.BytesIO()
        Image.fromarray(colour).save(buf, format="JPEG")                 # decode(encode(x)) with the Pillow of this run
        assert np.array_equal(got_colour, np.array(Image.open(io.BytesIO(buf.getvalue()))))
        assert np.array_equal(got_pose.astype(np.float32), torch.inverse(pose).numpy())
    assert tx.read_manifest(tmp_path) == {i: (7, 100 + i) for i in range(7)}
    # any compression level decodes to the same pixels
    with tx.TSDFExporter(tmp_path / "l1", 13, 21, crop=(2, 11, 3, 20), ring=2, workers=1, png_compress_level=1) as ex:
        ex.add_packed(0, *frames[0])
    assert np.array_equal(_read_frame(tmp_path / "l1", 0)[1], _read_frame(tmp_path, 0)[1])
    with pytest.raises(ValueError):
        tx.TSDFExporter(tmp_path / "bad", 13, 21, crop=(2, 14, 3, 20))
    ex = tx.TSDFExporter(tmp_path / "shape", 13, 21, ring=1, workers=1)
    with pytest.raises(ValueError):
        ex.add_packed(0, *frames[0])                                     # 9 x 17 arrays into a 13 x 21 exporter
    ex.close()
    with pytest.raises(RuntimeError):
        ex.add_packed(0, *frames[0])


def test_worker_error_surfaces_in_close(tmp_path):
    frames = _host_frames(4)
    ex = tx.TSDFExporter(tmp_path, 9, 17, ring=2, workers=2)
    inner = ex._write

    def failing(out_dir, index, *rest):
        if index == 1:
            raise OSError("disk full (injected)")
        return inner(out_dir, index, *rest)
    ex._write = failing
    for i, (depth, colour, pose) in enumerate(frames):
        try:
            ex.add_packed(i, depth, colour, pose)                        # never hangs: a failed frame gives its slot back
        except RuntimeError as e:
            assert "disk full" in str(e)
    with pytest.raises(OSError, match="disk full"):
        ex.close()
    assert not os.path.exists(tmp_path / "frame-000001.depth.png") and os.path.exists(tmp_path / "frame-000000.depth.png")
    assert not os.path.exists(tmp_path / "frames.json")


def test_back_pressure_holds_with_a_ring_of_two(tmp_path):
    """With both slots taken by blocked writers a third add() waits; every slot is handed to one frame at a time."""
    frames = _host_frames(6)
    ex = tx.TSDFExporter(tmp_path, 9, 17, ring=2, workers=2)
    gate, entered = threading.Event(), threading.Semaphore(0)
    inner, busy, peak, lock = ex._write, [0], [0], threading.Lock()

    def gated(out_dir, index, depth, colour, *rest):
        with lock:
            busy[0] += 1
            peak[0] = max(peak[0], busy[0])
        entered.release()
        gate.wait(30)
        seen = (depth.copy(), colour.copy())
        inner(out_dir, index, depth, colour, *rest)
        assert np.array_equal(seen[0], depth) and np.array_equal(seen[1], colour)      # nobody refilled the slot meanwhile
        with lock:
            busy[0] -= 1
    ex._write = gated
    ex.add_packed(0, *frames[0])
    ex.add_packed(1, *frames[1])
    entered.acquire(timeout=30), entered.acquire(timeout=30)             # both writers hold their slot
    assert ex._free.qsize() == 0
    third = threading.Thread(target=lambda: [ex.add_packed(i, *frames[i]) for i in range(2, 6)])
    third.start()
    third.join(0.05)
    assert third.is_alive() and ex._jobs.qsize() == 0                    # blocked in add(): nothing was queued behind the ring
    gate.set()
    third.join(30)
    assert not third.is_alive()
    ex.close()
    assert peak[0] <= 2 and ex.written == 6
    for i, (depth, colour, _) in enumerate(frames):
        assert np.array_equal(_read_frame(tmp_path, i)[1].astype(np.int64), depth.astype(np.int64))


def test_manifest_merge_of_shards_equals_the_unsharded_file(tmp_path):
    frames = _host_frames(5)
    with tx.TSDFExporter(tmp_path / "whole", 9, 17, ring=2, workers=2) as ex:
        for i, f in enumerate(frames):
            ex.add_packed(i, *f, sequence=3, image_id=10 + i)
    for lo, hi in ((3, 5), (0, 3)):                                     # in any order
        with tx.TSDFExporter(tmp_path / "parts", 9, 17, ring=2, workers=2, merge_manifest=True) as ex:
            for i in range(lo, hi):
                ex.add_packed(i, *frames[i], sequence=3, image_id=10 + i)
    names = sorted(os.listdir(tmp_path / "whole"))
    assert names == sorted(os.listdir(tmp_path / "parts")) and "frames.json" in names
    for n in names:
        assert open(tmp_path / "whole" / n, "rb").read() == open(tmp_path / "parts" / n, "rb").read(), n
    doc = json.load(open(tmp_path / "whole" / "frames.json"))
    assert doc["version"] == 1 and list(doc["frames"]) == ["0", "1", "2", "3", "4"] and doc["frames"]["4"] == [3, 14]
    with tx.TSDFExporter(tmp_path / "whole", 9, 17, ring=1, workers=1) as ex:        # an unsharded run starts the manifest afresh
        ex.add_packed(0, *frames[0], sequence=3, image_id=10)
    assert tx.read_manifest(tmp_path / "whole") == {0: (3, 10)}


def test_intrinsics_file_and_the_callers_tensor(tmp_path):
    """camera-intrinsics.txt is the fixture's text; the caller's tensor is not shifted (the reference shifts it in place)."""
    for size in synth.TSDF_SIZES:
        name = f"{size[0]}x{size[1]}.a"
        for crop_name, crop in synth.TSDF_CROPS[size].items():
            k = torch.from_numpy(FIXTURE[name + ".intrinsics"].copy())
            before = k.clone()
            tx.save_intrinsics_for_tsdf(tmp_path, k, crop=crop)
            assert torch.equal(k, before)
            assert open(tmp_path / "camera-intrinsics.txt").read() == META["frames"][f"{name}.{crop_name}"]["intrinsics_text"]


# ------------------------------------------------------------------------------------------ C entry
def test_entry_is_declared_bound_and_documented(hip_lib):
    header = open(os.path.join(ROOT, "include", "monorec_hip.h")).read()
    assert re.search(r"\bint mr_tsdf_frame_f32\s*\(", header) and "mr_tsdf_frame_f32" in _lib.ABI
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)", header).group(1)) == _lib.MR_ABI_VERSION == hip_lib.mr_abi_version() >= 23
    assert len(_lib.ABI["mr_tsdf_frame_f32"][1]) == 14
    table = [line for line in open(os.path.join(ROOT, "INTEGRATION.md")) if line.startswith("|")]
    assert any("`mr_tsdf_frame_f32`" in line and "utils/util.py" in line for line in table)


def test_entry_rejects_bad_arguments_without_a_launch(hip_lib):
    """Every call below returns MR_ERR_BAD_ARGUMENT before anything is launched: this runs without a device, and the pointers are
    host memory nothing may touch."""
    h, w, ch, cw = 13, 21, 9, 17
    inv = (ctypes.c_float * (h * w))()
    kf = (ctypes.c_float * (3 * h * w))()
    out = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(out) + 63) // 64 * 64
    depth, colour = base, base + 1024
    masks = (ctypes.c_void_p * 9)(*[ctypes.addressof(inv)] * 9)
    none_masks = (ctypes.c_void_p * 1)(None)
    ninf, inf = float("-inf"), float("inf")

    def call(inv_p=ctypes.addressof(inv), kf_p=ctypes.addressof(kf), masks_p=none_masks, n=0, crop=(2, 11, 3, 20), lo=ninf, hi=inf,
             b=1, hh=h, ww=w, depth_p=depth, colour_p=colour):
        box = None if crop is None else (ctypes.c_int32 * 4)(*crop)
        return hip_lib.mr_tsdf_frame_f32(inv_p, kf_p, masks_p, n, 0.0, box, lo, hi, b, hh, ww, depth_p, colour_p, None)

    bad = [dict(inv_p=None), dict(kf_p=None), dict(depth_p=None), dict(colour_p=None), dict(b=0), dict(hh=0), dict(ww=-3),
           dict(crop=(2, 14, 3, 20)), dict(crop=(2, 11, 3, 22)), dict(crop=(-1, 11, 3, 20)), dict(crop=(2, 11, -1, 20)),
           dict(crop=(5, 5, 3, 20)), dict(crop=(2, 11, 20, 20)), dict(crop=(11, 2, 3, 20)),
           dict(n=9, masks_p=masks), dict(n=-1), dict(n=2, masks_p=None), dict(n=1, masks_p=none_masks),
           dict(lo=float("nan")), dict(hi=float("nan")), dict(depth_p=depth + 2), dict(colour_p=colour + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert b"argument" in hip_lib.mr_error_string(-1).lower()


# ------------------------------------------------------------------------------------------ command line, config
def test_command_line_and_config(tmp_path, capsys):
    base = {"arch": {"type": "MonoRecModel", "args": {"cv_depth_steps": 8}}, "data_set": {"type": "KittiOdometryDataset", "args": {}},
            "roi": [4, 60, 8, 120], "min_d": 3, "max_d": 30, "output_dir": "from_checkpoint"}
    (tmp_path / "ckpt").mkdir()
    json.dump(base, open(tmp_path / "ckpt" / "config.json", "w"))
    json.dump({"output_dir": "from_config", "use_mask": False}, open(tmp_path / "over.json", "w"))
    config, device = tx.load_config(["-r", str(tmp_path / "ckpt" / "model.pth"), "-c", str(tmp_path / "over.json"), "-d", "cuda:1"])
    assert device == "cuda:1" and config["output_dir"] == "from_config" and config["use_mask"] is False and config["roi"] == [4, 60, 8, 120]
    config, device = tx.load_config(["--resume", str(tmp_path / "ckpt" / "model.pth")])
    assert device == "cuda:0" and config == base
    for argv in ([], ["-c", str(tmp_path / "over.json")]):              # no file at all; a file without data_set / arch
        with pytest.raises(SystemExit):
            tx.load_config(argv)
    capsys.readouterr()
    # run() checks what it can before it touches a device
    with pytest.raises(ValueError, match="KittiOdometryDataset"):
        tx.run(dict(base, data_set={"type": "OxfordRobotCarDataset", "args": {}}))
    with pytest.raises(ValueError, match="MonoRecModel"):
        tx.run(dict(base, arch={"type": "OtherModel", "args": {}}))
    with pytest.raises(ValueError, match="rank"):
        tx.run(base, shard=(2, 2))


def test_dropin_rebinds_the_tsdf_functions(tmp_path):
    """python -m monorec_amd.dropin <script>: `from utils import save_frame_for_tsdf` and `utils.util.save_intrinsics_for_tsdf` resolve
    to the device implementations in a miniature checkout with the reference's import structure."""
    import subprocess
    import sys
    root = tmp_path
    (root / "model" / "monorec").mkdir(parents=True)
    (root / "utils").mkdir()
    for p in ("model/__init__.py", "model/monorec/__init__.py"):
        (root / p).write_text("")
    (root / "model" / "monorec" / "monorec_model.py").write_text("class MonoRecModel:\n    pass\n")
    (root / "model" / "model.py").write_text("from .monorec.monorec_model import MonoRecModel\n")
    (root / "utils" / "util.py").write_text("def save_frame_for_tsdf(*a, **k):\n    return 'reference'\n"
                                            "def save_intrinsics_for_tsdf(*a, **k):\n    return 'reference'\n"
                                            "def untouched(*a, **k):\n    return 'reference'\n")
    (root / "utils" / "__init__.py").write_text("from .util import *\n")
    (root / "script.py").write_text("import utils\nimport utils.util\nfrom utils import save_frame_for_tsdf\n"
                                    "print(save_frame_for_tsdf.__module__, utils.util.save_frame_for_tsdf.__module__,\n"
                                    "      utils.save_intrinsics_for_tsdf.__module__, utils.util.save_intrinsics_for_tsdf.__module__, utils.untouched())\n")
    out = subprocess.run([sys.executable, "-m", "monorec_amd.dropin", "script.py"], cwd=root, env=dict(os.environ, PYTHONPATH=ROOT),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["monorec_amd.tsdf_export"] * 4 + ["reference"]
