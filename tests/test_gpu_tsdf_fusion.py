"""GPU: TSDF fusion on the device - `mr_tsdf_integrate_f32` / `mr_tsdf_extract_f32` against the numpy restatement of
tests/tsdf_fusion_ref.py on an analytic scene, launch batching and order, unaligned volumes, the directory reader and the runner
against a one-at-a-time loop.  Every comparison is exact."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import tsdf_fusion_ref as ref
import tsdf_mesh_ref as mref
from monorec_amd import _lib, synth, tsdf_export as tx, tsdf_fusion as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = ref.INTRINSICS_60
K3 = torch.tensor([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=torch.float32)
VOLUMES = {"small": ref.SMALL, "wide": ref.WIDE}
ORDER = [0, 10, 1, 2, 3, 4, 5, 6, 7, 8, 9]             # the frame that looks away comes second: every count above 1 has it


@functools.lru_cache(maxsize=None)
def _frames():
    frames = ref.make_frames(K)
    return [frames[i] for i in ORDER]


def _on_device(frames):
    return (torch.from_numpy(np.stack([f[1] for f in frames])).to(DEV), torch.from_numpy(np.stack([f[2] for f in frames])).to(DEV),
            torch.from_numpy(np.stack([f[0] for f in frames])))


@functools.lru_cache(maxsize=None)
def _reference(name, count, colour, max_depth, reverse=False):
    """The restatement's volume after the first `count` frames, and the per-frame masks.  Shared, never modified."""
    vol = ref.new_volume(colour=colour, **VOLUMES[name])
    frames = _frames()[:count]
    stats = [ref.integrate(vol, ref.world_to_camera(pose), K, depth, image if colour else None, max_depth)
             for pose, depth, image in (frames[::-1] if reverse else frames)]
    return vol, stats


def _volume(name, colour=True, storage=None):
    spec = VOLUMES[name]
    return tf.TSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], colour=colour,
                         device=DEV, storage=storage)


def _assert_equal(volume, want, what=""):
    tsdf, weight, colour = volume.grids()
    assert np.array_equal(weight, want["weight"]), what
    assert np.array_equal(tsdf, want["tsdf"]), what
    if want["colour"] is None:
        assert colour is None
    else:
        assert np.array_equal(colour, want["colour"]), what


def _assert_not_degenerate(name):
    """On the restatement alone: the eleven frames reach every branch of the integration on this volume."""
    vol, stats = _reference(name, 11, True, np.inf)
    seeing = [s for s in stats if not s["behind"].all()]
    assert len(seeing) == 10 and stats[1]["behind"].all() and not stats[1]["updated"].any()          # one frame has every voxel behind it
    never = 1.0 - np.any([s["updated"] for s in stats], axis=0).mean()
    if name == "small":
        for s in seeing:
            assert s["band"].mean() >= 0.10 and s["clamped"].mean() >= 0.10 and s["occluded"].mean() >= 0.05 and s["nodepth"].any()
        assert never >= 0.20
    else:
        assert never >= 0.5
        for s in seeing:                                                   # most of this volume is outside: the issue's fractions, of what a frame's frustum holds
            held = s["inside"].sum()
            assert held >= 0.1 * s["inside"].size
            assert s["band"].sum() >= 0.10 * held and s["clamped"].sum() >= 0.10 * held and s["occluded"].sum() >= 0.05 * held and s["nodepth"].any()
        inside = np.any([s["inside"] for s in stats], axis=0)
        nx, ny, nz = vol["dims"]
        tiles = [inside[z:z + tf.TILE[2], y:y + tf.TILE[1], x:x + tf.TILE[0]]
                 for z in range(0, nz, tf.TILE[2]) for y in range(0, ny, tf.TILE[1]) for x in range(0, nx, tf.TILE[0])]
        outside = sum(1 for t in tiles if not t.any())
        straddle = sum(1 for t in tiles if t.any() and not t.all())
        assert outside * 4 >= len(tiles) and straddle * 4 >= len(tiles), (outside, straddle, len(tiles))


# ------------------------------------------------------------------------------------------ 1. integrate
@pytest.mark.parametrize("count", [1, 3, 8, 11])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_integrate_equals_the_restatement(hip_lib, name, count):
    """37 x 21 x 13 (odd nx: rows off the 16-byte boundary, the scalar tail) and 128 x 24 x 12 (16-byte rows, tiles outside and
    astride the frusta); 1, 3, 8 frames in one launch and 11 in two; with and without colour; with and without a depth limit."""
    assert VOLUMES["small"]["dims"][0] % 4 == 1 and VOLUMES["wide"]["dims"][0] % 4 == 0
    _assert_not_degenerate(name)
    depth, image, poses = _on_device(_frames()[:count])
    for colour in (True, False):
        for max_depth in (np.inf, 2.9):
            want, stats = _reference(name, count, colour, max_depth)
            if max_depth == 2.9 and count > 1:
                full, _ = _reference(name, count, colour, np.inf)
                assert not np.array_equal(full["weight"], want["weight"]) and want["weight"].any()      # the limit drops the wall, not all
            volume = _volume(name, colour)
            volume.integrate(depth, image if colour else None, poses, K3, None if max_depth == np.inf else max_depth)
            assert volume.frames == count
            _assert_equal(volume, want, (name, count, colour, max_depth))
    with pytest.raises(RuntimeError, match="CPU fallback"):
        volume.integrate(depth.cpu(), None, poses, K3)
    with pytest.raises(ValueError, match="colour"):
        _volume(name, True).integrate(depth, None, poses, K3)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cameras_in_and_around_the_volume_at_any_angle(hip_lib, seed):
    """Culling must never change a result: eight cameras at random places inside and just outside the wide volume, turned any way,
    with focal lengths from wide to narrow and random depth - tiles that hold a camera centre, tiles a side plane grazes, tiles behind."""
    rng = np.random.default_rng(seed)
    spec = VOLUMES["wide"]
    lo = np.array(spec["origin"])
    hi = lo + (np.array(spec["dims"]) - 1) * spec["voxel_size"]
    h, w = 24, 40
    want = ref.new_volume(**spec)
    volume = _volume("wide")
    depth = rng.integers(20, 400, size=(8, h, w)).astype(np.int16)
    depth[rng.random((8, h, w)) < 0.1] = 0
    image = rng.integers(0, 256, size=(8, h, w, 3)).astype(np.uint8)
    poses, ks, seen, behind, outside = [], [], 0.0, 0.0, 0.0
    for i in range(8):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        pose = np.eye(4)
        pose[:3, :3] = q
        pose[:3, 3] = lo - 0.3 + rng.random(3) * (hi - lo + 0.6)
        focal = float(rng.choice([12.0, 30.0, 90.0]))
        poses.append(pose.astype(np.float32))
        ks.append((focal, focal * 1.1, 19.5 + rng.normal(), 11.5 + rng.normal()))
        stats = ref.integrate(want, ref.world_to_camera(poses[-1]), ks[-1], depth[i], image[i])
        seen, behind, outside = seen + stats["updated"].mean(), behind + stats["behind"].mean(), outside + stats["outside"].mean()
    assert seen > 0.05 and behind > 1 and outside > 1 and want["weight"].max() >= 2          # (fractions of the volume, summed over the frames)
    k = torch.tensor([[[fx, 0, cx], [0, fy, cy], [0, 0, 1]] for fx, fy, cx, cy in ks], dtype=torch.float32)
    volume.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(image).to(DEV), torch.from_numpy(np.stack(poses)), k)
    _assert_equal(volume, want, seed)


HARD_SEED = 6                                  # of ref.camera_cases: the first seed at which every case below, on both volumes, meets its sums


@functools.lru_cache(maxsize=None)
def _hard_reference(name, kind, depth, shift):
    """(spec, frames, ks, the restatement's volume, [updated, behind, outside] summed over the frames as fractions of the volume)."""
    spec = ref.shifted(VOLUMES[name], shift)
    frames, ks = ref.camera_cases(VOLUMES[name], HARD_SEED, kind, depth, shift)
    want, sums = ref.new_volume(**spec), np.zeros(3)
    for (pose, depth_cm, image), k in zip(frames, ks):
        stats = ref.integrate(want, ref.world_to_camera(pose), k, depth_cm, image, np.inf if depth is None else depth)
        sums += [stats["updated"].mean(), stats["behind"].mean(), stats["outside"].mean()]
    return spec, frames, ks, want, sums


@pytest.mark.parametrize("depth", [None, 2.0], ids=["inf", "2m"])
@pytest.mark.parametrize("shift", [ref.ORIGIN, ref.FAR], ids=["origin", "far"])
@pytest.mark.parametrize("kind", ref.CAMERA_KINDS)
@pytest.mark.parametrize("name", ["wide", "small"])
def test_hard_cameras_poses_and_intrinsics_in_both_worlds(hip_lib, name, kind, shift, depth):
    """The tile cull where its margins are asked for: ref.camera_cases' eight cameras in one launch - poses that are no rotations
    (normalised per plane, or culling off), principal points outside the image, fy = 4 fx, one K per frame - round the origin and
    1.5 km from it, where FP32_SLACK * reach carries the margin and not 1e-3 voxel; on the wide volume and on the one with the odd nx."""
    spec, frames, ks, want, (updated, behind, outside) = _hard_reference(name, kind, depth, shift)
    assert updated > (0.05 if depth is None else 0.03) and behind > 1 and outside > 1 and want["weight"].max() >= 2, (updated, behind, outside)
    rows = np.linalg.norm(ref.world_to_camera(frames[0][0])[:, :3], axis=1)
    assert np.all(rows < 0.5) == (kind == "wild") and (np.abs(rows - 1).max() > 0.2) == (kind in ("scaled", "sheared", "wild"))
    depth_cm, image, poses = _on_device(frames)
    k = torch.tensor(np.stack([ref.k_matrix(v) for v in ks]), dtype=torch.float32)
    volume = tf.TSDFVolume(origin=spec["origin"], dims=spec["dims"], voxel_size=spec["voxel_size"], trunc=spec["trunc"], device=DEV)
    volume.integrate(depth_cm, image, poses, k, depth)
    if kind == "wild":
        # culling is off for these matrices; the restatement has one path for every matrix, the one `rigid` takes
        _assert_equal(volume, want, ("wild against the restatement's only path", name, shift, depth))
    _assert_equal(volume, want, (name, kind, shift, depth))


def test_voxel_indices_past_2_to_31(hip_lib):
    """The only cover of the 64-bit index path, and the one large test of this file: 2048 x 1024 x 1028 voxels without colour, 17.2 GB
    of device memory for about a second (plus 0.1 GB of temporaries: the untouched voxels are counted 64 slices at a time).  The
    last four z slices - one layer of tiles - have indices past 2^31.  A
    wide-angle camera stands between slices 1023 and 1024 and looks along z, so only those slices are in front of it; a constant depth
    puts a zero crossing between slices 1025 and 1026.  The block round the camera equals the restatement, nothing else is touched,
    and the extracted points are the restatement's."""
    dims, voxel, trunc = (2048, 1024, 1028), 0.01, 0.02
    assert dims[0] * dims[1] * 1024 == 2 ** 31
    offset, block = (960, 464, 1020), (128, 96, 8)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (10.237, 5.117, 10.235)
    k = (2.0, 2.0, 19.5, 11.5)
    depth = np.full((24, 40), 2, np.int16)
    want = ref.new_volume(block, (0.0, 0.0, 0.0), voxel, trunc, colour=False, offset=offset)
    stats = ref.integrate(want, ref.world_to_camera(pose), k, depth, None)
    edge = stats["updated"].copy()
    edge[4:, 1:-1, 1:-1] = False
    assert 1000 < stats["updated"].sum() and not edge.any() and stats["band"].any()          # all that is seen lies inside the block
    records = ref.extract(want)
    assert len(records) > 300
    volume = tf.TSDFVolume(origin=(0.0, 0.0, 0.0), dims=dims, voxel_size=voxel, trunc=trunc, colour=False, device=DEV, max_bytes=20 << 30)
    volume.integrate(torch.from_numpy(depth).to(DEV), None, torch.from_numpy(pose), torch.tensor([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]]))
    (x0, y0, z0), (bx, by, bz) = offset, block
    nx, ny, nz = dims
    tsdf = volume.tsdf.view(nz, ny, nx)[z0:z0 + bz, y0:y0 + by, x0:x0 + bx].cpu().numpy()
    weight = volume.weight.view(nz, ny, nx)[z0:z0 + bz, y0:y0 + by, x0:x0 + bx].cpu().numpy()
    assert np.array_equal(weight, want["weight"]) and np.array_equal(tsdf, want["tsdf"])
    assert float(volume.weight.sum(dtype=torch.float64)) == float(want["weight"].sum(dtype=np.float64))
    changed = sum(int((volume.tsdf[lo * ny * nx:(lo + 64) * ny * nx] != 1).sum()) for lo in range(0, nz, 64))
    assert changed == int((want["tsdf"] != 1).sum())
    got = volume.extract().cpu().numpy()
    assert np.array_equal(ref.sort_records(got), ref.sort_records(records))


# ------------------------------------------------------------------------------------------ 2. order and batching
@pytest.mark.parametrize("name", ["small", "wide"])
def test_one_launch_of_eight_equals_eight_launches_and_the_order_is_real(hip_lib, name):
    depth, image, poses = _on_device(_frames())
    batch, single, reverse, whole, loop = (_volume(name) for _ in range(5))
    batch.integrate(depth[:8], image[:8], poses[:8], K3)
    for i in range(8):
        single.integrate(depth[i], image[i], poses[i], K3)
    for key in ("tsdf", "weight", "colour"):
        assert torch.equal(getattr(batch, key), getattr(single, key)), key
    _assert_equal(batch, _reference(name, 8, True, np.inf)[0])
    back = list(range(7, -1, -1))
    reverse.integrate(depth[back], image[back], poses[back], K3)
    assert torch.equal(reverse.weight, batch.weight) and not torch.equal(reverse.tsdf, batch.tsdf)
    _assert_equal(reverse, _reference(name, 8, True, np.inf, reverse=True)[0])
    whole.integrate(depth, image, poses, K3)                               # eleven: a launch of eight and one of three
    for i in range(11):
        loop.integrate(depth[i:i + 1], image[i:i + 1], poses[i:i + 1], K3.expand(1, 3, 3))
    for key in ("tsdf", "weight", "colour"):
        assert torch.equal(getattr(whole, key), getattr(loop, key)), key
    assert whole.frames == loop.frames == 11


# ------------------------------------------------------------------------------------------ 3. unaligned views
@pytest.mark.parametrize("name", ["small", "wide"])
def test_volumes_that_start_off_a_16_byte_boundary(hip_lib, name):
    nx, ny, nz = VOLUMES[name]["dims"]
    n = nx * ny * nz
    storage = (torch.empty(n + 1, device=DEV)[1:], torch.empty(n + 1, device=DEV)[1:], torch.empty(n + 1, 4, dtype=torch.uint8, device=DEV)[1:])
    assert all(t.data_ptr() % 16 == 4 for t in storage)
    depth, image, poses = _on_device(_frames())
    volume = _volume(name, storage=storage)
    assert volume.tsdf.data_ptr() == storage[0].data_ptr()
    volume.integrate(depth, image, poses, K3)
    want, _ = _reference(name, 11, True, np.inf)
    _assert_equal(volume, want)
    assert np.array_equal(ref.sort_records(volume.extract().cpu().numpy()), ref.sort_records(ref.extract(want)))


# ------------------------------------------------------------------------------------------ 4. extract
def _ply(data):
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    return lines, body


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_extract_equals_the_restatement(hip_lib, name, colour, tmp_path):
    depth, image, poses = _on_device(_frames())
    volume = _volume(name, colour)
    assert volume.count() == 0 and tuple(volume.extract().shape) == (0, 6)         # untouched: no surface
    volume.integrate(depth, image if colour else None, poses, K3)
    want, _ = _reference(name, 11, colour, np.inf)
    counts = []
    for min_weight in (0, 2):
        expected = ref.sort_records(ref.extract(want, min_weight))
        records = volume.extract(min_weight)
        assert records.is_cuda and records.dtype == torch.float32 and volume.count(min_weight) == records.shape[0] == len(expected)
        assert np.array_equal(ref.sort_records(records.cpu().numpy()), expected)
        counts.append(len(expected))
        if colour:
            assert expected[:, 3:].max() > 100
        else:
            assert not expected[:, 3:].any()
    assert 500 < counts[1] < counts[0]
    buffer = io.BytesIO()
    assert volume.save_ply(buffer) == counts[0]
    assert volume.save_ply(tmp_path / "s.ply", min_weight=2) == counts[1]
    for data, count in ((buffer.getvalue(), counts[0]), (open(tmp_path / "s.ply", "rb").read(), counts[1])):
        lines, body = _ply(data)
        assert lines == ["ply", "format binary_little_endian 1.0", f"element vertex {count}"] + \
            [f"property float {f}" for f in ("x", "y", "z", "red", "green", "blue")]
        assert len(body) == count * 24
        assert np.array_equal(ref.sort_records(np.frombuffer(body, "<f4")), ref.sort_records(ref.extract(want, 0 if count == counts[0] else 2)))
    volume.save(tmp_path / "v.npz")
    again = tf.TSDFVolume.load(tmp_path / "v.npz", device=DEV)
    assert again.dims == volume.dims and again.origin == volume.origin and again.voxel_size == volume.voxel_size and again.trunc == volume.trunc
    assert again.has_colour == colour and again.frames == 11 and torch.equal(again.tsdf, volume.tsdf) and torch.equal(again.weight, volume.weight)
    assert torch.equal(again.extract().sort(0).values, volume.extract().sort(0).values)
    volume.reset()
    assert volume.count() == 0 and bool((volume.tsdf == 1).all()) and not bool(volume.weight.any())


# -- the tiled sweep of the extraction: volumes loaded directly (tsdf_fusion_ref.seam_volume), no integration
@functools.lru_cache(maxsize=None)
def _seams(dims, colour):
    """The seam volume and, per min_weight, its sorted records.  Shared, never modified."""
    vol = ref.seam_volume(dims, colour)
    return vol, {mw: ref.sort_records(ref.extract(vol, mw)) for mw in (0, 2)}


def _load(vol):
    """A device volume holding the arrays of a restatement's volume dict."""
    volume = tf.TSDFVolume(origin=vol["origin"], dims=vol["dims"], voxel_size=float(vol["voxel"]), trunc=float(vol["trunc"]),
                           colour=vol["colour"] is not None, device=DEV)
    volume.tsdf.copy_(torch.from_numpy(vol["tsdf"].reshape(-1)))
    volume.weight.copy_(torch.from_numpy(vol["weight"].reshape(-1)))
    if vol["colour"] is not None:
        volume.colour.copy_(torch.from_numpy(vol["colour"].reshape(-1, 4)))
    return volume


def _assert_every_seam_is_crossed(vol, min_weight):
    """On the restatement alone: crossings along x, y and z; on the edges 31|32, 7|8, 3|4 between the first tile and the next; and
    between the last-but-one and the last voxel of every axis.  An owner at index i owns the edge i | i + 1."""
    nx, ny, nz = vol["dims"]
    own_x, own_y, own_z = ref.crossing_owners(vol, min_weight)
    assert own_x.any() and own_y.any() and own_z.any()
    assert own_x[:, :, 31].any() and own_y[:, 7, :].any() and own_z[3].any()
    assert own_x[:, :, nx - 2].any() and own_y[:, ny - 2, :].any() and own_z[nz - 2].any()
    assert not vol["weight"].all() and (vol["weight"] == 1).any()             # unseen voxels, and voxels min_weight = 2 drops


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("dims", ref.SEAM_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_extract_across_tile_seams_and_ragged_ends(hip_lib, dims, colour):
    """33 x 9 x 5, 34 x 10 x 6, 65 x 17 x 9: one and two voxels beyond whole 32 x 8 x 4 tiles, so a tile's last voxel and its
    neighbour, the owner of an edge and the edge's far end, fall into different workgroups, and the last tiles are ragged."""
    vol, wants = _seams(dims, colour)
    volume = _load(vol)
    for min_weight in (0, 2):
        _assert_every_seam_is_crossed(vol, min_weight)
        expected = wants[min_weight]
        records = volume.extract(min_weight)
        assert volume.count(min_weight) == records.shape[0] == len(expected)
        assert np.array_equal(ref.sort_records(records.cpu().numpy()), expected)
        assert (expected[:, 3:].max() > 100) if colour else (not expected[:, 3:].any())
    assert len(wants[2]) < len(wants[0])


@pytest.mark.parametrize("dims,axis", [((40, 1, 9), 0), ((1, 9, 9), 1), ((9, 9, 1), 0)])
def test_extract_of_a_volume_one_voxel_thick(hip_lib, dims, axis):
    vol = ref.slab(dims, axis)
    expected = ref.sort_records(ref.extract(vol))
    assert len(expected) >= 9
    assert np.array_equal(ref.sort_records(_load(vol).extract().cpu().numpy()), expected)


def test_extract_with_a_capacity_below_the_count_writes_nothing_beyond_it(hip_lib):
    vol, wants = _seams((65, 17, 9), True)
    n = len(wants[0])
    volume = _load(vol)
    capacity = n // 3
    records = torch.full((n, 6), -7.0, dtype=torch.float32, device=DEV)
    cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().mr_tsdf_extract_f32(*volume._volume_args(), volume._origin, volume.voxel_size, 0.0, records.data_ptr(), capacity,
                                               cursor.data_ptr(), torch.cuda.current_stream().cuda_stream), "extract")
    assert int(cursor.item()) == n and capacity > 50
    assert bool((records[capacity:] == -7).all()) and not bool((records[:capacity, :3] == -7).any())
    known = {r.tobytes() for r in wants[0]}
    assert all(r.tobytes() in known for r in records[:capacity].cpu().numpy())


def test_extract_equals_the_mesh_vertices_on_the_axis_edges(hip_lib):
    """The header's promise on a seam volume: the points are the mesh's vertices on the edges e < 3, bit for bit."""
    vol, wants = _seams((65, 17, 9), True)
    volume = _load(vol)
    for min_weight in (0, 2):
        want = mref.mesh(vol, min_weight)
        diagonal = want["vertices"][want["keys"][:, 3] >= 3]
        assert np.array_equal(ref.sort_records(mref.axis_vertices(want)), wants[min_weight]) and len(diagonal) > 100
        points = volume.extract(min_weight).cpu().numpy()
        vertices = volume.mesh(min_weight)[0].cpu().numpy()
        assert np.array_equal(ref.sort_records(points), wants[min_weight])
        assert np.array_equal(ref.sort_records(np.concatenate([points, diagonal])), ref.sort_records(vertices))


# ------------------------------------------------------------------------------------------ 5. a directory of the export
def test_fuse_directory_equals_integrating_the_packed_arrays(hip_lib, tmp_path):
    """TSDFExporter writes the scene's keyframes (inverse depth and [-.5, .5] colour on the device, as the model hands them over);
    fusing the directory gives the tsdf / weight of integrating what pack_frames packed with the poses inverted, written, read and
    inverted again.  The colour went through JPEG: it is compared against the restatement fed the decoded files."""
    frames = _frames()                                                      # eleven: the reader's second chunk of eight is used
    h, w = frames[0][1].shape
    packed = []
    with tx.TSDFExporter(tmp_path, h, w, min_distance=0.5, max_distance=30, ring=3, workers=2) as exporter:
        for i, (pose, depth_cm, image) in enumerate(frames):
            with np.errstate(divide="ignore"):
                inv = torch.from_numpy(np.where(depth_cm > 0, 100.0 / depth_cm.astype(np.float64), 0.0).astype(np.float32)).to(DEV)
            keyframe = (torch.from_numpy(image).permute(2, 0, 1).float() / 255 - 0.5).to(DEV)
            exporter.add(10 * i, keyframe, inv, torch.from_numpy(pose))     # numbers 0, 10, .. 100
            depth, colour, _ = tx.pack_frames(inv, keyframe, None, 0.5, 30)
            packed.append((depth[0].clone(), colour[0].clone()))
    tx.save_intrinsics_for_tsdf(tmp_path, K3)
    assert sum(int((d > 0).sum()) for d, _ in packed) > 0.5 * 10 * h * w
    fused = tf.fuse_directory(tmp_path, volume=_volume("small"))
    assert fused.frames == 11
    listed = tf.list_export_directory(tmp_path)
    assert [n for n, _ in listed] == list(range(0, 110, 10))
    read = [tf.read_export_frame(base) for _, base in listed]
    direct = _volume("small")
    want = ref.new_volume(**ref.SMALL)
    for (depth, colour), (file_depth, file_colour, cam_to_world), (pose, _, _) in zip(packed, read, frames):
        again = torch.inverse(torch.from_numpy(np.loadtxt(io.StringIO(_savetxt(torch.inverse(torch.from_numpy(pose)).numpy()))).astype(np.float32)))
        assert torch.equal(again, cam_to_world) and np.array_equal(file_depth, depth.cpu().numpy())
        direct.integrate(depth, colour, again, K3)
        ref.integrate(want, ref.world_to_camera(cam_to_world.numpy()), K, file_depth, file_colour)
    assert torch.equal(fused.tsdf, direct.tsdf) and torch.equal(fused.weight, direct.weight) and bool((fused.weight > 0).any())
    _assert_equal(fused, want)
    assert not torch.equal(fused.colour, direct.colour)                    # JPEG is lossy
    sized = tf.fuse_directory(tmp_path, voxel_size=0.25, max_depth_m=4.0, device=DEV)
    assert bool((sized.weight > 0).any()) and sized.origin[2] <= 0 and min(sized.dims) > 4


def _savetxt(matrix):
    buffer = io.StringIO()
    np.savetxt(buffer, matrix)
    return buffer.getvalue()


# ------------------------------------------------------------------------------------------ 6. the runner
STEPS, KEYFRAMES = 16, 9


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return synth.make_kitti_tree(tmp_path_factory.mktemp("kitti"), sequences=(("03", 120, 400),), frames=20)


@pytest.fixture(scope="module")
def model(hip_lib):
    from monorec_amd import MonoRecModel
    m = MonoRecModel(cv_depth_steps=STEPS, hip_in_flight=4)
    sd = synth.seeded_state_dict(m.state_dict(), seed=0)
    sd["att_module.classifier.0.bias"] = sd["att_module.classifier.0.bias"] - 5.0          # a vote that keeps some pixels (test_gpu_tsdf_export.py)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _config(tree, out_dir, use_mask, fuse_batch):
    args = dict(dataset_dir=tree, sequences=["03"], depth_folder="image_depth_annotated", target_image_size=[64, 96], frame_count=2,
                lidar_depth=True, dso_depth=False, use_dso_poses=True)
    return {"name": "TSDF fusion", "n_gpu": 1, "roi": [4, 60, 8, 92], "start": 0, "end": KEYFRAMES, "min_d": 3, "max_d": 30,
            "use_mask": use_mask, "output_dir": str(out_dir), "voxel_size": 0.5, "trunc_voxels": 3, "fuse_batch": fuse_batch,
            "file_name": "surface.ply", "save_volume": os.path.join(str(out_dir), "volume.npz"),
            "arch": {"type": "MonoRecModel", "args": {"pretrain_mode": 0, "cv_depth_steps": STEPS}},
            "data_set": {"type": "KittiOdometryDataset", "args": args}}


_LOOPS = {}


def _one_at_a_time(config, model, geometry):
    """model(data) -> pack_frames -> integrate, one keyframe at a time with owned outputs and the vote as the unfused torch expression,
    into a volume of the runner's geometry.  Computed once per `use_mask`."""
    key = config["use_mask"]
    if key in _LOOPS:
        return _LOOPS[key]
    from monorec_amd import kitti
    from monorec_amd.pointcloud import static_mask
    dataset = kitti.KittiOdometryDataset(**dict(config["data_set"]["args"], device=DEV))
    loader = kitti.DeviceLoader(dataset, batch_size=1, start=config["start"], end=config["end"])
    volume = tf.TSDFVolume(origin=geometry["origin"], dims=geometry["dims"], voxel_size=config["voxel_size"],
                           trunc=config["voxel_size"] * config["trunc_voxels"], device=DEV)
    crop, lo, hi = config["roi"], config["min_d"], config["max_d"]
    buffer, fused = [], 0
    with torch.no_grad():
        for data, _ in loader:
            out = model(data)
            k = data["keyframe_intrinsics"][0].clone()
            k[0, 2] -= crop[2]
            k[1, 2] -= crop[0]
            entry = dict(keyframe=data["keyframe"].clone(), depth=out["result"].clone(), pose=data["keyframe_pose"][0],
                         mask=static_mask(out["cv_mask"], 32), k=k)
            if config["use_mask"]:
                buffer.append(entry)
                if len(buffer) < 5:
                    continue
                mask = (torch.sum(torch.stack([e["mask"] for e in buffer]), dim=0) > 5 - 1).to(dtype=torch.float32)
                entry = dict(buffer[2], depth=buffer[2]["depth"] * mask)
                del buffer[0]
            depth, colour, _ = tx.pack_frames(entry["depth"], entry["keyframe"], crop, lo, hi)
            volume.integrate(depth[0], colour[0], entry["pose"], entry["k"])
            fused += 1
    dataset.close()
    _LOOPS[key] = (volume.grids(), fused)
    return _LOOPS[key]


@pytest.mark.parametrize("fuse_batch", [1, 3])
@pytest.mark.parametrize("use_mask", [True, False])
def test_runner_equals_the_one_at_a_time_loop(tree, model, tmp_path, use_mask, fuse_batch):
    config = _config(tree, tmp_path, use_mask, fuse_batch)
    count = tf.run(config, model=model)
    with np.load(config["save_volume"]) as z:
        got = {k: z[k] for k in z.files}
    assert int(got["frames"]) == (KEYFRAMES - 4 if use_mask else KEYFRAMES)
    assert got["tsdf"].shape == tuple(int(d) for d in got["dims"][::-1]) and min(got["dims"]) > 4 and got["weight"].max() > 1
    (tsdf, weight, colour), fused = _one_at_a_time(config, model, dict(origin=got["origin"], dims=got["dims"]))
    assert fused == int(got["frames"])
    assert np.array_equal(got["weight"], weight) and np.array_equal(got["tsdf"], tsdf) and np.array_equal(got["colour"], colour)
    lines, body = _ply(open(tmp_path / "surface.ply", "rb").read())
    assert lines[2] == f"element vertex {count}" and len(body) == 24 * count and count > 0
    want = ref.extract(dict(dims=tuple(int(d) for d in got["dims"]), origin=tuple(got["origin"]), voxel=np.float32(got["voxel_size"]),
                            tsdf=tsdf, weight=weight, colour=colour))
    assert np.array_equal(ref.sort_records(np.frombuffer(body, "<f4")), ref.sort_records(want))
