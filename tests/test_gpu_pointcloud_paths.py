"""GPU (MI355X): every path of the point-cloud append (tests/pointcloud_paths.py; pinned by tests/test_pointcloud_paths.py) on its own through
the C ABI - `mr_pointcloud_append_f32` on a GENERAL camera (skewed K, rotation about (1, 2, 3), translation, another camera per batch element) -
and `PLYSaver` / `PointcloudBuilder` above it.

The records live in a buffer pre-filled with the sentinel bits 0x7A5A5A5A, with guard records below the base the kernel sees and beyond
`capacity`; the cursor is the first word of an int64 pair whose second word is a sentinel.
    a. on certified operands (powers of two, dyadic camera) the records equal the fp64 reference bit for bit,
    b. on uniform data the records equal `append_ref` - numpy fp32 with the kernel's roundings and an exact fmaf - bit for bit,
    c. and lie within the DERIVED 10 * 2^-24 * S of the fp64 reference (S: the absolute sum of the coordinate's terms).  Measured maximum of
       |got - ref64| / (2^-24 S) over all cases on the MI355X: 1.945 (depth/open_unmasked; MEASURED_MAX_U),
    d. nothing below the base, at or beyond `capacity`, or between the final count and `capacity` changes; no admitted record keeps the
       sentinel; *cursor = start + kept even beyond the capacity; the word after the cursor is untouched,
    e. a mismatch is reported with the record's (b, y, x), pass, wave and lane,
    f. three repetitions from the sentinel are bit-identical,
    g. non-finite and boundary depths: the decisions are the reference's, inf / NaN coordinates are compared by bits (a NaN with the canonical
       quiet NaN: the device returns 0xffc00000 for inf - inf, IEEE 754 leaves sign and payload open),
    h. refusals return MR_ERR_BAD_ARGUMENT and touch nothing."""
import ctypes
import io

import numpy as np
import pytest
import torch

import pointcloud_paths as pc
from monorec_amd import _lib
from oracle import monorec_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x7A5A5A5A
CURSOR_SENT = 0x7A5A5A5A7A5A5A5A
GUARD = 8                               # records: 192 bytes, so guard and base are both 16-byte aligned
MEASURED_MAX_U = 1.945                  # c. on the MI355X, the largest |got - ref64| / (2^-24 S) of any case (bound: 10)
_param = lambda cases: pytest.mark.parametrize("case", cases, ids=pc.ids(cases))          # noqa: E731


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True)).to(DEV)


class Launch:
    """The device operands of one call and the guarded outputs."""

    def __init__(self, ops):
        self.ops = ops
        self.inv_depth, self.image, self.kinv, self.pose = (_dev(ops[k]) for k in ("inv_depth", "image", "kinv", "pose"))
        self.masks = [_dev(m) for m in ops["masks"]]
        self.uniform = None if ops["uniform"] is None else _dev(ops["uniform"])
        self.capacity = ops["capacity"]
        self.ptrs = (ctypes.c_void_p * max(len(self.masks), 1))(*[m.data_ptr() for m in self.masks])
        self.roi = (ctypes.c_int32 * 4)(*ops["roi"]) if ops["roi"] is not None else None
        self.reset()

    def reset(self):
        self.backing = torch.full(((2 * GUARD + self.capacity) * 6,), SENT, dtype=torch.int32, device=DEV)
        self.base = self.backing.data_ptr() + GUARD * 24
        assert self.backing.data_ptr() % 16 == 0 and self.base % 16 == 0
        self.cursor = torch.tensor([self.ops["start"], CURSOR_SENT], dtype=torch.int64, device=DEV)

    def args(self, **over):
        o = self.ops
        a = dict(inv_depth=self.inv_depth.data_ptr(), ptrs=self.ptrs, num_masks=len(self.masks), vote_above=float(o["vote_above"]), image=self.image.data_ptr(),
                 kinv=self.kinv.data_ptr(), pose=self.pose.data_ptr(), uniform=None if self.uniform is None else self.uniform.data_ptr(),
                 dropout=float(o["dropout"]), min_d=float(o["min_d"]), max_d=float(o["max_d"]), roi=self.roi, b=o["b"], h=o["h"], w=o["w"], records=self.base,
                 capacity=self.capacity, cursor=self.cursor.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        a.update(over)
        return list(a.values())

    def run(self, lib, **over):
        return lib.mr_pointcloud_append_f32(*self.args(**over))

    def read(self):
        torch.cuda.synchronize()
        out = self.backing.cpu().numpy().view(np.uint32).reshape(-1, 6)
        return out[:GUARD], out[GUARD:GUARD + self.capacity], out[GUARD + self.capacity:], [int(v) for v in self.cursor.cpu()]

    def untouched(self):
        lo, body, hi, cur = self.read()
        return bool((lo == SENT).all() and (body == SENT).all() and (hi == SENT).all()) and cur == [self.ops["start"], CURSOR_SENT]


def _check_footprint_and_records(launch, ref, want_bits, what):
    """d. and e.: guards, the records before the start cursor and after the last admitted one, the admitted records, the cursor pair."""
    ops = launch.ops
    lo, body, hi, cur = launch.read()
    assert (lo == SENT).all(), f"{what}: written below the base"
    assert (hi == SENT).all(), f"{what}: written at or beyond the capacity"
    start, cap = ops["start"], launch.capacity
    admitted = int(ref.admitted.sum())
    assert admitted == max(0, min(len(want_bits), cap - start))
    if admitted:
        assert (body[:start] == SENT).all(), f"{what}: a record before the start cursor changed"
        got = pc.canonical_bits(body[start:start + admitted].view(np.float32))           # (a NaN equals a NaN; everything else bit for bit)
        assert np.array_equal(got, want_bits[:admitted]), f"{what}: {pc.first_difference(got, want_bits[:admitted], ref, ops['w'])}"
        assert (got != SENT).all(), f"{what}: an admitted record keeps the sentinel"
        assert (body[start + admitted:] == SENT).all(), f"{what}: written between the final count and the capacity"
    else:
        assert (body == SENT).all(), f"{what}: nothing is admitted, yet a record changed"
    assert cur[0] == ref.cursor == start + len(want_bits), f"{what}: cursor {cur[0]}, want {ref.cursor}"
    assert cur[1] == CURSOR_SENT, f"{what}: the word after the cursor changed"
    return body


@_param(pc.certified_cases())
def test_exact_on_certified_operands(hip_lib, case):
    """a. (with d., e.): every intermediate is exact, so the kernel's fp32 records EQUAL the fp64 reference.  batch 3 runs three cameras."""
    ops = pc.operands(case, exact=True)
    ref = pc.append_ref(ops)
    r64, _ = pc.append_ref64(ops)
    want = r64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), r64)
    launch = Launch(ops)
    _lib.check(launch.run(hip_lib), "mr_pointcloud_append_f32")
    _check_footprint_and_records(launch, ref, want.view(np.uint32), f"{case.entry}/{case.name} (certified)")


@_param(pc.CASES)
def test_restatement_bound_footprint_and_determinism(hip_lib, case):
    """b., c., d., e., f., g. on uniform data with the general camera."""
    ops = pc.operands(case)
    ref = pc.append_ref(ops)
    r64, S = pc.append_ref64(ops)
    launch = Launch(ops)
    bodies = []
    for _ in range(3):
        launch.reset()
        _lib.check(launch.run(hip_lib), "mr_pointcloud_append_f32")
        bodies.append(_check_footprint_and_records(launch, ref, ref.records.view(np.uint32), f"{case.entry}/{case.name}").copy())
    assert np.array_equal(bodies[0], bodies[1]) and np.array_equal(bodies[0], bodies[2])
    admitted = int(ref.admitted.sum())
    got = bodies[0][ops["start"]:ops["start"] + admitted].view(np.float32) if admitted else np.zeros((0, 6), np.float32)
    fin = np.isfinite(r64[:admitted, :3]) & np.isfinite(S[:admitted])
    with np.errstate(all="ignore"):
        ratio = np.abs(got[:, :3].astype(np.float64) - r64[:admitted, :3]) / (pc.U * S[:admitted])
    worst = float(ratio[fin].max()) if fin.any() else 0.0
    print(f"{case.entry}/{case.name}: {admitted} of {len(ref.records)} records admitted, max |got - ref64| / (2^-24 S) = {worst:.3f}")
    assert worst <= pc.BOUND_ROUNDINGS
    if case.path.startswith("open"):
        assert np.isnan(got[:, :3]).any() and np.isinf(got[:, :3]).any()                  # g.: inf / NaN coordinates were compared by bits above
        print("  NaN patterns on the device:", sorted({hex(int(v)) for v in got[:, :3].view(np.uint32)[np.isnan(got[:, :3])]}))


def test_refusals_touch_nothing(hip_lib):
    """h. every refusal returns MR_ERR_BAD_ARGUMENT before anything is launched."""
    c = pc.constants()
    case = next(k for k in pc.cases_of("masks") if k.path == "n5-hits2")
    launch = Launch(pc.operands(case))
    many = (ctypes.c_void_p * (c["max_masks"] + 1))(*[launch.masks[0].data_ptr()] * (c["max_masks"] + 1))
    holed = (ctypes.c_void_p * 5)(*[m.data_ptr() for m in launch.masks])
    holed[3] = None
    refusals = dict(too_many_masks=dict(ptrs=many, num_masks=c["max_masks"] + 1), null_mask_among_the_first=dict(ptrs=holed), negative_masks=dict(num_masks=-1),
                    null_mask_array=dict(ptrs=None), negative_capacity=dict(capacity=-1), batch_0=dict(b=0), height_0=dict(h=0), width_negative=dict(w=-3))
    refusals.update({f"null_{k}": {k: None} for k in ("inv_depth", "image", "kinv", "pose", "records", "cursor")})
    for name, over in refusals.items():
        assert launch.run(hip_lib, **over) == c["err_bad_argument"], name
        assert launch.untouched(), name
    _lib.check(launch.run(hip_lib), "mr_pointcloud_append_f32")                            # the same launch object is sound
    assert not launch.untouched()


@pytest.mark.parametrize("name", pc.FIXTURE_CASES)
def test_kernel_against_the_reference_fixture(hip_lib, name):
    """The records the reference's own PLYSaver appended (tests/golden/pointcloud_general.npz): same pixels, same order, same colours; the
    coordinates within the derived bound of the fp64 reference (the reference's sgemm order is host-dependent) and equal to append_ref."""
    z = np.load(pc.FIXTURE)
    meta = pc.fixture_cases()[name]
    ops = dict(pc.fixture_ops(z, name, meta))
    want = z[f"{name}.records"]
    ops["capacity"] = len(want) + 5
    ref = pc.append_ref(ops)
    launch = Launch(ops)
    _lib.check(launch.run(hip_lib), "mr_pointcloud_append_f32")
    body = _check_footprint_and_records(launch, ref, ref.records.view(np.uint32), name)
    got = body[:len(want)].view(np.float32)
    assert np.array_equal(got[:, 3:].view(np.uint32), want[:, 3:].view(np.uint32))
    r64, S = pc.append_ref64(ops)
    for rec in (got, want):
        assert (np.abs(rec[:, :3].astype(np.float64) - r64[:, :3]) <= pc.BOUND_ROUNDINGS * pc.U * S).all()


# ---- PLYSaver -----------------------------------------------------------------------------------------------------------------------------------
def _case(entry, name):
    return next(c for c in pc.CASES if (c.entry, c.name) == (entry, name))


def _tensors(ops):
    b, h, w = ops["b"], ops["h"], ops["w"]
    return dict(depth=_dev(ops["inv_depth"]).view(b, 1, h, w), image=_dev(ops["image"]).view(b, 3, h, w), intrinsics=_dev(ops["intrinsics"]),
                pose=_dev(ops["pose"]).view(b, 4, 4), masks=[_dev(m).view(b, 1, h, w) for m in ops["masks"]])


def _saver(ops, **kw):
    from monorec_amd.pointcloud import PLYSaver
    kw.setdefault("roi", ops["roi"])
    return PLYSaver(ops["h"], ops["w"], min_d=ops["min_d"], max_d=ops["max_d"], batch_size=ops["b"], **kw).to(DEV)


def _records(saver):
    return np.array(saver.data, dtype=np.float32).reshape(-1, 6)


def _same(got, ref, ops, what=""):
    assert got.shape == ref.records.shape, (what, got.shape, ref.records.shape)
    assert np.array_equal(got.view(np.uint32), ref.records.view(np.uint32)), f"{what}: {pc.first_difference(got.view(np.uint32), ref.records.view(np.uint32), ref, ops['w'])}"


def test_plysaver_with_dropout_0_keeps_the_points_whose_uniform_is_exactly_zero(hip_lib):
    """The reference thins only `if self.dropout > 0` (ply_utils.py:44); torch.rand can return 0.0, and the kernel's `uniform > dropout` would
    drop such a point when handed a `uniform` under dropout 0.  add_depthmap hands it over only with dropout > 0."""
    ops = pc.operands(_case("uniform", "null"))
    t = _tensors(ops)
    u = np.random.default_rng(1).random((ops["b"], ops["h"] * ops["w"])).astype(np.float32)
    u[:, ::4] = 0.0
    assert (pc.decisions(ops)[0] & (u == 0)).sum() > 20                                   # points only the deviation would drop
    saver = _saver(ops, dropout=0)
    saver.add_depthmap(t["depth"], t["image"], t["intrinsics"], t["pose"], uniform=_dev(u).view_as(t["depth"]))
    got = _records(saver)
    want = orc.pointcloud_records(t["depth"].cpu(), t["image"].cpu(), t["intrinsics"].cpu(), t["pose"].cpu(), ops["min_d"], ops["max_d"], None, 0,
                                  torch.from_numpy(u).view_as(t["depth"]), None, 1).numpy()
    assert got.shape == want.shape and np.array_equal(got[:, 3:], want[:, 3:])
    _same(got, pc.append_ref(ops, capacity=2 ** 62), ops, "dropout 0 with zeros in uniform")


def test_plysaver_draws_its_own_uniform_like_rand_like(hip_lib):
    ops = pc.operands(_case("uniform", "dropout_075"))
    t = _tensors(ops)
    torch.manual_seed(77)
    own = _saver(ops, dropout=pc.DROPOUT)
    own.add_depthmap(t["depth"], t["image"], t["intrinsics"], t["pose"])
    torch.manual_seed(77)
    u = torch.rand_like(t["depth"])
    given = _saver(ops, dropout=pc.DROPOUT)
    given.add_depthmap(t["depth"], t["image"], t["intrinsics"], t["pose"], uniform=u)
    ref = pc.append_ref(dict(ops, uniform=u.cpu().numpy().reshape(ops["b"], -1)), capacity=2 ** 62)
    assert 0.1 < len(ref.records) / u.numel() < 0.9
    _same(_records(given), ref, ops, "uniform given")
    _same(_records(own), ref, ops, "uniform drawn by add_depthmap")


def test_plysaver_grows_from_one_record_and_drains_in_order(hip_lib):
    """capacity 1, eight appends keeping between nothing and a whole plane, .data read after the 3rd and 6th, save() twice: every record
    exactly once, in order, across the doublings and the drains."""
    base = pc.operands(_case("batch", "b1"))
    b, plane = base["b"], base["h"] * base["w"]
    rng = np.random.default_rng(3)
    frames, want = [], []
    for i, pat in enumerate(("random", "none", "all", "lane0_wave0", "random", "empty_waves_between", "all", "random")):
        inv = rng.uniform(0.02, 1.0, (b, plane)).astype(np.float32)
        if pat != "random":
            inv = np.where(pc.keep_pattern(pat, b, plane), rng.uniform(0.1, 0.6, (b, plane)).astype(np.float32), np.float32(0))
        ops = dict(base, inv_depth=inv, image=rng.uniform(-0.5, 0.5, (b, 3, plane)).astype(np.float32))
        frames.append(ops)
        want.append(pc.append_ref(ops, capacity=2 ** 62).records)
    counts = [len(r) for r in want]
    assert counts[1] == 0 and counts[2] == plane and counts[3] == 2 and len(set(counts)) >= 6, counts
    saver = _saver(base, capacity=1)
    for i, ops in enumerate(frames):
        t = _tensors(ops)
        saver.add_depthmap(t["depth"], t["image"], t["intrinsics"], t["pose"])
        if i in (2, 5):
            assert len(saver.data) == 6 * sum(counts[:i + 1])
    files = [io.BytesIO(), io.BytesIO()]
    for f in files:
        saver.save(f)
    assert files[0].getvalue() == files[1].getvalue()
    head, _, body = files[0].getvalue().partition(b"end_header\n")
    assert f"element vertex {sum(counts)}".encode() in head
    allrec = np.concatenate(want)
    assert np.array_equal(np.frombuffer(body, dtype="<u4").reshape(-1, 6), allrec.view(np.uint32))
    assert np.array_equal(_records(saver).view(np.uint32), allrec.view(np.uint32))


def test_plysaver_makes_views_and_other_types_contiguous_fp32(hip_lib):
    """A non-contiguous depth view, an fp64 image and non-contiguous masks (each needs its own contiguous copy, alive until the launch)."""
    ops = pc.operands(_case("masks", "n5_hits2"))
    t = _tensors(ops)

    def strided(x):
        wide = torch.full(x.shape[:-1] + (2 * x.shape[-1],), float("nan"), device=DEV)
        wide[..., ::2] = x
        view = wide[..., ::2]
        assert not view.is_contiguous() and torch.equal(view, x)
        return view
    saver = _saver(ops)
    saver.add_depthmap(strided(t["depth"]), t["image"].double(), t["intrinsics"], t["pose"], static_masks=[strided(m) for m in t["masks"]], min_hits=2)
    _same(_records(saver), pc.append_ref(ops, capacity=2 ** 62), ops, "views / fp64")


def test_plysaver_negative_roi_is_the_reference_slicing(hip_lib):
    ops = pc.operands(_case("batch", "b3_negative_roi"))
    assert min(ops["roi"]) < 0
    t = _tensors(ops)
    saver = _saver(ops)
    saver.add_depthmap(t["depth"], t["image"], t["intrinsics"], t["pose"])
    got = _records(saver)
    _same(got, pc.append_ref(ops, capacity=2 ** 62), ops, "negative roi")
    want = pc.oracle_records(ops).numpy()                                                 # the reference's slicing, through the oracle
    assert got.shape == want.shape and np.array_equal(got[:, 3:], want[:, 3:])


# ---- PointcloudBuilder ---------------------------------------------------------------------------------------------------------------------------
def _builder_frames(n, h=25, w=41, seed=5):
    rng = np.random.default_rng(seed)
    k4, pose, kinv = pc.general_camera(n, h, w)
    frames = []
    for i in range(n):
        cv = (rng.random((1, 1, h, w)) * 0.09).astype(np.float32)
        cv[rng.random((1, 1, h, w)) < 0.015] = 0.5                                        # a few moving pixels, dilated by the 3 x 3 box of mask_fill 2
        frames.append(dict(inv_depth=rng.uniform(0.02, 1.0, (1, h * w)).astype(np.float32), image=rng.uniform(-0.5, 0.5, (1, 3, h * w)).astype(np.float32),
                           intrinsics=k4[i:i + 1].numpy(), pose=pose[i:i + 1].numpy().reshape(1, 16), kinv=kinv[i:i + 1].numpy(), cv_mask=cv))
    return frames


def _builder_ops(frames, j, length, min_hits, use_mask, h=25, w=41):
    """The operands of the append the builder makes once frames j .. j + length - 1 are buffered: the MIDDLE keyframe, the vote over all."""
    win, key = frames[j:j + length], frames[j + length // 2]
    masks = [orc.static_mask(torch.from_numpy(f["cv_mask"]), 2).numpy().reshape(1, h * w) for f in win] if use_mask else []
    return dict(b=1, h=h, w=w, inv_depth=key["inv_depth"], masks=masks, vote_above=float(len(masks) - min_hits), image=key["image"], kinv=key["kinv"],
                pose=key["pose"], intrinsics=key["intrinsics"], uniform=None, dropout=0.0, min_d=1.5, max_d=12.0, roi=None, start=0, capacity=2 ** 62,
                min_hits=min_hits)


def _feed(builder, f, h=25, w=41):
    data = dict(keyframe_pose=_dev(f["pose"]).view(1, 4, 4), keyframe_intrinsics=_dev(f["intrinsics"]), keyframe=_dev(f["image"]).view(1, 3, h, w))
    builder.add(data, dict(result=_dev(f["inv_depth"]).view(1, 1, h, w), cv_mask=_dev(f["cv_mask"])))


@pytest.mark.parametrize("length,min_hits,use_mask", [(3, 1, True), (3, 2, True), (5, 1, True), (5, 2, True), (5, 1, False)])
def test_builder_appends_the_middle_keyframe_under_the_vote(hip_lib, length, min_hits, use_mask):
    from monorec_amd.pointcloud import PLYSaver, PointcloudBuilder
    frames = _builder_frames(length + 2)
    saver = PLYSaver(25, 41, min_d=1.5, max_d=12.0).to(DEV)
    builder = PointcloudBuilder(saver, mask_fill=2, buffer_length=length, min_hits=min_hits, use_mask=use_mask)
    for f in frames:
        _feed(builder, f)
    got = _records(saver)
    want, chain = [], []
    for j in range(3):
        ops = _builder_ops(frames, j, length, min_hits, use_mask)
        want.append(pc.append_ref(ops).records)
        chain.append(pc.oracle_records(ops).numpy())
        assert 0.05 < len(want[-1]) / (25 * 41) < 0.9, (j, len(want[-1]))                 # the vote leaves something and drops something
        other = dict(ops, inv_depth=frames[j]["inv_depth"], image=frames[j]["image"])     # the first instead of the middle keyframe: other records
        assert not np.array_equal(pc.append_ref(other).records[:, 3:], want[-1][:, 3:])
    want, chain = np.concatenate(want), np.concatenate(chain)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert chain.shape == got.shape and np.array_equal(chain[:, 3:], got[:, 3:]) and np.allclose(chain, got, rtol=1e-5, atol=1e-4)


def test_builder_with_more_masks_than_the_kernel_votes_over_raises(hip_lib):
    from monorec_amd.pointcloud import PLYSaver, PointcloudBuilder
    length = pc.constants()["max_masks"] + 1
    frames = _builder_frames(length)
    saver = PLYSaver(25, 41, min_d=1.5, max_d=12.0).to(DEV)
    builder = PointcloudBuilder(saver, mask_fill=2, buffer_length=length)
    for f in frames[:-1]:
        _feed(builder, f)
    with pytest.raises(RuntimeError, match="mr_pointcloud_append_f32"):
        _feed(builder, frames[-1])
    assert len(saver.data) == 0                                                           # and no unmasked points were appended instead
