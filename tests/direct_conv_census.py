"""Census of the mr_conv2d_f32 instantiations the measured tables launch (host side, no GPU).

Every plan shape the tables were measured for is built on the CPU device; every conv_log entry that is a launch of the direct MFMA
kernel (csrc/conv_mfma.hip) is reduced to an INSTANTIATION KEY - what the compiled code of that launch depends on - and one spatially
shrunken representative per key is kept.  tests/test_direct_conv_census.py pins the census, tests/test_gpu_direct_conv_sweeps.py runs
every representative alone against an fp64 reference.

The key (`Key`):
    mb, nb, wv, kws      template parameters of conv_mfma_kernel
    mode                 0 fp32, 1 bf16, 2 bf16x3 MFMA arithmetic (template parameter BF16)
    staging              "x4" dwordx4 LDS-DMA, "dw" dword LDS-DMA, "reg" register-staged (template parameter DMA_IN + a.dma_x4)
    plane                the LDS plane pitch when sweep_chunk_pipe switches to its own instantiation for it (MR_PLANE_MENU), else 0.  Only a
                         launch with a pipelined chunk reaches that switch: every other sweep (generic, K split across waves, bf16, bf16x3)
                         reads the pitch at run time, so it is no part of their compiled code and is recorded as 0
    sweeps               the sweep functions the launch's chunks take: "pipe" (ck4 % 4 == 0), "generic", "kws", "bf16", "bf16x3"
    k, stride            (KH, KW) and (SH, SW): the loop bounds of the sweep / the lane pitch of the B reads
    phases               1 or 4
    splitk               split_k > 1 (raw partial sums + finishing launch)
    dual                 MB * NB == 1 (two partial sums per accumulator)
The pitch is not modelled here: it is recovered from what the library answers (mr_conv2d_lds_bytes = nbuf * (CK * PLANE + wmax) * 4) and
cross-checked against a restatement of derive()."""
import collections
import ctypes
import functools
import math
import os
import re

from monorec_amd import _lib, engine, synth
from monorec_amd._lib import ConvDesc, IN_DIRECT, IN_MAXPOOL2, IN_UPSAMPLE2, TF_NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W, F, D) of the plans the tables were measured for; fp32 plans are built for every conv_forms, the bf16 ones as they are.
# (8, 256, 512, 2, 32) is there for the batch-8 keys of the 32-hypothesis volume and the 16-frame mask encoder; every fp32 shape is also
# built once with one_channel_kernels=False (conv_forms "direct"): the table keeps the entries of the one-channel heads - the mask
# classifier and the depth predictions - as mr_conv2d_f32 launches, which is what MR_ONE_CHANNEL_KERNELS=0 runs.
FP32_SHAPES = [(1, 256, 512, 2, 32), (2, 256, 512, 2, 32), (4, 256, 512, 2, 32), (8, 256, 512, 4, 64), (1, 320, 640, 2, 32),
               (4, 320, 640, 2, 32), (1, 480, 640, 2, 32), (1, 512, 1024, 4, 48), (8, 256, 512, 2, 32)]
BF16_SHAPES = [(1, 256, 512, 2, 32), (1, 512, 1024, 4, 48)]
CONV_FORMS = ("table", "f2", "direct")
MAX_GMAC = 0.3                      # multiply-adds of a shrunken representative (fp64 CPU reference per case)

Key = collections.namedtuple("Key", "mb nb wv kws mode staging plane sweeps k stride phases splitk dual")
Case = collections.namedtuple("Case", "key spec sched mode name sig origin shrunk")


def key_id(key):
    """Readable pytest id of a key."""
    return (f"{('f32', 'bf16', 'bf16x3')[key.mode]}-mb{key.mb}nb{key.nb}wv{key.wv}{'kws' if key.kws else ''}-{key.staging}-pl{key.plane}-"
            f"{'+'.join(key.sweeps)}-k{key.k[0]}x{key.k[1]}s{key.stride[0]}x{key.stride[1]}-p{key.phases}{'-splitk' if key.splitk else ''}"
            f"{'-dual' if key.dual else ''}")


def _source():
    with open(os.path.join(ROOT, "monorec_amd", "csrc", "conv_mfma.hip")) as f:
        return f.read()


@functools.lru_cache(None)
def plane_menu():
    """The pitches MR_PLANE_MENU instantiates the pipelined sweep for, read from the kernel source."""
    m = re.search(r"#define MR_PLANE_MENU\(X\)((?:\s*X\(\d+\))+)", _source())
    return tuple(int(v) for v in re.findall(r"X\((\d+)\)", m.group(1)))


@functools.lru_cache(None)
def _limits():
    src = _source()
    return int(re.search(r"#define MR_MAX_G4 (\d+)", src).group(1)), int(re.search(r"#define MR_MAX_PPT (\d+)", src).group(1))


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):           # like the hip_lib fixture: hipcc cross-compiles without a GPU
        from monorec_amd import build
        build.build()
    return _lib.load()


def unpack_schedule(sched):
    """(mb, nb, split_k, ck, waves, kws) of a table entry / override (waves and kws default to 4 and 0)."""
    mb, nb, split_k, ck = (int(v) for v in sched[:4])
    return mb, nb, split_k, ck, (int(sched[4]) if len(sched) > 4 else 4), (1 if len(sched) > 5 and sched[5] else 0)


def src_channels_of(spec):
    return [int(s[1]) for s in spec["src_shapes"]]


def descriptor(spec, sched, mode):
    """The mr_conv_desc Plan.conv builds for `spec` under `sched`, with placeholder pointers: enough for mr_conv2d_lds_bytes."""
    mb, nb, split_k, ck, waves, kws = unpack_schedule(sched)
    cout, cin, kh, kw = spec["w_shape"]
    d = ConvDesc()
    n, _, hs, ws = spec["src_shapes"][0]
    for i, c in enumerate(src_channels_of(spec)):
        d.src[i], d.src_channels[i] = 1, c
    d.num_src, d.batch, d.src_h, d.src_w = len(spec["src_shapes"]), n, hs, ws
    d.in_mode, d.in_transform = spec["in_mode"], spec["tf"]
    d.kh, d.kw, d.stride_h, d.stride_w, d.pad_top, d.pad_left = kh, kw, spec["stride"][0], spec["stride"][1], spec["pad"][0], spec["pad"][1]
    d.out_h, d.out_w = spec["grid"]
    d.dst, d.out_channels, d.dst_total_channels, d.dst_channel_offset = 1, cout, spec["out_shape"][1], 0
    d.dst_plane_h, d.dst_plane_w = spec["out_shape"][2], spec["out_shape"][3]
    d.out_step_h, d.out_step_w, d.out_off_h, d.out_off_w = spec["out_step"][0], spec["out_step"][1], spec["out_off"][0], spec["out_off"][1]
    phases = spec["phases"]
    d.num_phases = 1 if phases is None else len(phases)
    for i, (pt, pl, oh, ow, pkh, pkw) in enumerate(phases or ()):
        d.phase_pad_top[i], d.phase_pad_left[i], d.phase_out_off_h[i], d.phase_out_off_w[i] = pt, pl, oh, ow
        d.phase_kh[i], d.phase_kw[i], d.phase_weights[i] = pkh, pkw, 1
    d.activation, d.act_p0, d.act_p1 = spec["act"], spec["p0"], spec["p1"]
    d.compute_dtype = int(mode)
    d.cout_blocks_per_wg, d.pixel_blocks_per_wave, d.split_k, d.chunk_channels = mb, nb, split_k, ck
    d.waves_per_wg, d.k_split_waves = waves, kws
    d.workspace = 1 if split_k > 1 else None
    d.packed_weights = 1
    return d


def geometry(spec, sched, mode):
    """Restatement of derive() (csrc/conv_mfma.hip) for one launch: tile shape, staging form, plane pitch, chunk list, LDS buffers."""
    mb, nb, split_k, ck, waves, kws = unpack_schedule(sched)
    cout, cin, kh, kw = spec["w_shape"]
    (sh, sw), (out_h, out_w) = spec["stride"], spec["grid"]
    ws = spec["src_shapes"][0][3]
    max_g4, max_ppt = _limits()
    blocks = nb if kws else waves * nb
    twb = 2 if (out_w >= 32 and blocks >= 2) else 1
    th = blocks // twb
    ih, iw = (th - 1) * sh + kh, (twb * 16 - 1) * sw + kw
    dma_in = spec["in_mode"] != IN_MAXPOOL2 and spec["tf"] == TF_NONE
    dma_x4 = dma_in and spec["in_mode"] == IN_DIRECT and ws % 4 == 0
    pads_left = [spec["pad"][1]] if spec["phases"] is None else [p[1] for p in spec["phases"]]
    xsh = max((4 - (pl & 3)) & 3 for pl in pads_left) if dma_x4 else 0
    iwa = (xsh + iw + 3) & ~3 if dma_x4 else iw
    if dma_x4 and math.ceil(ih * (iwa >> 2) / 64) > max_g4:
        dma_x4, iwa = False, iw
    plane = ih * iwa
    if sw == 1:
        while plane % 32 != 16:
            plane += 1
    elif dma_x4:
        plane = (plane + 3) & ~3
    else:
        plane |= 1
    unit = 16 if mode else 4
    cpads = [(c + unit - 1) // unit * unit for c in src_channels_of(spec)]
    chunks = [min(ck, cp - c0) for cp in cpads for c0 in range(0, cp, ck)]
    nbuf = 2 if math.ceil(len(chunks) / split_k) > 1 else 1
    wmax = kh * kw * max(min(cp, ck) for cp in cpads) * mb * (8 if mode == 1 else 16)
    floor = waves * mb * nb * 1024 if kws else 0
    return dict(twb=twb, th=th, tile=(th, twb * 16), staging="x4" if dma_x4 else ("dw" if dma_in else "reg"), plane=plane, chunks=chunks,
                nbuf=nbuf, wmax=wmax, lds=max(nbuf * (ck * plane + wmax) * 4, floor), floor=floor, ck=ck)


def library_plane(spec, sched, mode):
    """The plane pitch the LIBRARY chose for the launch (mr_conv2d_lds_bytes inverted), or None where the reduction scratch of a
    K-split-wave launch is larger than its pipeline buffers and hides it; raises ValueError when the library rejects the launch."""
    lds = int(_lib_loaded().mr_conv2d_lds_bytes(ctypes.byref(descriptor(spec, sched, mode))))
    if lds < 0:
        raise ValueError(f"mr_conv2d_lds_bytes: {lds}")
    g = geometry(spec, sched, mode)
    if g["floor"] and lds == g["floor"] and g["floor"] > g["nbuf"] * (g["ck"] * g["plane"] + g["wmax"]) * 4:
        return None
    floats, rem = divmod(lds, 4 * g["nbuf"])
    plane, rem2 = divmod(floats - g["wmax"], g["ck"])
    assert rem == 0 and rem2 == 0 and plane > 0, (lds, g)
    assert plane == g["plane"] and lds == g["lds"], ("derive() restated wrongly", spec, sched, plane, g)
    return plane


def launch_key(spec, sched, mode):
    """Instantiation key of one launch (module docstring)."""
    mb, nb, split_k, ck, waves, kws = unpack_schedule(sched)
    g = geometry(spec, sched, mode)
    plane = library_plane(spec, sched, mode)
    if kws:
        sweeps = ("kws",)
    elif mode:
        sweeps = (("bf16", "bf16x3")[mode - 1],)
    else:
        sweeps = tuple(sorted({"pipe" if (c >> 2) % 4 == 0 else "generic" for c in g["chunks"]}, key=("pipe", "generic").index))
    cout, cin, kh, kw = spec["w_shape"]
    return Key(mb, nb, waves, kws, int(mode), g["staging"], plane if ("pipe" in sweeps and plane in plane_menu()) else 0, sweeps, (kh, kw),
               tuple(spec["stride"]), 1 if spec["phases"] is None else len(spec["phases"]), split_k > 1, mb * nb == 1)


def is_direct_launch(c):
    """conv_log entry of a mr_conv2d_f32 launch: no reduced-multiply (winograd) and no B8 family key."""
    return "winograd" not in c and not c.get("b8")


def _macs(spec):
    cout, cin, kh, kw = spec["w_shape"]
    taps = kh * kw if spec["phases"] is None else sum(p[4] * p[5] for p in spec["phases"])
    return spec["src_shapes"][0][0] * spec["grid"][0] * spec["grid"][1] * cout * cin * taps


def resized(spec, out_h, out_w, batch):
    """`spec` at another output grid / batch: the sources follow the grid by the layer's own relation (stride, 2x2 max-pool, x2
    upsampling), the destination plane by its output step; channels, filter, stride, pad, modes, activation, residual, phases unchanged."""
    n, _, hs, ws = spec["src_shapes"][0]
    (sh, sw), (gh, gw) = spec["stride"], spec["grid"]
    mode = spec["in_mode"]
    hin, win = {IN_UPSAMPLE2: (2 * hs, 2 * ws), IN_MAXPOOL2: (hs // 2, ws // 2)}.get(mode, (hs, ws))
    nh, nw = out_h * sh - (gh * sh - hin), out_w * sw - (gw * sw - win)          # input plane of the convolution
    if mode == IN_UPSAMPLE2:
        if nh % 2 or nw % 2:
            return None
        nh, nw = nh // 2, nw // 2
    elif mode == IN_MAXPOOL2:
        nh, nw = 2 * nh, 2 * nw
    if nh < 1 or nw < 1:
        return None
    oh = out_h * spec["out_step"][0] + (spec["out_shape"][2] - gh * spec["out_step"][0])
    ow = out_w * spec["out_step"][1] + (spec["out_shape"][3] - gw * spec["out_step"][1])
    return dict(spec, src_shapes=[(batch, int(s[1]), nh, nw) for s in spec["src_shapes"]], grid=(out_h, out_w),
                out_shape=(batch, spec["out_shape"][1], oh, ow))


def shrink(spec, sched, mode, key):
    """A representative of `key` with about two tiles and a ragged remainder in each direction, batch 2: the first candidate grid
    whose key - re-derived through the library - is `key` and whose multiply-adds stay below MAX_GMAC (fewer tiles, then batch 1, where
    two tiles are too many).  None when no candidate keeps the key: the case then runs at its original size with batch 1."""
    g = geometry(spec, sched, mode)
    th, tw = g["tile"]
    ws = spec["src_shapes"][0][3]
    # row / column counts by preference: two tiles + remainder, then one tile + remainder (a one-row tile has no ragged remainder)
    rows = [[2 * th + r for r in range(th // 2 + 1, th)] + [2 * th + r for r in range(1, th // 2 + 1)],
            [th + r for r in range(th // 2 + 1, th)] + [th + r for r in range(1, th // 2 + 1)]] if th > 1 else [[3], [2]]
    if spec["grid"][1] >= 32:          # out_w >= 32 is what gave the schedule its tile shape (TWB): stay on that side of it
        cols = [[c for c in range(2 * tw + 1, 3 * tw) if c >= 32], [c for c in range(tw + 1, 2 * tw) if c >= 32]]
    else:
        cols = [list(range(17, 32)), list(range(1, 16))]
    best = None
    for batch in (2, 1):
        for ri, ci in ((0, 0), (0, 1), (1, 0), (1, 1)):
            found = None
            for oh in rows[ri]:
                for ow in cols[ci]:
                    cand = resized(spec, oh, ow, batch)
                    if cand is None or cand["src_shapes"][0][3] % 4 != ws % 4:
                        continue
                    try:
                        if launch_key(cand, sched, mode) == key:
                            found = cand
                            break
                    except ValueError:
                        continue
                if found is not None:
                    break
            if found is None:
                continue
            if _macs(found) <= MAX_GMAC * 1e9:
                return found
            if best is None or _macs(found) < _macs(best):
                best = found
    return best


@functools.lru_cache(None)
def launches():
    """[(spec, schedule, arithmetic mode, layer name, signature, origin)] of every mr_conv2d_f32 launch of the census plans."""
    from monorec_amd import MonoRecModel
    _lib_loaded()
    out, states = [], {}
    builds = ([(s, 0, f, True) for s in FP32_SHAPES for f in CONV_FORMS] + [(s, m, "table", True) for m in (1, 2) for s in BF16_SHAPES] +
              [(s, 0, "direct", False) for s in FP32_SHAPES])
    for (b, h, w, f, d), mode, forms, heads in builds:
        if d not in states:
            states[d] = synth.seeded_state_dict(MonoRecModel(cv_depth_steps=d).state_dict())
        plan = engine.Plan(states[d], b, h, w, f, d, (0.33, 0.0025), "cpu", bf16=mode, conv_forms=forms, one_channel_kernels=heads)
        for c in plan.conv_log:
            if is_direct_launch(c):
                sched = (c["mb"], c["nb"], c["split_k"], c["ck"], c["waves"], c["kws"])
                out.append((c["spec"], sched, int(c["bf16"]), c["name"], c["sig"],
                            f"b{b}_{h}x{w}_f{f}_d{d}_{('f32', 'bf16', 'bf16x3')[mode]}_{forms}{'' if heads else '_heads'}"))
    return out


@functools.lru_cache(None)
def census():
    """{key: Case}: one shrunken representative per instantiation key (the first launch that has it, in the order of `launches`)."""
    first = {}
    for spec, sched, mode, name, sig, origin in launches():
        key = launch_key(spec, sched, mode)
        if key not in first:
            first[key] = (spec, sched, mode, name, sig, origin)
    cases = {}
    for key, (spec, sched, mode, name, sig, origin) in first.items():
        small = shrink(spec, sched, mode, key)
        if small is None:
            small, shrunk = resized(spec, spec["grid"][0], spec["grid"][1], 1), False
        else:
            shrunk = True
        assert launch_key(small, sched, mode) == key, (key, small)
        cases[key] = Case(key, small, sched, mode, name, sig, origin, shrunk)
    return cases


def dense_spec(srcs_c, cout, k, stride, pad, hw, batch, act, p0=0.0, p1=0.0, in_mode=IN_DIRECT, tf=TF_NONE, residual=False):
    """`spec` of a single-phase layer written by hand (the schema of engine's conv_log): sources of `hw`, symmetric padding."""
    hin, win = {IN_UPSAMPLE2: (2 * hw[0], 2 * hw[1]), IN_MAXPOOL2: (hw[0] // 2, hw[1] // 2)}.get(in_mode, hw)
    ho, wo = (hin + 2 * pad[0] - k[0]) // stride[0] + 1, (win + 2 * pad[1] - k[1]) // stride[1] + 1
    return dict(src_shapes=[(batch, c, hw[0], hw[1]) for c in srcs_c], w_shape=(cout, sum(srcs_c), k[0], k[1]), stride=tuple(stride), pad=tuple(pad),
                grid=(ho, wo), in_mode=in_mode, tf=tf, act=act, p0=p0, p1=p1, residual=residual, out_shape=(batch, cout, ho, wo), out_step=(1, 1),
                out_off=(0, 0), phases=None)


def make_case(name, spec, sched, mode=0):
    """A hand-written case next to the census (what the tables do not launch but derive() accepts)."""
    return Case(launch_key(spec, sched, mode), spec, tuple(sched), mode, name, None, "extra", False)


def order_check_applies(case):
    """Check (c) - bit identity with an anchor schedule - is stated for fp32 launches whose outputs are ONE chain of MFMAs in chunk
    order: no split-K (partial sums meet in a finishing launch), no K split across waves, no dual partial sums (MB * NB == 1) - and
    needs a second schedule of that kind that the library accepts for the layer."""
    k = case.key
    return k.mode == 0 and not k.splitk and not k.kws and not k.dual and anchor_schedule(case) is not None


def anchor_schedule(case):
    """Check (c): (schedule, its plane pitch) with the same chunking (ck, split_k = 1, no K split across waves), another register tile /
    workgroup size and one partial sum per accumulator (MB * NB > 1).  Its pitch is NOT in the menu (the run-time-pitch sweep) wherever
    the layer has such a schedule; a layer whose every launchable tile lands on a menu pitch (rows of >= 32 outputs with deep chunks: the
    one tile off the menu does not fit the LDS) is anchored on another instantiation - another menu pitch or, last, another tile."""
    mb0, nb0, split_k, ck, wv0, kws = unpack_schedule(case.sched)
    if split_k != 1 or kws or case.mode != 0:
        return None
    found = []
    for wv in (4, 8):
        for nb in (2, 1, 4):
            for mb in (2, 1, 3, 4, 6):
                if (mb, nb, wv) == (mb0, nb0, wv0) or mb * nb == 1:
                    continue
                sched = (mb, nb, 1, ck, wv, 0)
                try:
                    key = launch_key(case.spec, sched, 0)
                except ValueError:
                    continue
                if key.sweeps != case.key.sweeps:
                    continue
                plane = library_plane(case.spec, sched, 0)
                rank = 0 if plane not in plane_menu() else (1 if plane != case.key.plane else 2)
                found.append((rank, len(found), sched, plane))
    if not found:
        return None
    rank, _, sched, plane = min(found)
    return sched, plane


def output_owner(spec, sched, mode, co, oy, ox):
    """Where the kernel computes output (co, oy, ox) of the convolution grid under `sched`: tile, cout group and block, wave, pixel block."""
    mb, nb, split_k, ck, waves, kws = unpack_schedule(sched)
    g = geometry(spec, sched, mode)
    th, tw = g["tile"]
    row, colb = oy % th, (ox % tw) // 16
    pb = row * 2 + colb if g["twb"] == 2 else row
    return dict(tile=(oy // th, ox // tw), cout_group=(co // 16) // mb, cout_block=(co // 16) % mb, wave="all" if kws else pb // nb,
                pixel_block=pb if kws else pb % nb, lane=(ox % 16) + 16 * ((co % 16) // 4))
