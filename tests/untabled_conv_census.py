"""Census of the convolution launches the nearest-signature RULES choose (host side, no GPU).

The three family censuses (direct_conv_census, reduced_conv_census, b8_conv_census) build their plans for the shapes the tables were
measured for.  An input shape without table entries runs on engine.nearest_schedules / nearest_form / choose_schedule /
Plan.b8_schedule: schedules and forms measured for one layer, run on another geometry - low-resolution planes narrower than 4, not
multiples of 4, smaller than one tile.  Here every plan of UNTABLED_SHAPES is built on the CPU device, every conv_log launch is reduced
with the family's OWN launch_key (nothing is restated) and extended by what the family keys leave out on purpose:

    extended key = (family, family key, sub_rows, sub_cols[, sub_m])
        sub_rows / sub_cols   the launch's output grid is smaller than one workgroup tile in that direction (direct:
                              geometry()["tile"]; B8: derive()'s th and 32; reduced: workgroup_tile() on the kernel's plane)
        sub_m                 reduced families only: the plane is smaller than one transform tile m in a direction the form transforms

A launch of an untabled plan is NEW when its extended key is the extended key of no case of the three family censuses (their
hand-written EXTRA cases included; the flags of those cases are computed, not assumed).  One representative per new extended key is made
by the family's own shrink(); a sub-tile direction keeps the launch's own extent (it is tiny already), and a launch that is sub-tile in
both directions runs as it is at batch min(batch, 2).  Every representative's extended key is re-derived through the library and must
equal the key it stands for.  tests/test_untabled_conv_census.py pins the census and closes it over a declared domain of shapes;
tests/test_gpu_untabled_conv_forms.py runs every representative alone under its family's checks."""
import collections
import functools

import b8_conv_census as b8c
import direct_conv_census as dcc
import reduced_conv_census as rcc
from monorec_amd import engine, synth

# (B, H, W, F, D).  The first ten: legal shapes with no or partial table entries, as surveyed - H/32 or W/32 equal to 1 (32x32), odd
# (96x320, 224x224, 352x1216, 160x480), W/32 no multiple of 4 (192x448, 128x192, 1216), a batch outside {1, 2, 4, 8} at a tabled
# resolution (3 x 256x512), 1 and 3 frames.
SURVEYED_SHAPES = [(1, 192, 448, 2, 32), (1, 128, 192, 2, 8), (3, 256, 512, 2, 32), (1, 384, 1280, 2, 32), (1, 96, 320, 2, 32),
                   (1, 224, 224, 1, 16), (5, 160, 480, 3, 32), (2, 352, 1216, 2, 32), (1, 64, 64, 2, 8), (1, 32, 32, 1, 4)]
# What the closure sweep of tests/test_untabled_conv_census.py forced in: each shape of its domain whose plans launched an extended key
# outside (family censuses + the shapes above it), in the order a greedy cover picked them.  (480x1280 is also the one resolution with
# more pixels than the largest tabled one, 512x1024.)
CLOSURE_SHAPES = [(3, 480, 1280, 3, 4), (3, 128, 96, 2, 8), (5, 32, 192, 2, 4), (5, 32, 1280, 1, 4), (3, 224, 192, 3, 4), (3, 96, 64, 3, 4),
                  (1, 192, 96, 1, 32), (5, 96, 192, 3, 8), (5, 352, 224, 1, 32), (5, 64, 32, 1, 4), (5, 384, 1280, 2, 4), (5, 32, 320, 1, 8),
                  (5, 32, 224, 3, 4), (1, 64, 192, 2, 8), (5, 128, 448, 1, 8), (3, 96, 96, 1, 8), (3, 384, 224, 3, 32), (3, 32, 64, 1, 4),
                  (1, 480, 448, 1, 32), (5, 256, 320, 2, 32), (3, 96, 1216, 2, 4), (3, 32, 1216, 1, 4), (1, 256, 1216, 1, 4), (1, 64, 224, 3, 8),
                  (5, 480, 640, 3, 32), (5, 128, 1216, 1, 8), (5, 32, 448, 2, 8), (3, 480, 320, 1, 8), (3, 224, 1280, 3, 32), (1, 256, 448, 2, 4),
                  (1, 256, 224, 2, 8), (1, 128, 64, 1, 8), (1, 64, 640, 2, 4)]
UNTABLED_SHAPES = SURVEYED_SHAPES + CLOSURE_SHAPES
# bf16x3 (arithmetic mode 2) plans: the smallest, a middle and the largest of the surveyed shapes
BF16X3_SHAPES = [(1, 32, 32, 1, 4), (1, 128, 192, 2, 8), (1, 384, 1280, 2, 32)]
# (arithmetic mode, conv_forms, one_channel_kernels) of the plans built per shape
BUILDS = [(0, "table", True), (0, "f2", True), (0, "direct", True), (0, "direct", False), (1, "table", True)]
MAX_GMAC = dcc.MAX_GMAC

# family: "direct" / "reduced" / "b8"; ext: the extended key; rule: the launch's signature is in none of the tables its family reads;
# args: what the family's functions take - direct (spec, sched, mode), reduced (Launch,), b8 (spec, sched)
Launch = collections.namedtuple("Launch", "family ext rule name sig origin args")
Rep = collections.namedtuple("Rep", "family ext case launch")          # case: a Case of the family's census module


# ---- extended keys ------------------------------------------------------------------------------------------------------------------------
def direct_ext(spec, sched, mode):
    th, tw = dcc.geometry(spec, sched, mode)["tile"]
    return ("direct", dcc.launch_key(spec, sched, mode), spec["grid"][0] < th, spec["grid"][1] < tw)


def b8_ext(spec, sched):
    key = b8c.launch_key(spec, sched)
    return ("b8", key, spec["grid"][0] < b8c.derive(spec, sched)["th"], spec["grid"][1] < 32)


def reduced_ext(launch):
    rows, cols = rcc.workgroup_tile(launch)
    h, w = launch.hw
    m = rcc.form_of(launch)[0]
    if launch.family == "up":                     # four multiplies per INPUT position: no tile of several positions
        sub_m = False
    elif rcc.dims_of(launch) == 1:
        sub_m = (w if launch.axis == 0 else h) < m
    else:
        sub_m = h < m or w < m
    return ("reduced", rcc.launch_key(launch), h < rows, w < cols, sub_m)


def ext_of(launch):
    return {"direct": direct_ext, "reduced": reduced_ext, "b8": b8_ext}[launch.family](*launch.args)


def ext_id(ext):
    """Readable pytest id of an extended key."""
    family, key = ext[:2]
    base = {"direct": dcc.key_id, "reduced": rcc.key_id, "b8": b8c.key_id}[family](key)
    return base + "".join(s for s, on in zip(("-subr", "-subc", "-subm"), ext[2:]) if on)


def mode_of(ext):
    """What the pinned counts are grouped by: the arithmetic mode (direct), the kernel family (reduced), nothing (B8)."""
    return {"direct": lambda k: k.mode, "reduced": lambda k: k.family, "b8": lambda k: "b8"}[ext[0]](ext[1])


@functools.lru_cache(None)
def existing_ext():
    """{extended key} of every case the three family censuses run on the device."""
    import test_gpu_direct_conv_sweeps as direct_gpu          # its EXTRA list lives there
    out = {direct_ext(c.spec, c.sched, c.mode) for c in list(dcc.census().values()) + direct_gpu.EXTRA}
    out |= {reduced_ext(c.launch) for c in rcc.all_cases()}
    out |= {b8_ext(c.spec, c.sched) for c in b8c.all_cases()}
    return out


# ---- launches of a plan ---------------------------------------------------------------------------------------------------------------------
_states = {}


def _state(depth_steps):
    from monorec_amd import MonoRecModel
    if depth_steps not in _states:
        _states[depth_steps] = synth.seeded_state_dict(MonoRecModel(cv_depth_steps=depth_steps).state_dict())
    return _states[depth_steps]


def build_plan(shape, mode=0, forms="table", heads=True):
    dcc._lib_loaded()
    b, h, w, f, d = shape
    return engine.Plan(_state(d), b, h, w, f, d, (0.33, 0.0025), "cpu", bf16=mode, conv_forms=forms, one_channel_kernels=heads)


def origin_of(shape, mode, forms, heads):
    b, h, w, f, d = shape
    return f"b{b}_{h}x{w}_f{f}_d{d}_{('f32', 'bf16', 'bf16x3')[mode]}_{forms}{'' if heads else '_heads'}"


def reduce_launch(c, origin):
    """`Launch` of one conv_log entry."""
    if c.get("b8"):
        args = (b8c.spec_of(c), (c["mb"], c["nb"], c["waves"]))
        return Launch("b8", b8_ext(*args), c["sig"] + f"_f{int(c['f32_source'])}" not in engine.B8_SCHEDULES, c["name"], c["sig"], origin, args)
    if "winograd" in c:
        launch = rcc.launch_of(c)
        sig = c["sig"][:-2] if launch.stride2 else c["sig"]          # a stride-2 pair has ONE table key; its halves log it + "_y" / "_x"
        return Launch("reduced", reduced_ext(launch), sig not in engine.WINOGRAD and sig not in engine.WINOGRAD_F2, c["name"], c["sig"], origin, (launch,))
    args = (c["spec"], (c["mb"], c["nb"], c["split_k"], c["ck"], c["waves"], c["kws"]), int(c["bf16"]))
    return Launch("direct", direct_ext(*args), c["sig"] not in engine.TUNED, c["name"], c["sig"], origin, args)


def plan_launches(shape, mode=0, forms="table", heads=True):
    origin = origin_of(shape, mode, forms, heads)
    return [reduce_launch(c, origin) for c in build_plan(shape, mode, forms, heads).conv_log]


def builds_of(shape):
    return BUILDS + ([(2, "table", True)] if shape in BF16X3_SHAPES else [])


@functools.lru_cache(None)
def launches():
    """Every convolution launch of every plan of UNTABLED_SHAPES."""
    return [l for shape in UNTABLED_SHAPES for build in builds_of(shape) for l in plan_launches(shape, *build)]


# ---- representatives --------------------------------------------------------------------------------------------------------------------------
def _as_it_is(launch, batch):
    """The launch's own layer at batch min(its batch, `batch`)."""
    if launch.family == "reduced":
        l = launch.args[0]
        return (l._replace(batch=min(l.batch, batch)),)
    spec = launch.args[0]
    gh, gw = spec["grid"]
    resized = dcc.resized if launch.family == "direct" else b8c.resized
    return (resized(spec, gh, gw, min(spec["src_shapes"][0][0], batch)),) + tuple(launch.args[1:])


def _shrunk(launch):
    """The family's own shrink() of the launch, a sub-tile direction put back to the launch's own extent; None where shrink() finds nothing."""
    sub_rows, sub_cols = launch.ext[2:4]
    if launch.family == "reduced":                 # shrink() never makes the plane larger than the layer: a sub-tile direction stays
        return (rcc.shrink(launch.args[0]),)
    spec, sched = launch.args[:2]
    if launch.family == "direct":
        small, resized = dcc.shrink(spec, sched, launch.args[2], launch.ext[1]), dcc.resized
    else:
        small, resized = b8c.shrink(spec, sched, launch.ext[1]), b8c.resized
    if small is None:
        return None
    if launch.family == "b8" and launch.ext[1].walk and not (sub_rows or sub_cols):
        return (small,) + tuple(launch.args[1:])               # a walk representative is what b8_conv_census.shrink says it is
    # (the direct shrink() may itself go below one tile of columns where the layer's rows have fewer than 32 outputs: a direction that is
    # NOT sub-tile in the launch then takes the launch's own extent instead)
    ext_fn = direct_ext if launch.family == "direct" else b8_ext
    found = []
    for batch in sorted({small["src_shapes"][0][0], 1}, reverse=True):
        for rows in ((spec["grid"][0],) if sub_rows else (small["grid"][0], spec["grid"][0])):
            for cols in ((spec["grid"][1],) if sub_cols else (small["grid"][1], spec["grid"][1])):
                cand = resized(spec, rows, cols, batch)
                try:
                    if cand is None or ext_fn(cand, *launch.args[1:]) != launch.ext:
                        continue
                except ValueError:
                    continue
                macs = macs_of(launch.family, (cand,))
                found.append((macs > MAX_GMAC * 1e9, -batch if macs <= MAX_GMAC * 1e9 else 0, macs, len(found), cand))
    # below MAX_GMAC at the larger batch where there is such a candidate, else the cheapest
    return None if not found else (min(found)[4],) + tuple(launch.args[1:])


def macs_of(family, args):
    return {"direct": lambda: dcc._macs(args[0]), "reduced": lambda: rcc.macs(args[0]), "b8": lambda: b8c.macs(args[0])}[family]()


def representative(launch):
    """`Rep` of the launch's extended key; its key is re-derived through the library."""
    ext_fn = {"direct": direct_ext, "reduced": reduced_ext, "b8": b8_ext}[launch.family]
    args = None
    if not (launch.ext[2] and launch.ext[3]):
        args = _shrunk(launch)
        try:
            if args is not None and ext_fn(*args) != launch.ext:
                args = None
        except ValueError:
            args = None
    if args is None:
        args = _as_it_is(launch, 2)
        if not (launch.ext[2] and launch.ext[3]) and macs_of(launch.family, args) > MAX_GMAC * 1e9:
            args = _as_it_is(launch, 1)
    assert ext_fn(*args) == launch.ext, (ext_id(launch.ext), launch.name, launch.origin)
    key = launch.ext[1]
    if launch.family == "direct":
        case = dcc.Case(key, args[0], tuple(args[1]), args[2], launch.name, launch.sig, launch.origin, args[0]["grid"] != launch.args[0]["grid"])
    elif launch.family == "reduced":
        case = rcc.Case(key, args[0], launch.name, launch.sig, launch.origin)
    else:
        case = b8c.Case(key, args[0], tuple(args[1]), launch.name, launch.sig, launch.origin)
    return Rep(launch.family, launch.ext, case, launch)


def _weight(launch):
    """What a representative of the launch costs per output position it cannot shed: multiply-adds per output x the extent of the
    sub-tile directions (they keep their size)."""
    if launch.family == "reduced":
        l = launch.args[0]
        per, (gh, gw) = l.cout * sum(l.srcs_c) * rcc.taps_of(l), l.hw
    else:
        spec = launch.args[0]
        per, (gh, gw) = macs_of(launch.family, launch.args) // (spec["src_shapes"][0][0] * spec["grid"][0] * spec["grid"][1]), spec["grid"]
    return per * (gh if launch.ext[2] else 1) * (gw if launch.ext[3] else 1)


@functools.lru_cache(None)
def census():
    """{extended key: Rep} of the NEW extended keys, in the order `launches` meets them; each stands on the cheapest launch that has
    it (`_weight`; the first of equals): the 512-channel layers of the encoder share most of their keys with lighter layers."""
    have, pick = existing_ext(), {}
    for l in launches():
        if l.ext not in have and (l.ext not in pick or _weight(l) < _weight(pick[l.ext])):
            pick[l.ext] = l
    return {ext: representative(l) for ext, l in pick.items()}


def cases(family):
    return [r for r in census().values() if r.family == family]


def rep_args(rep):
    c = rep.case
    return {"direct": lambda: (c.spec, c.sched, c.mode), "reduced": lambda: (c.launch,), "b8": lambda: (c.spec, c.sched)}[rep.family]()


def device_bytes(rep):
    """Upper bound of what the representative's GPU test holds on the device at once: sources (fp32, and a second copy in the other
    layout for B8), destination with its guards (as fp32), residual, weights per phase, split-K workspace."""
    c = rep.case
    if rep.family == "reduced":
        l = c.launch
        n, (h, w) = l.batch, l.hw
        up = 4 if l.family in ("t22", "up") else 1
        dst = n * (l.cout + 6) * h * w * up
        return 4 * (2 * n * sum(l.srcs_c) * h * w + dst * (2 if l.residual else 1) + 40 * l.cout * sum(l.srcs_c))
    spec = c.spec
    cout, cin, kh, kw = spec["w_shape"]
    n = spec["src_shapes"][0][0]
    src = sum(s[0] * s[1] * s[2] * s[3] for s in spec["src_shapes"])
    if rep.family == "b8":
        dst = n * (cout + 8) * (spec["grid"][0] * spec["out_step"][0] + 2) * (spec["grid"][1] * spec["out_step"][1] + 3)
        return 4 * (2 * src + dst + 4 * cout * cin * kh * kw)
    dst = n * (cout + 6) * spec["out_shape"][2] * spec["out_shape"][3]
    nph = 1 if spec["phases"] is None else len(spec["phases"])
    ws = c.sched[2] * nph * n * ((cout + 15) // 16 * 16) * spec["grid"][0] * spec["grid"][1] if c.key.splitk else 0
    return 4 * (src + dst * (2 if spec["residual"] else 1) + ws + 4 * cout * cin * kh * kw)


def sub_tile(launch):
    return any(launch.ext[2:])


# ---- the declared domain of the closure sweep -------------------------------------------------------------------------------------------------
SWEEP_H = (32, 64, 96, 128, 192, 224, 256, 352, 384, 480)
SWEEP_W = (32, 64, 96, 192, 224, 320, 448, 512, 640, 1216, 1280)
SWEEP_BUILDS = [(0, "table", True), (1, "table", True)]


def sweep_shapes():
    """One (B, H, W, F, D) per (H, W) of the domain (W >= H / 2), by ascending area; batch in {1, 3, 5}, frames in {1, 2, 3} and D in
    {4, 8, 32} rotate with periods 3, 9 and 27, so that each value meets small, middle and large planes."""
    pairs = sorted(((h, w) for h in SWEEP_H for w in SWEEP_W if 2 * w >= h), key=lambda p: (p[0] * p[1], p))
    return [((1, 3, 5)[i % 3], h, w, (1, 2, 3)[(i // 3) % 3], (4, 8, 32)[(i // 9) % 3]) for i, (h, w) in enumerate(pairs)]
