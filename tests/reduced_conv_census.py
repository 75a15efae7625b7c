"""Census of the reduced-multiply convolution launches the measured tables select (host side, no GPU).

Every fp32 plan shape the tables were measured for (direct_conv_census.FP32_SHAPES) is built on the CPU device for conv_forms "table" and
"f2"; every conv_log entry that carries `winograd` is reduced to an INSTANTIATION KEY - what the compiled code and the control flow of that
launch depend on - and one spatially shrunken representative per key is kept.  tests/test_reduced_conv_census.py pins the census,
tests/test_gpu_reduced_conv_forms.py runs every representative alone against an fp64 reference.

The families (csrc/) and their entry points:
    w22   conv_wino.hip     mr_conv3x3_winograd_f32       F(2x2,3x3): variant 0 LDS input transform, 1 register transform, 2 register
                                                          transform + 16-row workgroups for a 1..16-channel tail group
    w44   conv_wino44.hip   mr_conv3x3_winograd44_f32     F(4x4,3x3)
    w44s  conv_wino44s.hip  mr_conv3x3_winograd44s_f32    F(4x4,3x3), a tile's positions over two waves
    w44w  conv_wino44w.hip  mr_conv3x3_winograd44w_f32    F(4x4,3x3), one wave per SIMD
    t22   convt_wino.hip    mr_convt4x4s2_winograd_f32    layers.Refine as F(2x2,2x2) per output parity (variants as w22)
    f23   conv1d_wino.hip   mr_conv1d3_winograd_f32       1-D F(2,3) along x (axis 0) / y (axis 1)
    ct    conv1d_wino.hip   mr_conv1d_cooktoom_f32        Cook-Toom F(4,3) / F(2,7) / F(4,7) / F(4,4); the stride-2 halves over [even | odd] views
    up    conv1d_wino.hip   mr_upconv2x2_winograd_f32     layers.Upconv with 4 multiplies per 2x2 output block

The key (`Key`):
    family, entry        as above
    mbw                  blocks of output channels per workgroup: template parameter MBW (w22, t22, f23, ct, up); 1 for the F(4x4,3x3) kernels
    variant              w22 / t22: 0, 1 (template parameter REGB), 2 (REGB + the tail form); F(4x4,3x3): 3, 4, 5 (one kernel each)
    axis, m, r           template parameters AXIS, M, R of the 1-D kernels (-1, and the form's m and r, for the 2-D families)
    nsrc                 number of concatenated sources (the chunk loop crosses a source boundary)
    c8                   some source has C % 8 != 0 (its last chunk reads zero weights / channels past the tensor)
    cout_rem             what the LAST channel group of the launch holds of its mbw x (32 | 16) channels: "full"; "<k>b": k whole 16-channel
                         blocks and empty ones behind them ("half"); "<k>b+t": a partly filled 16-channel block ("tail"); + "/only" when
                         that group is the launch's only one
    residual, act        epilogue
    view                 strided source views (mr_wino_desc.src_row_pitch: the k x 1 stride-(2,1) half over [even rows | odd rows])
    split                mr_wino_desc.dst_split_columns (that half's result de-interleaved by column parity)

EXACTNESS.  A^T and B^T of every form are dyadic rationals and G is applied to each weight once, in double, then rounded
(monorec_amd/cooktoom.py).  With weights that are integer multiples of the least common denominator of G (its square for the 2-D forms)
and small-integer data, every transformed weight is an integer and every transformed input, product, channel sum and output is an
integer multiple of 1 / (den(A^T) den(B^T)) (squared in 2-D); fp32 evaluates these exactly, in any order, while the magnitudes times that
denominator stay below 2^24.  `exact_operands` returns such operands together with the bound max |A^T| (sum_c |U| |V|) |A| - computed from
those very operands in integer arithmetic - and accepts them when bound x denominators <= 2^23 (one bit of headroom for the intermediates
of the factored straight-line transform code).  F(4,7) has a G denominator of 90720 and cannot be certified at any usable density."""
import collections
import functools
import math
from fractions import Fraction

import torch

import direct_conv_census
from direct_conv_census import FP32_SHAPES
from monorec_amd import cooktoom, engine, synth
from monorec_amd._lib import ACT_LEAKY_RELU, ACT_NONE, ACT_RELU

CONV_FORMS = ("table", "f2")
MAX_GMAC = direct_conv_census.MAX_GMAC          # multiply-adds (of the direct sum) of a shrunken representative
EXACT_LIMIT = 2 ** 23

ENTRY = {"w22": "mr_conv3x3_winograd_f32", "w44": "mr_conv3x3_winograd44_f32", "w44s": "mr_conv3x3_winograd44s_f32",
         "w44w": "mr_conv3x3_winograd44w_f32", "t22": "mr_convt4x4s2_winograd_f32", "f23": "mr_conv1d3_winograd_f32",
         "ct": "mr_conv1d_cooktoom_f32", "up": "mr_upconv2x2_winograd_f32"}
FAMILY_OF_VARIANT = {0: "w22", 1: "w22", 2: "w22", 3: "w44", 4: "w44s", 5: "w44w"}
VARIANT_OF_FAMILY = {"w44": 3, "w44s": 4, "w44w": 5}

Key = collections.namedtuple("Key", "family entry mbw variant axis m r nsrc c8 cout_rem residual act view split")
# one launch: the kernel's (height, width) = the source plane; `srcs_c` the channels of the concatenated sources (a stride-2 half: [even | odd])
Launch = collections.namedtuple("Launch", "family mbw variant axis m r srcs_c cout hw batch act p0 residual view split stride2")
Case = collections.namedtuple("Case", "key launch name sig origin")


def key_id(key):
    """Readable pytest id of a key."""
    form = f"F{key.m}x{key.m}_{key.r}x{key.r}" if key.axis < 0 else f"F{key.m}_{key.r}{'xy'[key.axis]}"
    return (f"{key.family}-{form}-v{key.variant}mbw{key.mbw}-s{key.nsrc}{'c8' if key.c8 else ''}-co_{key.cout_rem.replace('/', '_')}-"
            f"{('none', 'relu', 'leaky')[(ACT_NONE, ACT_RELU, ACT_LEAKY_RELU).index(key.act)]}{'-res' if key.residual else ''}"
            f"{'-view' if key.view else ''}{'-split' if key.split else ''}")


def group_channels(launch):
    """Output channels of one workgroup's channel group."""
    if launch.family in ("w44", "w44s", "w44w"):
        return 32
    return (32 if launch.family in ("w22", "t22") else 16) * launch.mbw


def cout_remainder(launch):
    g = group_channels(launch)
    rem = launch.cout % g
    what = "full" if rem == 0 else f"{rem // 16}b" + ("+t" if rem % 16 else "")
    return what + ("/only" if launch.cout < g else "")


def form_of(launch):
    """(m, r) of the launch's bilinear form (per dimension)."""
    return {"w22": (2, 3), "w44": (4, 3), "w44s": (4, 3), "w44w": (4, 3), "t22": (2, 2), "up": (2, 2)}.get(launch.family, (launch.m, launch.r))


def launch_key(launch):
    m, r = form_of(launch)
    return Key(launch.family, ENTRY[launch.family], launch.mbw, launch.variant, launch.axis, m, r, len(launch.srcs_c),
               any(c % 8 for c in launch.srcs_c), cout_remainder(launch), bool(launch.residual), int(launch.act), bool(launch.view), bool(launch.split))


def launch_of(c):
    """`Launch` of a conv_log entry that carries `winograd`."""
    spec = c["spec"]
    srcs_c = tuple(int(s[1]) for s in spec["src_shapes"])
    common = dict(mbw=int(c["winograd"]), srcs_c=srcs_c, cout=int(c["cout"]), hw=tuple(c["out"]), batch=int(c["batch"]), act=int(spec["act"]),
                  p0=float(spec["p0"]), residual=bool(spec["residual"]))
    if c.get("upconv"):
        return Launch(family="up", variant=0, axis=-1, m=2, r=2, view=False, split=False, stride2=False, **common)
    if "wino_axis" in c:
        m, r, axis, s2 = int(c["wino_m"]), int(c["wino_taps"]), int(c["wino_axis"]), bool(c.get("stride2"))
        return Launch(family="f23" if (m, r) == (2, 3) else "ct", variant=0, axis=axis, m=m, r=r, view=s2 and axis == 1,
                      split=len(spec["out_shape"]) == 5, stride2=s2, **common)
    if c["phases"] == 4:
        return Launch(family="t22", variant=int(c["wino_variant"]), axis=-1, m=2, r=2, view=False, split=False, stride2=False, **common)
    fam = FAMILY_OF_VARIANT[int(c["wino_variant"])]
    m, r = (2, 3) if fam == "w22" else (4, 3)
    return Launch(family=fam, variant=int(c["wino_variant"]), axis=-1, m=m, r=r, view=False, split=False, stride2=False, **common)


def table_prefix(launch):
    """WINOGRAD key prefix of the launch's layer ('' 3x3, 't_', 'u_', 'x_' / 'y_' / 'x7_' / 'y7_'); None for a stride-2 half (its pair has one
    key, `s2k<taps>_`, and its builder fixes the activation: the half is launched through Plan._conv_winograd_1d)."""
    if launch.stride2:
        return None
    if launch.family in ("f23", "ct"):
        return engine.wino1d_prefix(launch.axis, launch.r)
    return {"t22": "t_", "up": "u_"}.get(launch.family, "")


def table_code(launch):
    """The WINOGRAD table value that decode_form turns into this launch's form."""
    if launch.family in ("w22", "w44", "w44s", "w44w", "t22"):
        return 10 * launch.variant + launch.mbw
    if launch.family == "ct":
        return 10 * launch.m + launch.mbw
    return launch.mbw


def signature(launch):
    """The WINOGRAD key the launch's builder looks up."""
    return table_prefix(launch) + engine.winograd_signature(launch.cout, list(launch.srcs_c), launch.hw[0], launch.hw[1], launch.batch)


def stride2_view(launch, base_ptr):
    """The strided source views Plan._conv_relu2_stride2 hands the k x 1 stride-(2,1) half: [even rows | odd rows] of ONE dense
    (n, c, 2 h, w) tensor at `base_ptr`, as the `view` argument of Plan._conv_winograd_1d."""
    (h, w), c = launch.hw, launch.srcs_c[0]
    return dict(ptrs=[base_ptr, base_ptr + w * 4], channels=[c, c], batch=launch.batch, height=h, width=w, row_pitch=2 * w, plane=2 * h * w)


def workgroup_tile(launch):
    """(rows, columns) of the kernel's (height, width) plane one workgroup covers.  The tail form (variant 2) covers its full groups by
    8-row and its tail group by 16-row workgroups: 16."""
    if launch.family in ("w22", "w44", "w44s", "w44w"):
        rec = engine.WINO3X3_FORMS[launch.variant]
        return (16 if rec.tail else rec.rows), rec.cols
    if launch.family == "t22":
        return (16 if launch.variant == 2 else 8), 32
    if launch.family == "ct":                       # Plan._conv_winograd_1d: 8 x 16 m outputs along x, 4 m x 32 along y
        return (8, 16 * launch.m) if launch.axis == 0 else (4 * launch.m, 32)
    return 8, 32


def taps_of(launch):
    """Multiply-adds per (kernel plane position, cout, cin) of the direct sum."""
    return {"w22": 9, "w44": 9, "w44s": 9, "w44w": 9, "t22": 16, "up": 16}.get(launch.family, launch.r)


def macs(launch):
    return launch.batch * launch.hw[0] * launch.hw[1] * launch.cout * sum(launch.srcs_c) * taps_of(launch)


def shrink(launch):
    """The representative of the launch's key: about two workgroup tiles plus a ragged remainder in each direction, batch 2 - one tile plus the
    remainder, then batch 1, where that is above MAX_GMAC; never larger than the layer itself.  The width stays a multiple of 4 (of 8 for a
    column-split / row-strided stride-2 half); channels, sources, form, activation and residual are unchanged."""
    rows, cols = workgroup_tile(launch)
    h0, w0 = launch.hw
    ragged_w = 8 if (launch.view or launch.split) else 12
    best = None
    for tiles, batch in ((2, 2), (1, 2), (1, 1)):
        cand = launch._replace(hw=(min(h0, tiles * rows + rows // 2 + 1), min(w0, tiles * cols + ragged_w)), batch=batch)
        if macs(cand) <= MAX_GMAC * 1e9:
            return cand
        if best is None or macs(cand) < macs(best):
            best = cand
    return best


@functools.lru_cache(None)
def launches():
    """[(Launch, layer name, signature, origin)] of every reduced-multiply launch of the census plans."""
    from monorec_amd import MonoRecModel
    direct_conv_census._lib_loaded()
    out, states = [], {}
    for forms in CONV_FORMS:
        for (b, h, w, f, d) in FP32_SHAPES:
            if d not in states:
                states[d] = synth.seeded_state_dict(MonoRecModel(cv_depth_steps=d).state_dict())
            plan = engine.Plan(states[d], b, h, w, f, d, (0.33, 0.0025), "cpu", conv_forms=forms)
            for c in plan.conv_log:
                if "winograd" in c:
                    out.append((launch_of(c), c["name"], c["sig"], f"b{b}_{h}x{w}_f{f}_d{d}_{forms}"))
    return out


@functools.lru_cache(None)
def census():
    """{key: Case}: one shrunken representative per instantiation key (the first launch that has it, in the order of `launches`)."""
    cases = {}
    for launch, name, sig, origin in launches():
        key = launch_key(launch)
        if key not in cases:
            small = shrink(launch)
            assert launch_key(small) == key
            cases[key] = Case(key, small, name, sig, origin)
    return cases


def make_case(name, family, srcs_c, cout, hw, batch=2, mbw=1, variant=0, axis=-1, m=None, r=None, act=ACT_LEAKY_RELU, p0=0.1, residual=False):
    """A hand-written case next to the census (what the tables do not launch but the library accepts)."""
    variant = VARIANT_OF_FAMILY.get(family, variant)
    if family in ("t22", "up"):
        act, p0 = (ACT_LEAKY_RELU, 0.1) if family == "t22" else (ACT_NONE, 0.0)         # fixed by Plan.refine / Plan.upconv
    fm, fr = (m, r) if family == "ct" else {"w22": (2, 3), "f23": (2, 3), "t22": (2, 2), "up": (2, 2)}.get(family, (4, 3))
    launch = Launch(family, mbw, variant, axis, fm, fr, tuple(srcs_c), cout, tuple(hw), batch, act, p0, residual, False, False, False)
    return Case(launch_key(launch), launch, name, None, "extra")


def _extra():
    out = []
    forms = [("w22v0", dict(family="w22", variant=0, mbw=2)), ("w22v1", dict(family="w22", variant=1, mbw=1)), ("w44", dict(family="w44")),
             ("w44s", dict(family="w44s")), ("w44w", dict(family="w44w")), ("t22v0", dict(family="t22", variant=0, mbw=2)),
             ("t22v1", dict(family="t22", variant=1, mbw=1)), ("f23x", dict(family="f23", axis=0, mbw=2)), ("f23y", dict(family="f23", axis=1, mbw=3)),
             ("ct43x", dict(family="ct", axis=0, m=4, r=3, mbw=2)), ("ct43y", dict(family="ct", axis=1, m=4, r=3, mbw=4)),
             ("ct47x", dict(family="ct", axis=0, m=4, r=7, mbw=2)), ("ct47y", dict(family="ct", axis=1, m=4, r=7, mbw=3)),
             ("up", dict(family="up", mbw=2))]
    # 3x3 variant 2 (code 21) and variant 5 (conv_wino44w) are launched by no table entry of the census plans; F(2,7) by none at all
    out.append(make_case("w22_variant2_tail", "w22", (32,), 48, (41, 76), variant=2))
    out.append(make_case("w22_variant2_tail_residual_relu", "w22", (24, 8), 80, (41, 76), variant=2, act=ACT_RELU, residual=True))
    out.append(make_case("w44w_two_tiles", "w44w", (32,), 64, (41, 140)))
    out.append(make_case("ct27x", "ct", (24,), 32, (21, 76), axis=0, m=2, r=7, mbw=2))
    out.append(make_case("ct27y", "ct", (24,), 32, (21, 76), axis=1, m=2, r=7, mbw=2))
    for tag, kw in forms:
        rows, cols = workgroup_tile(make_case("", srcs_c=(8,), cout=16, hw=(8, 8), **kw).launch)
        # a source with C % 8 != 0 (the tables have one such key: 32 + 3), ragged channels everywhere
        out.append(make_case(f"{tag}_c5+11_co40", srcs_c=(5, 11), cout=40, hw=(2 * rows + rows // 2 + 1, 2 * cols + 12), **kw))
        # lower and narrower than one workgroup tile
        out.append(make_case(f"{tag}_below_one_tile", srcs_c=(16,), cout=32, hw=(rows // 2 + 1, 12), **kw))
    for tag, kw in forms[:7] + [("w22v2", dict(family="w22", variant=2)), ("t22v2", dict(family="t22", variant=2))]:
        kw = dict(kw, mbw=1)
        rows, cols = workgroup_tile(make_case("", srcs_c=(8,), cout=12, hw=(8, 8), **kw).launch)
        out.append(make_case(f"{tag}_co12_tail_group_only", srcs_c=(10,), cout=12, hw=(rows + rows // 2 + 1, cols + 12), batch=1, **kw))
    return out


EXTRA = _extra()


def all_cases():
    return list(census().values()) + EXTRA


def case_id(case):
    return key_id(case.key) if case.origin != "extra" else "extra-" + case.name


# ------------------------------------------------------------------------------------------------------------------ exactness certificate
def _lcm(values):
    out = 1
    for v in values:
        out = out * v // math.gcd(out, v)
    return out


@functools.lru_cache(None)
def form_matrices(family, m, r):
    """(A^T, G, B^T) of the family's form in ONE dimension, as Fractions.  The Cook-Toom forms: cooktoom.cook_toom - the derivation the
    kernels' header and packers are generated from (F(2,3) is hand written in the kernels with the same matrices up to signs).  Refine: F(2,2)
    as csrc/convt_wino.hip packs it (G = [[1,0],[1,1],[0,1]]): y0 = g0 (d0 - d1) + (g0 + g1) d1, y1 = (g0 + g1) d1 + g1 (d2 - d1).  Upconv: the
    2-tap filter over the x2 nearest upsampling, y0 = (g0 + g1) d0, y1 = y0 + g1 (d1 - d0) (mr_upconv_pack_weights_f32: U = [sum, w.1; w1., w11])."""
    fr = lambda rows: [[Fraction(v) for v in row] for row in rows]
    if family == "t22":
        return fr([[1, 1, 0], [0, 1, 1]]), fr([[1, 0], [1, 1], [0, 1]]), fr([[1, -1, 0], [0, 1, 0], [0, -1, 1]])
    if family == "up":
        return fr([[1, 0], [1, 1]]), fr([[1, 1], [0, 1]]), fr([[1, 0], [-1, 1]])
    return cooktoom.cook_toom(m, r)


def form_scales(family, m, r):
    """(den(A^T), lcm of G's denominators, den(B^T)) of the form in one dimension."""
    at, g, bt = form_matrices(family, m, r)
    return tuple(_lcm([v.denominator for row in mat for v in row]) for mat in (at, g, bt))


def dims_of(launch):
    return 1 if launch.family in ("f23", "ct") else 2


def weight_shape(launch):
    cin = sum(launch.srcs_c)
    if launch.family == "t22":
        return (cin, launch.cout, 4, 4)                  # nn.ConvTranspose2d layout
    if launch.family == "up":
        return (launch.cout, cin, 2, 2)
    if dims_of(launch) == 2:
        return (launch.cout, cin, 3, 3)
    return (launch.cout, cin, 1, launch.r) if launch.axis == 0 else (launch.cout, cin, launch.r, 1)


def weight_unit(launch):
    """What the exact weights are integer multiples of: lcm(denominators of G) per dimension of the form."""
    return form_scales(launch.family, *form_of(launch))[1] ** dims_of(launch)


def pad_low(launch):
    """Zeros in front of the filter axis: (r - 1) // 2 ('same' for odd r; 1 for the 4-tap form over [even | odd] views)."""
    return (form_of(launch)[1] - 1) // 2


def _imat(mat, scale):
    return torch.tensor([[int(v * scale) for v in row] for row in mat], dtype=torch.float64)


def scaled_bound(launch, srcs, weight):
    """max over every output of |A^T| (sum_c |U| |V|) |A|, times the dyadic denominators of A^T and B^T (per dimension): an integer, computed
    in float64 on integers far below 2^53.  Every fp32 intermediate of the launch - transformed input, product, partial channel sum in any
    order, partial output transform - is an integer multiple of 1 / denominators whose magnitude this bounds.  Correlation forms (3x3 and
    1-D): from the operands' own tiles.  Refine and Upconv (0 / +-1 matrices, no denominators): the coarser
    rowsum(A)^2 * cin_total * (rowsum(G)^2 max|g|) * (rowsum(B)^2 max|d|), which is ample."""
    m, r = form_of(launch)
    at, g, bt = form_matrices(launch.family, m, r)
    den_a, unit, den_b = form_scales(launch.family, m, r)
    x = torch.cat(srcs, 1).double()
    w = weight.double()
    if launch.family in ("t22", "up"):
        rs = lambda mat: max(sum(abs(v) for v in row) for row in mat)
        return float(rs(at) ** 2 * x.shape[1] * (rs(g) ** 2 * w.abs().max().item()) * (rs(bt) ** 2 * x.abs().max().item()))
    n = m + r - 1
    ati, gi, bti = _imat(at, den_a).abs(), _imat(g, unit), _imat(bt, den_b)
    lo = pad_low(launch)
    if dims_of(launch) == 1:
        if launch.axis == 1:
            x, w = x.transpose(2, 3), w.transpose(2, 3)
        wi = w[:, :, 0, :] / unit                                               # (cout, cin, r) small integers
        tiles = -(-x.shape[3] // m)
        xp = torch.nn.functional.pad(x, (lo, tiles * m + r - 1 - lo - x.shape[3]))
        v = torch.einsum("bcytp,ip->ibcyt", xp.unfold(3, n, m), bti).abs()       # (n, b, c, y, t)
        u = torch.einsum("ocp,ip->ioc", wi, gi).abs()                           # (n, cout, cin)
        s = torch.bmm(u, v.permute(0, 2, 1, 3, 4).reshape(n, x.shape[1], -1))   # (n, cout, b y t)
        return float(torch.einsum("ki,iop->kop", ati, s).max().item())
    wi = w / (unit * unit)
    ty, tx = -(-x.shape[2] // m), -(-x.shape[3] // m)
    xp = torch.nn.functional.pad(x, (lo, tx * m + r - 1 - lo - x.shape[3], lo, ty * m + r - 1 - lo - x.shape[2]))
    v = torch.einsum("ip,bcyxpq,jq->ijcbyx", bti, xp.unfold(2, n, m).unfold(3, n, m), bti).abs()
    u = torch.einsum("ip,ocpq,jq->ijoc", gi, wi, gi).abs()
    s = torch.bmm(u.reshape(n * n, *u.shape[2:]), v.reshape(n * n, x.shape[1], -1)).reshape(n, n, w.shape[0], -1)
    return float(torch.einsum("ki,lj,ijop->klop", ati, ati, s).max().item())


# (weight range, data range, weight density, data density) by preference: the density goes down before anything else - the key fixes the channels
_ATTEMPTS = ((2, 3, 1.0, 1.0), (1, 1, 1.0, 1.0), (1, 1, 0.5, 1.0), (1, 1, 0.25, 1.0), (1, 1, 0.25, 0.5), (1, 1, 0.125, 0.5), (1, 1, 0.125, 0.25),
             (1, 1, 0.0625, 0.25))

Operands = collections.namedtuple("Operands", "srcs weight bound attempt")


def source_shapes(launch):
    return [(launch.batch, c, launch.hw[0], launch.hw[1]) for c in launch.srcs_c]


def _draw(launch, seed, wr, dr, wd, dd):
    g = torch.Generator().manual_seed(seed)
    unit = weight_unit(launch)

    def rnd(rng, density, shape):
        t = torch.randint(-rng, rng + 1, shape, generator=g).float()
        return t if density >= 1.0 else t * (torch.rand(shape, generator=g) < density).float()
    srcs = [rnd(dr, dd, s) for s in source_shapes(launch)]
    return srcs, rnd(wr, wd, weight_shape(launch)) * float(unit)


def exact_operands(case, seed):
    """Integer operands for the case's launch whose every fp32 intermediate is exact - `Operands(sources, weight, bound, attempt)` with the
    sources as the KERNEL sees them (a stride-2 half: [even | odd]) and the weight in the layout of its builder - or None when no attempt is
    accepted (F(4,7)).  Accepted: scaled_bound(...) <= 2^23, a statement about the operands alone."""
    launch = case.launch
    for attempt in _ATTEMPTS:
        srcs, weight = _draw(launch, seed, *attempt)
        assert float(weight.abs().max()) < 2 ** 24 and torch.equal(weight, (weight / weight_unit(launch)).round() * weight_unit(launch))
        bound = scaled_bound(launch, srcs, weight)
        if bound <= EXACT_LIMIT:
            return Operands(srcs, weight, bound, attempt)
    return None


def certifiable(key):
    """F(4,7) is the one form whose operands cannot be certified (G denominator 90720)."""
    return not (key.family == "ct" and (key.m, key.r) == (4, 7))


# ------------------------------------------------------------------------------------------------------------------ exact emulation of one tile
def _tile_1d(at, g, bt, taps, samples):
    """A^T [(G g) o (B^T d)] in Fractions: m outputs from n samples."""
    n = len(bt)
    u = [sum(g[i][j] * taps[j] for j in range(len(taps))) for i in range(n)]
    v = [sum(bt[i][c] * samples[c] for c in range(n)) for i in range(n)]
    return [sum(at[k][i] * u[i] * v[i] for i in range(n)) for k in range(len(at))]


def _tile_2d(at, g, bt, taps, patch):
    """A^T [(G g G^T) o (B^T d B)] A in Fractions: m x m outputs from an n x n patch."""
    n, r, m = len(bt), len(taps), len(at)
    u = [[sum(g[i][p] * taps[p][q] * g[j][q] for p in range(r) for q in range(r)) for j in range(n)] for i in range(n)]
    v = [[sum(bt[i][p] * patch[p][q] * bt[j][q] for p in range(n) for q in range(n)) for j in range(n)] for i in range(n)]
    return [[sum(at[k][i] * u[i][j] * v[i][j] * at[l][j] for i in range(n) for j in range(n)) for l in range(m)] for k in range(m)]


def emulate_tile(launch, srcs, weight, co, ty, tx, channels):
    """(form, direct): the output tile (ty, tx) of sample 0, output channel `co`, summed over `channels` of the concatenated input - once
    through the form in Fractions, once as the direct sum the layer is defined by (correlation with zero padding; Refine: ConvTranspose2d(4, 2)
    cropped by one; Upconv: nearest x2, zero pad right / below, 2x2 correlation).  Integer lists, m or m x m entries."""
    m, r = form_of(launch)
    at, g, bt = form_matrices(launch.family, m, r)
    n, lo = m + r - 1, pad_low(launch)
    x = torch.cat(srcs, 1)[0].long()
    hh, ww = x.shape[1:]
    px = lambda c, y, xx: int(x[c, y, xx]) if 0 <= y < hh and 0 <= xx < ww else 0
    w = weight.long()
    if dims_of(launch) == 1:
        form, direct = [Fraction(0)] * m, [0] * m
        for c in channels:
            taps = [int(v) for v in (w[co, c, 0, :] if launch.axis == 0 else w[co, c, :, 0])]
            line = (lambda i: px(c, ty, tx * m - lo + i)) if launch.axis == 0 else (lambda i: px(c, ty * m - lo + i, tx))
            form = [a + b for a, b in zip(form, _tile_1d(at, g, bt, taps, [line(i) for i in range(n)]))]
            direct = [d + sum(taps[j] * line(k + j) for j in range(r)) for k, d in enumerate(direct)]
        return form, direct
    add = lambda acc, t: [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(acc, t)]
    if launch.family == "t22":
        # Phase (py, qx) of the cropped transposed convolution is a 2x2 correlation on the input: output (2 y + py, 2 x + qx) =
        # sum_{i,j} d[y + py - 1 + i, x + qx - 1 + j] wt[3 - py - 2 i, 3 - qx - 2 j]; a tile is 2 x 2 outputs of ONE phase.  The direct side is
        # the definition: full[Y, X] = sum d[iy, ix] wt[Y - 2 iy, X - 2 ix], cropped by one.  Returned: the four phase tiles, 4 x 4 entries.
        form, direct = [[Fraction(0)] * 4 for _ in range(4)], [[0] * 4 for _ in range(4)]
        for c in channels:
            for py in range(2):
                for qx in range(2):
                    taps = [[int(w[c, co, 3 - py - 2 * i, 3 - qx - 2 * j]) for j in range(2)] for i in range(2)]
                    patch = [[px(c, ty * 2 + py - 1 + i, tx * 2 + qx - 1 + j) for j in range(3)] for i in range(3)]
                    t = _tile_2d(at, g, bt, taps, patch)
                    for k in range(2):
                        for l in range(2):
                            form[2 * py + k][2 * qx + l] += t[k][l]
                            yy, xx = 2 * (2 * ty + k) + py + 1, 2 * (2 * tx + l) + qx + 1             # position in the uncropped output
                            direct[2 * py + k][2 * qx + l] += sum(px(c, iy, ix) * int(w[c, co, yy - 2 * iy, xx - 2 * ix])
                                                                  for iy in range(max(0, (yy - 2) // 2), yy // 2 + 1) if 0 <= yy - 2 * iy < 4
                                                                  for ix in range(max(0, (xx - 2) // 2), xx // 2 + 1) if 0 <= xx - 2 * ix < 4)
        return form, direct
    form, direct = [[Fraction(0)] * m for _ in range(m)], [[0] * m for _ in range(m)]
    for c in channels:
        if launch.family == "up":
            taps = [[int(w[co, c, i, j]) for j in range(2)] for i in range(2)]
            patch = [[px(c, ty + i, tx + j) for j in range(2)] for i in range(2)]
            form = add(form, _tile_2d(at, g, bt, taps, patch))
            up = lambda yy, xx: px(c, yy // 2, xx // 2)           # x2 nearest; rows / columns past 2 h, 2 w are the zero padding
            direct = add(direct, [[sum(taps[i][j] * up(2 * ty + k + i, 2 * tx + l + j) for i in range(2) for j in range(2)) for l in range(2)]
                                  for k in range(2)])
            continue
        taps = [[int(w[co, c, i, j]) for j in range(r)] for i in range(r)]
        patch = [[px(c, ty * m - lo + i, tx * m - lo + j) for j in range(n)] for i in range(n)]
        form = add(form, _tile_2d(at, g, bt, taps, patch))
        direct = add(direct, [[sum(taps[i][j] * patch[k + i][l + j] for i in range(r) for j in range(r)) for l in range(m)] for k in range(m)])
    return form, direct


# ------------------------------------------------------------------------------------------------------------------ failure messages
def output_owner(launch, co, y, x):
    """Where the kernel computes position (y, x) of its plane (Refine / Upconv: the input position of the 2x2 output block) for output channel
    `co`: workgroup tile, channel group and 16-channel block within it."""
    rows, cols = workgroup_tile(launch)
    g = group_channels(launch)
    if launch.family in ("w22", "t22") and launch.variant == 2 and co // 32 != launch.cout // 32:
        rows = 8                                                     # a full group of the tail form: 8-row workgroups
    return dict(tile=(y // rows, x // cols), group=co // g, block=(co % g) // 16)
