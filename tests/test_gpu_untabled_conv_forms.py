"""GPU (MI355X): the convolution launches the nearest-signature rules choose for input shapes WITHOUT table entries, key by key, and
such shapes end to end.

tests/untabled_conv_census.py builds the plans of shapes the tables were not measured for, reduces every launch with the three family
censuses' own keys, extends the key by "the output grid is smaller than one workgroup tile (transform tile) in this direction" and keeps
one representative per extended key that no case of the family censuses has.  Each representative runs here ALONE under its family's
existing checks, which are the test functions of the family's GPU file, called unchanged:

  direct   tests/test_gpu_direct_conv_sweeps.py   a exact, b gaussian 2e-4 * max(1, |ref|max), c order identity where
                                                  order_check_applies, d footprint between guard channels, sentinel, repetitions
  reduced  tests/test_gpu_reduced_conv_forms.py   exact on certified operands (all keys but the F(4,7) ones: UNCERTIFIED pins how many),
                                                  the gaussian bar of that file, twins, footprint, determinism
  b8       tests/test_gpu_b8_conv_forms.py        bit-exact on fp32 and B8 destinations, gaussian, identity, footprint with guard rows /
                                                  columns and margins

FOOTPRINT OF A SUB-TILE GRID.  The direct and the B8 check cover a grid smaller than one tile as they stand: the direct destination lies
between guard channels, the B8 destination in a plane with guard rows below and guard columns right of the grid (its descriptor has a
destination pitch, dst_plane_h / dst_plane_w).  mr_wino_desc - the descriptor of every reduced-multiply entry point - has NO destination
pitch: the destination plane is the kernel's plane.  The reduced-form cases therefore keep that file's guard, 3 channels of sentinel in
front of and behind the destination; for a sub-tile plane the guard is as many floats as three planes, so a workgroup that stored its
whole tile past a short row or a low plane lands in it (or in the next row / channel of the slice, where the exact check sees it).

END TO END AT THE EDGES.  model(data) against the CPU oracle at the existing bars (fp32: test_gpu_model._check_against, depth within
1e-4; bf16: the bar test_c5_shape_in_fp32_and_bf16 states, depth within 1e-2 everywhere and 1e-3 on average) on shapes whose plans launch
sub-tile grids, which each test asserts from the plan's conv_log."""
import pytest
import torch

import test_gpu_b8_conv_forms as b8_gpu
import test_gpu_direct_conv_sweeps as direct_gpu
import test_gpu_model as model_gpu
import test_gpu_reduced_conv_forms as reduced_gpu
import reduced_conv_census
import untabled_conv_census as census
from monorec_amd import synth
from monorec_amd.model import MonoRecModel
from oracle import monorec_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNCERTIFIED = 0          # new reduced-form keys without an exact check: none beyond the F(4,7) kind, and no new key is of that kind


def _params(family):
    reps = census.cases(family)
    return pytest.mark.parametrize("rep", reps, ids=[census.ext_id(r.ext) for r in reps])


@_params("direct")
def test_untabled_direct_conv_instantiation(hip_lib, rep):
    direct_gpu.test_direct_conv_instantiation(hip_lib, rep.case)


@_params("reduced")
def test_untabled_reduced_conv_form(hip_lib, monkeypatch, rep):
    reduced_gpu.test_reduced_conv_form(hip_lib, monkeypatch, rep.case)


@_params("b8")
def test_untabled_b8_conv_form(hip_lib, rep):
    b8_gpu.test_b8_conv_form(hip_lib, rep.case)


def test_uncertified_reduced_keys_are_pinned(hip_lib):
    """Which new reduced-form keys run without the exact check (reduced_conv_census.certifiable is false: F(4,7))."""
    loose = [census.ext_id(r.ext) for r in census.cases("reduced") if not reduced_conv_census.certifiable(r.case.key)]
    assert len(loose) == UNCERTIFIED, loose


def _sub_tile_launches(model, h, w, mode):
    plan = next(p for k, p in model._plans.items() if k[2] == h and k[3] == w)
    origin = f"{h}x{w}"
    subs = [l for l in (census.reduce_launch(c, origin) for c in plan.conv_log) if census.sub_tile(l)]
    assert subs, "the plan launched no sub-tile grid"
    assert all(int(c.get("bf16", 0)) in (0, mode) for c in plan.conv_log)
    return subs


@pytest.mark.parametrize("shape", [(1, 32, 32, 1, 4), (3, 64, 96, 1, 8), (1, 96, 320, 2, 32)], ids=lambda s: "b%d_%dx%d_f%d_d%d" % s)
def test_edge_shapes_against_the_oracle(hip_lib, shape):
    """fp32, at the 1e-4 bar of the path: planes down to 1 x 1 (32x32), an odd batch, planes of 3 x 10."""
    b, h, w, f, d = shape
    model, sd = model_gpu._model(d, graph=False)
    batch = synth.make_batch(b, h, w, f, seed=9)
    with torch.no_grad():
        out = model(model_gpu._to_dev(batch))
        out = {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in out.items() if k in
               ("result", "cv_mask", "predicted_inverse_depths", "image_features", "cost_volume", "single_frame_cvs")}
    torch.cuda.synchronize()
    subs = _sub_tile_launches(model, h, w, 0)
    print("b%d_%dx%d_f%d_d%d" % shape, f"{len(subs)} sub-tile launches, e.g. {subs[0].name}: {census.ext_id(subs[0].ext)}")
    ref_out = orc.forward(sd, batch, cv_depth_steps=d)
    assert out["result"].shape == (b, 1, h, w) and len(out["single_frame_cvs"]) == f
    model_gpu._check_against(out, ref_out, "b%d_%dx%d_f%d_d%d" % shape)


def test_edge_shape_in_bf16_against_the_oracle(hip_lib):
    """64x64 with hip_bf16=True (B8 planes of 2 x 2 to 32 x 32) at the bar test_c5_shape_in_fp32_and_bf16 states for the mode: depth within
    1e-2 everywhere and 1e-3 on average."""
    b, h, w, f, d = 1, 64, 64, 2, 8
    m16 = MonoRecModel(cv_depth_steps=d, hip_in_flight=1, hip_bf16=True)
    sd = synth.seeded_state_dict(m16.state_dict(), seed=0)
    m16.load_state_dict(sd)
    m16 = m16.to(DEV).eval()
    batch = synth.make_batch(b, h, w, f, seed=9)
    with torch.no_grad():
        o16 = m16(model_gpu._to_dev(batch))
    torch.cuda.synchronize()
    subs = _sub_tile_launches(m16, h, w, 1)
    assert any(l.family == "b8" for l in subs)
    ref_out = orc.forward(sd, batch, cv_depth_steps=d)
    err = (o16["result"].cpu() - ref_out["result"]).abs()
    print("64x64, bf16 MFMA mode: result max|err| %.3e mean %.3e; %d sub-tile launches" % (err.max(), err.mean(), len(subs)))
    assert o16["result"].shape == (b, 1, h, w)
    assert err.max().item() <= 1e-2 and err.mean().item() <= 1e-3
