"""GPU (MI355X): MonoRecModel(hip_bf16=True, hip_lean_outputs=True) - the bf16 configuration whose cost-volume fusion kernel does not finalise
the dense fp32 single-frame volumes (mr_cost_volume_b8_lean_f32) - against the same model without the option: `single_frame_cvs` leaves the
output dict, every other output stays bit-identical, through forward() (outputs the caller owns: the arena layout skips `sfcv`) and through
submit() (views of the resident buffers)."""
import pytest
import torch

from monorec_amd import synth
from monorec_amd.model import MonoRecModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONSTANTS = ("inv_depth_min", "inv_depth_max", "cv_depth_steps")


def _model(depths, **kw):
    m = MonoRecModel(cv_depth_steps=depths, hip_in_flight=1, hip_bf16=True, **kw)
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=0))
    return m.to(DEV).eval()


def _snapshot(out):
    """The tensors of an output dict, cloned (submit() hands out views of buffers the next run overwrites)."""
    keep = {k: out[k].clone() for k in ("cost_volume", "cv_mask", "mask", "result") + CONSTANTS}
    keep["predicted_inverse_depths"] = [t.clone() for t in out["predicted_inverse_depths"]]
    keep["image_features"] = [t.clone() for t in out["image_features"]]
    if "single_frame_cvs" in out:
        keep["single_frame_cvs"] = [t.clone() for t in out["single_frame_cvs"]]
    return keep


def _assert_same_but_for_the_single_frame_volumes(got, want, tag):
    for k in ("cost_volume", "cv_mask", "mask", "result") + CONSTANTS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (tag, k)
    assert len(got["predicted_inverse_depths"]) == len(want["predicted_inverse_depths"]) == 4
    assert len(got["image_features"]) == len(want["image_features"]) == 5
    for k in ("predicted_inverse_depths", "image_features"):
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert torch.equal(a, b), (tag, k, i)
    assert not torch.isnan(got["result"]).any() and not torch.isnan(got["cost_volume"]).any()


def test_lean_outputs_drop_single_frame_cvs_and_move_nothing_else(hip_lib):
    full, lean = _model(32), _model(32, hip_lean_outputs=True)
    batches = [synth.make_batch(2, 64, 96, 2, seed=s) for s in (33, 34)]
    with torch.no_grad():
        want = [_snapshot(full(synth.clone_batch(b, DEV))) for b in batches]
        # forward(): a second call on another batch runs through the owned-output layout built by the first (no `sfcv` in it)
        got = [_snapshot(lean(synth.clone_batch(b, DEV))) for b in batches]
        view = _snapshot(lean.submit(synth.clone_batch(batches[0], DEV)).result())
        want_view = _snapshot(full.submit(synth.clone_batch(batches[0], DEV)).result())
    torch.cuda.synchronize()
    assert not torch.equal(want[0]["result"], want[1]["result"])
    for i in range(2):
        assert "single_frame_cvs" in want[i] and len(want[i]["single_frame_cvs"]) == 2
        assert "single_frame_cvs" not in got[i]
        _assert_same_but_for_the_single_frame_volumes(got[i], want[i], f"forward {i}")
    assert "single_frame_cvs" not in view and "single_frame_cvs" in want_view
    _assert_same_but_for_the_single_frame_volumes(view, want[0], "submit")
    _assert_same_but_for_the_single_frame_volumes(want_view, want[0], "submit, full")
    plans = [p for p in lean._plans.values() if p.own_layout is not None]                     # the plan forward() ran: its arenas hold no `sfcv`
    assert plans and all(p.lean_active and "sfcv" not in [n for kind in ("small", "big") for n, _, _ in p.own_layout[kind]] for p in plans)
    assert all("sfcv" in [n for n, _, _ in p.own_layout["big"]] for p in full._plans.values() if p.own_layout is not None)


def test_lean_outputs_change_nothing_where_the_plan_falls_back(hip_lib):
    """cv_depth_steps = 20 has no fusion kernel that writes the B8 copies: the plan runs mr_cost_volume_mode_f32, which finalises the single-frame
    volumes - they are handed out, equal to those of the model without the option, through forward() and submit()."""
    full, lean = _model(20), _model(20, hip_lean_outputs=True)
    batch = synth.make_batch(2, 64, 96, 2, seed=35)
    with torch.no_grad():
        want = _snapshot(full(synth.clone_batch(batch, DEV)))
        got = _snapshot(lean(synth.clone_batch(batch, DEV)))
        view = _snapshot(lean.submit(synth.clone_batch(batch, DEV)).result())
    torch.cuda.synchronize()
    for out, tag in ((got, "forward"), (view, "submit")):
        _assert_same_but_for_the_single_frame_volumes(out, want, tag)
        assert "single_frame_cvs" in out and len(out["single_frame_cvs"]) == 2
        for f in range(2):
            assert not torch.isnan(out["single_frame_cvs"][f]).any() and torch.equal(out["single_frame_cvs"][f], want["single_frame_cvs"][f]), (tag, f)


def test_lean_outputs_need_the_bf16_configuration():
    with pytest.raises(ValueError):
        MonoRecModel(cv_depth_steps=32, hip_lean_outputs=True)
