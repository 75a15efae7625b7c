"""GPU (MI355X): two invariants of engine.Plan that every throughput figure rests on, bit for bit (helpers: tests/plan_poison.py).

A. No launch of a forward reads memory this forward has not written.  Every scratch and output buffer of the plan is filled with zeros, with a
   payload NaN and with a huge finite value (which, unlike the NaN, survives a ReLU); the same batch is run after each fill.  Every output must be
   bit-identical across the three runs and fully written (no pattern element left), and no intermediate may differ where it was written.
B. The stages that run side by side on two streams are independent: every legal serial order of the four stages, each from poisoned scratch, gives
   the bits of the model-API run - so no interleaving of two streams can give others.
C. Teeth: controls that show the method can fail.

Equality between runs must never be equality of two answers wrong for one cause: the zero-fill run of the fixture shapes is compared with the
committed output of the reference (tests/golden `small`, `c1_256x512`; helper and tolerance of tests/test_gpu_model.py).  The other shapes are
anchored by the oracle tests of tests/test_gpu_model.py that run the same plans: test_batch_independence (batch 3),
test_other_input_shapes_against_the_oracle (192x448), test_bf16_mode_end_to_end / test_bf16_mode_with_depth_counts_off_the_fast_paths /
test_c5_shape_in_fp32_and_bf16 (bf16), test_bf16x3_mode_end_to_end, test_model_options_against_reference_fixture, test_cv_patch_size_through_the_model
and test_sfcv_without_mult_mask_through_the_model (the option variants).  No CPU oracle runs here."""
import pytest
import torch

import plan_poison as pp
from golden_util import Golden
from monorec_amd import synth
from monorec_amd.model import MonoRecModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESULT_ATOL = 1e-4          # tests/test_gpu_model.py: BASELINE.json north_star, depths within 1e-4 abs of the reference CPU output


# ---------------------------------------------------------------------------------------------------------------- configurations
# id -> (shape (B, H, W, F), depth steps, seed or fixture name, model options)
CONFIGS = {}
for _b in (2, 3):
    for _tag, _forms in (("table", False), ("f2", "f2"), ("direct", True)):
        CONFIGS[f"f32_b{_b}_{_tag}"] = ((_b, 64, 96, 2), 8, "small" if _b == 2 else 21, dict(hip_exact_convs=_forms))
CONFIGS["c2_table"] = ((1, 256, 512, 2), 32, "c1_256x512", {})
CONFIGS["c2_direct"] = ((1, 256, 512, 2), 32, "c1_256x512", dict(hip_exact_convs=True))
CONFIGS["f32_192x448_rules"] = ((1, 192, 448, 2), 32, 9, {})                               # no table entry: rule-chosen launches
CONFIGS["bf16_d8"] = ((1, 64, 96, 2), 8, 5, dict(hip_bf16=True))                           # off the B8 fast paths
CONFIGS["bf16_d32"] = ((1, 64, 96, 2), 32, 5, dict(hip_bf16=True))                         # sfcv_b8, cost_volume_b8
CONFIGS["bf16_d32_lean"] = ((1, 64, 96, 2), 32, 5, dict(hip_bf16=True, hip_lean_outputs=True))
CONFIGS["bf16_c5_lean"] = ((1, 512, 1024, 4), 48, 5, dict(hip_bf16=True, hip_lean_outputs=True))   # BASELINE configs[4]
CONFIGS["bf16x3"] = ((1, 64, 96, 2), 8, 3, dict(hip_bf16x3=True))
for _case, _kw in pp.OPTION_CASES.items():
    CONFIGS[f"opt_{_case}"] = ((2, 64, 96, 2), 8, 41, dict(_kw))
CONFIGS["f32_b2_skip_layer4"] = ((2, 64, 96, 2), 8, "small", dict(hip_skip_dead_layer4=True))
BIG = {"c2_table", "c2_direct", "f32_192x448_rules", "bf16_c5_lean"}     # snapshots stay on the device (a clone, not a pageable download)
KEEP = {"f32_b2_table", "c2_table", "c2_direct", "bf16_d32", "f32_b2_skip_layer4"}   # reused by parts B and C: built once per module


def _inputs(cid):
    (b, h, w, f), depths, src, kw = CONFIGS[cid]
    if isinstance(src, str):
        g = Golden(src)
        assert (g.batch, g.h, g.w, g.frames, g.depths) == (b, h, w, f, depths)
        batch = g.make_inputs()
    else:
        batch = synth.make_batch(b, h, w, f, seed=src)
    data = synth.clone_batch(batch, DEV)
    gen = torch.Generator().manual_seed(97)
    if kw.get("pretrain_mode") == 3:                  # monorec_model.py:711: cv_mask = data_dict["mvobj_mask"]
        data["mvobj_mask"] = (torch.rand(b, 1, h, w, generator=gen) > 0.7).float().to(DEV)
    if kw.get("simple_mask"):                         # SimpleMaskModule reads a previous prediction from the dict (:453)
        data["predicted_inverse_depths"] = [(0.0025 + 0.3 * torch.rand(b, 1, h, w, generator=gen)).to(DEV)]
    return data


class Env:
    """One configuration: the model (one slot, one stream: what submit() does per slot by default), its plan, the batch, and - after
    `poisoned_runs` - the snapshot of every plan buffer after a run from each of the three fills."""

    def __init__(self, cid, **more):
        self.cid = cid
        _, depths, _, kw = CONFIGS[cid]
        opts = dict(hip_in_flight=1, hip_slot_streams=1)
        opts.update(kw)
        opts.update(more)
        m = MonoRecModel(cv_depth_steps=depths, **opts)
        m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=0))
        self.model = m.to(DEV).eval()
        self.data = _inputs(cid)
        self.snap_dev = DEV if cid in BIG else "cpu"
        self.runs = None
        self.run()
        self.plans = list(self.model._plans.values())
        self.plan = self.plans[0]

    def run(self):
        with torch.no_grad():
            out = self.model.submit(dict(self.data)).result()
        torch.cuda.synchronize()
        return out

    def poisoned_runs(self):
        if self.runs is None:
            self.runs = {}
            for fill in pp.FILLS:
                pp.poison(self.plan, fill)
                torch.cuda.synchronize()
                self.run()
                self.runs[fill] = pp.snapshot(self.plan, self.snap_dev)
        return self.runs

    @property
    def base(self):
        return self.poisoned_runs()["zero"]


_ENVS = {}


def env_of(cid):
    if cid in _ENVS:
        return _ENVS[cid]
    e = Env(cid)
    if cid in KEEP:
        _ENVS[cid] = e
    return e


@pytest.fixture(scope="module", autouse=True)
def _release_plans():
    yield
    _ENVS.clear()
    torch.cuda.empty_cache()


def outputs_of(plan):
    return pp.members(plan, pp.OUTPUT)


def written(plan):
    """The classes a forward writes: what two plans of one configuration can be compared on (the resident `keyframe` / `frames` of a plan whose
    launches read the caller's tensors in place were never written at all)."""
    return pp.members(plan, pp.SCRATCH) + pp.members(plan, pp.OUTPUT)


def assert_same_bits(got, want, names, tag):
    for n in names:
        assert got[n].dtype == want[n].dtype and torch.equal(got[n], want[n].to(got[n].device)), f"{tag}: output {n} differs"


def assert_clean(snap, plan, tag):
    left = pp.poisoned_elements(snap, outputs_of(plan))
    assert not left, f"{tag}: outputs a forward left unwritten (pattern elements): {left}"


def anchor(cid, snap):
    """The zero-fill run against the committed output of the reference, where the configuration is a fixture's."""
    src = CONFIGS[cid][2]
    if isinstance(src, str):
        Golden(src).compare("result", snap["pred0"].view(torch.float32), atol=RESULT_ATOL)


def expected_constants(cid):
    return pp.EXPECTED_CONSTANTS[cid[4:]] if cid.startswith("opt_") else []


# ---------------------------------------------------------------------------------------------------------------- A. poisoned scratch
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_forward_from_poisoned_scratch(hip_lib, cid):
    """Run once, then poison (zeros / payload NaN / huge finite) -> run -> snapshot, three times: outputs bit-identical and fully written, no
    intermediate differs where it was written.  The class census of the configuration is asserted and printed."""
    e = env_of(cid)
    plan, kw = e.plan, CONFIGS[cid][3]
    counts = pp.class_counts(plan)
    print(f"{cid}: classes {counts}, {sum(t.numel() * t.element_size() for t in plan.buf.values()) / 1e6:.0f} MB")
    assert pp.members(plan, pp.CONSTANT) == expected_constants(cid)
    assert counts[pp.SCRATCH] > 20, counts
    assert any(n.startswith("splitk_workspace.") for n in pp.members(plan, pp.SCRATCH))
    bf16_bufs = [n for n in pp.members(plan, pp.SCRATCH) if plan.buf[n].dtype == torch.bfloat16]
    assert bool(bf16_bufs) == bool(kw.get("hip_bf16")), bf16_bufs
    if cid == "bf16_d8":
        assert "sfcv_b8" not in plan.buf and "cost_volume_b8" not in plan.buf
    if cid.startswith("bf16_d32") or cid == "bf16_c5_lean":
        assert {"sfcv_b8", "cost_volume_b8"} <= set(bf16_bufs)
        assert plan.lean_active == bool(kw.get("hip_lean_outputs")) and ("sfcv" in outputs_of(plan)) != plan.lean_active
    if cid == "f32_192x448_rules":
        from monorec_amd import engine
        assert not [c["sig"] for c in plan.conv_log if c.get("sig") in engine.TUNED]
    if cid.endswith("_direct"):
        assert not any(c.get("winograd") for c in plan.conv_log)
    runs = e.poisoned_runs()
    outs = outputs_of(plan)
    for fill in pp.FILLS:
        assert_clean(runs[fill], plan, f"{cid}, run from {fill}")
    for a, b in (("zero", "nan"), ("zero", "huge"), ("nan", "huge")):
        lines = pp.report(runs[a], runs[b])
        assert not lines, f"{cid}: a launch consumed stale memory - run from {a} vs run from {b}:\n" + "\n".join(lines)
        assert_same_bits(runs[b], runs[a], outs, f"{cid}, {a} vs {b}")
    print(f"{cid}: never written by a forward (elements): {pp.poisoned_elements(runs['nan'], written(plan)) or 'none'}")
    lines = pp.unwritten_sets_differ(runs["nan"], runs["huge"])
    assert not lines, f"{cid}: what a forward leaves unwritten depends on the fill (a stale NaN travelling as the pattern):\n" + "\n".join(lines)
    assert not any(bool(pp.is_poison(t).any()) for t in runs["zero"].values())
    anchor(cid, runs["zero"])


# ---------------------------------------------------------------------------------------------------------------- A. the other ways in
def _output_tensors(out, plan):
    """plan buffer name -> tensor of a result dict."""
    t = {"cost_volume": out["cost_volume"], "cv_mask": out["cv_mask"]}
    if "single_frame_cvs" in out:
        t["sfcv"] = torch.stack(list(out["single_frame_cvs"]))
    t.update({f"feat{i}": f for i, f in enumerate(out["image_features"])})
    t.update({f"pred{i}": p for i, p in enumerate(out["predicted_inverse_depths"])})
    assert sorted(t) == sorted(outputs_of(plan))
    return {n: pp.bits(v.contiguous()).clone() for n, v in t.items()}


def _six_keyframes(cid):
    (b, h, w, f), _, src, _ = CONFIGS[cid]
    first = _inputs(cid)                                                     # keyframe 0: the fixture's batch
    return [first] + [synth.clone_batch(synth.make_batch(b, h, w, f, seed=30 + i), DEV) for i in range(1, 6)]


@pytest.mark.parametrize("cid", ["f32_b2_table", "c2_table"])
def test_two_slots_on_two_streams_each_from_poisoned_scratch(hip_lib, cid):
    """hip_in_flight=2, hip_slot_streams=2: real two-stream concurrency (encoder / layer4 beside cost volume / mask / depth, only enc_done and
    tail_done between them), two keyframes on the GPU at once.  Six keyframes per round as in test_two_keyframes_in_flight_equal_sequential_forwards;
    both slots' plans poisoned between the rounds.  Every keyframe's outputs equal the clean round's bit for bit, keyframe 0 - the fixture's batch -
    equals the one-stream run of part A, and both plans (they hold keyframes 4 and 5) pass the report."""
    depths = CONFIGS[cid][1]
    m = MonoRecModel(cv_depth_steps=depths, hip_in_flight=2, hip_slot_streams=2)
    m.load_state_dict(synth.seeded_state_dict(m.state_dict(), seed=0))
    m = m.to(DEV).eval()
    frames = _six_keyframes(cid)
    dev = DEV if cid in BIG else "cpu"

    def one_round():
        """Two keyframes in flight; every result cloned (bits) when it is taken: the views are overwritten two submits later."""
        got, pending = [], []
        with torch.no_grad():
            for d in frames:
                pending.append(m.submit(dict(d)))
                if len(pending) == 2:
                    got.append(_output_tensors(pending.pop(0).result(), next(iter(m._plans.values()))))
            while pending:
                got.append(_output_tensors(pending.pop(0).result(), next(iter(m._plans.values()))))
        torch.cuda.synchronize()
        return got
    one_round()                                                              # builds the two plans
    plans = list(m._plans.values())
    assert len(plans) == 2 and m._slot_streams(0, torch.device(DEV))["enc"] is not m._slot_streams(0, torch.device(DEV))["main"]
    rounds, snaps = {}, {}
    for fill in pp.FILLS:
        for p in plans:
            pp.poison(p, fill)
        torch.cuda.synchronize()
        rounds[fill] = one_round()
        snaps[fill] = [pp.snapshot(p, dev) for p in plans]
    outs = outputs_of(plans[0])
    for fill in pp.FILLS:
        for i in range(6):
            assert not pp.poisoned_elements(rounds[fill][i], outs), (fill, i)
            assert_same_bits(rounds[fill][i], rounds["zero"][i], outs, f"{cid}, keyframe {i}, round from {fill}")
        for s in range(2):
            lines = pp.report(snaps["zero"][s], snaps[fill][s])
            assert not lines, f"{cid}, slot {s}, round from {fill}:\n" + "\n".join(lines)
    base = env_of(cid).base
    assert_same_bits(rounds["nan"][0], base, outs, f"{cid}, keyframe 0 on two streams vs the one-stream run")
    anchor(cid, {"pred0": rounds["zero"][0]["pred0"]})


@pytest.mark.parametrize("cid", ["f32_b2_table", "c2_table"])
def test_graph_replay_from_poisoned_scratch(hip_lib, cid):
    """hip_graph=True: warm, capture and replay passes first, then poison before each further replay - the captured launches read nothing stale
    either, and reproduce the eager one-stream run of part A on every written buffer."""
    e = Env(cid, hip_graph=True, hip_slot_streams=None)                      # (one slot: the encoder stages on a second stream)
    for _ in range(2):
        e.run()
    assert len(e.model._graphs) >= 3 and all(not isinstance(g, str) for g in e.model._graphs.values())
    runs = e.poisoned_runs()
    base, outs, names = env_of(cid).base, outputs_of(e.plan), written(e.plan)
    for fill in pp.FILLS:
        assert_clean(runs[fill], e.plan, f"{cid} graph, run from {fill}")
        assert_same_bits(runs[fill], base, outs, f"{cid} graph replay from {fill} vs eager")
        lines = pp.report({n: base[n] for n in names}, {n: runs[fill][n] for n in names})
        assert not lines, f"{cid} graph replay from {fill}:\n" + "\n".join(lines)


@pytest.mark.parametrize("cid", ["f32_b2_table", "c2_table"])
def test_forward_into_poisoned_owned_arenas(hip_lib, cid):
    """forward(): the outputs are produced in arenas the caller owns, every launch re-targeted by Plan.rebind_outputs.  The arenas are filled with
    the pattern right after they are allocated (a wrapper on this instance's _bind_owned_outputs, test only), the resident buffers too: a launch
    the relocation table missed would leave pattern elements in the caller's arena (its writer still aims at the resident buffer) or feed its
    reader the pattern.  The returned dict must equal the clean forward() - and the submit() run of part A - bit for bit."""
    e = Env(cid, hip_slot_streams=None)
    m, plan = e.model, e.plan
    assert plan.outputs_rebindable
    with torch.no_grad():
        clean = _output_tensors(m(dict(e.data)), plan)
    torch.cuda.synchronize()
    outs = outputs_of(plan)
    assert_same_bits(clean, env_of(cid).base, outs, f"{cid}: forward() vs submit()")
    original, state = m._bind_owned_outputs, {"fill": None, "views": 0}

    def poisoned_arenas(plan_, device, streams):
        owned = original(plan_, device, streams)
        for name, t in owned.items():
            if name != "consts":
                pp.fill(t, state["fill"])
                state["views"] += 1
        torch.cuda.synchronize()
        return owned
    m._bind_owned_outputs = poisoned_arenas
    try:
        for fill in pp.FILLS:
            state["fill"], state["views"] = fill, 0
            pp.poison(plan, fill)
            torch.cuda.synchronize()
            with torch.no_grad():
                out = m(dict(e.data))
            torch.cuda.synchronize()
            assert state["views"] == len(outs), (state, outs)
            resident = {plan.buf[n].data_ptr() for n in outs}
            assert all(t.data_ptr() not in resident for t in [out["cost_volume"], out["cv_mask"], out["result"]] + list(out["image_features"]))
            got = _output_tensors(out, plan)
            assert not pp.poisoned_elements(got, outs), f"{cid}, forward() from {fill}: {pp.poisoned_elements(got, outs)}"
            assert_same_bits(got, clean, outs, f"{cid}, forward() into arenas filled with {fill}")
            assert int(out["cv_depth_steps"]) == CONFIGS[cid][1] and float(out["inv_depth_min"]) == float(torch.tensor(0.33))
    finally:
        m._bind_owned_outputs = original


# ---------------------------------------------------------------------------------------------------------------- B. stage order
@pytest.mark.parametrize("cid", ["f32_b2_table", "c2_table", "c2_direct", "bf16_d32", "f32_b2_skip_layer4"])
def test_every_legal_stage_order_gives_the_same_bits(hip_lib, cid):
    """The four stages by hand on one stream, in every linear extension of (encoder < encoder_tail, encoder < main, cv < main) - pp.REQUIRED_ORDERS
    and `encoder, cv, encoder_tail, main` -, each from NaN-poisoned scratch: outputs and every written intermediate equal the
    model-API run of part A.  Serial orders are deterministic, so a dependence between `cv` and `encoder`, or between `main` and `encoder_tail` -
    which the two-stream schedule would turn into a race - shows here every time."""
    e = env_of(cid)
    plan, base = e.plan, e.base
    orders = pp.legal_orders()
    assert set(pp.REQUIRED_ORDERS) <= set(orders)
    if cid == "f32_b2_skip_layer4":
        assert not plan.stages["encoder_tail"] and "feat4" not in plan.buf and "splitk_workspace.encoder_tail" not in plan.buf
    else:
        assert plan.stages["encoder_tail"] and "feat4" in plan.buf
    stream = torch.cuda.current_stream()
    for order in orders:
        pp.poison(plan, "nan")
        torch.cuda.synchronize()
        pp.run_stages(plan, order, stream)
        torch.cuda.synchronize()
        snap = pp.snapshot(plan, e.snap_dev)
        assert_clean(snap, plan, f"{cid}, order {order}")
        assert_same_bits(snap, base, outputs_of(plan), f"{cid}, order {order}")
        lines = pp.report(base, snap)
        assert not lines, f"{cid}, order {order} vs the model-API run:\n" + "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- C. teeth
def test_teeth_a_stale_image_feature_reaches_the_depth(hip_lib):
    """Control: `encoder`, `encoder_tail` and `cv` by hand, then `feat1` overwritten with the payload NaN before `main` - what `main` would see if it
    did not wait for the encoder.  The depth must change and go non-finite (the mask and depth nets use LeakyReLU, which keeps a NaN)."""
    e = env_of("f32_b2_table")
    plan, base = e.plan, e.base
    stream = torch.cuda.current_stream()
    pp.poison(plan, "nan")
    torch.cuda.synchronize()
    plan.rebind_outputs(None)
    for stage in ("encoder", "encoder_tail", "cv"):
        plan.run_stage(stage, stream.cuda_stream)
    pp.fill(plan.buf["feat1"], "nan")
    plan.run_stage("main", stream.cuda_stream)
    torch.cuda.synchronize()
    snap = pp.snapshot(plan, e.snap_dev)
    assert not torch.equal(snap["pred0"], base["pred0"])
    assert not bool(torch.isfinite(snap["pred0"].view(torch.float32)).all())
    lines = pp.report(base, snap)
    # `feat1` itself holds the pattern and is skipped - and so does every intermediate the payload NaN went through unchanged (an fma hands on
    # the payload of its NaN operand: mask.dec1.a = 0x7fc0dead throughout).  It surfaces where the sign flips, (1 - mask) * cost_volume =
    # 0xffc0dead, and in everything the depth net makes of that; nothing that does not depend on `feat1` moved
    # (and the head's abs() flips it back: `pred0` may hold the very pattern again - then the pattern count of the outputs shows it, as in part A)
    assert lines and lines[0].startswith("cost_volume:"), lines
    assert any(l.startswith("pred0:") for l in lines) or "pred0" in pp.poisoned_elements(snap, ["pred0"]), lines
    assert not any(l.startswith(("feat", "resnet.", "sfcv", "mask.enc", "mask.cvf", "mask.dec0", "splitk_workspace.enc", "splitk_workspace.cv"))
                   for l in lines), lines
    # the gap of the report, closed: buffers behind `feat1` hold "unwritten" elements that the run from the huge value does not have
    assert [l for l in pp.unwritten_sets_differ(snap, e.poisoned_runs()["huge"]) if not l.startswith("feat1:")]
    pp.run_stages(plan, pp.REQUIRED_ORDERS[0], stream)                       # (and a plain pass puts everything back)
    torch.cuda.synchronize()
    assert pp.report(base, pp.snapshot(plan, e.snap_dev)) == []


@pytest.mark.parametrize("fill", pp.POISONS)
def test_teeth_an_illegal_stage_order_is_seen(hip_lib, fill):
    """Control of part B: `main` ahead of `encoder` - the order a missing enc_done wait would allow - from poisoned scratch.  `main` then reads image
    features nobody has written: the depth differs from the model-API run (with either pattern: the huge value needs no NaN to get through)."""
    e = env_of("f32_b2_table")
    plan, base = e.plan, e.base
    stream = torch.cuda.current_stream()
    pp.poison(plan, fill)
    torch.cuda.synchronize()
    pp.run_stages(plan, ("cv", "main", "encoder", "encoder_tail"), stream)
    torch.cuda.synchronize()
    snap = pp.snapshot(plan, e.snap_dev)
    assert not torch.equal(snap["pred0"], base["pred0"]) and not torch.equal(snap["cv_mask"], base["cv_mask"])
    assert_same_bits(snap, base, ["feat0", "feat1", "feat2", "feat3", "feat4", "sfcv"], "stages that ran on their inputs")
    # (a payload NaN can pass through an fma chain unchanged and be ignored by the report: then the pattern count of the outputs shows it)
    assert pp.report(base, snap) or pp.poisoned_elements(snap, outputs_of(plan))
    pp.run_stages(plan, pp.REQUIRED_ORDERS[1], stream)
    torch.cuda.synchronize()
    assert pp.report(base, pp.snapshot(plan, e.snap_dev)) == []


def test_teeth_split_k_workspaces_carry_nothing_between_forwards(hip_lib):
    """c2 with hip_exact_convs=True: every stage has split-K launches (asserted from conv_log - otherwise the statement below is empty).  After a
    run the workspaces do hold partial sums; overwriting `splitk_workspace.main`, and then all of them, with either pattern changes no output of
    the next forward: every finisher sums only slabs its own launch filled."""
    e = env_of("c2_direct")
    plan, base = e.plan, e.base
    for stage in pp.STAGES:
        names = {n for n, _ in plan.stages[stage]}
        split = [(c["name"], c["split_k"]) for c in plan.conv_log if c["name"] in names and c["split_k"] > 1]
        assert split, f"no split-K launch in stage {stage}: the workspace control below would assert nothing"
        ws = base[f"splitk_workspace.{stage}"]
        assert bool((ws != 0).any()), f"splitk_workspace.{stage} was never written: the control asserts nothing"
    outs = outputs_of(plan)
    for names in (["splitk_workspace.main"], [f"splitk_workspace.{s}" for s in pp.STAGES]):
        for fill in pp.POISONS:
            for n in names:
                pp.fill(plan.buf[n], fill)
            torch.cuda.synchronize()
            e.run()
            snap = pp.snapshot(plan, e.snap_dev)
            assert_same_bits(snap, base, outs, f"workspaces {names} filled with {fill}")
            assert pp.report(base, snap) == []


def test_teeth_the_report_sees_a_single_stale_element(hip_lib):
    """Control of the comparison itself on device snapshots: one element of one intermediate changed after a run is reported, by name, and one
    pattern element planted in an output is counted."""
    e = env_of("f32_b2_table")
    plan, base = e.plan, e.base
    e.run()
    assert pp.report(base, pp.snapshot(plan, DEV)) == []
    plan.buf["mask.dec2.a"].view(-1)[17] += 1.0
    pp.fill(plan.buf["pred2"].view(-1)[5:6], "huge")
    torch.cuda.synchronize()
    snap = pp.snapshot(plan, DEV)
    lines = pp.report(base, snap)
    assert len(lines) == 1 and lines[0].startswith("mask.dec2.a: 1 of ") and "flat index 17" in lines[0], lines
    assert pp.poisoned_elements(snap, outputs_of(plan)) == {"pred2": 1}
    assert not torch.equal(snap["pred2"], base["pred2"].to(DEV))
    e.run()
