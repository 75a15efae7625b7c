"""Poisoned-scratch helpers for engine.Plan (no GPU needed to import; tests/test_plan_poison.py checks them on the CPU,
tests/test_gpu_plan_poison.py uses them on the MI355X).

Two invariants of a plan are tested with them, both bit for bit:
  1. no launch of a forward reads memory this forward has not written - every buffer the plan allocates is `torch.empty`, so a
     violation is invisible on the zero pages of a fresh process and wrong in a long-running one;
  2. the stages MonoRecModel runs side by side on two streams are independent - every legal SERIAL order of the four stages, each
     started from poisoned scratch, gives the same bits, hence so does every interleaving of two streams.

The method: fill every buffer a forward is supposed to (re)write with a recognisable bit pattern, run, and compare the raw bits of
every buffer between runs that started from different fills.  Elements that still hold a pattern were neither written nor - since
nothing downstream moved - consumed; they are ignored by `report`.  Inputs and tables are never poisoned: `geom`, `depths` and
`pix_depths` steer the sampling addresses of the cost volume; the aim is to detect stale reads, not to provoke a fault."""
import collections
import itertools
import re

import torch

from monorec_amd import engine

# fill name -> (fp32 bits, bf16 bits).  "nan": a quiet NaN with a payload (an arithmetic result is the canonical 0x7fc00000 / 0x7fc0, or
# carries another operand's payload through a conversion that drops the low 16 bits: 0x7fc0dead -> 0x7fc0 / 0x7fc1, never 0x7fdd).
# "huge": a finite value next to FLT_MAX / the largest bf16 - unlike a NaN it survives fmaxf(x, 0) (ReLU(NaN) = 0),
# and no layer of the network produces 3.4e38.  "zero": the clean baseline, what a fresh process mostly gets from the allocator.
PATTERNS = {"nan": (0x7FC0DEAD, 0x7FDD), "huge": (0x7F7FBEEF, 0x7F7F), "zero": (0, 0)}
POISONS = ("nan", "huge")
FILLS = ("zero", "nan", "huge")

INPUT, CONSTANT, OUTPUT, SCRATCH = "input", "constant", "output", "scratch"
STAGES = ("encoder", "encoder_tail", "cv", "main")

_INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
_BITS_AT = {torch.int32: 0, torch.int16: 1}


def bits(tensor):
    """The raw bits of an fp32 / bf16 tensor as an int32 / int16 view (an int32 / int16 tensor - a snapshot - is returned as it is)."""
    if tensor.dtype in _BITS_AT:
        return tensor
    if tensor.dtype not in _INT_OF:
        raise TypeError(f"plan buffers are fp32 or bf16, got {tensor.dtype}")
    return tensor.detach().view(_INT_OF[tensor.dtype])


def pattern_bits(pattern, dtype):
    """The bits of fill `pattern` for elements of `dtype` (fp32 / bf16, or the int32 / int16 of their snapshots)."""
    return PATTERNS[pattern][_BITS_AT[_INT_OF.get(dtype, dtype)]]


def fill(tensor, pattern):
    """Set every element of `tensor` to the bits of `pattern` (through an integer view: no float conversion touches the payload)."""
    b = bits(tensor)
    b.fill_(pattern_bits(pattern, b.dtype))
    return tensor


def is_poison(tensor, pattern=None):
    """Boolean map: which elements hold exactly the bits of `pattern` ("nan" / "huge"; None: either).  An ordinary NaN, inf and FLT_MAX do not."""
    b = bits(tensor)
    names = POISONS if pattern is None else (pattern,)
    if any(n not in POISONS for n in names):
        raise ValueError(f"{pattern!r} is no poison pattern (zeros are values a forward may well write)")
    hit = torch.zeros(b.shape, dtype=torch.bool, device=b.device)
    for n in names:
        hit |= b == pattern_bits(n, b.dtype)
    return hit


# ---------------------------------------------------------------------------------------------------------------- classes of plan.buf
_INPUT_NAMES = ("keyframe", "frames", "geom", "kinv", "proj", "depths", "pix_depths", "prev_depth")
# everything a forward writes and another launch of the same forward reads (or nobody: a workspace tail); a new buffer of the engine
# has to be entered here - or in another class - before the tests run again
_SCRATCH_RE = re.compile(r"""^(
    keyframe_norm | resnet\.pool | resnet\.l[1-4]b[01]\.(t|idt|o)
  | splitk_workspace\.(encoder|encoder_tail|cv|main)
  | sfcv_b8 | cost_volume_b8 | feat[0-3]_b8
  | mask\.sfcv_mean | mask\.enc[0-4]\.(a|x) | mask\.enc[1-4]\.pool | mask\.cvf[0-4] | mask\.dec[0-3]\.(up|a|x)
  | depth\.enc[0-4]\.[01]\.(mid|out)
  | depth\.dec0 | depth\.dec[12](\.t|\.mid)? | depth\.dec3 | depth\.dec4(\.mid|\.a)?
)$""", re.X)
_ZERO_FEAT_RE = re.compile(r"^mask\.zero_feat[0-3]$")


def classify(plan):
    """name -> class for every entry of `plan.buf`, in allocation order; raises on a name it cannot place.
      input     fed per forward by the model (or a table): never poisoned
      constant  zeroed when the plan is built and never written by a launch (the reference's `sfcv * 0`, `features * 0`, the zero mask of
                pretrain_mode 1, the zero volumes of no_cv) - and pretrain_mode 3's `cv_mask`, which the MODEL copies in per forward: never poisoned
      output    engine.OUTPUT_BUFFERS (without `sfcv` where the lean fusion kernel leaves raw per-frame costs in it)
      scratch   everything else a launch writes
    `plan` needs `.buf`; `.pretrain_mode`, `.no_cv` and `.lean_active` default to the full model's."""
    pm, no_cv = int(getattr(plan, "pretrain_mode", 0)), bool(getattr(plan, "no_cv", False))
    lean = bool(getattr(plan, "lean_active", False))
    out = collections.OrderedDict()
    for name in plan.buf:
        if name in _INPUT_NAMES:
            cls = INPUT
        elif name == "mask.zero_input" or _ZERO_FEAT_RE.match(name):
            cls = CONSTANT
        elif name == "cv_mask" and pm in (1, 3):
            cls = CONSTANT
        elif name in ("sfcv", "cost_volume") and no_cv:
            cls = CONSTANT
        elif name == "sfcv" and lean:
            cls = SCRATCH
        elif name in engine.OUTPUT_BUFFERS:
            cls = OUTPUT
        elif _SCRATCH_RE.match(name):
            cls = SCRATCH
        else:
            raise KeyError(f"plan buffer {name!r} is in no class of tests/plan_poison.py: say whether a forward writes it")
        out[name] = cls
    return out


def members(plan, cls):
    return [n for n, c in classify(plan).items() if c == cls]


def class_counts(plan):
    return dict(collections.Counter(classify(plan).values()))


def _span(t):
    """(storage address, first byte, one past the last byte) a tensor can touch."""
    if t.numel() == 0:
        return (t.untyped_storage().data_ptr(), 0, 0)
    lo = t.storage_offset() * t.element_size()
    extent = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return (t.untyped_storage().data_ptr(), lo, lo + extent * t.element_size())


def _overlap(a, b):
    return a[0] == b[0] and a[1] < b[2] and b[1] < a[2]


def _inside(a, b):
    return a[0] == b[0] and b[1] <= a[1] and a[2] <= b[2]


def poison(plan, pattern):
    """Fill the scratch and output classes of `plan` with `pattern`; returns the names filled.  Views are followed by storage range: a
    range is filled once, and a buffer that shares bytes with an input or a constant (as `kinv` / `proj` do with `geom`) is an error,
    not a fill.  Enqueued on the current stream: synchronise before running the plan on another one."""
    cls = classify(plan)
    keep = [(n, _span(plan.buf[n])) for n, c in cls.items() if c in (INPUT, CONSTANT)]
    todo = [(n, _span(plan.buf[n])) for n, c in cls.items() if c in (SCRATCH, OUTPUT)]
    for name, s in todo:                                   # checked for all of them before the first byte is written
        for other, k in keep:
            if _overlap(s, k):
                raise ValueError(f"{name!r} ({cls[name]}) shares memory with {other!r} ({cls[other]}): it cannot be poisoned")
    done, filled = [], []
    for name, s in todo:
        if any(_inside(s, d) for d in done):
            continue
        fill(plan.buf[name], pattern)
        done.append(s)
        filled.append(name)
    return filled


def snapshot(plan, device="cpu"):
    """name -> copy of the raw bits (int32 for fp32, int16 for bf16) of every plan buffer, in allocation order; on the CPU by default,
    `device` = the plan's for the large shapes (a device clone instead of a pageable download)."""
    return collections.OrderedDict((n, bits(t).to(device, copy=True)) for n, t in plan.buf.items())


def report(a, b, patterns=POISONS):
    """Compare two snapshots: one line per buffer, in allocation order, whose elements differ where NEITHER side holds one of `patterns` -
    the first line names the first intermediate that went wrong, and therefore the launch.  Elements a forward neither writes nor reads
    (a workspace tail, a pad lane nobody consumes) still hold the pattern on a poisoned side and are ignored by construction.  Empty = equal."""
    if isinstance(patterns, str):
        patterns = (patterns,)
    lines = []
    for name, x in a.items():
        y = b.get(name)
        if y is None or x.shape != y.shape or x.dtype != y.dtype:
            lines.append(f"{name}: present / shaped differently on the two sides")
            continue
        x = bits(x)
        y = bits(y).to(x.device)
        bad = x != y
        if not bool(bad.any()):
            continue
        for p in patterns:
            pb = pattern_bits(p, x.dtype)
            bad &= (x != pb) & (y != pb)
        n = int(bad.sum())
        if n:
            i = int(torch.nonzero(bad.reshape(-1))[0])
            mask = 0xFFFFFFFF if x.dtype == torch.int32 else 0xFFFF
            lines.append(f"{name}: {n} of {x.numel()} elements differ, first at flat index {i}: "
                         f"0x{int(x.reshape(-1)[i]) & mask:x} vs 0x{int(y.reshape(-1)[i]) & mask:x}")
    lines += [f"{name}: missing on the first side" for name in b if name not in a]
    return lines


def unwritten_sets_differ(from_nan, from_huge):
    """The elements a forward never writes are the same whatever the scratch held: where the run from the payload NaN still holds that
    NaN, the run from the huge value must hold the huge value, and nowhere else.  This closes the one gap of `report`: an fma hands on
    the payload of a NaN operand, so a stale NaN can travel through intermediates as the very pattern - which `report` takes for
    "not written" - while a stale huge value cannot.  One line per buffer whose two sets differ; empty = equal."""
    lines = []
    for name, x in from_nan.items():
        a, b = is_poison(x, "nan"), is_poison(from_huge[name], "huge").to(x.device)
        if not torch.equal(a, b):
            lines.append(f"{name}: {int(a.sum())} elements still hold the NaN pattern after the run from it, {int(b.sum())} the huge value "
                         f"after the run from that, {int((a != b).sum())} positions differ")
    return lines


def poisoned_elements(snap, names):
    """name -> number of elements of `snap[name]` that hold a poison pattern, for the names with any (an output must have none)."""
    counts = {n: int(is_poison(snap[n]).sum()) for n in names}
    return {n: k for n, k in counts.items() if k}


# the option variants the tests run (the seven of tests/test_gpu_model.py's OPTION_CASES, then cv_patch_size and sfcv_mult_mask) and the
# constant class each must have - exactly, asserted per configuration; every other configuration has none
OPTION_CASES = {"pm1": dict(pretrain_mode=1), "pm2": dict(pretrain_mode=2), "pm3": dict(pretrain_mode=3), "nocv": dict(no_cv=True),
                "mask_nocv": dict(mask_use_cv=False), "mask_nofeats": dict(mask_use_feats=False), "simple": dict(simple_mask=True),
                "patch5": dict(cv_patch_size=5), "nomult": dict(sfcv_mult_mask=False)}
EXPECTED_CONSTANTS = {"pm1": ["cv_mask"], "pm2": [], "pm3": ["cv_mask"], "nocv": ["sfcv", "cost_volume"], "mask_nocv": ["mask.zero_input"],
                      "mask_nofeats": [f"mask.zero_feat{i}" for i in range(4)], "simple": [], "patch5": [], "nomult": []}


# ---------------------------------------------------------------------------------------------------------------- stage orders
# the orders the GPU tests must run: today's one-stream order of forward(), the order of submit() (cost volume first), and the two in
# which layer4 - encoder_tail - runs after everything else, as it may on the second stream
REQUIRED_ORDERS = (("encoder", "encoder_tail", "cv", "main"), ("cv", "encoder", "encoder_tail", "main"),
                   ("cv", "encoder", "main", "encoder_tail"), ("encoder", "cv", "main", "encoder_tail"))


def legal_orders():
    """Every serial order of the four stages the two-stream schedule of MonoRecModel._submit_locked can be linearised to: `encoder` before
    `encoder_tail` (same stream) and before `main` (enc_done), `cv` before `main` (same stream); `encoder_tail` is free against `cv` and `main`."""
    ok = []
    for p in itertools.permutations(STAGES):
        at = {s: i for i, s in enumerate(p)}
        if at["encoder"] < at["encoder_tail"] and at["encoder"] < at["main"] and at["cv"] < at["main"]:
            ok.append(p)
    return ok


def run_stages(plan, order, stream):
    """Drive `plan.run_stage` by hand in `order` on `stream` (a torch stream), after one forward through the model API has bound the inputs
    and uploaded `geom`.  All four stages, each once: `main` multiplies `cost_volume` by the mask in place, so a pass without `cv` would
    apply the mask twice."""
    if sorted(order) != sorted(STAGES):
        raise ValueError(f"a hand-driven pass runs each of {STAGES} once, got {tuple(order)}")
    plan.rebind_outputs(None)
    for stage in order:
        plan.run_stage(stage, stream.cuda_stream)
