"""The persistent frame engine against the launch path where a KV split outgrows the registers of an attention workgroup.

csrc/frame_engine.h keeps ENG_KVST = 6 steps of 16 cached positions per split in registers, prefetched for the workgroup's next
turn; past 96 positions per split the registers become a rolling window (the blk loop and its refill).  The bit-identity
tests of test_engine_gpu.py stop at 948 positions, where no split holds more than 64: none of them runs blk >= 1 or a refill.
The cases below do, in the XCD-local form (32 splits; wraps from 3072 positions) and in the general form (FT_NO_XL, forced
split counts, four kv heads; wraps from 96 positions at one split), and they add the other corners no test reached: splits
that are empty or hold only the new row, split counts 2 and 4, second and third attention turns of a workgroup of the general
form, a split count that changes between two decode calls of one context, the last row of the cache, and the row the last
frame appended.

Method of test_engine_gpu.py: s1-mini widths, 2 + 2 layers unless stated, bf16; prefill + decode with <|im_end|> banned so
every run has its full length; the launch path (FT_NO_ENGINE) once per case and sampling, then the slow-stack engine alone and
both engines.  First frame, every decoded frame, the frame count, the vocabulary logits and the hidden state must be equal
bit for bit; the launch path is pinned to float64 at these lengths by test_ar_kernels_gpu.py.

What ran is taken from the library (ft_test_ar_attn_plan: the split count of the last call, whether the engine is the
XCD-local kernel), never from a restatement of its choice; tests/engine_walk.py (integers only) turns the (split count, pos)
pairs that really ran into the corners of the walk they reached, and the last test asserts that those cover the required set
of both forms.  tests/test_engine_walk_host.py asserts the same of the case lists without a GPU."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import engine_walk as W
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import make_prompt
from tests.test_ar_gpu import medium_shape

pytestmark = pytest.mark.gpu


@dataclasses.dataclass(frozen=True)
class Case:
    """calls: ((frames asked of one ft_ar_decode call, the split count that call must pick), ...).  flags: the engine_state
    flags of the "slow engine only" and "both engines" runs.  greedy: also run with top_p 1e-6 (cheap cases only)."""
    name: str
    form: str                       # "xl" (the XCD-local kernel) or "general"
    max_seq_len: int
    Lp: int
    calls: tuple
    env: tuple = ()
    over: tuple = ()
    greedy: bool = False
    flags: tuple = (1, 3)

    @property
    def n_slots(self):
        return self.max_seq_len + (-self.max_seq_len) % 8

    def frames(self):
        """[(call index, split count, pos)] of every decode frame the case runs: frame i of the run is at pos = Lp + i, and a
        call stops at the last row of the cache."""
        out, pos = [], self.Lp
        for ci, (n, nsplit) in enumerate(self.calls):
            for _ in range(min(n, self.n_slots - pos)):
                out.append((ci, nsplit, pos))
                pos += 1
        return out

    def pairs(self):
        return [(ns, pos) for _, ns, pos in self.frames()]


NO_XL = (("FT_NO_XL", "1"),)


def forced(n):
    return (("FT_ATTN_NSPLIT", str(n)),)


XL_CASES = [
    Case("xl-2", "xl", 8192, 2, ((64, 32),), greedy=True),                  # empty splits, a split of only the new row, chunk 1 -> 2 -> 3
    Case("xl-3064", "xl", 8192, 3064, ((24, 32),)),                         # chunk 96 -> 97, the first wrap
    Case("xl-3096", "xl", 8192, 3096, ((16, 32),)),                         # the new row in blk 1, the skipped refill (st 0)
    Case("xl-3448", "xl", 8192, 3448, ((16, 32),)),                         # the fourth wave starts to wrap (skipped refill st 0, 1)
    Case("xl-4592", "xl", 8192, 4592, ((16, 32),)),                         # the skipped refill of st 2
    Case("xl-5616", "xl", 8192, 5616, ((16, 32),)),                         # the skipped refill of st 4
    Case("xl-6136", "xl", 8192, 6136, ((16, 32),)),                         # blk 2 (skipped refill st 4, 5)
    Case("xl-8176-end", "xl", 8192, 8176, ((24, 32),)),                     # cache end: 16 frames of 24; blk 2 on all waves, new row in blk 2
    Case("xl-4080-end", "xl", 4096, 4080, ((24, 32),)),                     # cache end of a 4096-row cache
]

GENERAL_CASES = [
    # one split
    Case("g1-88", "general", 512, 88, ((40, 1),), NO_XL, greedy=True),     # crosses 96, 97, 100, 104, 108 and 112
    Case("g1-120", "general", 512, 120, ((64, 1),), NO_XL),                 # 120..183: the skipped refill of st 1 .. 5
    Case("g1-184", "general", 512, 184, ((16, 1),), NO_XL, greedy=True),   # blk 2
    Case("g1-496-end", "general", 512, 496, ((24, 1),), NO_XL),             # to the cache end (blk 5)
    # 8 splits, fewer positions than splits
    Case("g8-2", "general", 1024, 2, ((24, 8),), NO_XL, greedy=True),      # empty splits, a split of only the new row
    # 16 splits
    Case("g16-1528", "general", 4096, 1528, ((32, 16),), NO_XL),
    Case("g16-3040", "general", 4096, 3040, ((24, 16),), NO_XL),            # chunk 192
    # 32 splits on the general merge (4 elements per workgroup and head): the call's pos_end passes 3072
    Case("g32-3060", "general", 4096, 3060, ((24, 32),), NO_XL),
    # one context, two decode calls, the split count changes between them (the engine's graph key)
    Case("g8to16-740", "general", 1024, 740, ((16, 8), (32, 16)), NO_XL),
    # forced split counts
    Case("f2-300", "general", 1024, 300, ((16, 2),), forced(2), greedy=True),
    Case("f4-300", "general", 1024, 300, ((16, 4),), forced(4), greedy=True),
    Case("f8-1000", "general", 2048, 1000, ((16, 8),), forced(8)),          # chunk 126
    # four kv heads: the general form without FT_NO_XL
    Case("kv4-1528", "general", 4096, 1528, ((16, 16),), (), (("n_local_heads", 4),)),
    Case("kv4-3096", "general", 4096, 3096, ((16, 32),), (), (("n_local_heads", 4),)),
    # second turns: the roles rotate with period 256 / (Hkv nsplit)
    Case("turns-9x8", "general", 1024, 300, ((16, 8),), NO_XL, (("n_layer", 9),)),             # period 4: three turns
    Case("turns-5x16", "general", 4096, 1600, ((16, 16),), NO_XL, (("n_layer", 5),)),          # period 2: wrapped, prefetched
    Case("turns-kv4-5x16", "general", 4096, 1600, ((16, 16),), (), (("n_layer", 5), ("n_local_heads", 4))),
]

# the last appended row: (name, form, max_seq_len, Lp of slot 0, split count, env)
LAST_ROW_CASES = [
    ("last-xl-3096", "xl", 8192, 3096, 32, ()),
    ("last-g16-1528", "general", 4096, 1528, 16, NO_XL),
]

RAN = {"xl": set(), "general": set()}           # (split count, pos) pairs that really ran on the engine
SWITCHES = ("FT_NO_ENGINE", "FT_NO_FAST_ENGINE", "FT_NO_XL", "FT_ATTN_NSPLIT", "FT_NO_PAIR", "FT_NO_QKV0", "FT_NO_RELAY",
            "FT_NO_GRAPH")
_BF16 = {}


def shape_of(max_seq_len, over):
    return dataclasses.replace(medium_shape(**dict(over)), max_seq_len=max_seq_len)


def make_engine(monkeypatch, shape, mode, env, max_batch=1, max_new_tokens=128):
    """mode: False = launch path, "slow" = the slow-stack engine only, True = both engines."""
    from fish_tts_amd.ar_engine import ARHipEngine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if not mode:
        monkeypatch.setenv("FT_NO_ENGINE", "1")
    elif mode == "slow":
        monkeypatch.setenv("FT_NO_FAST_ENGINE", "1")
    w = cached_random_weights(shape, seed=0)
    if id(w) not in _BF16:
        _BF16.clear()
        _BF16[id(w)] = {k: v.to(torch.bfloat16) for k, v in w.items()}
    eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                      precision="bf16", device=0, max_batch=max_batch, max_new_tokens=max_new_tokens)
    eng.load_state_dict(_BF16[id(w)])
    return eng


def run_case(monkeypatch, case, mode, top_p):
    shape = shape_of(case.max_seq_len, case.over)
    prompt = make_prompt(shape, case.Lp, seed=4, n_vq=max(0, case.Lp - 40)).numpy()
    eng = make_engine(monkeypatch, shape, mode, case.env, max_new_tokens=sum(n for n, _ in case.calls) + 8)
    try:
        flags = eng.engine_state()[0]
        sp = eng._sampling(0.7, top_p, 1.1, seed=7, ban_eos=True)
        first = eng.prefill(prompt, sp, slot=0)
        frames, plans = [], []
        for n, _ in case.calls:
            f, cnt = eng.decode(n, [sp], poll=64)
            frames.append(f[0, : cnt[0]].copy())
            plans.append(eng.attn_plan())
        logits, hidden = eng.debug_state()
        _, aborted, where = eng.engine_state()
    finally:
        eng.close()
    assert aborted == 0, f"{case.name}: a hand-off timed out in phase {where}"
    return dict(flags=flags, first=first, frames=frames, plans=plans, logits=logits, hidden=hidden)


def report(case, what, ci, i):
    """Where to look: the case, the differing frame, its pos and the corners of the walk that frame runs."""
    fr = [f for f in case.frames() if f[0] == ci]
    _, ns, pos = fr[min(i, len(fr) - 1)]
    return f"{case.name}: {what} differs first at frame {i} of decode call {ci}, pos {pos}: {W.describe(ns, pos)}"


def compare(case, mode, a, b):
    want_xl = 1 if case.form == "xl" else 0
    assert a["flags"] == 0 and b["flags"] == case.flags[0 if mode == "slow" else 1], (case.name, mode, a["flags"], b["flags"])
    plan = case.frames()
    for ci, (n, nsplit) in enumerate(case.calls):
        ran = [f for f in plan if f[0] == ci]
        for side, r in (("launch path", a), ("engine", b)):
            ns, xl, n_slots = r["plans"][ci]
            assert ns == nsplit, f"{case.name} call {ci}, {side}: {ns} splits, the case is written for {nsplit}"
            assert n_slots == case.n_slots, (case.name, n_slots)
            assert xl == (want_xl if side == "engine" else 0), f"{case.name}, {side}: xl {xl}"
            assert len(r["frames"][ci]) == len(ran), f"{case.name} call {ci}, {side}: {len(r['frames'][ci])} frames, expected {len(ran)}"
        RAN[case.form].update((b["plans"][ci][0], pos) for _, _, pos in ran)
    assert np.array_equal(a["first"], b["first"]), f"{case.name} {mode}: the first frame differs"
    for ci in range(len(case.calls)):
        fa, fb = a["frames"][ci], b["frames"][ci]
        if not np.array_equal(fa, fb):
            raise AssertionError(f"[{mode}] " + report(case, "the frames", ci, int(np.argmax((fa != fb).any(axis=1)))))
    last = len(case.calls) - 1
    for what in ("logits", "hidden"):
        assert np.array_equal(a[what].view(np.uint32), b[what].view(np.uint32)), \
            f"[{mode}] " + report(case, f"the last frame's {what}", last, len(a["frames"][last]) - 1)


def check_case(monkeypatch, case):
    for top_p in (0.8, 1e-6) if case.greedy else (0.8,):
        a = run_case(monkeypatch, case, False, top_p)
        for mode in ("slow", True):
            compare(case, mode, a, run_case(monkeypatch, case, mode, top_p))


@pytest.mark.parametrize("case", XL_CASES, ids=lambda c: c.name)
def test_xcd_local_engine_equals_launch_path(monkeypatch, case):
    """The default form on a chip of 8 XCDs x 32 CUs: 32 splits at every length.  The windows wrap from 3072 positions, all
    four waves from 3456, twice from 6144; at Lp 2 most splits are empty; the two -end cases are asked for 24 frames and both
    paths return the 16 the cache has room for."""
    check_case(monkeypatch, case)


@pytest.mark.parametrize("case", GENERAL_CASES, ids=lambda c: c.name)
def test_general_engine_equals_launch_path(monkeypatch, case):
    """The general form (FT_NO_XL, a forced split count, four kv heads): what other chips and the four-kv-head shape class
    run.  One split wraps from 96 positions, 16 splits from 1536; split counts 2 and 4 take the merge loop's tail; deeper
    stacks give a workgroup a second and third attention turn, planned and prefetched during the one before."""
    check_case(monkeypatch, case)


@pytest.mark.parametrize("name,form,max_seq_len,Lp,nsplit,env", LAST_ROW_CASES, ids=[c[0] for c in LAST_ROW_CASES])
def test_last_appended_row_is_read_by_the_launch_path(monkeypatch, name, form, max_seq_len, Lp, nsplit, env):
    """A frame's own K/V append is read only by later frames, so the append of a run's last engine frame escapes the
    comparisons above.  What a server does when a second caller arrives: slot 0 decodes 8 one-slot frames (the engine), slot
    1 is prefilled, then 6 two-slot lock-step frames run on the launch path and read every row the engine appended.  The
    same call sequence on an FT_NO_ENGINE context must give the same frames in both slots."""
    shape = shape_of(max_seq_len, ())
    p0 = make_prompt(shape, Lp, seed=4, n_vq=Lp - 40).numpy()
    p1 = make_prompt(shape, 24, seed=5, n_vq=3).numpy()

    def run(mode):
        eng = make_engine(monkeypatch, shape, mode, env, max_batch=2, max_new_tokens=32)
        try:
            flags = eng.engine_state()[0]
            sp = [eng._sampling(0.7, 0.8, 1.1, seed=7, ban_eos=True), eng._sampling(0.7, 0.8, 1.1, seed=8, ban_eos=True)]
            out = [eng.prefill(p0, sp[0], slot=0)]
            f, cnt = eng.decode(8, sp[:1], poll=64)
            plan = eng.attn_plan()
            out += [f[0, : cnt[0]].copy(), eng.prefill(p1, sp[1], slot=1)]
            f, cnt = eng.decode(6, sp, poll=64)
            out += [f[0, : cnt[0]].copy(), f[1, : cnt[1]].copy()]
            out += list(eng.debug_state(0)) + list(eng.debug_state(1))
            _, aborted, where = eng.engine_state()
        finally:
            eng.close()
        assert aborted == 0, f"{name}: a hand-off timed out in phase {where}"
        return flags, plan, out
    fa, pa, a = run(False)
    fb, pb, b = run(True)
    assert fa == 0 and fb == 3, (fa, fb)
    assert pa[0] == nsplit and pb[0] == nsplit and pb[1] == (1 if form == "xl" else 0) and pa[1] == 0, (pa, pb)
    assert [len(x) for x in a[1:5:2]] == [8, 6] and len(a[4]) == 6 and [len(x) for x in b[1:5:2]] == [8, 6] and len(b[4]) == 6
    RAN[form].update((pb[0], Lp + i) for i in range(8))
    names = ("first frame of slot 0", "one-slot frames of slot 0", "first frame of slot 1", "two-slot frames of slot 0",
             "two-slot frames of slot 1", "logits of slot 0", "hidden state of slot 0", "logits of slot 1", "hidden state of slot 1")
    for what, x, y in zip(names, a, b):
        same = np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else np.array_equal(x, y)
        assert same, f"{name}: the {what} differ; the last engine frame ran at pos {Lp + 7}: {W.describe(nsplit, Lp + 7)}"


def test_the_runs_reached_every_corner_of_the_walk():
    """Runs after the cases in file order (on its own there is nothing to judge: it fails and says so).  The (split count,
    pos) pairs the engine really ran, split counts as the library reported them, must reach every event of
    engine_walk.required_events for both forms."""
    for form in ("xl", "general"):
        assert RAN[form], f"no {form} case ran before this test: run the whole file"
        ev = W.events_of(RAN[form])
        missing = W.required_events(form) - ev
        print(f"\n{form}: {len(RAN[form])} (split count, pos) pairs ran, split counts {sorted({n for n, _ in RAN[form]})}, "
              f"{len(ev)} events reached")
        assert not missing, f"{form}: not reached: {sorted(missing)}"
