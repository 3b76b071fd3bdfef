"""GPU: a whole prompt pass held to float64 LAUNCH BY LAUNCH, in the context's own buffers.

Every kernel of the prompt pass is compared with float64 through its own hook (tests/test_pf_kernels_gpu.py) - on temporaries,
the rows starting at row 0, NaN behind them.  The host code of csrc/engine.hip that strings those launches into a prompt call
(prefill_gemm, ft_ar_prefill_at, ft_ar_prefill_slow, ft_ar_prefill_slow_many) was judged through logits and tokens only: which
layer's weight, gain and bias a launch gets, the residual's buffer, the ragged token layout at the PASS's row stride, pf_seqs /
pf_rows of a fill cut into several passes, the gather of the last rows into ctx->x, slot and pos0 in the cache base, stale
workspace rows behind a shorter prompt, the hand-over into the tail at m0 = slot, and every position-by-position prompt
(pos_off = pos0 + t).

Here the launch trace (ft_test_ar_trace_*, kinds 3, 4, 5) records every launch of one traced prompt call and
tests/prompt_ref.py recomputes each planned launch from its recorded inputs under the bounds of tests/pf_ref.py, tests/ar_ref.py
and tests/draw_ref.py, unchanged.  Every traced call runs beside an untraced twin context: the first frame, the state, ctx->x,
every cache and the debug logits bit-equal.

Shapes: the MFMA prompt path at medium_shape(n_text=1009, num_codebooks=4) - dim 1024, ffn 3072, 2 + 2 layers - with max_batch 9;
the fall-backs at tiny_shape() / tiny_shape_b().  None is the workload's own: they are the smallest at which each thing can
still go wrong."""
import contextlib
import dataclasses
import os
import time

import numpy as np
import pytest
import torch

from tests import draw_ref as D
from tests import frame_ref as FR
from tests import prompt_ref as PR
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import make_prompt, tiny_shape, tiny_shape_b
from tests.test_ar_gpu import medium_shape

pytestmark = pytest.mark.gpu

SWITCHES = ("FT_NO_ENGINE", "FT_NO_PAIR", "FT_NO_QKV0", "FT_NO_ATTN_WIDE", "FT_NO_HEAD_STREAM", "FT_NO_WIDE", "FT_NO_GRAPH", "FT_ATTN_NSPLIT", "FT_NO_XL",
            "FT_PREFILL_GEMM", "FT_PREFILL_ATTN_V0", "FT_PREFILL_V0", "FT_NO_RAGGED_PREFILL")
NEW = 8
MB = 9
_W = {}
TOTAL = FR.Report()
PREDICTED = set()
CASES = []
TIMES = []
T0 = time.time()
N_CASES = 25                                                   # traced calls the module's cases judge


def mfma_shape(msl):
    return dataclasses.replace(medium_shape(n_text=1009, num_codebooks=4), max_seq_len=msl)


def ref_weights(shape, fmt):
    """One float64 copy of a shape's weights at a time (0.7 GB at the medium shape); the rope table follows max_seq_len."""
    from fish_tts_amd.ar_engine import _rope_table
    base = dataclasses.replace(shape, max_seq_len=64)
    key = (tuple(sorted((k, str(v)) for k, v in base.__dict__.items())), fmt)
    if key not in _W:
        _W.clear()
        _W[key] = FR.weights(cached_random_weights(base, seed=0), base, fmt)
    W = dict(_W[key])
    W["rope"] = _rope_table(shape.max_seq_len, shape.head_dim, shape.rope_base).to(torch.float64)
    return W


class Ctx:
    """One engine context (the frame engine off: a traced call never runs on it) and the float64 side's view of it.  The switches
    are set for the construction and for each call (pf_attn and ft_ar_prefill_slow_many read theirs per call), and put back."""

    def __init__(self, shape, fmt, max_batch, env=None):
        from fish_tts_amd.ar_engine import ARHipEngine
        self.env = dict(env or {})
        self.shape, self.fmt = shape, fmt
        with self.switches():
            dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}[fmt]
            self.eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                                   precision="fp32" if fmt == "f32" else fmt, device=0, max_batch=max_batch, max_new_tokens=NEW)
            self.eng.load_state_dict({k: v.to(dt) for k, v in cached_random_weights(dataclasses.replace(shape, max_seq_len=64), seed=0).items()})
        self.cfg = FR.Cfg(shape, fmt, max_batch, NEW, frozenset(k for k in self.env if k == "FT_NO_WIDE"))
        self.pc = PR.PCfg(self.cfg, int(self.env.get("FT_PREFILL_GEMM", 2)), frozenset(k for k in self.env if k.startswith("FT_PREFILL_") or k == "FT_NO_RAGGED_PREFILL"))
        assert ("MFMA launches" in self.eng.frame_path()) == self.cfg.wide_ok, self.eng.frame_path()
        self.W = None

    @contextlib.contextmanager
    def switches(self):
        saved = {n: os.environ.get(n) for n in SWITCHES}
        for n in SWITCHES:
            os.environ.pop(n, None)
        os.environ["FT_NO_ENGINE"] = "1"
        os.environ.update({k: str(v) for k, v in self.env.items()})
        try:
            yield
        finally:
            for n, v in saved.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)

    def weights(self):
        if self.W is None:
            self.W = ref_weights(self.shape, self.fmt)
            self.W["qkv0_tab"] = self.eng.test_qkv0_tab(0, self.cfg.fastV) if self.cfg.wide_ok else None
        return self.W

    def close(self):
        self.eng.close()

    def sampling(self, m):
        kw = dict(temperature=0.7, top_p=1e-6, repetition_penalty=1.1, seed=0) if m % 2 == 0 else \
            dict(temperature=0.7, top_p=0.8, repetition_penalty=1.1, seed=1000 + 17 * m)
        return self.eng._sampling(ban_eos=True, **kw), D.Ctl(kw["top_p"], kw["temperature"], kw["repetition_penalty"], True, kw["seed"])

    def run(self, call, prompts):
        """The call itself; -> the first frame of a kind-3 call."""
        with self.switches():
            if call.kind == PR.KIND_AT:
                return self.eng.prefill(prompts[0], self.sampling(call.slots[0])[0], slot=call.slots[0], pos0=call.pos0s[0])
            if call.kind == PR.KIND_SLOW:
                return self.eng.prefill_slow(prompts[0], slot=call.slots[0], pos0=call.pos0s[0])
            return self.eng.prefill_slow_many(prompts, list(call.slots), pos0s=list(call.pos0s))


def prompts_of(shape, call, seed):
    return [make_prompt(shape, lp, seed=100 * seed + i, n_vq=min(2, max(lp - 2, 0))).numpy() for i, lp in enumerate(call.lps)]


def same_everything(cx, tw, call, what):
    """The traced context against its untraced twin: state, hid_in_xo, every cache, ctx->x rows and logits of the call's slots."""
    a, b = cx.eng.test_slots(), tw.eng.test_slots()
    for k in ("tok", "tokn", "pos", "nf", "done", "seq", "ctl", "hid_in_xo", "kv"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs from the untraced twin's"
    ca, cb = cx.eng.read_caches(), tw.eng.read_caches()
    for key in ca:
        assert np.array_equal(FR._bits(ca[key][0]), FR._bits(cb[key][0])) and np.array_equal(FR._bits(ca[key][1]), FR._bits(cb[key][1])), f"{what}: cache {key}"
    for m in call.slots:
        la, ha = cx.eng.debug_state(m)
        lb, hb = tw.eng.debug_state(m)
        assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32)), f"{what}: the hidden row of slot {m}"
        if call.kind == PR.KIND_AT:
            assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), f"{what}: the debug logits of slot {m}"
    return a


def settle(what, rep, t0):
    print(f"\n{what}: {rep.judged} launches judged, {rep.elements} elements, largest share of a bound {rep.worst:.3f} ({rep.worst_at}); "
          f"{rep.draw_rows} draw rows, the cut not placed by the reference in {rep.unplaced}; judged with another launch: {sorted(set(rep.left_out))}; "
          f"{time.time() - t0:.1f} s")
    assert not rep.flags, f"{what}: " + "\n".join(f"{n}: {w}" for n, w in rep.flags[:12])
    assert set(rep.left_out) <= {f"draw.0.{k}" for k in ("cut", "count", "race")}, rep.left_out
    assert rep.unplaced <= max(2, rep.draw_rows // 10), (rep.unplaced, rep.draw_rows)
    TOTAL.merge(rep)
    CASES.append(what)
    TIMES.append((time.time() - t0, what))


def traced(cx, tw, call, seed, what, prompts=None):
    """One traced call beside its untraced twin, judged.  -> (trace, report, the state after)."""
    t0 = time.time()
    prompts = prompts or prompts_of(cx.shape, call, seed)
    c0 = cx.eng.read_caches()
    cx.eng.trace_arm()
    out = cx.run(call, prompts)
    trace, c1 = cx.eng.trace_read(), cx.eng.read_caches()
    out_tw = tw.run(call, prompts)
    assert np.array_equal(out, out_tw), f"{what}: the traced call's result differs from the untraced twin's"
    after = same_everything(cx, tw, call, what)
    assert trace["kind"] == call.kind and all(r["held"] for r in trace["launches"])
    assert not after["hid_in_xo"][list(call.slots)].any(), f"{what}: a prompt pass leaves the slot's hidden state in ctx->x (hid_in_xo = 0)"
    ctls = [cx.sampling(call.slots[0])[1]] if call.kind == PR.KIND_AT else None
    rep = PR.judge(cx.pc, cx.weights(), call, prompts, ctls, trace, c0, c1)
    PREDICTED.update(PR.reached(cx.pc, call))
    settle(what, rep, t0)
    return trace, rep, after


def pair(shape, fmt, max_batch=MB, env=None):
    return Ctx(shape, fmt, max_batch, env), Ctx(shape, fmt, max_batch, env)


@contextlib.contextmanager
def two(shape, fmt, max_batch=MB, env=None):
    cx, tw = pair(shape, fmt, max_batch, env)
    try:
        yield cx, tw
    finally:
        cx.close()
        tw.close()


def cls_of(trace, name):
    return [r["cls"][0] for r in trace["launches"] if r["name"] == name][0]


def restored_prefix(cs, slot_from, n_prefill, n_keep, slot_to, seed):
    """On every context of `cs`: a prompt of n_prefill positions on slot_from, its first n_keep K/V rows restored into slot_to."""
    for c in cs:
        with c.switches():
            c.eng.prefill(make_prompt(c.shape, n_prefill, seed=seed, n_vq=2).numpy(), c.sampling(slot_from)[0], slot=slot_from)
            pf = c.eng.kv_save(n_keep, slot_from)
            c.eng.kv_restore(pf, slot_to)


# ------------------------------------------------------------------------------------------------------ the MFMA prompt path
def kind3_at_slot3(cx, tw, Lp, what=""):
    call = PR.Call(PR.KIND_AT, (3,), (Lp,), (0,))
    trace, rep, _ = traced(cx, tw, call, Lp, f"bf16 kind 3 slot 3 Lp {Lp}{what}")
    names = [r["name"] for r in trace["launches"]]
    assert names[0] == "pf.embed" and names[names.index("pf.last") + 1] == "head" and all(r["m0"] == 3 for r in trace["launches"])
    assert cls_of(trace, "pf.0.attn") == (4 if Lp >= 16 else 0)
    assert cls_of(trace, "pf.0.wqkv") == (PR.PF.ID_SKINNY1 if Lp <= 16 else PR.PF.ID_SKINNY2 if Lp <= 32 else PR.PF.ID_SKINNY4 if Lp <= 128 else PR.PF.ID_LIN64)
    assert trace["state"][1]["pos"][3] == Lp and trace["state"][1]["nf"][3] == 1


@pytest.mark.parametrize("Lp", (1, 15, 16, 17, 33))
def test_kind3_slot3_lengths(Lp):
    """Lp at pos0 = 0 on slot 3: the per-position attention inside an MFMA pass below 16 rows, skinny<1 | 2 | 4>, both sides of 16 and 32."""
    with two(mfma_shape(192), "bf16") as (cx, tw):
        kind3_at_slot3(cx, tw, Lp)


def test_kind3_stale_rows_behind_a_shorter_prompt():
    """129 rows (lingemm<64,64>, past 128), then 17 rows straight after on the same context: rows 17 .. 128 of every workspace
    buffer are finite and plausible, and must come back bit-unchanged from every launch."""
    with two(mfma_shape(192), "bf16") as (cx, tw):
        kind3_at_slot3(cx, tw, 129)
        kind3_at_slot3(cx, tw, 17, " after 129")


def test_restored_prefix_tails():
    """ft_ar_prefill_at behind a restored prefix of 24 positions: a 17-row tail (tiled) and a 3-row tail (per position, pos0 > 0)."""
    with two(mfma_shape(192), "bf16") as (cx, tw):
        restored_prefix((cx, tw), 2, 40, 24, 5, seed=7)
        for Lp in (17, 3):
            c0 = cx.eng.read_caches()
            trace, rep, _ = traced(cx, tw, PR.Call(PR.KIND_AT, (5,), (Lp,), (24,)), 30 + Lp, f"bf16 kind 3 slot 5 Lp {Lp} behind 24 restored positions")
            c1 = cx.eng.read_caches()
            for key in c0:
                if key[0] == "slow":
                    for a, b in zip(c0[key], c1[key]):
                        assert np.array_equal(a[5][:, :24], b[5][:, :24]) and np.array_equal(a[5][:, 24 + Lp:], b[5][:, 24 + Lp:]), key
                        assert not np.array_equal(a[5][:, 24:24 + Lp], b[5][:, 24:24 + Lp])
            assert cls_of(trace, "pf.1.attn") == (4 if Lp == 17 else 0) and trace["state"][1]["pos"][5] == 24 + Lp


def test_kind4_ends_at_the_last_row():
    with two(mfma_shape(192), "bf16") as (cx, tw):
        trace, rep, _ = traced(cx, tw, PR.Call(PR.KIND_SLOW, (1,), (33,), (0,)), 4, "bf16 kind 4 slot 1 Lp 33")
        assert trace["launches"][-1]["name"] == "pf.last" and trace["state"][1]["pos"][1] == 0


def live_batch(cs, n):
    """Slots 0 .. n - 1 of every context live and one lock-step frame in (on the MFMA launches: hid_in_xo = 1)."""
    for c in cs:
        with c.switches():
            ps = [make_prompt(c.shape, 9 + m, seed=500 + m, n_vq=2).numpy() for m in range(n)]
            c.eng.prefill_many(ps, [c.sampling(m)[0] for m in range(n)], slot0=0)
            c.eng.decode(1, [c.sampling(m)[0] for m in range(n)])
        assert c.eng.test_slots(kv=False)["hid_in_xo"][:n].all()


def test_kind5_ragged():
    """5 and 8 prompts as the rows of one pass (243 and 248 rows: lingemm<64,64>), slots shuffled, two behind restored prefixes with
    different pos0, one slot left out with its live utterance.  The refilled slots' hid_in_xo is cleared by the pass itself."""
    with two(mfma_shape(384), "bf16") as (cx, tw):
        live_batch((cx, tw), MB)
        before = cx.eng.test_slots()
        restored_prefix((cx, tw), 8, 40, 24, 6, seed=8)
        restored_prefix((cx, tw), 8, 30, 10, 2, seed=9)
        for c in (cx, tw):                                      # slot 8's own utterance again, one frame in
            with c.switches():
                c.eng.prefill(make_prompt(c.shape, 12, seed=508, n_vq=2).numpy(), c.sampling(8)[0], slot=8)
        call = PR.Call(PR.KIND_MANY, (6, 0, 3, 2, 7, 5, 1, 8), (33, 1, 130, 2, 15, 64, 1, 2), (24, 0, 0, 10, 0, 0, 0, 0))
        live = cx.eng.test_slots()
        trace, rep, after = traced(cx, tw, call, 5, "bf16 kind 5 ragged, 8 prompts, 248 rows")
        assert [r["name"] for r in trace["launches"]][0] == "pf.embed" and trace["launches"][-1]["rows"] == 8 and cls_of(trace, "pf.0.w13") == PR.PF.ID_LIN64
        for k in ("tok", "pos", "nf", "done", "seq", "hid_in_xo"):
            assert np.array_equal(after[k][4], live[k][4]), f"slot 4, left out, lost its {k}"
        assert after["hid_in_xo"][4] == 1 and np.array_equal(after["kv"][:, :, 4], live["kv"][:, :, 4])
        call = PR.Call(PR.KIND_MANY, (7, 2, 0, 5, 3), (130, 64, 33, 15, 1), (0,) * 5)
        trace, rep, _ = traced(cx, tw, call, 6, "bf16 kind 5 ragged, 5 prompts, 243 rows")
        assert cls_of(trace, "pf.1.attn") == 4 and before["hid_in_xo"].all()


def test_kind5_two_passes():
    """max_seq_len 128: six prompts of about 40 positions are two passes of three; the second holds fewer than wide_min sequences
    and still runs ragged."""
    with two(mfma_shape(128), "bf16") as (cx, tw):
        call = PR.Call(PR.KIND_MANY, (4, 1, 7, 0, 6, 2), (40, 41, 39, 40, 38, 42), (0,) * 6)
        trace, rep, _ = traced(cx, tw, call, 7, "bf16 kind 5 in two passes")
        names = [r["name"] for r in trace["launches"]]
        assert names[0] == "pass0.pf.embed" and "pass1.pf.embed" in names and names[-1] == "pass1.pf.last" and "pass2.pf.embed" not in names
        assert [r["rows"] for r in trace["launches"] if r["name"].endswith("pf.embed")] == [120, 120]


def test_kind5_513_rows():
    """321 + 130 + 33 + 16 + 13 rows: lingemm<128,128> on the wide products, NG = 2 (the longest above 320)."""
    with two(mfma_shape(640), "bf16") as (cx, tw):
        call = PR.Call(PR.KIND_MANY, (2, 8, 0, 5, 3), (321, 130, 33, 16, 13), (0,) * 5)
        trace, rep, _ = traced(cx, tw, call, 8, "bf16 kind 5 ragged, 513 rows")
        assert cls_of(trace, "pf.0.wqkv") == PR.PF.ID_LIN128 and cls_of(trace, "pf.0.w13") == PR.PF.ID_LIN128 and cls_of(trace, "pf.0.wo") == PR.PF.ID_LIN64
        assert cls_of(trace, "pf.0.attn") == 2


@pytest.mark.parametrize("env", [{"FT_PREFILL_GEMM": 1}, {"FT_PREFILL_GEMM": 0}, {"FT_PREFILL_ATTN_V0": 1}], ids=["gemm1", "gemm0", "attn_v0"])
def test_switches_lp33(env):
    with two(mfma_shape(192), "bf16", env=env) as (cx, tw):
        trace, rep, _ = traced(cx, tw, PR.Call(PR.KIND_AT, (3,), (33,), (0,)), 9, f"bf16 kind 3 Lp 33 {env}")
        want = {"gemm1": PR.PF.ID_LIN64, "gemm0": PR.PF.ID_TAP_128, "attn_v0": PR.PF.ID_SKINNY4}
        key = "attn_v0" if "FT_PREFILL_ATTN_V0" in env else f"gemm{env['FT_PREFILL_GEMM']}"
        assert cls_of(trace, "pf.0.wqkv") == want[key] and cls_of(trace, "pf.0.attn") == (0 if key == "attn_v0" else 4)


def test_switch_no_ragged_prefill():
    with two(mfma_shape(192), "bf16", env={"FT_NO_RAGGED_PREFILL": 1}) as (cx, tw):
        call = PR.Call(PR.KIND_MANY, (4, 0, 7, 2, 5), (17, 9, 33, 16, 20), (0,) * 5)
        trace, rep, _ = traced(cx, tw, call, 10, "bf16 kind 5, 5 prompts under FT_NO_RAGGED_PREFILL")
        assert [r["name"] for r in trace["launches"] if r["name"].endswith("pf.embed")] == [f"pass{i}.pf.embed" for i in range(5)]


# ------------------------------------------------------------------------------------------------------ the fall-backs
def test_fallback_four_single_passes():
    """bf16 medium, 4 prompts (below wide_min): one trace over four single passes, the inner calls neither end nor restart it."""
    with two(mfma_shape(192), "bf16") as (cx, tw):
        call = PR.Call(PR.KIND_MANY, (5, 1, 8, 2), (17, 3, 33, 16), (0,) * 4)
        trace, rep, _ = traced(cx, tw, call, 11, "bf16 kind 5, 4 prompts one by one")
        assert trace["M"] == 4 and [r["m0"] for r in trace["launches"] if r["name"].endswith("pf.last")] == [5, 1, 8, 2]


def test_fallback_fp16_position_by_position():
    with two(dataclasses.replace(tiny_shape(), max_seq_len=64), "fp16") as (cx, tw):
        call = PR.Call(PR.KIND_MANY, (3, 0, 6, 1, 4), (4, 2, 5, 1, 3), (0,) * 5)
        trace, rep, _ = traced(cx, tw, call, 12, "fp16 tiny kind 5, 5 prompts position by position")
        names = [r["name"] for r in trace["launches"]]
        assert names[0] == "pass0.t0.embed" and names[-1] == "pass4.t2.slow.1.w2"


@pytest.mark.parametrize("which", ["tiny", "tiny_b"])
def test_fallback_f32_kind3(which):
    """fp32: every position through the decode kernels at pos_off = pos0 + t; at pos0 = 0 and behind a 5-position restored prefix."""
    shape = dataclasses.replace(tiny_shape() if which == "tiny" else tiny_shape_b(), max_seq_len=64)
    with two(shape, "f32", max_batch=4) as (cx, tw):
        trace, rep, _ = traced(cx, tw, PR.Call(PR.KIND_AT, (1,), (9,), (0,)), 13, f"f32 {which} kind 3 slot 1 Lp 9")
        assert [r["pos_off"] for r in trace["launches"] if r["name"].endswith(".slow.0.wqkv")] == list(range(9))
        restored_prefix((cx, tw), 0, 12, 5, 1, seed=14)
        trace, rep, _ = traced(cx, tw, PR.Call(PR.KIND_AT, (1,), (9,), (5,)), 15, f"f32 {which} kind 3 slot 1 Lp 9 behind 5 restored positions")
        assert [r["pos_off"] for r in trace["launches"] if r["name"].endswith(".slow.1.attn")] == list(range(5, 14))
        assert trace["state"][1]["pos"][1] == 14 and ("fproj" in [r["name"] for r in trace["launches"]]) == (which == "tiny_b")


def test_bf16_tiny_goldens_combination():
    """What the bf16 tiny goldens rest on: head_dim 16 keeps the attention position by position inside an MFMA pass, K = 64 sends
    wqkv to tapgemm64<64,64>, N = 64 sends wo to the fall-back tapgemm<128,64>."""
    with two(dataclasses.replace(tiny_shape(), max_seq_len=64), "bf16", max_batch=4) as (cx, tw):
        trace, rep, _ = traced(cx, tw, PR.Call(PR.KIND_AT, (2,), (20,), (0,)), 16, "bf16 tiny kind 3 slot 2 Lp 20")
        assert cls_of(trace, "pf.0.wqkv") == PR.PF.ID_TAP64_64 and cls_of(trace, "pf.0.wo") == PR.PF.ID_TAP_64 and cls_of(trace, "pf.0.attn") == 0


def test_arming_rules_of_the_prompt_calls():
    """A traced kind-3 call never runs on the frame engine; an armed trace is taken by the next prompt call and by no later one."""
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import ARHipEngine, HipError
    cx = Ctx(dataclasses.replace(tiny_shape(), max_seq_len=64), "f32", 2)
    try:
        p = make_prompt(cx.shape, 3, seed=1).numpy()
        cx.eng.trace_arm()
        cx.eng.prefill_slow(p, slot=1)
        info = np.zeros(5, dtype=np.int32)
        n = cx.eng.lib.ft_test_ar_trace_count(cx.eng._h, info.ctypes.data_as(L.C.c_void_p))
        assert n > 0 and info[0] == PR.KIND_SLOW and info[3] == 0
        cx.eng.prefill_slow(p, slot=0)                                    # not armed: the record of the traced call stays
        assert cx.eng.lib.ft_test_ar_trace_count(cx.eng._h, info.ctypes.data_as(L.C.c_void_p)) == n and info[1] == 1
    finally:
        cx.close()
    shape = dataclasses.replace(medium_shape(), max_seq_len=1024)        # the widths the frame engine is instantiated for
    saved = os.environ.pop("FT_NO_ENGINE", None)
    try:
        eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id, precision="bf16", device=0,
                          max_batch=2, max_new_tokens=NEW)
        eng.load_state_dict({k: v.to(torch.bfloat16) for k, v in cached_random_weights(shape, seed=0).items()})
    finally:
        if saved is not None:
            os.environ["FT_NO_ENGINE"] = saved
    try:
        assert eng.engine_state()[0] == 3, eng.frame_path()
        eng.trace_arm()                                                  # two slots: arming is allowed, the one-row prompt call is not
        with pytest.raises(HipError) as e:
            eng.prefill(make_prompt(shape, 5, seed=1).numpy(), eng._sampling(0.7, 0.8, 1.1), slot=0)
        assert f"({L.FT_ERR_STATE})" in str(e.value), str(e.value)
    finally:
        eng.close()


def test_classes_and_names_reached():
    """Last: what the module's cases reached, against what the restated rules predict for them."""
    reached = sorted(TOTAL.classes)
    pf = sorted({k[0] for n, k in reached if n.startswith("pf.l.") and n.split(".")[-1] in ("wqkv", "wo", "w13", "w2")})
    paths = sorted({k[0] for n, k in reached if n == "pf.l.attn"})
    print(f"\nreached {len(reached)} (launch, class) pairs over {len(TOTAL.names)} launch names")
    print("PF_ID classes reached: " + ", ".join(PR.PF.ID_NAMES[i] for i in pf) + f"; attention paths {paths}")
    print("not reached: tapgemm64<128,128> (needs K % 256 != 0 at 512 rows or more: no such width here); tapgemm<128,128> is reached under FT_PREFILL_GEMM=0 only")
    print(f"all cases: {len(CASES)} traced calls, {TOTAL.judged} launches judged, {TOTAL.elements} elements, flagged {len(TOTAL.flags)}, largest share of a bound "
          f"{TOTAL.worst:.3f} ({TOTAL.worst_at}); per launch kind {({k: round(v, 3) for k, v in sorted(TOTAL.shares.items())})}; {TOTAL.draw_rows} draw rows, cut not placed in "
          f"{TOTAL.unplaced}; module wall time so far {time.time() - T0:.0f} s; slowest case {max(TIMES)[0]:.1f} s ({max(TIMES)[1]})" if TIMES else "")
    assert TOTAL.classes == PREDICTED, sorted(TOTAL.classes ^ PREDICTED)
    if len(CASES) < N_CASES:                                     # a selection of the cases ran: what follows is about all of them
        return
    assert len(CASES) == N_CASES, CASES
    assert pf == [PR.PF.ID_SKINNY1, PR.PF.ID_SKINNY2, PR.PF.ID_SKINNY4, PR.PF.ID_LIN128, PR.PF.ID_LIN64, PR.PF.ID_TAP64_64, PR.PF.ID_TAP_128, PR.PF.ID_TAP_64], pf
    assert paths == [0, 2, 4]
    assert {"pf.embed", "pf.last", "pf.l.append", "t.embed", "t.slow.l.attn", "head", "fproj", "draw.0.finish", "draw.0"} <= TOTAL.names, TOTAL.names
