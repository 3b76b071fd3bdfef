"""Host: the checker of tests/prompt_ref.py on emulated launch traces of the prompt calls.  A trace emulated from the plan
(pf_ref.emulate_*, ar_ref's embedding, frame_ref.emulate for the position-by-position launches and the tail) passes with no
flag; each injected fault of the host code that strings the prompt launches together is flagged at the launches, rows, slots or
bytes it touches and nowhere else:

  next_layer_weight   layer l + 1's weight on pf.0.wo
  other_gain          ffn_norm's gain on norm1
  resid_from_xn       the residual added from pf_xn
  stride_lp           the token rows of a ragged pass read at each prompt's own Lp
  stale_seqs          the second pass of a fill run with the first pass's pf_seqs / pf_rows
  row_plus_1          gather from row first + rows
  row_i               gather into row i instead of slots[i]
  row_lp              the single pass's copy from row Lp
  no_pos0             pos0 left out of the appended position
  slot0               the append into slot 0 instead of `slot`
  row_S               row S of pf_g written
  pos_off_minus_1     a position-by-position launch at pos_off - 1
  missing / extra     a planned launch without an entry, an entry without a planned launch
  x_row0              the tail reading ctx->x row 0 instead of row `slot`

Shapes: the MFMA prompt pass at its smallest lock-step widths (dim 1024, 8 x 128 heads over 4 kv heads, ffn 1024, 2 + 1 layers,
a 1024-entry vocabulary, whose draw is one launch) in bf16, and the position-by-position prompt at tiny_shape in f32."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ar as O
from tests import ar_ref as A
from tests import draw_ref as D
from tests import frame_ref as FR
from tests import prompt_ref as PR
from tests.shapes import make_prompt, tiny_shape
from tests.test_ar_gpu import medium_shape

_C = {}
MB = 7


def mfma_case():
    if "mfma" not in _C:
        n_text, n_sem = 497, 512
        shape = medium_shape(n_text=n_text, vocab_size=1024, n_head=8, n_local_heads=4, intermediate_size=1024, codebook_size=512, num_codebooks=2,
                             n_fast_layer=1, fast_intermediate_size=1024, max_seq_len=64, semantic_begin_id=n_text + 15,
                             semantic_end_id=n_text + 15 + n_sem - 1, im_end_id=n_text + 4)
        cfg = FR.Cfg(shape, "bf16", MB, 8)
        assert cfg.wide_ok and cfg.draw_path(0) == 0
        _C["mfma"] = (PR.PCfg(cfg), FR.weights(O.random_weights(shape, seed=0), shape, "bf16"))
    return _C["mfma"]


def pos_case():
    if "pos" not in _C:
        shape = dataclasses.replace(tiny_shape(), num_codebooks=4, max_seq_len=32)
        cfg = FR.Cfg(shape, "f32", 4, 8)
        _C["pos"] = (PR.PCfg(cfg), FR.weights(O.random_weights(shape, seed=0), shape, "f32"))
    return _C["pos"]


def start(cfg, seed=1):
    """Every slot mid-utterance: a live frame store, its own position, finite caches (a stale read is a wrong number)."""
    s, g, mb = cfg.shape, np.random.default_rng(seed), cfg.max_batch
    st = dict(tok=g.integers(0, 200, (mb, cfg.R)).astype(np.int32), pos=(9 + g.integers(0, 12, mb)).astype(np.int32),
              nf=(2 + np.arange(mb) % 3).astype(np.int32), done=(np.arange(mb) % 4 == 1).astype(np.int32),
              seq=g.integers(0, cfg.fastV, (mb, cfg.R, cfg.cap)).astype(np.int32))
    caches = {}
    for kind_, nl, Hkv, rows, hd in (("slow", s.n_layer, s.n_local_heads, cfg.n_slots, s.head_dim),
                                     ("fast", s.n_fast_layer, s.fast_n_local_heads, s.num_codebooks, s.fast_head_dim)):
        for l in range(nl):
            caches[(kind_, l)] = tuple(A.wbits(torch.from_numpy(g.standard_normal((mb, Hkv, rows, hd))).to(torch.float64), cfg.fmt) for _ in range(2))
    return st, caches


CALLS = {
    # kind 3 on slot 3 behind a 5-row restored prefix: 17 rows (the tiled attention), the tail at m0 = 3
    "at": PR.Call(PR.KIND_AT, (3,), (17,), (5,)),
    # kind 4 at slot 2
    "slow": PR.Call(PR.KIND_SLOW, (2,), (18,), (0,)),
    # kind 5, ragged, slots shuffled, one behind a prefix: 5 prompts in one pass of 54 rows
    "many": PR.Call(PR.KIND_MANY, (4, 0, 6, 2, 5), (3, 17, 1, 16, 17), (0, 7, 0, 0, 2)),
    # kind 5 in two passes of a 64-row workspace: 5 + 1 prompts
    "two": PR.Call(PR.KIND_MANY, (1, 3, 0, 5, 2, 6), (12, 11, 13, 12, 12, 9), (0, 0, 3, 0, 0, 0)),
}
_RUNS = {}


def run(which, bug=None):
    key = (which, bug)
    if key in _RUNS:
        return _RUNS[key]
    pos = which.startswith("pos")
    pc, W = pos_case() if pos else mfma_case()
    call = {"pos_at": PR.Call(PR.KIND_AT, (1,), (4,), (3,)), "pos_many": PR.Call(PR.KIND_MANY, (2, 0), (3, 2), (0, 4))}[which] if pos else CALLS[which]
    cfg = pc.frame
    prompts = [make_prompt(cfg.shape, lp, seed=10 + i, n_vq=min(2, max(lp - 2, 0))).numpy() for i, lp in enumerate(call.lps)]
    ctls = [D.Ctl(0.8, 0.7, 1.1, seed=23)]
    st, caches = start(cfg)
    pr = PR.Prompt(pc, W, call, prompts, ctls)
    trace, c1 = PR.emulate(pr, PR.blank(pc, seed=5), st, caches, bug=bug)
    rep = PR.Prompt(pc, W, call, prompts, ctls).judge(trace, caches, c1)
    _RUNS[key] = (pr, rep, trace)
    return _RUNS[key]


@pytest.mark.parametrize("which", ["at", "slow", "many", "two", "pos_at", "pos_many"])
def test_emulated_trace_passes(which):
    pr, rep, trace = run(which)
    assert not rep.flags, rep.flags[:6]
    assert rep.judged >= len(trace["launches"]) - len(rep.left_out) and rep.elements > 0
    names = [r["name"] for r in trace["launches"]]
    if which == "at":
        assert names[0] == "pf.embed" and names[names.index("pf.last") + 1] == "head" and names[-1].startswith("draw.")
        assert ("pf.l.attn", (4, -1, -1, -1)) in rep.classes and ("pf.l.wo", (PR.PF.ID_SKINNY2, -1, -1, -1)) in rep.classes
    if which == "slow":
        assert names[-1] == "pf.last"
    if which == "two":
        assert names[0] == "pass0.pf.embed" and "pass1.pf.last" in names and len(pr.plan) == 2 and len(pr.plan[1].seqs) == 1
    if which == "pos_at":
        assert names[0] == "t0.embed" and "t3.slow.1.w2" in names and "head" in names and not any(n.startswith("t3.head") for n in names)
        assert [r["pos_off"] for r in trace["launches"] if r["name"].endswith("slow.0.wqkv")] == [3, 4, 5, 6]
    if which == "pos_many":
        assert names[0] == "pass0.t0.embed" and names[-1] == "pass1.t1.slow.1.w2"


def flagged(which, bug):
    pr, rep, trace = run(which, bug)
    assert rep.flags, f"{bug} went unseen"
    return pr, rep, set(rep.flagged())


def test_next_layers_weight_on_wo():
    _, rep, names = flagged("at", ("pf.0.wo", "next_layer_weight"))
    assert names == {"pf.0.wo"}, rep.flags[:4]


def test_the_other_norms_gain():
    _, rep, names = flagged("at", ("pf.1.norm1", "other_gain"))
    assert names == {"pf.1.norm1"}, rep.flags[:4]


def test_residual_from_the_normalised_rows():
    _, rep, names = flagged("slow", ("pf.0.w2", "resid_from_xn"))
    assert names == {"pf.0.w2"}, rep.flags[:4]


def test_ragged_token_rows_at_the_prompts_own_stride():
    pr, rep, names = flagged("many", ("pf.embed", "stride_lp"))
    assert names == {"pf.embed"}, rep.flags[:4]
    rows = eval(rep.flags[0][1].split("rows ")[1].split(", cols")[0])
    assert 0 not in rows, "the first prompt's first token row sits at offset 0 under either stride"


def test_second_pass_with_the_first_passs_sequences():
    pr, rep, names = flagged("two", ("pass1", "stale_seqs"))
    # the stale rows send pass 1's appends into pass 0's slot 1: those rows of the caches after the call are no longer pass 0's
    ok = {f"pass{k}.pf.{l}.{op}" for k in (0, 1) for l in (0, 1) for op in ("append", "attn")} | {"pass1.pf.embed", "pass1.pf.last", "caches"}
    assert names <= ok, sorted(names - ok)
    assert {"pass1.pf.embed", "pass1.pf.0.append", "pass1.pf.last"} <= names
    assert any("buffer 40" in msg for n, msg in rep.flags if n == "pass1.pf.embed")


@pytest.mark.parametrize("fault", ["row_plus_1", "row_i"])
def test_gather(fault):
    _, rep, names = flagged("many", ("pf.last", fault))
    assert names == {"pf.last"}, rep.flags[:4]
    if fault == "row_i":
        assert any("outside the launch's rows" in msg for _, msg in rep.flags)


def test_single_pass_copies_row_lp():
    _, rep, names = flagged("slow", ("pf.last", "row_lp"))
    assert names == {"pf.last"}, rep.flags[:4]


def test_append_without_pos0():
    _, rep, names = flagged("at", ("pf.1.append", "no_pos0"))
    assert names <= {"pf.1.append", "pf.1.attn", "caches"} and "pf.1.append" in names, rep.flags[:4]
    assert not any("pf.0" in n for n in names)


def test_append_into_slot_0():
    _, rep, names = flagged("at", ("pf.0.append", "slot0"))
    assert names <= {"pf.0.append", "pf.0.attn", "caches"} and {"pf.0.append", "caches"} <= names, rep.flags[:4]
    assert any("slot 0" in msg for n, msg in rep.flags if n == "caches")


def test_row_s_of_pf_g_written():
    _, rep, names = flagged("slow", ("pf.1.w13", "row_S"))
    assert names == {"pf.1.w13"}, rep.flags[:4]
    assert "first at [18, 0]" in rep.flags[0][1], rep.flags[0]


def test_position_launch_one_position_early():
    _, rep, names = flagged("pos_at", ("t2.slow.0.attn", "pos_off_minus_1"))
    # position 2's append lands on the row position 1 appended: that row of the caches after the call is no longer position 1's
    assert all(n.startswith("t2.") or n in ("caches", "t1.slow.0.attn", "t1.slow.1.attn") for n in names) and "t2.slow.0.attn" in names, rep.flags[:6]


@pytest.mark.parametrize("which,name", [("many", "pf.1.norm2"), ("pos_at", "t1.slow.0.w13")])
def test_missing_and_extra_launch(which, name):
    _, rep, names = flagged(which, (name, "missing"))
    assert name in names and ("planned, not in the trace" in m for _, m in rep.flags), rep.flags[:4]
    _, rep, names = flagged(which, (name, "extra"))
    assert names == {name} and all("does not have" in m for _, m in rep.flags), rep.flags[:4]


def test_tail_reads_row_0():
    _, rep, names = flagged("at", ("tail", "x_row0"))
    assert "head" in names and not any(n.startswith("pf.") for n in names), rep.flags[:4]


def test_plan_cuts_and_classes():
    pc, _ = mfma_case()
    ps = PR.passes(pc, CALLS["two"])
    assert [[q.slot for q in p.seqs] for p in ps] == [[1, 3, 0, 5, 2], [6]] and all(p.ragged for p in ps) and ps[1].prefix == "pass1."
    assert [p.prefix for p in PR.passes(pc, PR.Call(PR.KIND_MANY, (0, 1, 2, 3), (5, 5, 5, 5), (0,) * 4))] == [f"pass{i}." for i in range(4)]
    assert not PR.PCfg(pc.frame, switches=frozenset({"FT_NO_RAGGED_PREFILL"})).ragged(5) and PR.PCfg(pc.frame, switches=frozenset({"FT_PREFILL_V0"})).v0
    rows = PR.judged_rows(513, PR.PF.ID_LIN128, [PR.PF.Seq(0, 321, 0, 0), PR.PF.Seq(321, 192, 0, 1)])
    assert {0, 7, 127, 128, 255, 256, 383, 384, 511, 512, 320, 321}.issubset(rows.tolist()) and len(rows) < 513
    assert len(PR.judged_rows(256, 0, [])) == 256
