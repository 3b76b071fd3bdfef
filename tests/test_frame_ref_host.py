"""Host: the checker of tests/frame_ref.py on emulated launch traces.  A trace emulated from the plan (the float32 emulations of
tests/ar_ref.py and tests/wide_ref.py, the reference's own draws) passes; each injected fault of the host code that strings the
launches together is flagged at the launches it touches and nowhere else:

  other_gain        one launch gets another layer's norm gain
  rows_m_minus_m0   a launch of a slot range reads its input rows at m - m0
  pair_pos0_input   the position-1 rows of the paired codebook pass are fed position 0's input
  neighbour_code    a draw leaves the q k v table row of the neighbouring row's code
  row_outside       a launch writes a row outside its range
  missing / extra   a planned launch without an entry, an entry without a planned launch

Shapes: the lock-step MFMA path at its smallest widths (dim 1024, ffn 1024, 1 + 2 layers, 3 codebooks: the paired pass, one table
step that is also the last step) in fp16 - whose large draw is one launch - and the GEMV path at tiny_shape in f32."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ar as O
from tests import ar_ref as A
from tests import draw_ref as D
from tests import frame_ref as FR
from tests.shapes import tiny_shape
from tests.test_ar_gpu import medium_shape

_C = {}


def wide_case():
    if "wide" not in _C:
        shape = dataclasses.replace(medium_shape(n_text=1009, num_codebooks=3, n_layer=1, intermediate_size=1024, fast_intermediate_size=1024),
                                    max_seq_len=32)
        cfg = FR.Cfg(shape, "fp16", 8, 8)
        W = FR.weights(O.random_weights(shape, seed=0), shape, "fp16")
        W["qkv0_tab"] = FR.emulate_qkv0_tab(cfg, W)
        _C["wide"] = (cfg, W)
    return _C["wide"]


def tiny_case():
    if "tiny" not in _C:
        shape = dataclasses.replace(tiny_shape(), num_codebooks=4, max_seq_len=32)
        cfg = FR.Cfg(shape, "f32", 6, 8)
        _C["tiny"] = (cfg, FR.weights(O.random_weights(shape, seed=0), shape, "f32"))
    return _C["tiny"]


def start(cfg, m0, M, kind, seed=1):
    """The state, the caches and the controls a call finds: every slot mid-utterance at its own position, slot m0 + 1 frozen."""
    s, g, MB = cfg.shape, np.random.default_rng(seed), cfg.max_batch
    tok = np.zeros((MB, cfg.R), dtype=np.int32)
    code = g.integers(0, s.semantic_end_id - s.semantic_begin_id + 1, MB)
    tok[:, 0], tok[:, 1] = s.semantic_begin_id + code, code
    tok[:, 2:] = g.integers(0, cfg.fastV, (MB, cfg.R - 2))
    tok[0, 0] = 7                                              # a text token: the embedding's other branch
    first = kind == "first"
    st = dict(tok=tok, pos=np.zeros(MB, dtype=np.int32) if first else (9 + g.integers(0, 12, MB)).astype(np.int32),
              nf=np.zeros(MB, dtype=np.int32) if first else (2 + np.arange(MB) % 3).astype(np.int32), done=np.zeros(MB, dtype=np.int32),
              seq=g.integers(0, cfg.fastV, (MB, cfg.R, cfg.cap)).astype(np.int32))
    if not first:
        st["done"][m0 + 1] = 1
    caches = {}
    for kind_, nl, Hkv, rows, hd in (("slow", s.n_layer, s.n_local_heads, cfg.n_slots, s.head_dim),
                                     ("fast", s.n_fast_layer, s.fast_n_local_heads, s.num_codebooks, s.fast_head_dim)):
        for l in range(nl):
            caches[(kind_, l)] = tuple(A.wbits(torch.from_numpy(g.standard_normal((MB, Hkv, rows, hd))).to(torch.float64), cfg.fmt) for _ in range(2))
    ctls = [D.Ctl(1e-6, 0.7, 1.1, seed=0) if m % 2 == 0 else D.Ctl(0.8, 0.7, 1.1, seed=11 + m) for m in range(M)]
    return st, caches, ctls


def run(case, kind, m0, M, bug=None):
    cfg, W = case
    st, caches, ctls = start(cfg, m0, M, kind)
    next_pos = [10 + i for i in range(M)] if kind == "first" else None
    fr = FR.Frame(cfg, W, kind, m0, M, ctls, pos_end=30, next_pos=next_pos)
    trace, c1 = FR.emulate(fr, FR.blank(cfg, seed=5), st, caches, bug=bug)
    rep = FR.Frame(cfg, W, kind, m0, M, ctls, pos_end=30, next_pos=next_pos).bind(trace).judge(trace, caches, c1)
    assert rep.unplaced <= max(1, rep.draw_rows // 10), (rep.unplaced, rep.draw_rows)
    return fr, rep


def consumers(fr, name):
    return {p.name for p in fr.plan if any(who == name for _, who in p.src.values())}


@pytest.mark.parametrize("which,kind,m0,M", [("wide", "decode", 0, 5), ("wide", "first", 3, 5), ("tiny", "decode", 0, 3), ("tiny", "first", 2, 3)])
def test_emulated_trace_passes(which, kind, m0, M):
    fr, rep = run(wide_case() if which == "wide" else tiny_case(), kind, m0, M)
    assert not rep.flags, rep.flags[:6]
    assert rep.judged >= len(fr.plan) - len(rep.left_out) and rep.elements > 0
    assert rep.names == {FR.generic_name(p.name) for p in fr.plan}
    assert rep.classes == FR.reached(fr.cfg, kind, m0, M, 30)
    if which == "wide":
        names = [p.name for p in fr.plan]
        assert "fast.pair.0.wqkv" in names and "fast.2.0.wqkv" not in names and "fast.2.1.wqkv" in names      # paired pass; the table step skips layer 0's Wqkv
        assert ("xo_rows" in names) == (kind == "first") and ("embed" in names) == (kind == "decode")
        assert rep.left_out == (["slow.0.attn"] if kind == "decode" else [])          # the split partials: judged at their merge


@pytest.mark.parametrize("which,kind,m0,M,name,fault", [
    ("wide", "decode", 0, 5, "fast.2.1.w13", "other_gain"),
    ("wide", "decode", 0, 5, "fast.pair.0.wqkv", "pair_pos0_input"),
    ("wide", "decode", 0, 5, "draw.1", "neighbour_code"),
    ("wide", "decode", 0, 5, "slow.0.w2", "row_outside"),
    ("wide", "first", 3, 5, "head", "rows_m_minus_m0"),
    ("wide", "first", 3, 5, "fast.pair.1.wo", "rows_m_minus_m0"),
    ("wide", "first", 3, 5, "fast.2.1.w2", "row_outside"),
    ("tiny", "first", 2, 3, "fast.3.0.wqkv", "rows_m_minus_m0"),
    ("tiny", "decode", 0, 3, "slow.1.w13", "other_gain"),
    ("tiny", "decode", 0, 3, "fast.2.1.w2", "row_outside"),
])
def test_fault_is_flagged_where_it_is(which, kind, m0, M, name, fault):
    fr, rep = run(wide_case() if which == "wide" else tiny_case(), kind, m0, M, bug=(name, fault))
    assert rep.flagged() == [name], rep.flags[:8]


@pytest.mark.parametrize("name", ["fast.2.1.wo", "head", "draw.1"])
def test_missing_and_extra_launch(name):
    fr, rep = run(wide_case(), "decode", 0, 5, bug=(name, "extra"))
    assert rep.flagged() == [name] and any("does not have" in w for _, w in rep.flags), rep.flags[:6]
    fr, rep = run(wide_case(), "decode", 0, 5, bug=(name, "missing"))
    got = set(rep.flagged())
    assert name in got and any("not in the trace" in w for n, w in rep.flags if n == name), rep.flags[:6]
    # what reads the missing launch's output finds another producer under it: those launches are touched too
    assert got - {name} <= consumers(fr, name) | {"state"}, rep.flags[:8]


def test_plan_follows_the_switches():
    cfg, _ = wide_case()
    names = lambda c, kind, m0, M: [p.name for p in FR.plan(c, kind, m0, M, 30)]
    sw = lambda *s: dataclasses.replace(cfg, switches=frozenset(s))
    assert "fast.pair.0.attn" not in names(sw("FT_NO_PAIR"), "decode", 0, 5) and "fast.1.0.wqkv" in names(sw("FT_NO_PAIR"), "decode", 0, 5)
    assert "fast.2.0.wqkv" in names(sw("FT_NO_QKV0"), "decode", 0, 5)
    assert "embed" in names(sw("FT_NO_WIDE"), "decode", 0, 5) and "xo_rows" not in names(sw("FT_NO_WIDE"), "first", 3, 5)
    assert {p.cls[0] for p in FR.plan(cfg, "decode", 0, 5, 30) if p.name == "head"} == {FR.WR.ID_HEAD}
    assert {p.cls[0] for p in FR.plan(sw("FT_NO_HEAD_STREAM"), "decode", 0, 5, 30) if p.name == "head"} == {FR.WR.ID_S11}
    big = dataclasses.replace(cfg, max_batch=40)
    assert "fast.pair.0.attn" in names(big, "decode", 0, 8) and "fast.pair.0.attn" not in names(big, "decode", 0, 40)     # 48 + 40 > 64
    assert "slow.0.attn.merge" in names(cfg, "decode", 0, 5) and "slow.0.attn.merge" not in names(big, "decode", 0, 16)   # attn_wide_kernel from 128 blocks
    assert all(p.op == "glin" or not p.name.endswith("wqkv") for p in FR.plan(cfg, "decode", 0, 3, 30))                   # 2..4 rows: the GEMV launches
