"""Float64 side of the launch trace of a lock-step frame (include/fishtts_hip_test.h: ft_test_ar_trace_*; host only; test
infrastructure, the sibling of tests/ar_ref.py, tests/wide_ref.py and tests/draw_ref.py, whose restatements and bounds it uses
UNCHANGED - no tolerance is defined here).

The kernels of a frame are each held to float64 through their own hooks, on temporaries, with the batch in rows 0 .. M - 1.
What no hook sees is the host code of csrc/engine.hip that strings them into a frame (slow_stack and fast_stack, enqueue_layer
under enqueue_slow and enqueue_fast_step, gemv_linear and wide_linear, enqueue_fproj, enqueue_head, enqueue_sample,
enqueue_frame_tail, the enqueue_tail of ft_ar_first_frames): which weight, gain and bias a launch gets, which buffer it
reads and writes, at which row offset m0, with how many rows in the paired codebook pass, and whether layer 0's Wqkv launch
is skipped because the draw left the table row.

`plan` restates that host code from DESIGN.md and the comments of engine.hip - from the shape, the type, max_batch, (m0, M), the
switches and the kind of call - as the ordered list of launches, each with its name, its rows and columns, the class its
dispatcher must pick (ar_ref.want_id, the wide rule below), the buffers it writes and, per input, the launch that produced
it.  `judge` walks a recorded trace against the plan: every entry must match a planned launch and every planned launch an
entry; each launch is recomputed from its RECORDED inputs, so an error is charged to the launch that made it:

  embed                       ar_ref.embed_ref; the octet-major copy is the f32 value's pattern exactly
  lock-step Linear            wide_ref.linear_ref under wide_ref.check / ar_ref.check (an f32 store holds 16-bit values)
  lock-step slow attention    wide_ref.attn_ref(splits = the class); with more than one split the partials' launch and
                              attn_combine_rows_kernel are judged as one, at the merge (as tests/test_wide_kernels_gpu.py does)
  gemv                        ar_ref.gemv_ref
  decode attention, Wo        ar_ref.decode_attn_ref + check_parts, merge_ref into gemv_ref (one split: the finished y)
  codebook attention          ar_ref.fast_attn_ref; the paired pass's position 1 from cache row 0 AS RETURNED
  xo_rows                     a copy of bits
  draws                       draw_ref.judge, as tests/test_draw_kernels_gpu.py uses it: the hook's sentinels become "this
                              element equals the record before" (see _draw_got); the four launches of the large draw are one unit

and on every buffer a launch wrote: every element of every written row inside the bound; every element the launch must not
write bit-equal to the record before (the trace's record before the first launch for a buffer's first write).  The filler
rows of the paired pass (between M and xo_pair: computed from whatever those operand rows hold, read by nobody) may change.
In every cache the appended row passes ar_ref.check_cache's conditions and every other row of every slot is bit-unchanged; the
state after the call is what the drawn codes imply, a frozen row's pos, nf, done and seq are unchanged.

The logits of a live frame are nobody's choice: where draw_ref.reference rejects a row's logits as an INPUT (BandTooWide,
NormaliserTooClose: the reference cannot place the top-p cut itself), the row keeps every condition of draw_ref.judge but the
two that read the cut, `winner` and `cut`, and is counted (Report.unplaced; a few per cent of the top-p rows).

`emulate` produces such a trace from the plan with the float32 emulations of the same modules (and the reference's own draw),
with or without an injected fault: tests/test_frame_ref_host.py."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from tests import ar_ref as A
from tests import draw_ref as D
from tests import wide_ref as WR
from tests.codec_stage_ref import F32, F64

# buffer ids of the trace (AR_TB_*, include/fishtts_hip_test.h)
(TB_X, TB_QKV, TB_Y, TB_G, TB_LOGITS, TB_HID, TB_FEMB, TB_XF, TB_QKVF, TB_GF, TB_FLOG, TB_PART_O, TB_PART_ML) = range(13)
TB_XO_X, TB_XO_XF, TB_XO_FEMB, TB_XO_Y, TB_XO_G = range(20, 25)
TB_TOKN, TB_TOK, TB_POS, TB_NF, TB_DONE, TB_SEQ, TB_CUT, TB_CHUNK_CNT, TB_PART_IDX = range(30, 39)
XO = (TB_XO_X, TB_XO_XF, TB_XO_FEMB, TB_XO_Y, TB_XO_G)
DRAW_STATE = (TB_TOKN, TB_TOK, TB_POS, TB_NF, TB_DONE, TB_SEQ, TB_FEMB)
DRAW_XO_FEMB, DRAW_XO_PAIR, DRAW_QKV0_TAB = 4, 8, 16
COMBINE = -2                                     # cls[0] of gemv_attn_combine_kernel


# ------------------------------------------------------------------------------------------------------ the context, restated
@dataclass(frozen=True)
class Cfg:
    shape: object
    fmt: str                                     # "bf16" | "fp16" | "f32"
    max_batch: int
    new: int                                     # max_new_tokens
    switches: frozenset = frozenset()            # FT_NO_PAIR, FT_NO_QKV0, FT_NO_ATTN_WIDE, FT_NO_HEAD_STREAM, FT_NO_WIDE
    cus: int = 256

    @property
    def R(self):
        return self.shape.num_codebooks + 1

    @property
    def cap(self):
        return self.new + 24

    @property
    def fastV(self):
        return min(1024, self.shape.codebook_size)

    @property
    def n_slots(self):
        return self.shape.max_seq_len + (-self.shape.max_seq_len) % 8

    @property
    def wide_ok(self):
        """ar_alloc's rule: the widths csrc/wide_kernels.h covers, a 16-bit type, FT_NO_WIDE unset."""
        s = self.shape
        HD, HDf = s.n_head * s.head_dim, s.fast_n_head * s.fast_head_dim
        qkvN, fqkvN = (s.n_head + 2 * s.n_local_heads) * s.head_dim, (s.fast_n_head + 2 * s.fast_n_local_heads) * s.fast_head_dim
        tiles = s.dim % 32 == 0 and HD % 32 == 0 and s.intermediate_size % 32 == 0
        k_ok = lambda K: K in (1024, 2048, 3072)
        return (self.fmt == "fp16" or (self.fmt == "bf16" and tiles)) and "FT_NO_WIDE" not in self.switches \
            and not s.fast_attention_qkv_bias and not s.fast_attention_o_bias and s.fast_dim == s.dim \
            and all(k_ok(K) for K in (s.dim, HD, s.intermediate_size, HDf, s.fast_intermediate_size)) \
            and qkvN % 32 == 0 and fqkvN % 32 == 0 and s.intermediate_size % 16 == 0 and s.fast_intermediate_size % 16 == 0 \
            and s.dim % 16 == 0 and s.vocab_size % 32 == 0 and self.fastV % 16 == 0

    @property
    def xo_pair(self):
        return (self.max_batch + 15) // 16 * 16 if self.wide_ok else 0

    @property
    def xo_ldm(self):
        return 2 * self.xo_pair

    def wide(self, M):
        return self.wide_ok and 5 <= M <= 64

    def pair(self, M):
        s = self.shape
        return self.wide(M) and "FT_NO_PAIR" not in self.switches and s.num_codebooks >= 2 and s.n_fast_layer > 0 and self.xo_pair + M <= 64

    @property
    def tab(self):
        s = self.shape
        return self.wide_ok and "FT_NO_QKV0" not in self.switches and s.num_codebooks > 2 and s.n_fast_layer >= 1

    def nsplit(self, pos_end):
        """The KV splits of the decode attention (ar_alloc, pick_nsplit): one kv head per XCD at 16 / 8 x 128 on a 256-CU chip
        pins 32; else 8 / 16 / 32 by the context's length, inside what the cache's length allows."""
        s, ns = self.shape, self.n_slots
        if s.n_local_heads == 8 and s.n_head == 16 and s.head_dim == 128 and self.cus == 256:
            return 32
        base = 8 if ns > 512 else 1
        cap_ = 32 if ns > 3072 else 16 if ns > 768 else base
        if cap_ <= 1:
            return base
        return min(8 if pos_end <= 768 else 16 if pos_end <= 3072 else 32, cap_)

    def draw_path(self, cb):
        V = self.shape.vocab_size if cb == 0 else self.fastV
        return 0 if V <= 1024 else 2 if self.fmt == "bf16" else 1


def wide_id(cfg: Cfg, epi: int, M: int, N: int, K: int, head: bool = False) -> int:
    """wide_gemm's choice (engine.hip), restated: WIDE_ID_*."""
    if epi == WR.RESID:
        return WR.ID_R11
    if epi == WR.SWIGLU:
        return WR.ID_G22 if M > 16 else WR.ID_G12
    if head and M <= 32 and K == 1024 and N % 16 == 0 and N >= 4096 and "FT_NO_HEAD_STREAM" not in cfg.switches:
        return WR.ID_HEAD
    if N >= 32768:
        return WR.ID_S22 if M > 16 else WR.ID_S12
    return WR.ID_S12 if N >= 4096 and M > 16 else WR.ID_S11


def wide_splits(cfg: Cfg, M: int, nsplit: int) -> int:
    """wide_attn's choice: 0 attn_wide_kernel, else the KV splits of the fall-back."""
    s = cfg.shape
    Gq = s.n_head // s.n_local_heads
    HD = s.head_dim
    lds = 4 * ((Gq + 2) * HD + 8 * Gq + 4 * (64 // max(HD // 8, 1)) * Gq * HD + Gq * cfg.n_slots)        # attn_wide_lds_floats (ar_kernels.h)
    if "FT_NO_ATTN_WIDE" not in cfg.switches and M * s.n_local_heads >= 128 and s.head_dim == 128 and Gq in (1, 2, 4) and lds <= 65536:
        return 0
    ns = 1
    while ns < nsplit and M * s.n_local_heads * ns < 256:
        ns *= 2
    return ns


# ------------------------------------------------------------------------------------------------------ the plan
@dataclass
class PL:
    name: str
    op: str
    m0: int
    rows: int
    cols: int
    cls: tuple
    writes: tuple
    src: Dict[str, tuple] = field(default_factory=dict)      # role -> (buffer id, the launch that produced it)
    a: dict = field(default_factory=dict)


def _cls(*v):
    return tuple(v) + (-1,) * (4 - len(v))


def plan(cfg: Cfg, kind: str, m0: int, M: int, pos_end: int = 0) -> List[PL]:
    """kind: "decode" (ft_ar_decode, one frame of rows 0 .. M - 1; m0 must be 0) or "first" (ft_ar_first_frames(m0, M))."""
    s, fmt = cfg.shape, cfg.fmt
    assert kind in ("decode", "first") and (kind == "first" or m0 == 0)
    ncb, D_, F, Df, Ff = s.num_codebooks, s.dim, s.intermediate_size, s.fast_dim, s.fast_intermediate_size
    H, Hkv, hd, Hf, Hkvf, hdf = s.n_head, s.n_local_heads, s.head_dim, s.fast_n_head, s.fast_n_local_heads, s.fast_head_dim
    HD, HDf, qkvN, fqkvN = H * hd, Hf * hdf, (H + 2 * Hkv) * hd, (Hf + 2 * Hkvf) * hdf
    wide, pair = cfg.wide(M), cfg.pair(M)
    out: List[PL] = []
    prod: Dict[int, str] = {}
    P = lambda b: (b, prod.get(b, "begin"))

    def add(name, op, rows, cols, cls, writes, src=None, **a):
        out.append(PL(name, op, m0, rows, cols, cls, tuple(writes), dict(src or {}), a))
        for b in writes:
            prod[b] = name

    gid = lambda epi, N, K: _cls(*A.want_id(fmt, epi, M, N, K))
    if kind == "decode":
        nsplit = cfg.nsplit(pos_end)
        add("embed", "embed", M, D_, _cls(), (TB_X, TB_XO_X) if wide else (TB_X,), wide=wide)
        for l in range(s.n_layer):
            n = f"slow.{l}"
            if wide:
                add(f"{n}.wqkv", "wlin", M, qkvN, _cls(wide_id(cfg, WR.STORE, M, qkvN, D_)), (TB_QKV,), dict(x=P(TB_XO_X)), stack="slow", l=l,
                    w="wqkv", gain="attn_norm", bias="bqkv", epi=WR.STORE, K=D_, out=TB_QKV)
                ns = wide_splits(cfg, M, nsplit)
                if ns > 1:
                    add(f"{n}.attn", "wattn_parts", M, HD, _cls(ns), (TB_PART_O, TB_PART_ML), dict(qkv=P(TB_QKV)), l=l)
                    add(f"{n}.attn.merge", "wattn", M, HD, _cls(ns), (TB_XO_Y,), dict(qkv=P(TB_QKV)), l=l, splits=ns)
                else:
                    add(f"{n}.attn", "wattn", M, HD, _cls(ns), (TB_XO_Y,), dict(qkv=P(TB_QKV)), l=l, splits=ns)
                add(f"{n}.wo", "wlin", M, D_, _cls(WR.ID_R11), (TB_XO_X,), dict(x=P(TB_XO_Y), resid=P(TB_XO_X)), stack="slow", l=l, w="wo", bias="bo",
                    epi=WR.RESID, K=HD, out=TB_XO_X)
                add(f"{n}.w13", "wlin", M, F, _cls(wide_id(cfg, WR.SWIGLU, M, 2 * F, D_)), (TB_XO_G,), dict(x=P(TB_XO_X)), stack="slow", l=l, w="w13",
                    gain="ffn_norm", epi=WR.SWIGLU, K=D_, out=TB_XO_G)
                add(f"{n}.w2", "wlin", M, D_, _cls(WR.ID_R11), (TB_XO_X,), dict(x=P(TB_XO_G), resid=P(TB_XO_X)), stack="slow", l=l, w="w2", epi=WR.RESID,
                    K=F, out=TB_XO_X)
                continue
            add(f"{n}.wqkv", "glin", M, qkvN, gid(A.EPI_STORE, qkvN, D_), (TB_QKV,), dict(x=P(TB_X)), stack="slow", l=l, w="wqkv", gain="attn_norm",
                bias="bqkv", pro=A.PRO_RMSNORM, epi=A.EPI_STORE, K=D_, out=TB_QKV)
            add(f"{n}.attn", "gattn", M, HD, _cls(nsplit), (TB_PART_O, TB_PART_ML) if nsplit > 1 else (TB_Y,), dict(qkv=P(TB_QKV)), l=l, nsplit=nsplit)
            wo_cls = _cls(COMBINE, 2 if A.rows_per_wave(D_, M) >= 2 else 1, A.pick_nt(HD, fmt)) if nsplit > 1 else gid(A.EPI_RESID, D_, HD)
            src = dict(resid=P(TB_X), po=P(TB_PART_O), pml=P(TB_PART_ML)) if nsplit > 1 else dict(resid=P(TB_X), y=P(TB_Y))
            add(f"{n}.wo", "gwo", M, D_, wo_cls, (TB_X,), src, l=l, nsplit=nsplit)
            add(f"{n}.w13", "glin", M, F, gid(A.EPI_SWIGLU, 2 * F, D_), (TB_G,), dict(x=P(TB_X)), stack="slow", l=l, w="w13", gain="ffn_norm",
                pro=A.PRO_RMSNORM, epi=A.EPI_SWIGLU, K=D_, out=TB_G)
            add(f"{n}.w2", "glin", M, D_, gid(A.EPI_RESID, D_, F), (TB_X,), dict(x=P(TB_G), resid=P(TB_X)), stack="slow", l=l, w="w2", pro=A.PRO_NONE,
                epi=A.EPI_RESID, K=F, out=TB_X)
    hidb = TB_X
    if Df != D_:
        add("fproj", "glin", M, Df, gid(A.EPI_STORE, Df, D_), (TB_HID,), dict(x=P(TB_X)), stack="top", w="fproj_w", bias="fproj_b", pro=A.PRO_NONE,
            epi=A.EPI_STORE, K=D_, out=TB_HID)
        hidb = TB_HID
    V = s.vocab_size
    if wide:
        if kind == "first":
            add("xo_rows", "xo_rows", M, D_, _cls(), (TB_XO_X,), dict(x=P(TB_X)))
        add("head", "wlin", M, V, _cls(wide_id(cfg, WR.STORE, M, V, D_, head=True)), (TB_LOGITS,), dict(x=P(TB_XO_X)), stack="top", w="head", gain="norm",
            epi=WR.STORE, K=D_, out=TB_LOGITS)
    else:
        add("head", "glin", M, V, gid(A.EPI_STORE, V, D_), (TB_LOGITS,), dict(x=P(TB_X)), stack="top", w="head", gain="norm", pro=A.PRO_RMSNORM,
            epi=A.EPI_STORE, K=D_, out=TB_LOGITS)

    def draw(cb):
        path = cfg.draw_path(cb)
        what = path
        lb = TB_LOGITS if cb == 0 else TB_FLOG
        w = (lb,) + DRAW_STATE[:6] + (TB_FEMB,)
        if wide:
            what |= DRAW_XO_PAIR if cb == 0 and pair else DRAW_XO_FEMB
            if 1 <= cb and cb + 1 < ncb and cfg.tab:
                what |= DRAW_QKV0_TAB
            w = w + (TB_XO_FEMB, TB_XO_X, TB_QKVF)
        last = cb == ncb - 1
        if path == 2:
            add(f"draw.{cb}.cut", "draw_aux", M, V, _cls(what), (TB_LOGITS, TB_CUT))
            add(f"draw.{cb}.count", "draw_aux", M, V, _cls(what), (TB_CUT, TB_CHUNK_CNT))
            add(f"draw.{cb}.race", "draw_aux", M, V, _cls(what), (TB_PART_IDX,))
        add(f"draw.{cb}" + (".finish" if path == 2 else ""), "draw", M, V if cb == 0 else cfg.fastV, _cls(what), w, dict(logits=P(lb), tokn=P(TB_TOKN)), cb=cb, last=last,
            what=what, unit=4 if path == 2 else 1)

    draw(0)

    def step(cb, pr):
        n = "fast.pair" if pr else f"fast.{cb}"
        rows = cfg.xo_pair + M if pr else M
        for l in range(s.n_fast_layer):
            if wide:
                xin = TB_XO_X if (cb == 0 or pr) else TB_XO_FEMB
                xl = xin if l == 0 else TB_XO_XF
                if not (l == 0 and cb >= 2 and not pr and cfg.tab):
                    add(f"{n}.{l}.wqkv", "wlin", rows, fqkvN, _cls(wide_id(cfg, WR.STORE, rows, fqkvN, Df)), (TB_QKVF,), dict(x=P(xl)), stack="fast", l=l,
                        w="wqkv", gain="attn_norm", epi=WR.STORE, K=Df, out=TB_QKVF, pair=pr)
                add(f"{n}.{l}.attn", "fattn", 2 * M if pr else M, HDf, _cls(), (TB_XO_Y,), dict(qkv=P(TB_QKVF)), l=l, c=cb, pair=pr, wide=True)
                add(f"{n}.{l}.wo", "wlin", rows, Df, _cls(WR.ID_R11), (TB_XO_XF,), dict(x=P(TB_XO_Y), resid=P(xl)), stack="fast", l=l, w="wo", epi=WR.RESID,
                    K=HDf, out=TB_XO_XF, pair=pr)
                add(f"{n}.{l}.w13", "wlin", rows, Ff, _cls(wide_id(cfg, WR.SWIGLU, rows, 2 * Ff, Df)), (TB_XO_G,), dict(x=P(TB_XO_XF)), stack="fast", l=l,
                    w="w13", gain="ffn_norm", epi=WR.SWIGLU, K=Df, out=TB_XO_G, pair=pr)
                add(f"{n}.{l}.w2", "wlin", rows, Df, _cls(WR.ID_R11), (TB_XO_XF,), dict(x=P(TB_XO_G), resid=P(TB_XO_XF)), stack="fast", l=l, w="w2",
                    epi=WR.RESID, K=Ff, out=TB_XO_XF, pair=pr)
                continue
            xl = (hidb if cb == 0 else TB_FEMB) if l == 0 else TB_XF
            add(f"{n}.{l}.wqkv", "glin", M, fqkvN, gid(A.EPI_STORE, fqkvN, Df), (TB_QKVF,), dict(x=P(xl)), stack="fast", l=l, w="wqkv", gain="attn_norm",
                bias="bqkv", pro=A.PRO_RMSNORM, epi=A.EPI_STORE, K=Df, out=TB_QKVF)
            add(f"{n}.{l}.attn", "fattn", M, HDf, _cls(), (TB_Y,), dict(qkv=P(TB_QKVF)), l=l, c=cb, pair=False, wide=False)
            add(f"{n}.{l}.wo", "glin", M, Df, gid(A.EPI_RESID, Df, HDf), (TB_XF,), dict(x=P(TB_Y), resid=P(xl)), stack="fast", l=l, w="wo", bias="bo",
                pro=A.PRO_NONE, epi=A.EPI_RESID, K=HDf, out=TB_XF)
            add(f"{n}.{l}.w13", "glin", M, Ff, gid(A.EPI_SWIGLU, 2 * Ff, Df), (TB_GF,), dict(x=P(TB_XF)), stack="fast", l=l, w="w13", gain="ffn_norm",
                pro=A.PRO_RMSNORM, epi=A.EPI_SWIGLU, K=Df, out=TB_GF)
            add(f"{n}.{l}.w2", "glin", M, Df, gid(A.EPI_RESID, Df, Ff), (TB_XF,), dict(x=P(TB_GF), resid=P(TB_XF)), stack="fast", l=l, w="w2", pro=A.PRO_NONE,
                epi=A.EPI_RESID, K=Ff, out=TB_XF)
        if cb == 0:
            return
        if wide:
            xb = TB_XO_XF if s.n_fast_layer > 0 else TB_XO_FEMB
            add(f"fast.{cb}.head", "wlin", M, cfg.fastV, _cls(wide_id(cfg, WR.STORE, M, cfg.fastV, Df)), (TB_FLOG,), dict(x=P(xb)), stack="top", w="fast_out",
                gain="fast_norm", epi=WR.STORE, K=Df, out=TB_FLOG, x_off=cfg.xo_pair if pr else 0)
        else:
            add(f"fast.{cb}.head", "glin", M, cfg.fastV, gid(A.EPI_STORE, cfg.fastV, Df), (TB_FLOG,), dict(x=P(TB_XF)), stack="top", w="fast_out",
                gain="fast_norm", pro=A.PRO_RMSNORM, epi=A.EPI_STORE, K=Df, out=TB_FLOG)
        draw(cb)

    cb0 = 0
    if pair:
        step(1, True)
        cb0 = 2
    for cb in range(cb0, ncb):
        step(cb, False)
    return out


# ------------------------------------------------------------------------------------------------------ weights
def weights(sd, shape, fmt: str) -> dict:
    """The state dict as the device holds it: exact values of the model's type in float64, w1 / w3 interleaved, the tied head."""
    from fish_tts_amd.ar_engine import _rope_table
    r = lambda k: A.store(sd[k].to(F64), fmt) if k in sd else None

    def layers(prefix, n):
        out = []
        for i in range(n):
            p = f"{prefix}.{i}"
            out.append(dict(wqkv=r(f"{p}.attention.wqkv.weight"), bqkv=r(f"{p}.attention.wqkv.bias"), attn_norm=r(f"{p}.attention_norm.weight"),
                            qn=r(f"{p}.attention.q_norm.weight"), kn=r(f"{p}.attention.k_norm.weight"), wo=r(f"{p}.attention.wo.weight"),
                            bo=r(f"{p}.attention.wo.bias"), ffn_norm=r(f"{p}.ffn_norm.weight"),
                            w13=WR.interleave_w13(r(f"{p}.feed_forward.w1.weight"), r(f"{p}.feed_forward.w3.weight")), w2=r(f"{p}.feed_forward.w2.weight")))
        return out
    V = min(1024, shape.codebook_size)
    top = dict(emb=r("embeddings.weight"), cb_emb=r("codebook_embeddings.weight"), norm=r("norm.weight"), fproj_w=r("fast_project_in.weight"),
               fproj_b=r("fast_project_in.bias"), fast_emb=r("fast_embeddings.weight"), fast_norm=r("fast_norm.weight"), fast_out=r("fast_output.weight")[:V])
    top["head"] = top["emb"] if shape.tie_word_embeddings else r("output.weight")
    return dict(slow=layers("layers", shape.n_layer), fast=layers("fast_layers", shape.n_fast_layer), top=top,
                rope=_rope_table(shape.max_seq_len, shape.head_dim, shape.rope_base).to(F64),
                frope=_rope_table(shape.num_codebooks, shape.fast_head_dim, shape.rope_base).to(F64), qkv0_tab=None)


# ------------------------------------------------------------------------------------------------------ buffers
def xo_read(buf: np.ndarray, rows, width: int) -> np.ndarray:
    """Octet-major [W / 8][ldm][8] -> the 16-bit patterns of `rows`, [len(rows), width]."""
    return np.ascontiguousarray(buf[:width // 8][:, np.asarray(rows), :].transpose(1, 0, 2).reshape(len(rows), width))


def xo_write(buf: np.ndarray, rows, bits: np.ndarray) -> None:
    buf[:bits.shape[1] // 8][:, np.asarray(rows), :] = bits.reshape(len(rows), -1, 8).transpose(1, 0, 2)


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _rowmask(buf: np.ndarray, bid: int, rows, cols: int) -> np.ndarray:
    """The elements a launch may write: `rows` x the first `cols` columns of buffer `bid`."""
    m = np.zeros(buf.shape, dtype=bool)
    if len(rows) == 0:
        return m
    if bid in XO:
        m[:cols // 8][:, np.asarray(rows), :] = True
    else:
        m[np.asarray(rows), :cols] = True
    return m


@dataclass
class Report:
    flags: List[tuple] = field(default_factory=list)             # (launch name, what)
    judged: int = 0
    elements: int = 0
    worst: float = 0.0
    worst_at: str = ""
    classes: set = field(default_factory=set)                    # (op, cls) reached
    names: set = field(default_factory=set)
    left_out: List[str] = field(default_factory=list)            # launches not judged on their own, by name
    draws: D.Tally = field(default_factory=D.Tally)
    draw_rows: int = 0                                           # rows of all draw launches judged ...
    unplaced: int = 0                                            # ... of which the reference could not place the top-p cut (see _draw_rows)
    shares: Dict[str, float] = field(default_factory=dict)       # launch kind (the name's last part) -> the largest share of a bound

    def flagged(self) -> List[str]:
        return sorted({n for n, _ in self.flags})

    def note(self, name, checked, worst):
        self.judged += 1
        self.elements += int(checked)
        kind = name.split(" ")[0].split(".")[-1]
        self.shares[kind] = max(self.shares.get(kind, 0.0), float(worst))
        if worst > self.worst:
            self.worst, self.worst_at = float(worst), name

    def merge(self, o: "Report"):
        self.flags += o.flags; self.judged += o.judged; self.elements += o.elements
        if o.worst > self.worst:
            self.worst, self.worst_at = o.worst, o.worst_at
        self.classes |= o.classes; self.names |= o.names; self.left_out += o.left_out
        for k, v in o.shares.items():
            self.shares[k] = max(self.shares.get(k, 0.0), v)
        self.draw_rows += o.draw_rows; self.unplaced += o.unplaced
        for k in ("probes", "left_out", "draws", "allowed"):
            setattr(self.draws, k, getattr(self.draws, k) + getattr(o.draws, k))
        self.draws.widest_band = max(self.draws.widest_band, o.draws.widest_band)


def generic_name(name: str) -> str:
    """slow.1.wqkv -> slow.l.wqkv; fast.3.0.attn -> fast.c.l.attn; draw.2 -> draw.c (what the last test lists)."""
    p = name.split(".")
    if p[0] == "slow":
        p[1] = "l"
    elif p[0] == "fast":
        if p[1] != "pair":
            p[1] = "c"
        if len(p) > 3:
            p[2] = "l"
    elif p[0] == "draw":
        p[1] = "c" if p[1] != "0" else "0"
    return ".".join(p)


def reached(cfg: Cfg, kind: str, m0: int, M: int, pos_end: int = 0) -> set:
    """The (generic name, class) pairs the restated rules predict for one call."""
    return {(generic_name(p.name), p.cls) for p in plan(cfg, kind, m0, M, pos_end)}


# ------------------------------------------------------------------------------------------------------ the walk
class Frame:
    """One traced call: the plan, the weights, the sampling controls of every slot, the caches before and after."""

    def __init__(self, cfg: Cfg, W: dict, kind: str, m0: int, M: int, ctls: List[D.Ctl], pos_end: int = 0, next_pos=None):
        self.cfg, self.W, self.kind, self.m0, self.M, self.ctls, self.next_pos = cfg, W, kind, m0, M, ctls, next_pos
        self.plan = plan(cfg, kind, m0, M, pos_end)
        s = cfg.shape
        fe = W["top"]["fast_emb"].to(F32).numpy()
        self.model = D.DrawModel(fmt=cfg.fmt, V=s.vocab_size, fastV=cfg.fastV, ncb=s.num_codebooks, cap=cfg.cap, sem_begin=s.semantic_begin_id,
                                 im_end=s.im_end_id, cbsize=s.codebook_size, fast_emb=fe, MB=cfg.max_batch, xo_pair=cfg.xo_pair,
                                 qkv0_tab=W.get("qkv0_tab"))
        self.rows = np.arange(m0, m0 + M)

    # ---- pieces shared by judge and emulate
    def _lw(self, p: PL):
        st = p.a["stack"]
        return self.W["top"] if st == "top" else self.W[st][p.a["l"]]

    def _lin_rows(self, p: PL):
        """(input rows, output rows, rows the launch may write) of a Linear."""
        r = self.rows
        if p.a.get("pair"):
            both = np.concatenate([r, r + self.cfg.xo_pair])
            return both, both, np.arange(self.m0, self.m0 + p.rows)
        return r + p.a.get("x_off", 0), r, r

    def _val(self, buf: np.ndarray, bid: int, rows, cols: int) -> torch.Tensor:
        """Exact values of `rows` x the first `cols` columns of a recorded buffer."""
        if bid in XO:
            return A.wvalues(xo_read(buf, rows, cols), self.cfg.fmt)
        return torch.from_numpy(np.ascontiguousarray(buf[np.asarray(rows), :cols])).to(F64)

    def _lin_ref(self, p: PL, cur, gain_from=None):
        fmt, lw = self.cfg.fmt, self._lw(p)
        xr, orows, _ = self._lin_rows(p)
        xb, _ = p.src["x"]
        X = self._val(cur[xb][1], xb, xr, p.a["K"])
        gain = (gain_from or lw).get(p.a.get("gain")) if p.a.get("gain") else None
        bias = lw.get(p.a.get("bias")) if p.a.get("bias") else None
        resid = None
        if "resid" in p.src:
            rb_, _ = p.src["resid"]
            resid = self._val(cur[rb_][1], rb_, xr if p.op == "wlin" else orows, p.cols)
        return X, lw[p.a["w"]], gain, bias, resid, orows

    # ---- judging
    def judge(self, trace: dict, caches0: dict, caches1: dict) -> Report:
        rep, cfg, fmt = Report(), self.cfg, self.cfg.fmt
        recs = trace["launches"]
        cur = {b: ("begin", a) for b, a in trace["begin"].items()}
        flag = lambda n, msg: rep.flags.append((n, msg))
        if trace["kind"] != (1 if self.kind == "decode" else 2) or trace["m0"] != self.m0 or trace["M"] != self.M:
            flag("call", f"the trace is of kind {trace['kind']} rows {trace['m0']}+{trace['M']}")
        # every entry a planned launch, every planned launch an entry: aligned by name (a missing or an extra entry costs that entry alone)
        i = j = 0
        pairs = []
        while i < len(self.plan) or j < len(recs):
            if i < len(self.plan) and j < len(recs) and self.plan[i].name == recs[j]["name"]:
                pairs.append((self.plan[i], recs[j])); i += 1; j += 1
            elif j < len(recs) and recs[j]["name"] not in {p.name for p in self.plan[i:]}:
                flag(recs[j]["name"], "an entry the plan does not have here"); pairs.append((None, recs[j])); j += 1
            elif j < len(recs) and j > 0 and recs[j]["name"] == recs[j - 1]["name"]:
                flag(recs[j]["name"], "an entry the plan does not have here (a second launch)"); pairs.append((None, recs[j])); j += 1
            elif i < len(self.plan):
                flag(self.plan[i].name, "planned, not in the trace"); i += 1
            else:
                flag(recs[j]["name"], "an entry the plan does not have here"); pairs.append((None, recs[j])); j += 1
        unit_prev = None
        for p, rec in pairs:
            if p is None:
                for b, a in rec["bufs"].items():
                    cur[b] = (rec["name"], a)
                continue
            rep.names.add(generic_name(p.name)); rep.classes.add((generic_name(p.name), tuple(rec["cls"])))
            if (rec["m0"], rec["rows"], rec["cols"]) != (p.m0, p.rows, p.cols):
                flag(p.name, f"m0 / rows / cols {(rec['m0'], rec['rows'], rec['cols'])}, planned {(p.m0, p.rows, p.cols)}")
            if tuple(rec["cls"]) != p.cls:
                flag(p.name, f"class {tuple(rec['cls'])}, the rules predict {p.cls}")
            if set(rec["bufs"]) != set(p.writes):
                flag(p.name, f"writes buffers {sorted(rec['bufs'])}, planned {sorted(p.writes)}")
            for role, (b, who) in p.src.items():
                if cur[b][0] != who:
                    flag(p.name, f"input {role} was last written by {cur[b][0]}, planned {who}")
            if p.op == "draw_aux" and unit_prev is None:
                unit_prev = {b: a for b, (_, a) in cur.items()}
            try:
                masks = getattr(self, "_j_" + p.op)(p, rec, cur, rep, caches0, caches1, unit_prev)
            except Exception as e:                                     # a launch the checker cannot even read is a finding of that launch
                flag(p.name, f"{type(e).__name__}: {e}")
                masks = {}
            if p.op == "draw":
                unit_prev = None
            for b, a in rec["bufs"].items():
                if b in masks and b in cur and cur[b][1] is not None:
                    keep = ~masks[b]
                    if not np.array_equal(_bits(a)[keep], _bits(cur[b][1])[keep]):
                        where = np.argwhere(keep & (_bits(a) != _bits(cur[b][1])))
                        flag(p.name, f"buffer {b}: {len(where)} elements outside the launch's rows changed, first at {where[0].tolist()}")
                cur[b] = (rec["name"], a)
        self._final(trace, cur, caches0, caches1, rep)
        return rep

    def _chk(self, p, rep, got, ref, what=""):
        """got: f32 values or 16-bit patterns of the written rows; every element, ar_ref.check (which is wide_ref.check plus,
        for an f32 store of a 16-bit model, "holds a value of the type")."""
        ver = A.check(got, ref.ref, ref.err, self.cfg.fmt)
        rep.note(p.name, ver.checked, ver.worst)
        if ver.flagged or ver.checked != ref.ref.numel():
            rep.flags.append((p.name, f"{what}{ver.flagged} of {ver.checked} elements outside the bound, worst {ver.worst:.3f}, rows {ver.rows[:8]}, cols {ver.cols[:8]}"))

    def _out_rows(self, rec, bid, rows, cols):
        buf = rec["bufs"][bid]
        return xo_read(buf, rows, cols) if bid in XO else np.ascontiguousarray(buf[np.asarray(rows), :cols])

    def _j_embed(self, p, rec, cur, rep, c0, c1, up):
        s, fmt, t = self.cfg.shape, self.cfg.fmt, self.W["top"]
        toks = self._tok0[self.rows]
        ref = A.embed_ref(fmt, t["emb"], t["cb_emb"], toks, s.num_codebooks, s.codebook_size, s.semantic_begin_id, s.semantic_end_id,
                          bool(s.scale_codebook_embeddings))
        x = self._out_rows(rec, TB_X, self.rows, s.dim)
        self._chk(p, rep, x, ref)
        masks = {TB_X: _rowmask(rec["bufs"][TB_X], TB_X, self.rows, s.dim)}
        if p.a["wide"]:
            if not np.array_equal(xo_read(rec["bufs"][TB_XO_X], self.rows, s.dim), A.wbits(torch.from_numpy(x), fmt)):
                rep.flags.append((p.name, "the octet-major copy is not the f32 value's pattern"))
            masks[TB_XO_X] = _rowmask(rec["bufs"][TB_XO_X], TB_XO_X, self.rows, s.dim)
        return masks

    def _j_wlin(self, p, rec, cur, rep, c0, c1, up):
        X, Wm, gain, bias, resid, orows = self._lin_ref(p, cur)
        ref = WR.linear_ref(self.cfg.fmt, p.a["epi"], X, Wm, gain, bias, resid, eps=self.cfg.shape.norm_eps)
        self._chk(p, rep, self._out_rows(rec, p.a["out"], orows, p.cols), ref)
        return {p.a["out"]: _rowmask(rec["bufs"][p.a["out"]], p.a["out"], self._lin_rows(p)[2], p.cols)}

    def _j_glin(self, p, rec, cur, rep, c0, c1, up):
        X, Wm, gain, bias, resid, orows = self._lin_ref(p, cur)
        ref = A.gemv_ref(self.cfg.fmt, p.a["pro"], p.a["epi"], X, Wm, gain, bias, resid, eps=self.cfg.shape.norm_eps)
        self._chk(p, rep, self._out_rows(rec, p.a["out"], orows, p.cols), ref)
        return {p.a["out"]: _rowmask(rec["bufs"][p.a["out"]], p.a["out"], orows, p.cols)}

    def _j_xo_rows(self, p, rec, cur, rep, c0, c1, up):
        x = np.ascontiguousarray(cur[TB_X][1][self.rows, :p.cols])
        if not np.array_equal(xo_read(rec["bufs"][TB_XO_X], self.rows, p.cols), A.wbits(torch.from_numpy(x), self.cfg.fmt)):
            rep.flags.append((p.name, "the octet-major rows are not the patterns of the f32 rows"))
        rep.note(p.name, len(self.rows) * p.cols, 0.0)
        return {TB_XO_X: _rowmask(rec["bufs"][TB_XO_X], TB_XO_X, self.rows, p.cols)}

    def _slow_attn_in(self, p, cur, c0):
        s, l = self.cfg.shape, p.a["l"]
        qkv = self._val(cur[TB_QKV][1], TB_QKV, self.rows, (s.n_head + 2 * s.n_local_heads) * s.head_dim)
        pos = [int(v) for v in self._pos0[self.rows]]
        lw = self.W["slow"][l]
        kc, vc = c0[("slow", l)]
        return qkv, pos, lw["qn"], lw["kn"], kc[self.rows], vc[self.rows]

    def _cache_check(self, p, rep, kc0, vc0, c1, key, pos, kref, vref):
        kc1, vc1 = c1[key]
        vk, v_ok, same = A.check_cache(self.cfg.fmt, kc0, vc0, kc1[self.rows], vc1[self.rows], pos, kref, vref)
        rep.note(p.name + " (K row)", vk.checked, vk.worst)
        if vk.flagged or not v_ok or not same:
            rep.flags.append((p.name, f"cache: appended K rows {vk.rows[:8]} worst {vk.worst:.3f}, V copies {v_ok}, other rows unchanged {same}"))

    def _j_wattn_parts(self, p, rec, cur, rep, c0, c1, up):
        rep.left_out.append(p.name)              # the partials of the split lock-step attention: judged with their merge
        return {}

    def _j_wattn(self, p, rec, cur, rep, c0, c1, up):
        s, fmt = self.cfg.shape, self.cfg.fmt
        qkv, pos, qn, kn, kc, vc = self._slow_attn_in(p, cur, c0)
        ref = WR.attn_ref(fmt, qkv, pos, qn, kn, kc, vc, self.W["rope"], s.n_head, s.n_local_heads, s.head_dim, s.norm_eps, splits=p.a["splits"])
        self._chk(p, rep, self._out_rows(rec, TB_XO_Y, self.rows, p.cols), ref.y)
        self._cache_check(p, rep, kc, vc, c1, ("slow", p.a["l"]), pos, ref.k, ref.v)
        return {TB_XO_Y: _rowmask(rec["bufs"][TB_XO_Y], TB_XO_Y, self.rows, p.cols)}

    def _parts(self, buf_o, buf_ml, ns):
        s = self.cfg.shape
        H, hd, m0, M = s.n_head, s.head_dim, self.m0, self.M
        po = buf_o.reshape(-1)[m0 * H * ns * hd:(m0 + M) * H * ns * hd].reshape(M, H, ns, hd)
        pml = buf_ml.reshape(-1)[m0 * H * ns * 2:(m0 + M) * H * ns * 2].reshape(M, H, ns, 2)
        return po, pml

    def _j_gattn(self, p, rec, cur, rep, c0, c1, up):
        s, fmt, ns = self.cfg.shape, self.cfg.fmt, p.a["nsplit"]
        H, Hkv, hd = s.n_head, s.n_local_heads, s.head_dim
        qkv, pos, qn, kn, kc, vc = self._slow_attn_in(p, cur, c0)
        if ns == 1:
            if fmt == "f32":
                pr = A.decode_attn_ref(fmt, qkv, pos, qn, kn, kc, vc, self.W["rope"], H, Hkv, hd, 1, s.norm_eps)
                yref, kref, vref = WR.Ref(pr.y[:, :, 0].reshape(self.M, -1), pr.y_err[:, :, 0].reshape(self.M, -1), None), pr.k, pr.v
            else:
                ar = WR.attn_ref(fmt, qkv, pos, qn, kn, kc, vc, self.W["rope"], H, Hkv, hd, s.norm_eps, splits=1)
                yref, kref, vref = ar.y, ar.k, ar.v
            self._chk(p, rep, self._out_rows(rec, TB_Y, self.rows, H * hd), yref)
            masks = {TB_Y: _rowmask(rec["bufs"][TB_Y], TB_Y, self.rows, H * hd)}
        else:
            pr = A.decode_attn_ref(fmt, qkv, pos, qn, kn, kc, vc, self.W["rope"], H, Hkv, hd, ns, s.norm_eps)
            kref, vref = pr.k, pr.v
            po, pml = self._parts(rec["bufs"][TB_PART_O], rec["bufs"][TB_PART_ML], ns)
            vp = A.check_parts(po, pml, pr)
            rep.note(p.name, vp.checked, vp.worst)
            if vp.flagged:
                rep.flags.append((p.name, f"partials flagged at (row, head, split) {vp.where[:8]}, worst {vp.worst:.3f}"))
            masks = {}
            for b, w in ((TB_PART_O, hd), (TB_PART_ML, 2)):
                m = np.zeros(rec["bufs"][b].shape, dtype=bool)
                m.reshape(-1)[self.m0 * H * ns * w:(self.m0 + self.M) * H * ns * w] = True
                masks[b] = m
        self._cache_check(p, rep, kc, vc, c1, ("slow", p.a["l"]), pos, kref, vref)
        return masks

    def _j_gwo(self, p, rec, cur, rep, c0, c1, up):
        s, fmt, ns = self.cfg.shape, self.cfg.fmt, p.a["nsplit"]
        lw, HD = self.W["slow"][p.a["l"]], s.n_head * s.head_dim
        resid = self._val(cur[TB_X][1], TB_X, self.rows, s.dim)
        if ns == 1:
            ref = A.gemv_ref(fmt, 0, A.EPI_RESID, self._val(cur[TB_Y][1], TB_Y, self.rows, HD), lw["wo"], bias=lw["bo"], resid=resid)
        else:
            po, pml = self._parts(cur[TB_PART_O][1], cur[TB_PART_ML][1], ns)
            _, _, yr, er = A.merge_ref(po, pml, fmt)
            ref = A.gemv_ref(fmt, 0, A.EPI_RESID, yr, lw["wo"], bias=lw["bo"], resid=resid, dx_in=er)
        self._chk(p, rep, self._out_rows(rec, TB_X, self.rows, s.dim), ref)
        return {TB_X: _rowmask(rec["bufs"][TB_X], TB_X, self.rows, s.dim)}

    def _j_fattn(self, p, rec, cur, rep, c0, c1, up):
        s, fmt, l, c = self.cfg.shape, self.cfg.fmt, p.a["l"], p.a["c"]
        H, Hkv, hd = s.fast_n_head, s.fast_n_local_heads, s.fast_head_dim
        N, lw, yb = (H + 2 * Hkv) * hd, self.W["fast"][l], TB_XO_Y if p.a["wide"] else TB_Y
        kc1, vc1 = (a[self.rows] for a in c1[("fast", l)])             # rows < c were appended earlier in this frame and judged there
        b = lambda t: A.wbits(t, fmt)
        jobs = [(0, self.rows), (1, self.rows + self.cfg.xo_pair)] if p.a["pair"] else [(c, self.rows)]
        wrote = []
        for cc, rr in jobs:
            qkv = self._val(cur[TB_QKVF][1], TB_QKVF, rr, N)
            ref = A.fast_attn_ref(fmt, qkv, cc, lw["qn"], lw["kn"], kc1, vc1, self.W["frope"], H, Hkv, hd, s.norm_eps)
            self._chk(p, rep, self._out_rows(rec, yb, rr, H * hd), ref.y, f"position {cc}: ")
            vk = A.check(kc1[:, :, cc], ref.k.ref, ref.k.err, fmt)
            rep.note(p.name + " (K row)", vk.checked, vk.worst)
            if vk.flagged or not np.array_equal(_bits(vc1[:, :, cc]), _bits(b(ref.v))):
                rep.flags.append((p.name, f"cache row {cc}: K rows {vk.rows[:8]} worst {vk.worst:.3f}, or V is not a copy"))
            wrote.append(rr)
        return {yb: _rowmask(rec["bufs"][yb], yb, np.concatenate(wrote), H * hd)}

    def _j_draw_aux(self, p, rec, cur, rep, c0, c1, up):
        rep.left_out.append(p.name)              # the first three launches of the large draw: judged as one unit at .finish
        nchunk = (self.cfg.shape.vocab_size + 1023) // 1024
        masks = {}
        for b, a in rec["bufs"].items():
            m = np.zeros(a.shape, dtype=bool)
            if b in (TB_CHUNK_CNT, TB_PART_IDX):
                m.reshape(-1)[self.m0 * nchunk:(self.m0 + self.M) * nchunk] = True
            else:
                m[self.rows] = True
            masks[b] = m
        return masks

    def _draw_got(self, p, bufs, prev):
        """What draw_ref.judge reads, from the recorded buffers: rows m0 .. of each, with the hook's sentinel wherever an
        element the launch has no business writing equals the record before (a changed one keeps its value and is flagged)."""
        cfg, M, m0, cb, what = self.cfg, self.M, self.m0, p.a["cb"], p.a["what"]
        R, n_tab, nchunk = cfg.R, 0, (cfg.shape.vocab_size + 1023) // 1024
        path = what & 3

        def sent(b, keep, fill, lo=m0, flat=False):
            if b not in bufs:                                            # a buffer this draw's records do not hold: untouched by construction
                a = prev[b]
                g = (a.reshape(-1)[lo:] if flat else a[lo:] if b not in XO else a[:, lo:, :]).copy()
                _bits(g)[...] = fill
                return g
            a, was = bufs[b], prev[b]
            if flat:
                a, was = a.reshape(-1)[lo:], was.reshape(-1)[lo:]
            elif b in XO:
                a, was = a[:, lo:, :], was[:, lo:, :]
            else:
                a, was = a[lo:], was[lo:]
            g = np.ascontiguousarray(a).copy()
            same = (_bits(g) == _bits(np.ascontiguousarray(was))) & ~keep
            _bits(g)[same] = fill
            return g
        shape_of = lambda b, flat=False, lo=m0: (prev[b].reshape(-1)[lo:] if flat else prev[b][:, lo:, :] if b in XO else prev[b][lo:]).shape
        rows_keep = lambda b: np.arange(shape_of(b)[0])[(...,) + (None,) * (len(shape_of(b)) - 1)] < M
        k_tokn = np.zeros(shape_of(TB_TOKN), dtype=bool)
        k_tokn[:M, [0, 1] if cb == 0 else [cb + 1]] = True
        k_tok = np.zeros(shape_of(TB_TOK), dtype=bool)
        k_tok[:M] = bool(p.a["last"])
        lb = TB_LOGITS if cb == 0 else TB_FLOG
        got = dict(what=what, path=path, tokn=sent(TB_TOKN, k_tokn, D.SENT), tok=sent(TB_TOK, k_tok, D.SENT),
                   seq=sent(TB_SEQ, np.broadcast_to(rows_keep(TB_SEQ), shape_of(TB_SEQ)), D.SENT).reshape(-1, R, cfg.cap),
                   logits=sent(lb, np.broadcast_to(rows_keep(lb), shape_of(lb)), D.FILL32),
                   femb=sent(TB_FEMB, np.broadcast_to(rows_keep(TB_FEMB), shape_of(TB_FEMB)), D.FILL32))
        for name, b in (("pos", TB_POS), ("nf", TB_NF), ("done", TB_DONE)):
            k = np.arange(cfg.max_batch - m0) < M
            got[name] = sent(b, k, D.SENT, flat=True)
        if p.a["last"]:
            # the hook draws into a frame of sentinels; in a real frame the other columns of tokn hold what the frame's earlier
            # draws left, and the last draw copies the whole row into tok and the frame store: those copies become the sentinel
            others = np.ones(R, dtype=bool)
            others[[0, 1] if cb == 0 else [cb + 1]] = False
            for i in range(M):
                was = prev[TB_TOKN][m0 + i]
                t = got["tok"][i]
                t[others & (t == was)] = D.SENT
                nf = int(prev[TB_NF].reshape(-1)[m0 + i])
                if not int(prev[TB_DONE].reshape(-1)[m0 + i]) and nf < cfg.cap:
                    col = got["seq"][i][:, nf]
                    col[others & (col == was)] = D.SENT
        if cfg.wide(M):
            Df = cfg.shape.fast_dim
            for name, b, used, r0 in (("xo_femb", TB_XO_FEMB, what & DRAW_XO_FEMB, 0), ("xo_x", TB_XO_X, what & DRAW_XO_PAIR, cfg.xo_pair)):
                k = np.zeros(shape_of(b), dtype=bool)
                if used:
                    k[:(Df + 7) // 8, r0:r0 + M, :] = True
                got[name] = sent(b, k, D.FILL16)
            n_tab = self.model.qkv0_tab.shape[1] if what & DRAW_QKV0_TAB else 0
        else:
            got["xo_femb"] = got["xo_x"] = None
        wq = prev[TB_QKVF].shape[1]
        kq = np.zeros(prev[TB_QKVF].reshape(-1)[m0 * wq:].shape, dtype=bool)
        kq[:M * n_tab] = True
        got["qkvf"] = sent(TB_QKVF, kq, D.FILL32, lo=m0 * wq, flat=True)
        kc_ = np.zeros(shape_of(TB_CUT), dtype=bool)
        kc_[:M] = path == 2
        got["cut"] = sent(TB_CUT, kc_, D.FILL32).view(np.uint32)
        for name, b in (("chunk_cnt", TB_CHUNK_CNT), ("part_idx", TB_PART_IDX)):
            k = np.zeros(prev[b].reshape(-1)[m0 * nchunk:].shape, dtype=bool)
            k[:M * nchunk] = path == 2
            got[name] = sent(b, k, D.FILL32, lo=m0 * nchunk, flat=True)
        return got

    def _draw_rows(self, p, prev):
        cb = p.a["cb"]
        lb = TB_LOGITS if cb == 0 else TB_FLOG
        rows = []
        for m in self.rows:
            r = D.Row(logits=np.ascontiguousarray(prev[lb][m]), ctl=self.ctls[m - self.m0], nf=int(prev[TB_NF].reshape(-1)[m]),
                      hist=prev[TB_SEQ][m].reshape(self.cfg.R, self.cfg.cap), pos=int(prev[TB_POS].reshape(-1)[m]), done=int(prev[TB_DONE].reshape(-1)[m]),
                      tag=f"{p.name} slot {m}")
            try:
                r.ref = D.reference(self.model, cb, r)
            except D.BandTooWide:
                # The logits of a live frame are nobody's choice.  Where the reference itself cannot place the top-p cut on them
                # (draw_ref: "a bad input, not a finding"; about 2 reach / p at the cut of all top-p draws, a few per cent), the
                # row keeps every other condition of the judge and loses the two that read the cut: `winner` and `cut`.
                r.ref = _reference_unplaced(self.model, cb, r)
                r.tag += " [cut not placed]"
            rows.append(r)
        return rows

    def _j_draw(self, p, rec, cur, rep, c0, c1, up):
        prev = up if up is not None else {b: a for b, (_, a) in cur.items()}
        bufs = dict(rec["bufs"])
        if p.a["unit"] > 1:                                              # cut, chunk_cnt, part_idx as the unit's earlier launches left them
            for b in (TB_CUT, TB_CHUNK_CNT, TB_PART_IDX, TB_LOGITS):
                bufs[b] = rec["bufs"].get(b, cur[b][1]) if b != TB_LOGITS else rec["bufs"][TB_LOGITS]
        rows = self._draw_rows(p, prev)
        got = self._draw_got(p, bufs, prev)
        fl = D.judge(self.model, p.a["cb"], p.a["last"], rows, got, rep.draws)
        unplaced = {i for i, r in enumerate(rows) if r.tag.endswith("[cut not placed]")}
        rep.unplaced += len(unplaced)
        rep.draw_rows += len(rows)
        fl = [f for f in fl if not (f.row in unplaced and f.field in ("winner", "cut", "chunk_cnt"))]
        rep.note(p.name, sum(np.asarray(v).size for v in got.values() if isinstance(v, np.ndarray)), 0.0)
        for f in fl:
            rep.flags.append((p.name, str(f)))
        masks, M, m0 = {}, self.M, self.m0
        for b, a in rec["bufs"].items():
            m = np.zeros(a.shape, dtype=bool)
            if b in (TB_POS, TB_NF, TB_DONE):
                m.reshape(-1)[m0:m0 + M] = True
            elif b == TB_XO_FEMB:
                m[:, m0:m0 + M, :] = bool(p.a["what"] & DRAW_XO_FEMB)
            elif b == TB_XO_X:
                m[:, m0 + self.cfg.xo_pair:m0 + self.cfg.xo_pair + M, :] = bool(p.a["what"] & DRAW_XO_PAIR)
            elif b == TB_QKVF:
                m[m0:m0 + M] = bool(p.a["what"] & DRAW_QKV0_TAB)
            else:
                m[m0:m0 + M] = True
            masks[b] = m
        return masks

    def _final(self, trace, cur, c0, c1, rep):
        """The state after the call is what the drawn codes imply; every cache row of a slot outside the call is bit-unchanged,
        and so are the slow caches of a call with no slow stack."""
        cfg, s0, s1, R = self.cfg, trace["state"][0], trace["state"][1], self.cfg.R
        tokn = cur[TB_TOKN][1]
        inside = np.zeros(cfg.max_batch, dtype=bool)
        inside[self.rows] = True
        for m in range(cfg.max_batch):
            want = {k: np.array(s0[k][m]) for k in ("tok", "pos", "nf", "done", "seq")}
            if inside[m]:
                want["tok"] = tokn[m]
                if not s0["done"][m]:
                    nf = int(s0["nf"][m])
                    if nf < cfg.cap:
                        want["seq"] = want["seq"].copy(); want["seq"][:, nf] = tokn[m]
                    want["nf"] = nf + 1
                    want["pos"] = int(s0["pos"][m]) + 1 if self.kind == "decode" else int(self.next_pos[m - self.m0])
                    want["done"] = 1 if int(tokn[m][0]) == cfg.shape.im_end_id else 0
                elif self.kind == "first":
                    want["pos"] = int(self.next_pos[m - self.m0])
            for k, w in want.items():
                if not np.array_equal(np.asarray(s1[k][m]), np.asarray(w)):
                    rep.flags.append(("state", f"slot {m} {k}: {np.asarray(s1[k][m]).reshape(-1)[:12].tolist()}, the drawn codes imply {np.asarray(w).reshape(-1)[:12].tolist()}"))
        for key in c0:
            k0, v0 = c0[key]
            k1, v1 = c1[key]
            untouched = ~inside if (key[0] == "fast" or self.kind == "decode") else np.ones(cfg.max_batch, dtype=bool)
            if not (np.array_equal(_bits(k0[untouched]), _bits(k1[untouched])) and np.array_equal(_bits(v0[untouched]), _bits(v1[untouched]))):
                rep.flags.append(("caches", f"{key}: a cache row of a slot outside the call changed"))

    def bind(self, trace):
        """The token column and the positions the call found (the record before the first launch)."""
        self._tok0, self._pos0 = trace["state"][0]["tok"], trace["state"][0]["pos"]
        return self


def _reference_unplaced(model, cb, row):
    """draw_ref.reference without its two conditions on the input (the band's width, the normaliser's reach)."""
    saved = D.MAX_BAND, D._normaliser_reach
    D.MAX_BAND, D._normaliser_reach = 1 << 30, (lambda *a, **k: 0.0)
    try:
        return D.reference(model, cb, row)
    finally:
        D.MAX_BAND, D._normaliser_reach = saved


def judge(cfg, W, kind, m0, M, ctls, trace, caches0, caches1, pos_end=0, next_pos=None) -> Report:
    return Frame(cfg, W, kind, m0, M, ctls, pos_end, next_pos).bind(trace).judge(trace, caches0, caches1)


# ------------------------------------------------------------------------------------------------------ emulation
def blank(cfg: Cfg, seed: int = 0) -> dict:
    """Every traceable buffer of a context, filled with seeded finite values of the right type (what earlier frames left)."""
    s, g = cfg.shape, np.random.default_rng(seed)
    MB, R = cfg.max_batch, cfg.R
    qkvN, fqkvN = (s.n_head + 2 * s.n_local_heads) * s.head_dim, (s.fast_n_head + 2 * s.fast_n_local_heads) * s.fast_head_dim
    y_ld = max(s.n_head * s.head_dim, s.fast_n_head * s.fast_head_dim)
    nchunk, ns = (s.vocab_size + 1023) // 1024, 32
    f = lambda r, c: A.store(torch.from_numpy(g.standard_normal((r, c))).to(F64), cfg.fmt).to(F32).numpy()
    out = {TB_X: f(MB, s.dim), TB_QKV: f(MB, qkvN), TB_Y: f(MB, y_ld), TB_G: f(MB, s.intermediate_size), TB_LOGITS: f(MB, s.vocab_size),
           TB_FEMB: f(MB, s.fast_dim), TB_XF: f(MB, s.fast_dim), TB_QKVF: f(2 * ((MB + 15) // 16 * 16), fqkvN), TB_GF: f(MB, s.fast_intermediate_size),
           TB_FLOG: f(MB, cfg.fastV), TB_PART_O: f(1, MB * s.n_head * ns * s.head_dim), TB_PART_ML: f(1, MB * s.n_head * ns * 2),
           TB_TOKN: np.zeros((MB, R), dtype=np.int32), TB_TOK: np.zeros((MB, R), dtype=np.int32), TB_POS: np.zeros((1, MB), dtype=np.int32),
           TB_NF: np.zeros((1, MB), dtype=np.int32), TB_DONE: np.zeros((1, MB), dtype=np.int32), TB_SEQ: np.zeros((MB, R * cfg.cap), dtype=np.int32),
           TB_CUT: np.zeros((MB, 8), dtype=np.int32), TB_CHUNK_CNT: np.zeros((1, MB * nchunk), dtype=np.int32),
           TB_PART_IDX: np.zeros((1, MB * nchunk), dtype=np.int32)}
    if s.fast_dim != s.dim:
        out[TB_HID] = f(MB, s.fast_dim)
    if cfg.wide_ok:
        for b, w in ((TB_XO_X, s.dim), (TB_XO_XF, s.fast_dim), (TB_XO_FEMB, s.fast_dim), (TB_XO_Y, y_ld),
                     (TB_XO_G, max(s.intermediate_size, s.fast_intermediate_size))):
            out[b] = A.wbits(torch.from_numpy(g.standard_normal((w // 8, cfg.xo_ldm, 8))).to(F64), cfg.fmt)
    return out


def emulate(fr: Frame, begin: dict, state0: dict, caches0: dict, bug: Optional[tuple] = None):
    """A trace (the dict ARHipEngine.trace_read returns) and the caches after the call, from the plan and the float32
    emulations of tests/ar_ref.py and tests/wide_ref.py.  bug = (launch name, fault): see tests/test_frame_ref_host.py."""
    cfg, fmt, s, W = fr.cfg, fr.cfg.fmt, fr.cfg.shape, fr.W
    rows, M, m0 = fr.rows, fr.M, fr.m0
    cur = {b: ("begin", a.copy()) for b, a in begin.items()}
    c1 = {k: (kc.copy(), vc.copy()) for k, (kc, vc) in caches0.items()}
    st = {k: np.array(v) for k, v in state0.items()}
    fr._tok0, fr._pos0 = st["tok"], st["pos"]
    cur[TB_TOK] = ("begin", st["tok"].copy()); cur[TB_POS] = ("begin", st["pos"].reshape(1, -1).copy())
    cur[TB_NF] = ("begin", st["nf"].reshape(1, -1).copy()); cur[TB_DONE] = ("begin", st["done"].reshape(1, -1).copy())
    cur[TB_SEQ] = ("begin", st["seq"].reshape(cfg.max_batch, -1).copy())
    begin = {b: a.copy() for b, (_, a) in cur.items()}
    recs = []
    val16 = lambda t: A.wbits(t, fmt)

    def put(buf, bid, rr, v):
        if bid in XO:
            xo_write(buf, rr, val16(v))
        else:
            buf[np.asarray(rr), :v.shape[1]] = v.to(F32).numpy()

    for p in fr.plan:
        fault = bug[1] if bug and bug[0] == p.name else None
        out = {b: cur[b][1].copy() for b in p.writes}
        if p.op == "embed":
            t = W["top"]
            v = A.emulate_embed(fmt, t["emb"], t["cb_emb"], st["tok"][rows], s.num_codebooks, s.codebook_size, s.semantic_begin_id, s.semantic_end_id,
                                bool(s.scale_codebook_embeddings))
            put(out[TB_X], TB_X, rows, v)
            if p.a["wide"]:
                put(out[TB_XO_X], TB_XO_X, rows, v)
        elif p.op in ("wlin", "glin"):
            other = None
            if fault == "other_gain":
                other = W[p.a["stack"]][(p.a["l"] + 1) % len(W[p.a["stack"]])]
            X, Wm, gain, bias, resid, orows = fr._lin_ref(p, cur, gain_from=other)
            xb = p.src["x"][0]
            if fault == "rows_m_minus_m0":
                X = fr._val(cur[xb][1], xb, fr._lin_rows(p)[0] - m0, p.a["K"])
            if fault == "pair_pos0_input":
                X = torch.cat([X[:M], X[:M]])
            if p.op == "wlin":
                v = WR.emulate_linear(fmt, p.a["epi"], X, Wm, gain, bias, resid, eps=s.norm_eps)
            else:
                v = A.emulate_gemv(fmt, p.a["pro"], p.a["epi"], X, Wm, gain, bias, resid, eps=s.norm_eps)
            put(out[p.a["out"]], p.a["out"], orows, v)
            if fault == "row_outside":
                put(out[p.a["out"]], p.a["out"], [int(orows[-1]) + 1], v[-1:])
        elif p.op == "xo_rows":
            put(out[TB_XO_X], TB_XO_X, rows, torch.from_numpy(cur[TB_X][1][rows, :p.cols]).to(F64))
        elif p.op in ("wattn", "gattn"):
            H, Hkv, hd = s.n_head, s.n_local_heads, s.head_dim
            qkv, pos, qn, kn, kc, vc = fr._slow_attn_in(p, cur, caches0)
            if p.op == "wattn":
                y, k = WR.emulate_attn(fmt, qkv.to(F32), pos, None if qn is None else qn.to(F32), None if kn is None else kn.to(F32), kc, vc, W["rope"], H, Hkv, hd, s.norm_eps)
                put(out[TB_XO_Y], TB_XO_Y, rows, y)
            else:
                assert p.a["nsplit"] == 1, "the emulated GEMV frame keeps one KV split"
                po, pml, k, _, _ = A.emulate_decode_attn(fmt, qkv.to(F32), pos, qn, kn, kc, vc, W["rope"], H, Hkv, hd, 1, s.norm_eps)
                put(out[TB_Y], TB_Y, rows, A.emulate_merge(fmt, po, pml))
            K1, V1 = c1[("slow", p.a["l"])]
            v = qkv[:, (H + Hkv) * hd:].reshape(M, Hkv, hd)
            for i, m in enumerate(rows):
                K1[m, :, pos[i]], V1[m, :, pos[i]] = val16(k[i]), val16(v[i])
        elif p.op == "wattn_parts":
            pass
        elif p.op == "gwo":
            lw, HD = W["slow"][p.a["l"]], s.n_head * s.head_dim
            v = A.emulate_gemv(fmt, 0, A.EPI_RESID, fr._val(cur[TB_Y][1], TB_Y, rows, HD), lw["wo"], None, lw["bo"], fr._val(cur[TB_X][1], TB_X, rows, s.dim))
            put(out[TB_X], TB_X, rows, v)
        elif p.op == "fattn":
            H, Hkv, hd = s.fast_n_head, s.fast_n_local_heads, s.fast_head_dim
            N, lw, yb = (H + 2 * Hkv) * hd, W["fast"][p.a["l"]], TB_XO_Y if p.a["wide"] else TB_Y
            K1, V1 = c1[("fast", p.a["l"])]
            q0 = None
            for cc, rr in ([(0, rows), (1, rows + cfg.xo_pair)] if p.a["pair"] else [(p.a["c"], rows)]):
                qkv = fr._val(cur[TB_QKVF][1], TB_QKVF, rr, N).to(F32)
                y, k = A.emulate_fast_attn(fmt, qkv, cc, lw["qn"], lw["kn"], K1[rows], V1[rows], W["frope"], H, Hkv, hd, s.norm_eps,
                                           k0_from=q0 if (p.a["pair"] and cc == 1) else None)
                q0 = qkv
                put(out[yb], yb, rr, y)
                v = qkv[:, (H + Hkv) * hd:].reshape(M, Hkv, hd)
                for i, m in enumerate(rows):
                    K1[m, :, cc], V1[m, :, cc] = val16(k[i]), val16(v[i].to(F64))
        elif p.op == "draw_aux":
            raise AssertionError("the emulated frames draw with one launch (fp16 / f32 or a small vocabulary)")
        elif p.op == "draw":
            _emulate_draw(fr, p, cur, out, fault)
        recs.append(dict(name=p.name, m0=p.m0, rows=p.rows, cols=p.cols, cls=p.cls, held=True, bufs=out))
        for b, a in out.items():
            cur[b] = (p.name, a)
    st1 = dict(tok=cur[TB_TOK][1].copy(), pos=cur[TB_POS][1].reshape(-1).copy(), nf=cur[TB_NF][1].reshape(-1).copy(),
               done=cur[TB_DONE][1].reshape(-1).copy(), seq=cur[TB_SEQ][1].reshape(cfg.max_batch, cfg.R, cfg.cap).copy())
    if fr.kind == "first":
        st1["pos"][rows] = np.asarray(fr.next_pos)
    st0 = dict(st, seq=st["seq"].reshape(cfg.max_batch, cfg.R, cfg.cap))
    if bug and bug[1] == "missing":
        recs = [r for r in recs if r["name"] != bug[0]]
    if bug and bug[1] == "extra":
        i = [r["name"] for r in recs].index(bug[0])
        recs.insert(i + 1, dict(recs[i], bufs={b: a.copy() for b, a in recs[i]["bufs"].items()}))
    return dict(kind=1 if fr.kind == "decode" else 2, m0=m0, M=M, launches=recs, state=[st0, st1], begin=begin), c1


def _emulate_draw(fr: Frame, p: PL, cur, out, fault):
    """sample_small_kernel / sample_block_kernel as the reference draws, then finish_draw's bookkeeping."""
    cfg, model, cb, what, M, m0 = fr.cfg, fr.model, p.a["cb"], p.a["what"], fr.M, fr.m0
    prev = {b: a for b, (_, a) in cur.items()}
    R, cap, Df = cfg.R, cfg.cap, cfg.shape.fast_dim
    lb = TB_LOGITS if cb == 0 else TB_FLOG
    codes = []
    for i, row in enumerate(fr._draw_rows(p, prev)):
        m = m0 + i
        q = torch.from_numpy(D.noise_of(model, cb, row)).to(D.DT[cfg.fmt])
        w = int(torch.argmax(torch.from_numpy(row.ref.probs).to(D.DT[cfg.fmt]) / q))
        code = min(max(w - model.sem_begin, 0), model.cbsize - 1) if cb == 0 else w
        codes.append(code)
        if cb == 0:
            out[TB_TOKN][m, 0], out[TB_TOKN][m, 1] = w, code
        else:
            out[TB_TOKN][m, cb + 1] = w
        if what & 3:
            out[lb][m] = row.ref.after
    n = len(codes)
    for i in range(n):
        m, code = m0 + i, codes[(i + 1) % n if fault == "neighbour_code" else i]
        emb = model.fast_emb[codes[i]]
        out[TB_FEMB][m] = emb
        if what & (DRAW_XO_FEMB | DRAW_XO_PAIR):
            b, r0 = (TB_XO_X, m + cfg.xo_pair) if what & DRAW_XO_PAIR else (TB_XO_FEMB, m)
            xo_write(out[b], [r0], D.bits16(emb, cfg.fmt).reshape(1, Df))
        if what & DRAW_QKV0_TAB:
            t = torch.from_numpy(model.qkv0_tab[code].view(np.int16).copy()).view(D.DT[cfg.fmt]).to(torch.float32).numpy()
            out[TB_QKVF][m, :len(t)] = t
        if p.a["last"]:
            out[TB_TOK][m] = out[TB_TOKN][m]
            if not int(prev[TB_DONE].reshape(-1)[m]):
                nf = int(prev[TB_NF].reshape(-1)[m])
                if nf < cap:
                    out[TB_SEQ].reshape(-1, R, cap)[m, :, nf] = out[TB_TOKN][m]
                out[TB_POS].reshape(-1)[m] += 1
                out[TB_NF].reshape(-1)[m] = nf + 1
                if int(out[TB_TOKN][m, 0]) == model.im_end:
                    out[TB_DONE].reshape(-1)[m] = 1


def emulate_qkv0_tab(cfg: Cfg, W: dict) -> np.ndarray:
    """The lock-step batches' table of fast layer 0's q k v by drawn code (wide_qkv0_build): the launch itself on the embedding rows."""
    l0 = W["fast"][0]
    v = WR.emulate_linear(cfg.fmt, WR.STORE, W["top"]["fast_emb"][:cfg.fastV], l0["wqkv"], l0["attn_norm"], eps=cfg.shape.norm_eps)
    return A.wbits(v, cfg.fmt)
