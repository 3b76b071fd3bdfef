"""Float64 side of the launch trace of a PROMPT call (include/fishtts_hip_test.h: ft_test_ar_trace_*, kinds 3, 4, 5; host only;
test infrastructure, the sibling of tests/frame_ref.py).  No tolerance is defined here: every bound is tests/pf_ref.py's
(linear_ref, norm_ref, append_ref, attn_ref, decode_ref, check, check_cache), tests/ar_ref.py's (the embed and every
position-by-position launch, through frame_ref's judges of a one-row frame) or draw_ref.judge's (the tail, through frame_ref as
a first-frames call of one row at m0 = slot).

Every kernel of the prompt pass is held to float64 through its own hook, on temporaries.  What no hook sees is the host code
that strings them together: prefill_gemm, ft_ar_prefill_at, ft_ar_prefill_slow and ft_ar_prefill_slow_many of csrc/engine.hip.
`plan` restates that host code - from the shape, the type, max_batch, the switches (FT_PREFILL_GEMM, FT_PREFILL_ATTN_V0,
FT_PREFILL_V0, FT_NO_RAGGED_PREFILL, FT_NO_WIDE) and the call (kind, slots, Lp, pos0) - as the passes a fill is cut into and,
per pass, the ordered launches with their rows, the class pf_ref.want_id or the attention rule predicts, the buffers they write
and the producer of every input.  `judge` walks a recorded trace against it:

  pf.embed                 ar_ref.embed_ref on the token rows read from the RECORDED d_prompt at the pass's row stride S; d_prompt,
                           pf_seqs and pf_rows (they ride with the pass's first record) are exactly what the plan lays out
  pf.<l>.norm1 | norm2     pf_ref.norm_ref with the layer's attention_norm | ffn_norm gain
  pf.<l>.wqkv|wo|w13|w2    pf_ref.linear_ref (WQKV, RESID, W13, RESID) from the recorded operand and residual rows
  pf.<l>.append            pf_ref.append_ref: the finished queries (tiled path) and, in the layer's cache, the appended rows through
                           pf_ref.check_cache (its K bound and V copies; "every other row bit-unchanged" is taken here on the whole
                           cache of every slot, the hook's NaN fill does not exist in a context)
  pf.<l>.attn              pf_ref.attn_ref (NG of the record's class) or pf_ref.decode_ref position by position
  pf.last                  a copy of bits: row first + rows - 1 of pf_x into row `slot` of ctx->x
  t<k>.embed, t<k>.slow..  frame_ref's judges of a one-row decode frame at m0 = slot, position pos0 + k (the record's pos_off)
  fproj, head, draw, fast  frame_ref's judges of a first-frames call of one row at m0 = slot

and on every buffer a launch wrote, every element outside the launch's rows is bit-equal to the record before: rows S ..
max_seq_len - 1 of the workspace, every other slot's row of ctx->x.  Above 256 rows a product is recomputed on the rows of
`judged_rows` (first 8, the first and last row tile of the class, both sides of every tile edge, every sequence's first and
last row, 256 seeded rows); everything else on every row.  The state after the call is slot_ref.reset of every slot of the
call on the state before, then what the call leaves.

`emulate` produces such a trace from the plan with pf_ref.emulate_*, ar_ref and frame_ref.emulate, with or without an injected
fault of the host code: tests/test_prompt_ref_host.py."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from tests import ar_ref as A
from tests import frame_ref as FR
from tests import pf_ref as PF
from tests import slot_ref as SR
from tests.codec_stage_ref import F32, F64
from tests.frame_ref import PL, Report, TB_TOKN, TB_X, _bits, _cls

# buffer ids of the trace's prompt workspace (AR_TB_*, include/fishtts_hip_test.h)
PF_X, PF_QKV, PF_Y = 13, 14, 15
PF_XN, PF_YBF, PF_QBF, PF_G = 25, 26, 27, 28
PROMPT, PF_SEQS, PF_ROWS = 39, 40, 41
UPLOADS = (PROMPT, PF_SEQS, PF_ROWS)
H16 = (PF_XN, PF_YBF, PF_QBF, PF_G)
KIND_AT, KIND_SLOW, KIND_MANY = 3, 4, 5
ALL_ROWS = 256
FMT = "bf16"


@dataclass(frozen=True)
class PCfg:
    frame: FR.Cfg                                # shape, type, max_batch, FT_NO_WIDE among its switches
    gemm_mode: int = 2                           # FT_PREFILL_GEMM
    switches: frozenset = frozenset()            # FT_PREFILL_ATTN_V0, FT_PREFILL_V0, FT_NO_RAGGED_PREFILL

    @property
    def v0(self):
        """ar_alloc's rule: position by position for every type but bf16 and every width off the MFMA tiles."""
        s = self.frame.shape
        return "FT_PREFILL_V0" in self.switches or self.frame.fmt != "bf16" or s.dim % 32 != 0 or (s.n_head * s.head_dim) % 32 != 0 \
            or s.intermediate_size % 32 != 0

    def flash(self, lp: int, ragged: bool) -> bool:
        s = self.frame.shape
        return ragged or ("FT_PREFILL_ATTN_V0" not in self.switches and s.head_dim in (64, 128) and lp >= 16)

    def ragged(self, n: int) -> bool:
        s = self.frame.shape
        return self.frame.fmt == "bf16" and not self.v0 and self.frame.wide_ok and n >= 5 and s.head_dim in (64, 128) \
            and "FT_PREFILL_ATTN_V0" not in self.switches and "FT_NO_RAGGED_PREFILL" not in self.switches


@dataclass(frozen=True)
class Call:
    kind: int
    slots: tuple
    lps: tuple
    pos0s: tuple


@dataclass
class Pass:
    prefix: str                                  # "" or "pass<k>."
    mode: str                                    # "gemm" (prefill_gemm) | "pos" (position by position)
    seqs: List[PF.Seq]                           # {first row, rows, first cache position, slot}
    idx: List[int]                               # the call's prompts in this pass
    ragged: bool
    tail: bool                                   # kind 3: the first frame follows
    launches: List[PL] = field(default_factory=list)

    @property
    def S(self):
        return sum(q.rows for q in self.seqs)


def passes(pc: PCfg, call: Call) -> List[Pass]:
    """The passes a call is cut into (ft_ar_prefill_slow_many: as many prompts as the workspace's max_seq_len rows hold)."""
    n, msl = len(call.slots), pc.frame.shape.max_seq_len
    mode = "pos" if pc.v0 else "gemm"
    if call.kind != KIND_MANY or not pc.ragged(n):
        return [Pass(f"pass{i}." if call.kind == KIND_MANY and n > 1 else "", mode, [PF.Seq(0, call.lps[i], call.pos0s[i], call.slots[i])], [i], False,
                     call.kind == KIND_AT) for i in range(n)]
    out, i0 = [], 0
    while i0 < n:
        i1, S, seqs = i0, 0, []
        while i1 < n and S + call.lps[i1] <= msl:
            seqs.append(PF.Seq(S, call.lps[i1], call.pos0s[i1], call.slots[i1]))
            S += call.lps[i1]
            i1 += 1
        assert i1 > i0, "a prompt longer than the workspace"
        out.append(Pass("", "gemm", seqs, list(range(i0, i1)), True, False))
        i0 = i1
    if len(out) > 1:
        for k, p in enumerate(out):
            p.prefix = f"pass{k}."
    return out


def plan(pc: PCfg, call: Call) -> List[Pass]:
    """The passes with the launches of every prefill_gemm pass; a position-by-position pass is planned per position by frame_ref."""
    s = pc.frame.shape
    D_, F, H, Hkv, hd = s.dim, s.intermediate_size, s.n_head, s.n_local_heads, s.head_dim
    HD, qkvN = H * hd, (H + 2 * Hkv) * hd
    out = passes(pc, call)
    for ps in out:
        if ps.mode != "gemm":
            continue
        S, prod = ps.S, {}
        m0 = 0 if ps.ragged else ps.seqs[0].slot
        P = lambda b: (b, prod.get(b, "begin"))

        def add(name, op, rows, cols, cls, writes, src=None, **a):
            ps.launches.append(PL(ps.prefix + name, op, m0, rows, cols, cls, tuple(writes), dict(src or {}), a))
            for b in writes:
                prod[b] = ps.prefix + name
        gid = lambda N, K: _cls(PF.want_id(pc.gemm_mode, S, N, K))
        max_lp = max(q.rows for q in ps.seqs)
        flash = pc.flash(max_lp, ps.ragged)
        path = (4 if max_lp <= 320 else 2) if flash else 0
        add("pf.embed", "embed", S, D_, _cls(), (PF_X,))
        for l in range(s.n_layer):
            n = f"pf.{l}."
            add(n + "norm1", "norm", S, D_, _cls(), (PF_XN,), dict(x=P(PF_X)), l=l, gain="attn_norm")
            add(n + "wqkv", "lin", S, qkvN, gid(qkvN, D_), (PF_QKV,), dict(x=P(PF_XN)), l=l, w="wqkv", bias="bqkv", form=PF.WQKV, K=D_, N=qkvN, out=PF_QKV)
            add(n + "append", "append", S, HD, _cls(1 if flash else 0), (PF_QBF,), dict(qkv=P(PF_QKV)), l=l, flash=flash)
            src = dict(q=P(PF_QBF)) if flash else dict(qkv=P(PF_QKV))
            add(n + "attn", "attn", S, HD, _cls(path), (PF_YBF,) if flash else (PF_Y, PF_YBF), src, l=l, flash=flash, NG=path)
            add(n + "wo", "lin", S, D_, gid(D_, HD), (PF_X,), dict(x=P(PF_YBF), resid=P(PF_X)), l=l, w="wo", bias="bo", form=PF.RESID, K=HD, N=D_, out=PF_X)
            add(n + "norm2", "norm", S, D_, _cls(), (PF_XN,), dict(x=P(PF_X)), l=l, gain="ffn_norm")
            add(n + "w13", "lin", S, F, gid(2 * F, D_), (PF_G,), dict(x=P(PF_XN)), l=l, w="w13", bias=None, form=PF.W13, K=D_, N=2 * F, out=PF_G)
            add(n + "w2", "lin", S, D_, gid(D_, F), (PF_X,), dict(x=P(PF_G), resid=P(PF_X)), l=l, w="w2", bias=None, form=PF.RESID, K=F, N=D_, out=PF_X)
        add("pf.last", "last", len(ps.seqs) if ps.ragged else 1, D_, _cls(), (TB_X,), dict(x=P(PF_X)))
    return out


def prompt_layout(prompts: Sequence[np.ndarray], ps: Pass, R: int):
    """d_prompt, pf_seqs and pf_rows of a pass as the host lays them out: row r of the token matrix at r * S, the prompts' columns
    back to back (the stride is the PASS's S, not a prompt's Lp)."""
    S = ps.S
    tok = np.zeros(R * S, dtype=np.int32)
    for q, i in zip(ps.seqs, ps.idx):
        p = np.asarray(prompts[i], dtype=np.int32).reshape(R, -1)
        assert p.shape[1] == q.rows
        for r in range(R):
            tok[r * S + q.row0:r * S + q.row0 + q.rows] = p[r]
    seqs = np.array([[q.row0, q.rows, q.pos0, q.slot] for q in ps.seqs], dtype=np.int32)
    rows = np.array([[q.slot, q.pos0 + t] for q in ps.seqs for t in range(q.rows)], dtype=np.int32)
    return tok, seqs, rows


BM = {PF.ID_SKINNY1: 16, PF.ID_SKINNY2: 32, PF.ID_SKINNY4: 64, PF.ID_LIN128: 128, PF.ID_LIN64: 64, PF.ID_TAP64_128: 128, PF.ID_TAP64_64: 64,
      PF.ID_TAP_128: 128, PF.ID_TAP_64: 128}


def judged_rows(S: int, cls_id: int, seqs: Sequence[PF.Seq], seed: int = 0) -> np.ndarray:
    """All rows up to 256; above: the first 8, every row of the first and last row tile of the class picked, the row on each side of
    every row-tile boundary, every sequence's first and last row, 256 seeded rows."""
    if S <= ALL_ROWS:
        return np.arange(S)
    bm = BM.get(cls_id, 128)
    keep = set(range(8)) | set(range(min(bm, S))) | set(range((S - 1) // bm * bm, S))
    for e in range(bm, S, bm):
        keep |= {e - 1, e}
    for q in seqs:
        keep |= {q.row0, q.row0 + q.rows - 1}
    keep |= set(np.random.default_rng(seed).choice(S, 256, replace=False).tolist())
    return np.array(sorted(keep))


def _state_obj(st: dict, MB: int) -> SR.State:
    z = lambda *sh: np.zeros(sh, dtype=np.int32)
    return SR.State(dict(max_batch=MB), np.zeros(0, dtype=np.uint8), seq=np.array(st["seq"]), tok=np.array(st["tok"]), tokn=z(MB, 1),
                    pos=np.array(st["pos"]), nf=np.array(st["nf"]), done=np.array(st["done"]), ctl=z(MB, 1), hid_in_xo=np.zeros(MB, dtype=np.uint8))


def _align(names: List[str], recs: List[dict], flag):
    """frame_ref's alignment by name: a missing or an extra entry costs that entry alone.  -> [(plan index | None, rec)]."""
    i = j = 0
    pairs = []
    while i < len(names) or j < len(recs):
        if i < len(names) and j < len(recs) and names[i] == recs[j]["name"]:
            pairs.append((i, recs[j])); i += 1; j += 1
        elif j < len(recs) and recs[j]["name"] not in set(names[i:]):
            flag(recs[j]["name"], "an entry the plan does not have here"); pairs.append((None, recs[j])); j += 1
        elif j < len(recs) and j > 0 and recs[j]["name"] == recs[j - 1]["name"]:
            flag(recs[j]["name"], "an entry the plan does not have here (a second launch)"); pairs.append((None, recs[j])); j += 1
        elif i < len(names):
            flag(names[i], "planned, not in the trace"); i += 1
        else:
            flag(recs[j]["name"], "an entry the plan does not have here"); pairs.append((None, recs[j])); j += 1
    return pairs


class Prompt:
    """One traced prompt call: the plan, the weights, the prompts the host passed, the caches before and after."""

    def __init__(self, pc: PCfg, W: dict, call: Call, prompts: Sequence[np.ndarray], ctls=None):
        self.pc, self.cfg, self.W, self.call, self.prompts, self.ctls = pc, pc.frame, W, call, prompts, ctls
        self.plan = plan(pc, call)
        self.pos_end = [max(q.pos0 + q.rows for q in ps.seqs) for ps in self.plan]

    # ---- the one-row frames frame_ref judges: a position of a position-by-position pass, or the tail
    def frame_plan(self, ps: Pass, k: int, what: str, pos_end: int) -> List[PL]:
        """what: "slow" (enqueue_slow_only), "frame" (enqueue_frame: the last position of a kind-3 call), "tail" (after prefill_gemm)."""
        slot = ps.seqs[0].slot
        if what == "tail":
            pl = FR.plan(self.cfg, "first", slot, 1)
        else:
            pl = [dataclasses.replace(p, m0=slot) for p in FR.plan(self.cfg, "decode", 0, 1, pos_end)]
        if what == "slow":
            pl = [p for p in pl if p.name == "embed" or p.name.startswith("slow.")]
        return pl

    def frame(self, ps: Pass, k: int, what: str, pos_end: int) -> FR.Frame:
        q = ps.seqs[0]
        fr = FR.Frame(self.cfg, self.W, "first", q.slot, 1, self.ctls or [None], pos_end, next_pos=[q.pos0 + q.rows])
        fr.kind = "first" if what == "tail" else "decode"
        fr.plan = self.frame_plan(ps, k, what, pos_end)
        fr._final = lambda *a: None                                    # the state after the call is judged here, for the whole call
        MB, R = self.cfg.max_batch, self.cfg.R
        fr._tok0, fr._pos0 = np.zeros((MB, R), dtype=np.int32), np.zeros(MB, dtype=np.int64)
        if what != "tail":
            fr._tok0[q.slot] = np.asarray(self.prompts[ps.idx[0]]).reshape(R, -1)[:, k]
            fr._pos0[q.slot] = q.pos0 + k
        return fr

    def segments(self):
        """[(pass, what, k, prefix of the records' names, planned names)] in launch order."""
        out = []
        for ip, ps in enumerate(self.plan):
            if ps.mode == "gemm":
                out.append((ps, "gemm", 0, "", [p.name for p in ps.launches]))
                if ps.tail:
                    out.append((ps, "tail", 0, ps.prefix, [ps.prefix + p.name for p in self.frame_plan(ps, 0, "tail", self.pos_end[ip])]))
                continue
            Lp = ps.seqs[0].rows
            for k in range(Lp):
                what = "frame" if ps.tail and k == Lp - 1 else "slow"
                names = []
                for p in self.frame_plan(ps, k, what, self.pos_end[ip]):
                    pre = ps.prefix + (f"t{k}." if p.name == "embed" or p.name.startswith("slow.") else "")
                    names.append(pre + p.name)
                out.append((ps, what, k, ps.prefix, names))
        return out

    # ---- judging
    def judge(self, trace: dict, caches0: dict, caches1: dict) -> Report:
        rep, cfg, call = Report(), self.cfg, self.call
        flag = lambda n, msg: rep.flags.append((n, msg))
        n = len(call.slots)
        want_call = (call.kind, call.slots[0] if call.kind != KIND_MANY else 0, 1 if call.kind != KIND_MANY else n)
        if (trace["kind"], trace["m0"], trace["M"]) != want_call:
            flag("call", f"the trace is of kind {trace['kind']} rows {trace['m0']}+{trace['M']}, the call is {want_call}")
        segs = self.segments()
        names = [nm for sg in segs for nm in sg[4]]
        pairs = _align(names, trace["launches"], flag)
        owner = []                                                     # plan index -> segment
        for si, sg in enumerate(segs):
            owner += [si] * len(sg[4])
        by_seg: Dict[int, list] = {si: [] for si in range(len(segs))}
        last = 0
        for pi, rec in pairs:
            last = owner[pi] if pi is not None else last
            by_seg[last].append((pi, rec))
        cur = {b: ("begin", a) for b, a in trace["begin"].items()}
        prog = {k: (kc.copy(), vc.copy()) for k, (kc, vc) in caches0.items()}       # the caches as the launches judged so far left them
        st = _state_obj(trace["state"][0], cfg.max_batch)
        for si, (ps, what, k, pre, seg_names) in enumerate(segs):
            ip = self.plan.index(ps)
            if what == "gemm":
                for q in ps.seqs:
                    st = self._reset(st, q.slot, cur)
                self._judge_gemm(ps, by_seg[si], cur, rep, prog, caches1)
                continue
            if k == 0 and what != "tail":
                st = self._reset(st, ps.seqs[0].slot, cur)
            self._judge_frame(ps, what, k, pre, by_seg[si], cur, rep, prog, caches1, st, self.pos_end[ip])
        self._final(trace, cur, caches0, caches1, prog, st, rep)
        return rep

    def _reset(self, st, slot, cur):
        """slot_ref.reset, and the buffers it clears as the record before the next launch that writes them."""
        st = SR.reset(st, slot)
        i32 = lambda a, sh: np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(sh))
        for b, a, sh in ((FR.TB_POS, st.pos, (1, -1)), (FR.TB_NF, st.nf, (1, -1)), (FR.TB_DONE, st.done, (1, -1)), (FR.TB_SEQ, st.seq, (self.cfg.max_batch, -1))):
            cur[b] = (cur[b][0], i32(a, sh))
        return st

    def _judge_frame(self, ps, what, k, pre, pairs, cur, rep, prog, c1, st, pos_end):
        q = ps.seqs[0]
        fr = self.frame(ps, k, what, pos_end)
        tpre = pre + f"t{k}."
        strip = lambda nm: nm[len(tpre):] if nm.startswith(tpre) else nm[len(pre):] if nm.startswith(pre) else nm
        recs = []
        for _, rec in pairs:
            r = dict(rec, name=strip(rec["name"]), bufs={b: a for b, a in rec["bufs"].items() if b not in UPLOADS})
            recs.append(r)
            if rec["name"].startswith(tpre) and rec.get("pos_off", q.pos0 + k) != q.pos0 + k:
                rep.flags.append((rec["name"], f"ran at pos_off {rec['pos_off']}, position {k} of a prompt at pos0 {q.pos0} runs at {q.pos0 + k}"))
            if PROMPT in rec["bufs"]:
                self._check_uploads(ps, rec, cur, rep)
        # the state this one-row frame finds: the slot reset (its device position is 0: the position is the launch's pos_off)
        sd = dict(tok=st.tok, pos=st.pos, nf=st.nf, done=st.done, seq=st.seq)
        begin = {b: a for b, (_, a) in cur.items() if b < PF_X or 20 <= b < 25 or 30 <= b < PROMPT}
        sub = dict(kind=2 if what == "tail" else 1, m0=q.slot, M=1, launches=recs, state=[sd, sd], begin=begin)
        # the caches this frame finds and leaves: the appended row of every layer comes from the caches after the call
        c0s, c1s = {}, {}
        for key, (kc, vc) in prog.items():
            if key[0] == "slow" and what != "tail":
                k1, v1 = kc.copy(), vc.copy()
                p = q.pos0 + k
                if 0 <= p < kc.shape[2]:
                    k1[q.slot, :, p], v1[q.slot, :, p] = c1[key][0][q.slot, :, p], c1[key][1][q.slot, :, p]
                c0s[key], c1s[key] = (kc, vc), (k1, v1)
                prog[key] = (k1, v1)
            else:
                c0s[key], c1s[key] = (kc, vc), c1[key]
        r = fr.judge(sub, c0s, c1s)
        back = {p.name: nm for p, nm in zip(fr.plan, [n_ for n_ in self.segments_names(ps, what, k, pos_end)])}
        r.flags = [(back.get(nm, (pre + nm) if nm not in ("call",) else nm), msg) for nm, msg in r.flags]
        r.names = {("t." + nm if what != "tail" and (nm == "embed" or nm.startswith("slow.")) else nm) for nm in r.names}
        r.classes = {(("t." + nm if what != "tail" and (nm == "embed" or nm.startswith("slow.")) else nm), c) for nm, c in r.classes}
        if r.worst_at:
            r.worst_at = back.get(r.worst_at, pre + r.worst_at)
        rep.merge(r)
        for rec in recs:
            for b, a in rec["bufs"].items():
                cur[b] = (rec["name"], a)

    def segments_names(self, ps, what, k, pos_end):
        out = []
        for p in self.frame_plan(ps, k, what, pos_end):
            out.append(ps.prefix + (f"t{k}." if what != "tail" and (p.name == "embed" or p.name.startswith("slow.")) else "") + p.name)
        return out

    def _check_uploads(self, ps, rec, cur, rep):
        """d_prompt (and, in a ragged pass, pf_seqs and pf_rows) exactly what the plan lays out; what lies behind them unchanged."""
        tok, seqs, rows = prompt_layout(self.prompts, ps, self.cfg.R)
        want = [(PROMPT, tok.reshape(-1))]
        if ps.ragged:
            want += [(PF_SEQS, seqs.reshape(-1)), (PF_ROWS, rows.reshape(-1))]
        for b, w in want:
            if b not in rec["bufs"]:
                rep.flags.append((rec["name"], f"the record does not hold the uploaded buffer {b}"))
                continue
            got, was = rec["bufs"][b].reshape(-1), cur[b][1].reshape(-1)
            if not np.array_equal(got[:len(w)], w):
                at = int(np.argwhere(got[:len(w)] != w)[0][0])
                rep.flags.append((rec["name"], f"buffer {b} is not the plan's layout, first at word {at}: {int(got[at])}, planned {int(w[at])}"))
            if not np.array_equal(got[len(w):], was[len(w):]):
                rep.flags.append((rec["name"], f"buffer {b} changed behind the pass's {len(w)} words"))
        for b in UPLOADS:
            if b in rec["bufs"]:
                if not ps.ragged and b != PROMPT and not np.array_equal(rec["bufs"][b], cur[b][1]):
                    rep.flags.append((rec["name"], f"buffer {b} changed in a single pass"))
                cur[b] = (rec["name"], rec["bufs"][b])

    def _rows16(self, a, rows, cols):
        return PF.values(np.ascontiguousarray(a[np.asarray(rows), :cols]), FMT)

    def _rows32(self, a, rows, cols):
        return torch.from_numpy(np.ascontiguousarray(a[np.asarray(rows), :cols])).to(F64)

    def _note(self, p, rep, ver, n, what=""):
        rep.note(p.name, ver.checked, ver.worst)
        if ver.flagged or ver.checked != n:
            rep.flags.append((p.name, f"{what}{ver.flagged} of {ver.checked} elements outside the bound, worst {ver.worst:.3f}, rows {ver.rows[:8]}, cols {ver.cols[:8]}"))

    def _judge_gemm(self, ps, pairs, cur, rep, prog, c1):
        cfg, s, W = self.cfg, self.cfg.shape, self.W
        H, Hkv, hd, S = s.n_head, s.n_local_heads, s.head_dim, ps.S
        allr = np.arange(S)
        by_name = {p.name: p for p in ps.launches}
        for pi, rec in pairs:
            p = by_name.get(rec["name"]) if pi is not None else None
            if p is None:
                for b, a in rec["bufs"].items():
                    cur[b] = (rec["name"], a)
                continue
            gname = FR.generic_name(p.name[len(ps.prefix):]).replace(f"pf.{p.a.get('l')}.", "pf.l.") if "l" in p.a else p.name[len(ps.prefix):]
            rep.names.add(gname); rep.classes.add((gname, tuple(rec["cls"])))
            if (rec["m0"], rec["rows"], rec["cols"]) != (p.m0, p.rows, p.cols):
                rep.flags.append((p.name, f"m0 / rows / cols {(rec['m0'], rec['rows'], rec['cols'])}, planned {(p.m0, p.rows, p.cols)}"))
            if tuple(rec["cls"]) != p.cls:
                rep.flags.append((p.name, f"class {tuple(rec['cls'])}, the rules predict {p.cls}"))
            if PROMPT in rec["bufs"] or p.op == "embed":
                self._check_uploads(ps, rec, cur, rep)
            wrote = {b: a for b, a in rec["bufs"].items() if b not in UPLOADS}
            if set(wrote) != set(p.writes):
                rep.flags.append((p.name, f"writes buffers {sorted(wrote)}, planned {sorted(p.writes)}"))
            for role, (b, who) in p.src.items():
                if cur[b][0] != who:
                    rep.flags.append((p.name, f"input {role} was last written by {cur[b][0]}, planned {who}"))
            try:
                masks = getattr(self, "_g_" + p.op)(ps, p, rec, cur, rep, prog, c1, allr)
            except Exception as e:                                     # a launch the checker cannot even read is a finding of that launch
                rep.flags.append((p.name, f"{type(e).__name__}: {e}"))
                masks = {}
            for b, a in wrote.items():
                if b in cur and cur[b][1] is not None:
                    keep = ~masks[b] if b in masks else np.ones(a.shape, dtype=bool)
                    if not np.array_equal(_bits(a)[keep], _bits(cur[b][1])[keep]):
                        where = np.argwhere(keep & (_bits(a) != _bits(cur[b][1])))
                        rep.flags.append((p.name, f"buffer {b}: {len(where)} elements outside the launch's rows changed, first at {where[0].tolist()}"))
                cur[b] = (rec["name"], a)

    @staticmethod
    def _mask(a, rows, cols):
        m = np.zeros(a.shape, dtype=bool)
        m[np.asarray(rows), :cols] = True
        return m

    def _g_embed(self, ps, p, rec, cur, rep, prog, c1, allr):
        s, t, S, R = self.cfg.shape, self.W["top"], ps.S, self.cfg.R
        dp = cur[PROMPT][1].reshape(-1)                                # the recorded d_prompt, read at the pass's row stride S
        toks = np.stack([dp[r * S:r * S + S] for r in range(R)], axis=1)
        ref = A.embed_ref(FMT, t["emb"], t["cb_emb"], toks, s.num_codebooks, s.codebook_size, s.semantic_begin_id, s.semantic_end_id,
                          bool(s.scale_codebook_embeddings))
        got = np.ascontiguousarray(rec["bufs"][PF_X][:S, :s.dim])
        self._note(p, rep, A.check(got, ref.ref, ref.err, FMT), S * s.dim)
        return {PF_X: self._mask(rec["bufs"][PF_X], allr, s.dim)}

    def _g_norm(self, ps, p, rec, cur, rep, prog, c1, allr):
        s, S = self.cfg.shape, ps.S
        ref = PF.norm_ref(self._rows32(cur[PF_X][1], allr, s.dim), self.W["slow"][p.a["l"]][p.a["gain"]], s.norm_eps)
        self._note(p, rep, PF.check(np.ascontiguousarray(rec["bufs"][PF_XN][:S, :s.dim]), ref.ref, ref.err), S * s.dim)
        return {PF_XN: self._mask(rec["bufs"][PF_XN], allr, s.dim)}

    def _g_lin(self, ps, p, rec, cur, rep, prog, c1, allr):
        lw, S = self.W["slow"][p.a["l"]], ps.S
        sel = judged_rows(S, p.cls[0], ps.seqs, seed=p.a["l"])
        xb = p.src["x"][0]
        X = self._rows16(cur[xb][1], sel, p.a["K"])
        resid = self._rows32(cur[PF_X][1], sel, p.cols) if "resid" in p.src else None
        bias = lw.get(p.a["bias"]) if p.a["bias"] else None
        ref = PF.linear_ref(p.a["form"], PF.linear_pre(X, lw[p.a["w"]], seed=p.a["l"]), bias=bias, resid=resid)
        out = rec["bufs"][p.a["out"]]
        self._note(p, rep, PF.check(np.ascontiguousarray(out[sel, :p.cols]), ref.ref, ref.err), len(sel) * p.cols)
        return {p.a["out"]: self._mask(out, allr, p.cols)}

    def _g_append(self, ps, p, rec, cur, rep, prog, c1, allr):
        s, l, S = self.cfg.shape, p.a["l"], ps.S
        H, Hkv, hd = s.n_head, s.n_local_heads, s.head_dim
        lw = self.W["slow"][l]
        pos = [q.pos0 + t for q in ps.seqs for t in range(q.rows)]
        qkv = self._rows32(cur[PF_QKV][1], allr, (H + 2 * Hkv) * hd)
        app = PF.append_ref(qkv, pos, lw["qn"], lw["kn"], self.W["rope"], H, Hkv, hd, s.norm_eps)
        kc0, vc0 = prog[("slow", l)]
        kc1, vc1 = c1[("slow", l)]
        cv = PF.check_cache(kc0, vc0, kc1, vc1, ps.seqs, app, Hkv, hd)
        rep.note(p.name + " (K rows)", cv.k.checked, cv.k.worst)
        if cv.k.flagged or cv.k.checked != S * Hkv * hd or not cv.v_equal:
            rep.flags.append((p.name, f"cache: {cv.k.flagged} appended K elements outside the bound (rows {cv.k.rows[:8]}, worst {cv.k.worst:.3f}), V copies {cv.v_equal}"))
        k1, v1 = kc0.copy(), vc0.copy()
        for q in ps.seqs:
            sl = slice(q.pos0, q.pos0 + q.rows)
            k1[q.slot, :, sl], v1[q.slot, :, sl] = kc1[q.slot, :, sl], vc1[q.slot, :, sl]
        prog[("slow", l)] = (k1, v1)
        if p.a["flash"]:
            self._note(p, rep, PF.check(np.ascontiguousarray(rec["bufs"][PF_QBF][:S, :H * hd]), app.q.ref, app.q.err), S * H * hd, "finished queries: ")
            return {PF_QBF: self._mask(rec["bufs"][PF_QBF], allr, H * hd)}
        return {}                                                      # the decode kernel keeps its queries in LDS: pf_qbf whole as before

    def _g_attn(self, ps, p, rec, cur, rep, prog, c1, allr):
        s, l, S = self.cfg.shape, p.a["l"], ps.S
        H, Hkv, hd = s.n_head, s.n_local_heads, s.head_dim
        lw = self.W["slow"][l]
        kc1, vc1 = prog[("slow", l)]                                   # as the append left them (every later launch leaves them alone)
        y = np.ascontiguousarray(rec["bufs"][PF_YBF][:S, :H * hd])
        if p.a["flash"]:
            ref = PF.attn_ref(np.ascontiguousarray(cur[PF_QBF][1][:S, :H * hd]), kc1, vc1, ps.seqs, int(rec["cls"][0]) or p.a["NG"], H, Hkv, hd, seed=l)
            self._note(p, rep, PF.check(y, ref.ref, ref.err), S * H * hd)
            return {PF_YBF: self._mask(rec["bufs"][PF_YBF], allr, H * hd)}
        qkv = self._rows32(cur[PF_QKV][1], allr, (H + 2 * Hkv) * hd)
        ar = PF.decode_ref(qkv, kc1, vc1, ps.seqs[0], lw["qn"], lw["kn"], self.W["rope"], H, Hkv, hd, s.norm_eps)
        self._note(p, rep, PF.check(y, ar.y.ref, ar.y.err), S * H * hd)
        y32 = np.ascontiguousarray(rec["bufs"][PF_Y][:S, :H * hd])
        if not np.array_equal(y32.view(np.uint32), PF.values(y, FMT).to(F32).numpy().view(np.uint32)):
            rep.flags.append((p.name, "pf_y is not the f32 value of pf_ybf"))
        return {PF_YBF: self._mask(rec["bufs"][PF_YBF], allr, H * hd), PF_Y: self._mask(rec["bufs"][PF_Y], allr, H * hd)}

    def _g_last(self, ps, p, rec, cur, rep, prog, c1, allr):
        D_ = self.cfg.shape.dim
        x, pfx = rec["bufs"][TB_X], cur[PF_X][1]
        slots = [q.slot for q in ps.seqs]
        for q in ps.seqs:
            if not np.array_equal(_bits(x[q.slot, :D_]), _bits(pfx[q.row0 + q.rows - 1, :D_])):
                rep.flags.append((p.name, f"row {q.slot} of ctx->x is not row {q.row0 + q.rows - 1} of pf_x"))
        rep.note(p.name, len(slots) * D_, 0.0)
        return {TB_X: self._mask(x, slots, D_)}

    def _final(self, trace, cur, c0, c1, prog, st, rep):
        cfg, call, s1 = self.cfg, self.call, trace["state"][1]
        if call.kind == KIND_AT:
            m, tokn = call.slots[0], cur[TB_TOKN][1]
            st = st.copy()
            st.tok[m] = tokn[m]
            st.seq[m][:, 0] = tokn[m]
            st.nf[m], st.pos[m] = 1, call.pos0s[0] + call.lps[0]
            st.done[m] = 1 if int(tokn[m][0]) == cfg.shape.im_end_id else 0
        for k in ("tok", "pos", "nf", "done", "seq"):
            got, want = np.asarray(s1[k]), np.asarray(getattr(st, k))
            if not np.array_equal(got, want):
                m = int(np.argwhere((got != want).reshape(cfg.max_batch, -1).any(axis=1))[0][0])
                rep.flags.append(("state", f"slot {m} {k}: {got[m].reshape(-1)[:12].tolist()}, the call must leave {want[m].reshape(-1)[:12].tolist()}"))
        inside = np.zeros(cfg.max_batch, dtype=bool)
        inside[list(call.slots)] = True
        for key in c0:
            if key[0] == "slow":
                for which, (a, b) in enumerate(zip(prog[key], c1[key])):
                    if not np.array_equal(_bits(a), _bits(b)):
                        m, h, r = (int(v) for v in np.argwhere((_bits(a) != _bits(b)).any(axis=-1))[0])
                        rep.flags.append(("caches", f"{key} {'KV'[which]}: slot {m} kv head {h} row {r} is not what the judged launches left"))
            else:
                out = ~inside if call.kind == KIND_AT else np.ones(cfg.max_batch, dtype=bool)
                if not all(np.array_equal(_bits(a[out]), _bits(b[out])) for a, b in zip(c0[key], c1[key])):
                    rep.flags.append(("caches", f"{key}: a codebook cache row outside the call's first frame changed"))


def judge(pc, W, call, prompts, ctls, trace, caches0, caches1) -> Report:
    return Prompt(pc, W, call, prompts, ctls).judge(trace, caches0, caches1)


def reached(pc: PCfg, call: Call) -> set:
    """The (generic name, class) pairs the restated rules predict for one call."""
    out = set()
    pl = plan(pc, call)
    for ip, ps in enumerate(pl):
        pos_end = max(q.pos0 + q.rows for q in ps.seqs)
        for p in ps.launches:
            nm = p.name[len(ps.prefix):]
            out.add((nm.replace(f"pf.{p.a['l']}.", "pf.l.") if "l" in p.a else nm, p.cls))
        slot = ps.seqs[0].slot
        if ps.mode == "pos":
            full = [dataclasses.replace(p, m0=slot) for p in FR.plan(pc.frame, "decode", 0, 1, pos_end)]
            for p in full:
                slow = p.name == "embed" or p.name.startswith("slow.")
                if slow:
                    out.add(("t." + FR.generic_name(p.name), p.cls))
                elif ps.tail:
                    out.add((FR.generic_name(p.name), p.cls))
        elif ps.tail:
            out |= {(FR.generic_name(p.name), p.cls) for p in FR.plan(pc.frame, "first", slot, 1)}
    return out


# ------------------------------------------------------------------------------------------------------ emulation
def blank(pc: PCfg, seed: int = 0) -> dict:
    """frame_ref.blank plus the prompt workspace, every row finite and plausible (what an earlier, longer prompt left)."""
    cfg, s, g = pc.frame, pc.frame.shape, np.random.default_rng(seed + 7)
    out = FR.blank(cfg, seed)
    msl, HD, qkvN = s.max_seq_len, s.n_head * s.head_dim, (s.n_head + 2 * s.n_local_heads) * s.head_dim
    f32 = lambda r, c: PF.round16(torch.from_numpy(g.standard_normal((r, c))).to(F32), FMT).numpy()
    b16 = lambda r, c: PF.h16_bits(torch.from_numpy(g.standard_normal((r, c))), FMT)
    out[PROMPT] = g.integers(0, 200, (1, cfg.R * msl)).astype(np.int32)
    if not pc.v0:
        out.update({PF_X: f32(msl, s.dim), PF_QKV: f32(msl, qkvN), PF_Y: f32(msl, HD), PF_XN: b16(msl, s.dim), PF_YBF: b16(msl, HD),
                    PF_QBF: b16(msl, HD), PF_G: b16(msl, s.intermediate_size), PF_SEQS: g.integers(0, 9, (cfg.max_batch, 4)).astype(np.int32),
                    PF_ROWS: g.integers(0, 9, (msl, 2)).astype(np.int32)})
    return out


def emulate(pr: Prompt, begin: dict, state0: dict, caches0: dict, bug: Optional[tuple] = None):
    """A trace (the dict ARHipEngine.trace_read returns) and the caches after the call.  bug = (launch name, fault), see
    tests/test_prompt_ref_host.py; ("pass1", "stale_seqs") and ("tail", "x_row0") name a pass and the tail."""
    pc, cfg, s, W, call = pr.pc, pr.cfg, pr.cfg.shape, pr.W, pr.call
    H, Hkv, hd, D_, R, MB = s.n_head, s.n_local_heads, s.head_dim, s.dim, cfg.R, cfg.max_batch
    cur = {b: a.copy() for b, a in begin.items()}
    st0 = {k: np.array(v) for k, v in state0.items()}
    for b, k in ((FR.TB_TOK, "tok"), (FR.TB_POS, "pos"), (FR.TB_NF, "nf"), (FR.TB_DONE, "done"), (FR.TB_SEQ, "seq")):
        cur[b] = st0[k].reshape(MB, -1).copy() if k in ("tok", "seq") else st0[k].reshape(1, -1).copy()
    begin = {b: a.copy() for b, a in cur.items()}
    c1 = {k: (kc.copy(), vc.copy()) for k, (kc, vc) in caches0.items()}
    recs = []
    fault_of = lambda name: bug[1] if bug and bug[0] == name else None

    def reset(m):
        cur[FR.TB_SEQ][m] = 0
        for b in (FR.TB_POS, FR.TB_NF, FR.TB_DONE):
            cur[b].reshape(-1)[m] = 0

    def state_now():
        return dict(tok=cur[FR.TB_TOK].copy(), pos=cur[FR.TB_POS].reshape(-1).copy(), nf=cur[FR.TB_NF].reshape(-1).copy(),
                    done=cur[FR.TB_DONE].reshape(-1).copy(), seq=cur[FR.TB_SEQ].reshape(MB, R, cfg.cap).copy())

    def run_frame(ps, what, k, ip):
        """One one-row frame through frame_ref.emulate; its records get their names and pos_off back."""
        q = ps.seqs[0]
        fr = pr.frame(ps, k, what, pr.pos_end[ip])
        sd = state_now()
        sd["tok"] = fr._tok0.copy() if what != "tail" else sd["tok"]
        off = -1 if fault_of(f"{ps.prefix}t{k}.slow.0.attn") == "pos_off_minus_1" else 0
        sd["pos"] = sd["pos"].copy()
        if what != "tail":
            sd["pos"][q.slot] = q.pos0 + k + off
        fb = {b: a for b, a in cur.items() if b < PF_X or 20 <= b < 25 or 30 <= b < PROMPT}
        if bug and bug == ("tail", "x_row0") and what == "tail":
            fb = dict(fb)
            fb[TB_X] = fb[TB_X].copy()
            fb[TB_X][q.slot] = fb[TB_X][0]
        tr, cc = FR.emulate(fr, fb, sd, c1)
        tok_keep = cur[FR.TB_TOK].copy()
        names = pr.segments_names(ps, what, k, pr.pos_end[ip])
        for r, nm in zip(tr["launches"], names):
            r["name"], r["pos_off"] = nm, (q.pos0 + k + off if what != "tail" else 0)
            if FR.TB_TOK in r["bufs"]:                                 # the position's tokens came from d_prompt: d_tok is as the call found it
                a = r["bufs"][FR.TB_TOK]
                same = (a == sd["tok"]).all(axis=1)
                a[same] = tok_keep[same]
            if what == "frame" and FR.TB_POS in r["bufs"]:             # the device's position is 0 + the launch's pos_off: the draw leaves 1
                r["bufs"][FR.TB_POS].reshape(-1)[q.slot] -= q.pos0 + k + off
            for b, a in r["bufs"].items():
                cur[b] = a
            recs.append(r)
        for key in cc:
            c1[key] = cc[key]
        if what == "slow":                                             # no draw ran: the slot's state is what the reset left
            cur[FR.TB_TOK] = tok_keep
        cur[FR.TB_POS] = cur[FR.TB_POS].copy()
        cur[FR.TB_POS].reshape(-1)[q.slot] = 0 if what == "slow" else cur[FR.TB_POS].reshape(-1)[q.slot]

    for ip, ps in enumerate(pr.plan):
        for q in ps.seqs:
            reset(q.slot)
        tok, seqs, rows = prompt_layout(pr.prompts, ps, R)
        cur[PROMPT] = cur[PROMPT].copy()
        cur[PROMPT].reshape(-1)[:len(tok)] = tok
        ups = [PROMPT]
        if ps.ragged:
            ups += [PF_SEQS, PF_ROWS]
            if not (bug == (f"pass{ip}", "stale_seqs")):
                cur[PF_SEQS] = cur[PF_SEQS].copy(); cur[PF_SEQS].reshape(-1)[:seqs.size] = seqs.reshape(-1)
                cur[PF_ROWS] = cur[PF_ROWS].copy(); cur[PF_ROWS].reshape(-1)[:rows.size] = rows.reshape(-1)
        first = True
        if ps.mode == "pos":
            for k in range(ps.seqs[0].rows):
                n0 = len(recs)
                run_frame(ps, "frame" if ps.tail and k == ps.seqs[0].rows - 1 else "slow", k, ip)
                if first:
                    recs[n0]["bufs"][PROMPT] = cur[PROMPT].copy()
                    first = False
            continue
        S = ps.S
        # the sequences the device walks: its own pf_seqs in a ragged pass
        dev = [PF.Seq(*[int(v) for v in r_]) for r_ in cur[PF_SEQS][:len(ps.seqs)]] if ps.ragged else ps.seqs
        dev = [dataclasses.replace(q, rows=min(q.rows, S - q.row0)) for q in dev if q.row0 < S]        # (a stale table: inside the launched rows)
        dev_rows = [PF.Seq(i, 1, int(r_[1]), int(r_[0])) for i, r_ in enumerate(cur[PF_ROWS][:S])] if ps.ragged else dev
        for p in ps.launches:
            fault = fault_of(p.name)
            out = {b: cur[b].copy() for b in p.writes}
            lw = W["slow"][p.a["l"]] if "l" in p.a else None
            allr = np.arange(S)
            if p.op == "embed":
                dp = cur[PROMPT].reshape(-1)
                if fault == "stride_lp":                               # each sequence's token rows read at its own Lp
                    toks = np.zeros((S, R), dtype=np.int32)
                    for q in ps.seqs:
                        for r in range(R):
                            toks[q.row0:q.row0 + q.rows, r] = dp[r * q.rows + q.row0:r * q.rows + q.row0 + q.rows]
                else:
                    toks = np.stack([dp[r * S:r * S + S] for r in range(R)], axis=1)
                v = A.emulate_embed(FMT, W["top"]["emb"], W["top"]["cb_emb"], toks, s.num_codebooks, s.codebook_size, s.semantic_begin_id,
                                    s.semantic_end_id, bool(s.scale_codebook_embeddings))
                out[PF_X][:S, :D_] = v.to(F32).numpy()
            elif p.op == "norm":
                gain = lw["ffn_norm" if fault == "other_gain" else p.a["gain"]]
                out[PF_XN][:S, :D_] = PF.h16_bits(PF.emulate_norm(pr._rows32(cur[PF_X], allr, D_), gain, s.norm_eps), FMT)
            elif p.op == "lin":
                Wm = W["slow"][(p.a["l"] + 1) % s.n_layer][p.a["w"]] if fault == "next_layer_weight" else lw[p.a["w"]]
                X = pr._rows16(cur[p.src["x"][0]], allr, p.a["K"])
                resid = None
                if "resid" in p.src:
                    resid = pr._rows16(cur[PF_XN], allr, p.cols) if fault == "resid_from_xn" else pr._rows32(cur[PF_X], allr, p.cols)
                bias = lw.get(p.a["bias"]) if p.a["bias"] else None
                v = PF.emulate_linear(p.a["form"], X, Wm, bias, resid)
                if p.a["out"] in H16:
                    out[p.a["out"]][:S, :p.cols] = PF.h16_bits(v, FMT)
                    if fault == "row_S":
                        out[p.a["out"]][S, :p.cols] = out[p.a["out"]][S - 1, :p.cols]
                else:
                    out[p.a["out"]][:S, :p.cols] = v.to(F32).numpy()
            elif p.op == "append":
                use = [dataclasses.replace(q, pos0=0) if fault == "no_pos0" else dataclasses.replace(q, slot=0) if fault == "slot0" else q for q in dev_rows]
                kc, vc = c1[("slow", p.a["l"])]
                qv, k1, v1 = _emulate_append(pr._rows32(cur[PF_QKV], allr, (H + 2 * Hkv) * hd), kc, vc, use, lw["qn"], lw["kn"], W["rope"], H, Hkv, hd, s.norm_eps)
                c1[("slow", p.a["l"])] = (k1, v1)
                if p.a["flash"]:
                    out[PF_QBF][:S, :H * hd] = PF.h16_bits(qv, FMT)
            elif p.op == "attn":
                kc, vc = c1[("slow", p.a["l"])]
                assert p.a["flash"], "the emulated prefill_gemm passes run the tiled attention"
                y = PF.emulate_attn(np.ascontiguousarray(cur[PF_QBF][:S, :H * hd]), kc, vc, dev, p.a["NG"], H, Hkv, hd)
                out[PF_YBF][:S, :H * hd] = PF.h16_bits(y, FMT)
            elif p.op == "last":
                for i, q in enumerate(dev):
                    src = q.row0 + q.rows - (0 if fault in ("row_plus_1", "row_lp") else 1)
                    out[TB_X][i if fault == "row_i" else q.slot, :D_] = cur[PF_X][src, :D_]
            rec = dict(name=p.name, m0=p.m0, rows=p.rows, cols=p.cols, cls=p.cls, pos_off=0, held=True, bufs=out)
            if first:
                for b in ups:
                    rec["bufs"][b] = cur[b].copy()
                first = False
            recs.append(rec)
            for b in p.writes:
                cur[b] = out[b]
        if ps.tail:
            run_frame(ps, "tail", 0, ip)
    if call.kind == KIND_AT:
        cur[FR.TB_POS] = cur[FR.TB_POS].copy()
        cur[FR.TB_POS].reshape(-1)[call.slots[0]] = call.pos0s[0] + call.lps[0]
    if bug and bug[1] == "missing":
        recs = [r for r in recs if r["name"] != bug[0]]
    if bug and bug[1] == "extra":
        i = [r["name"] for r in recs].index(bug[0])
        recs.insert(i + 1, dict(recs[i], bufs={b: a.copy() for b, a in recs[i]["bufs"].items() if b not in UPLOADS}))
    st0["seq"] = st0["seq"].reshape(MB, R, cfg.cap)
    n = len(call.slots)
    return dict(kind=call.kind, m0=call.slots[0] if call.kind != KIND_MANY else 0, M=1 if call.kind != KIND_MANY else n, launches=recs,
                state=[st0, state_now()], begin=begin), c1


def _emulate_append(qkv, kc, vc, seqs, qn, kn, tab, H, Hkv, hd, eps):
    """pf_ref.emulate_append without the hook's NaN fill: the context's caches keep every other row."""
    keep_k, keep_v = kc.copy(), vc.copy()
    q, k1, v1 = PF.emulate_append(qkv, kc, vc, seqs, qn.to(F32), kn.to(F32), tab, H, Hkv, hd, eps)
    for sq in PF.as_seqs(seqs):
        sl = slice(sq.pos0, sq.pos0 + sq.rows)
        keep_k[sq.slot, :, sl], keep_v[sq.slot, :, sl] = k1[sq.slot, :, sl], v1[sq.slot, :, sl]
    return q, keep_k, keep_v
