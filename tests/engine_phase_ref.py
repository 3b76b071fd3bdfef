"""Float64 check of the persistent frame engine (csrc/frame_engine.h), PHASE BY PHASE, from what its launches leave in their
hand-off buffers (host only; test infrastructure, the sibling of tests/ar_ref.py, whose references, bound and emulations it
uses unchanged).

Every vector a phase of the engine hands over stays in device memory after the launch as {tag16 | bf16} granules or PK3
triples.  The buffers are double-buffered - the codebook loop's by step parity with one buffer per layer, the slow stack's by
layer parity - so the loop's last two steps at every layer and the slow stack's last two layers are still there, each with
its recorded input and its recorded output.  ft_test_engine_handoffs (include/fishtts_hip_test.h) copies them out; this file

  plans   which (step, layer, phase) of a launch left what where (`plan_loop`, `plan_slow`), for the forms the kernels
          take: depth, codebook count, the paired first pass, the layer-0 q k v table, PK3 or plain SwiGLU granules, the
          resident form.  A phase whose output never reaches a buffer (layer 0's q k v from step 2 on with the table; the
          tail of the last layer at position 0 of the paired pass; position 0's logits) is LISTED as "not handed off".
  checks  each planned phase against ar_ref's restatement of the launch-path kernel the engine claims to reproduce row for
          row, from its RECORDED input, under ar_ref.check's bound (half a ulp of bf16 plus the derived error of that
          product), every unit of every vector, all frames of a run as the rows of one product:
              RMSNorm + Wqkv (+ bias)     gx[li]                      gemv_ref(PRO_RMSNORM, EPI_STORE)
              attention, Wo + residual    gqkv[li], K/V history, x    fast_attn_ref, its rounded y and that rounding's reach
                                                                      into gemv_ref(EPI_RESID, dx_in) (the loop keeps y in LDS)
              RMSNorm + W13 + SwiGLU      gxb[li]                     gemv_ref(EPI_SWIGLU)
              W2 + residual               gg[li], gxb[li]             gemv_ref(EPI_RESID)
              fast_norm + head rows       gx[n_layer]                 gemv_ref(PRO_RMSNORM, EPI_STORE)
          slow stack: the same four products; its attention is recorded twice - the split partials (decode_attn_ref,
          check_parts) and the merged y in gy (merge_ref from the RECORDED partials) - and Wo reads the recorded gy.
          Inputs that are never handed off are exact and used as such: step 0 reads `hid`, step s >= 1 row toks[s] of
          fast_embeddings, a table step row toks[s] of the loop's own q k v table (that row is itself checked against the
          product it replaces); slow layer 0 reads embed_ref's row of the input column (its rounding's reach travels on).
          The loop's K/V history lives in LDS: it is taken from a launch-path twin's cache (fast_attn_kernel's kc / vc,
          pinned by tests/test_ar_rows_gpu.py), whose rows of the last two positions must agree with norm_rope of the
          engine's recorded q k v; at two codebooks the engine's own records hold the whole history and no twin is used.
  tags    every unit a phase of the last launch wrote carries that launch's tag of its step / layer; a replica unit that
          carries it is bit-equal to the source.

`emulate_loop` restates a codebook-loop launch in float32 from ar_ref's emulations and fills the same records, honest or
with one planted fault: tests/test_engine_phase_ref_host.py pins the checker on it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from tests import ar_ref as A
from tests.codec_stage_ref import F32, F64, from_raw, h16_bits

FMT = "bf16"
EPOCH_STEP = 64                     # frame_engine.h: ENG_EPOCH_STEP
NB = 256                            # ENG_NB
CHECKED, NOT_HANDED = "checked", "not handed off"
LOOP_KINDS = ("qkv", "attn_wo", "w13", "w2")
SLOW_KINDS = ("qkv", "attn", "merge", "wo", "w13", "w2")


def tag16(e: int) -> int:
    return 0x8000 | (e & 0x7FFF)


def tag32(e: int) -> int:
    return 0x80000000 | (e & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------ the plan
@dataclass(frozen=True)
class LoopCfg:
    n_layer: int
    ncb: int
    pair: bool
    qkv0: bool                      # the layer-0 q k v table is present (more than two codebooks, FT_NO_QKV0 unset)
    pk3: bool                       # the SwiGLU vector travels as PK3 triples (F % 384 == 0, 12 values per workgroup)
    resident: bool

    @staticmethod
    def of(rec: dict) -> "LoopCfg":
        return LoopCfg(int(rec["n_layer"]), int(rec["ncb"]), bool(rec["pair"]), bool(rec["qkv0"]), bool(rec["pk3"]), bool(rec["resident"]))


@dataclass(frozen=True)
class Phase:
    step: int                       # codebook step (loop) / -1 (slow stack)
    layer: int                      # n_layer for the head
    kind: str
    status: str
    src: tuple                      # what it reads: ("x", par, layer) ... a buffer; ("hid",), ("emb", step), ("tab", step), ("hist", layer), ("embed",), ("cache", layer)
    dst: Optional[tuple]            # the buffer it leaves its output in
    why: str = ""
    extra: bool = False             # a record of an EARLIER step that no later step overwrote (not one of the last two)

    @property
    def key(self):
        return (self.step, self.layer, self.kind)


def loop_steps(cfg: LoopCfg) -> List[int]:
    return list(range(max(0, cfg.ncb - 2), cfg.ncb))


def plan_loop(cfg: LoopCfg) -> List[Phase]:
    """The phases of one fast_engine_kernel launch whose records are on the device afterwards."""
    nL, out, last2 = cfg.n_layer, [], loop_steps(cfg)
    for s in sorted(set(last2) | ({0, 1} if cfg.qkv0 else set())):
        par = s & 1
        for li in range(nL):
            last = li == nL - 1
            x_src = ("x", par, li) if li > 0 else (("hid",) if s == 0 else ("emb", s))
            if s not in last2:
                if li == 0:
                    out.append(Phase(s, 0, "qkv", CHECKED, (x_src,), ("qkv", par, 0),
                                     "survives the launch: from step 2 on layer 0's q k v is a table row, nobody writes this buffer again", True))
                continue
            tab = cfg.qkv0 and s >= 2 and li == 0
            skipped = cfg.pair and s == 0 and last
            if tab:
                out.append(Phase(s, 0, "qkv", NOT_HANDED, (x_src,), None, "a row of the layer-0 q k v table, looked up by every workgroup"))
                out.append(Phase(s, 0, "qkv_tab", CHECKED, (x_src,), ("tab", s), "the table row against the product it replaces", True))
            else:
                out.append(Phase(s, li, "qkv", CHECKED, (x_src,), ("qkv", par, li)))
            q_src = ("tab", s) if tab else ("qkv", par, li)
            why = "position 0 of the paired pass only feeds the K/V history: the tail of its last layer is not computed" if skipped else ""
            st = NOT_HANDED if skipped else CHECKED
            # the paired first pass writes plain granules wherever position 0 goes on after the attention (eng_gemv2_part)
            g = "g3" if cfg.pk3 and not (cfg.pair and s <= 1 and not last) else "g"
            out.append(Phase(s, li, "attn_wo", st, (q_src, ("hist", li), x_src), None if skipped else ("xb", par, li), why))
            out.append(Phase(s, li, "w13", st, (("xb", par, li),), None if skipped else (g, par, li), why))
            out.append(Phase(s, li, "w2", st, ((g, par, li), ("xb", par, li)), None if skipped else ("x", par, li + 1), why))
        if s in last2:
            if s >= 1:
                out.append(Phase(s, nL, "head", CHECKED, (("x", par, nL),), ("log", par, 0)))
            else:
                out.append(Phase(s, nL, "head", NOT_HANDED, (("x", par, nL),), None, "the logits of position 0 are discarded"))
    return out


def loop_phase_keys(cfg: LoopCfg) -> set:
    """Every (step, layer, phase) of the last two steps, restated without the plan: what a plan must account for."""
    return {(s, li, k) for s in loop_steps(cfg) for li in range(cfg.n_layer) for k in LOOP_KINDS} | \
           {(s, cfg.n_layer, "head") for s in loop_steps(cfg)}


def slow_layers(n_layer: int) -> List[int]:
    return list(range(max(0, n_layer - 2), n_layer))


def plan_slow(n_layer: int, nsplit: int, pk3: bool) -> List[Phase]:
    """The phases of one slow_engine_kernel launch whose records are on the device afterwards (layer li in parity li & 1)."""
    out, g = [], "g3" if pk3 else "g"
    for li in slow_layers(n_layer):
        par = li & 1
        x_src = ("x", par, 0) if li > 0 else ("embed",)
        out.append(Phase(-1, li, "qkv", CHECKED, (x_src,), ("qkv", par, 0)))
        if nsplit > 1:
            out.append(Phase(-1, li, "attn", CHECKED, (("qkv", par, 0), ("cache", li)), ("part", par, 0)))
            out.append(Phase(-1, li, "merge", CHECKED, (("part", par, 0),), ("y", par, 0)))
        else:
            out.append(Phase(-1, li, "attn", CHECKED, (("qkv", par, 0), ("cache", li)), ("y", par, 0)))
            out.append(Phase(-1, li, "merge", NOT_HANDED, (), None, "one KV split: the attention workgroup writes y itself"))
        out.append(Phase(-1, li, "wo", CHECKED, (("y", par, 0), x_src), ("xb", par, 0)))
        out.append(Phase(-1, li, "w13", CHECKED, (("xb", par, 0),), (g, par, 0)))
        out.append(Phase(-1, li, "w2", CHECKED, ((g, par, 0), ("xb", par, 0)), ("x", (li + 1) & 1, 0)))
    return out


def slow_phase_keys(n_layer: int) -> set:
    return {(-1, li, k) for li in slow_layers(n_layer) for k in SLOW_KINDS}


def resident_pairs(F: int, nb: int = NB, res: int = 8) -> np.ndarray:
    """Indices of the SwiGLU units the gathering waves compute in the resident form: the last `res` of every workgroup's share."""
    per = F // nb
    return np.concatenate([np.arange(b * per + per - res, (b + 1) * per) for b in range(nb)])


# ------------------------------------------------------------------------------------------------------ weights
def _w(t) -> torch.Tensor:
    return t.to(torch.bfloat16).to(F64)


@dataclass
class StackWeights:
    layers: List[dict]
    H: int
    Hkv: int
    hd: int
    eps: float
    rope: torch.Tensor
    extra: dict = field(default_factory=dict)


def _layers(sd, prefix: str, n: int) -> List[dict]:
    out = []
    for i in range(n):
        p = f"{prefix}.{i}"
        g = lambda k: _w(sd[k]) if k in sd else None
        out.append(dict(wqkv=g(f"{p}.attention.wqkv.weight"), bqkv=g(f"{p}.attention.wqkv.bias"), attn_norm=g(f"{p}.attention_norm.weight"),
                        qn=g(f"{p}.attention.q_norm.weight"), kn=g(f"{p}.attention.k_norm.weight"), wo=g(f"{p}.attention.wo.weight"),
                        bo=g(f"{p}.attention.wo.bias"), ffn_norm=g(f"{p}.ffn_norm.weight"),
                        w13=torch.stack([g(f"{p}.feed_forward.w1.weight"), g(f"{p}.feed_forward.w3.weight")], dim=1).reshape(-1, sd[f"{p}.feed_forward.w1.weight"].shape[1]),
                        w2=g(f"{p}.feed_forward.w2.weight")))
    return out


def loop_weights(sd, shape) -> StackWeights:
    """The codebook loop's weights as the device holds them (bf16 values; w1 / w3 rows interleaved), from a state dict."""
    from fish_tts_amd.ar_engine import _rope_table
    V = min(1024, shape.codebook_size)
    return StackWeights(_layers(sd, "fast_layers", shape.n_fast_layer), shape.fast_n_head, shape.fast_n_local_heads, shape.fast_head_dim,
                        float(shape.norm_eps), _rope_table(shape.num_codebooks, shape.fast_head_dim, shape.rope_base).to(F64),
                        dict(fast_norm=_w(sd["fast_norm.weight"]), fast_out=_w(sd["fast_output.weight"])[:V], fast_emb=_w(sd["fast_embeddings.weight"])))


def slow_weights(sd, shape) -> StackWeights:
    from fish_tts_amd.ar_engine import _rope_table
    return StackWeights(_layers(sd, "layers", shape.n_layer), shape.n_head, shape.n_local_heads, shape.head_dim, float(shape.norm_eps),
                        _rope_table(shape.max_seq_len, shape.head_dim, shape.rope_base).to(F64),
                        dict(emb=_w(sd["embeddings.weight"]), cb_emb=_w(sd["codebook_embeddings.weight"]), ncb=shape.num_codebooks,
                             cbsize=shape.codebook_size, sem_begin=shape.semantic_begin_id, sem_end=shape.semantic_end_id,
                             scale=bool(shape.scale_codebook_embeddings)))


# ------------------------------------------------------------------------------------------------------ records and report
@dataclass
class LoopFrame:
    rec: dict                       # ft_test_engine_handoffs(which = 1) after the launch
    hid: np.ndarray                 # f32 [D]: step 0's input
    toks: np.ndarray                # [ncb + 1]: the frame the launch finished (token, then the codes)
    hist: Optional[list] = None     # per layer (kc, vc) uint16 [Hkv][ncb][hd] of the launch-path twin after the same frame
    tabs: dict = field(default_factory=dict)     # step -> uint16 [QKVN]: the row of the loop's q k v table the step looked up


@dataclass
class SlowFrame:
    rec: dict                       # ft_test_engine_handoffs(which = 0) after the frame
    pos: int                        # the position the launch appended
    toks_in: np.ndarray             # [ncb + 1]: the input column (the frame before)
    caches: Dict[int, tuple]        # layer -> (k, v) uint16 [Hkv][pos + 1][hd] after the launch
    hid: Optional[np.ndarray] = None


@dataclass
class Report:
    flagged: List[str] = field(default_factory=list)
    checked: set = field(default_factory=set)               # keys of the phases that were judged
    listed: Dict[tuple, str] = field(default_factory=dict)  # key -> status of every planned phase
    worst: Dict[str, float] = field(default_factory=dict)   # kind -> largest |got - ref| / bound
    units: int = 0
    phases: int = 0
    tag_units: int = 0
    replica_units: int = 0                                  # replica units found under the current tag (and equal to the source)
    where: List[tuple] = field(default_factory=list)        # (key, frames, columns) of every flagged phase

    def note(self, ph: Phase, ver, frames: int, what: str = "", side: bool = False):
        """side: a check beside the planned phases (the twin's rows, the appended cache row): counted, not a phase."""
        kind = ph.kind if ph.step >= 0 else "slow " + ph.kind
        self.worst[kind] = max(self.worst.get(kind, 0.0), ver.worst)
        self.units += ver.checked
        if not side:
            self.phases += frames
            self.checked.add(ph.key)
        if ver.flagged:
            self.where.append((ph.key, ver.rows, ver.cols))
            self.flagged.append(f"step {ph.step} layer {ph.layer} {ph.kind}{what}: {ver.flagged} of {ver.checked} units outside the bound, largest "
                                f"|got - ref| / bound {ver.worst:.3f}, frames {ver.rows[:8]}, units {ver.cols[:12]}")

    def merge(self, o: "Report"):
        self.flagged += o.flagged; self.checked |= o.checked; self.listed.update(o.listed); self.where += o.where
        for k, v in o.worst.items():
            self.worst[k] = max(self.worst.get(k, 0.0), v)
        self.units += o.units; self.phases += o.phases; self.tag_units += o.tag_units; self.replica_units += o.replica_units
        return self


def _bits(frames, name: str, par: int, li: int, copy: int = 0) -> np.ndarray:
    return np.stack([f.rec[name][copy, par, li] for f in frames])


def _vals(bits) -> torch.Tensor:
    return from_raw(np.ascontiguousarray(bits), FMT).to(F64)


def _tags(rep: Report, frames, ph: Phase, want: List[int]):
    """Every unit of the vector a phase wrote carries the launch's tag; replica units under that tag equal the source."""
    if ph.dst[0] in ("tab", "part"):
        return
    name, par, li = ph.dst
    for f, w in zip(frames, want):
        t = f.rec[name + "_tag"][0, par, li]
        bad = np.nonzero(t != w)[0]
        rep.tag_units += t.size
        if bad.size:
            rep.flagged.append(f"step {ph.step} layer {ph.layer} {ph.kind}: {bad.size} units of {name}[{par}][{li}] carry another tag than "
                               f"{w:#x} (first: unit {int(bad[0])} with {int(t[bad[0]]):#x})")
            rep.where.append((ph.key + ("tag",), [frames.index(f)], bad[:12].tolist()))
        v0 = f.rec[name][0, par, li]
        for cp in range(1, f.rec[name].shape[0]):
            m = f.rec[name + "_tag"][cp, par, li] == w
            rep.replica_units += int(m.sum())
            diff = np.nonzero(m & (f.rec[name][cp, par, li] != v0))[0]
            if diff.size:
                rep.flagged.append(f"step {ph.step} layer {ph.layer} {ph.kind}: replica {cp - 1} of {name}[{par}][{li}] holds {diff.size} units "
                                   f"under the current tag that differ from the source (first: unit {int(diff[0])})")
                rep.where.append((ph.key + ("replica", cp - 1), [frames.index(f)], diff[:12].tolist()))


# ------------------------------------------------------------------------------------------------------ the codebook loop
def _loop_input(W: StackWeights, frames, src: tuple) -> torch.Tensor:
    if src[0] == "hid":
        return torch.from_numpy(np.stack([f.hid for f in frames]).astype(np.float32)).to(F64)
    if src[0] == "emb":
        return torch.stack([W.extra["fast_emb"][int(f.toks[src[1]])] for f in frames])
    if src[0] == "tab":
        return _vals(np.stack([f.tabs[src[1]] for f in frames]))
    return _vals(_bits(frames, *src))


def check_loop(cfg: LoopCfg, W: StackWeights, frames: List[LoopFrame], seed: int = 0) -> Report:
    """All planned phases of the codebook-loop launches of `frames` (one context, one run), frame f = row f of each product."""
    rep = Report()
    H, Hkv, hd, eps, nL = W.H, W.Hkv, W.hd, W.eps, cfg.n_layer
    F_ = len(frames)
    kvw = Hkv * hd
    for ph in plan_loop(cfg):
        if not ph.extra:
            assert ph.key not in rep.listed, ph.key
            rep.listed[ph.key] = ph.status
        if ph.status != CHECKED:
            continue
        s, li = ph.step, ph.layer
        l = W.layers[li] if li < nL else None
        want = [tag16(int(f.rec["epoch"]) - EPOCH_STEP + s) for f in frames]
        if ph.kind in ("qkv", "qkv_tab"):
            x = _loop_input(W, frames, ph.src[0])
            ref = A.gemv_ref(FMT, A.PRO_RMSNORM, A.EPI_STORE, x=x, W=l["wqkv"], gain=l["attn_norm"], bias=l["bqkv"], eps=eps, seed=seed)
            got = np.stack([f.tabs[s] for f in frames]) if ph.kind == "qkv_tab" else _bits(frames, *ph.dst)
        elif ph.kind == "attn_wo":
            qkv = _loop_input(W, frames, ph.src[0])
            x = _loop_input(W, frames, ph.src[2])
            kc = np.zeros((F_, Hkv, cfg.ncb, hd), dtype=np.uint16)
            vc = np.zeros_like(kc)
            kerr = None
            if frames[0].hist is not None:
                for i, f in enumerate(frames):
                    kc[i], vc[i] = f.hist[li]
            elif s > 0:
                # two codebooks: position 0's K / V are restated from the engine's own record of its q k v
                assert s == 1, "a K/V history deeper than one position needs the launch-path twin"
                q0 = _vals(_bits(frames, "qkv", 0, li))
                r0 = A.fast_attn_ref(FMT, q0, 0, l["qn"], l["kn"], kc, vc, W.rope, H, Hkv, hd, eps)
                k0, e0 = A.rch(r0.k.ref, r0.k.err, FMT)
                kc[:, :, 0] = h16_bits(k0, FMT).reshape(F_, Hkv, hd)
                vc[:, :, 0] = _bits(frames, "qkv", 0, li)[:, (H + Hkv) * hd:].reshape(F_, Hkv, hd)
                kerr = e0[:, :, None, :]
            ar = A.fast_attn_ref(FMT, qkv, s, l["qn"], l["kn"], kc, vc, W.rope, H, Hkv, hd, eps, k_hist_err=kerr)
            if frames[0].hist is not None:
                # the twin's rows of this position against the engine's recorded q k v (K within norm_rope's bound, V a copy)
                kt = np.stack([f.hist[li][0][:, s] for f in frames])
                vt = np.stack([f.hist[li][1][:, s] for f in frames])
                vk = A.check(kt, ar.k.ref, ar.k.err, FMT)
                rep.note(Phase(s, li, "twin_k", CHECKED, (), None), vk, F_, " (the twin's K row against the recorded q k v)", side=True)
                vq = h16_bits(qkv[:, (H + Hkv) * hd:], FMT).reshape(F_, Hkv, hd)
                if not np.array_equal(vt, vq):
                    rep.flagged.append(f"step {s} layer {li}: the twin's V row differs from the v part of the engine's recorded q k v")
                    rep.where.append(((s, li, "twin_v"), [], []))
            yr, ey = A.rch(ar.y.ref, ar.y.err, FMT)
            ref = A.gemv_ref(FMT, A.PRO_NONE, A.EPI_RESID, x=yr, W=l["wo"], bias=l["bo"], resid=x, eps=eps, seed=seed, dx_in=ey)
            got = _bits(frames, *ph.dst)
        elif ph.kind == "w13":
            ref = A.gemv_ref(FMT, A.PRO_RMSNORM, A.EPI_SWIGLU, x=_vals(_bits(frames, *ph.src[0])), W=l["w13"], gain=l["ffn_norm"], eps=eps, seed=seed)
            got = _bits(frames, *ph.dst)
        elif ph.kind == "w2":
            ref = A.gemv_ref(FMT, A.PRO_NONE, A.EPI_RESID, x=_vals(_bits(frames, *ph.src[0])), W=l["w2"], resid=_vals(_bits(frames, *ph.src[1])),
                             eps=eps, seed=seed)
            got = _bits(frames, *ph.dst)
        else:
            assert ph.kind == "head", ph.kind
            ref = A.gemv_ref(FMT, A.PRO_RMSNORM, A.EPI_STORE, x=_vals(_bits(frames, *ph.src[0])), W=W.extra["fast_out"], gain=W.extra["fast_norm"],
                             eps=eps, seed=seed)
            got = _bits(frames, *ph.dst)
        rep.note(ph, A.check(got, ref.ref, ref.err, FMT), F_)
        _tags(rep, frames, ph, want)
    return rep


# ------------------------------------------------------------------------------------------------------ the slow stack
def check_slow(W: StackWeights, frames: List[SlowFrame], seed: int = 0) -> Report:
    """All planned phases of the slow-stack launches of `frames`: the last two layers, frame f = row f of each product."""
    rep = Report()
    H, Hkv, hd, eps, nL = W.H, W.Hkv, W.hd, W.eps, len(W.layers)
    X = W.extra
    F_ = len(frames)
    ns = int(frames[0].rec["nsplit"])
    pos = np.array([f.pos for f in frames])
    for ph in plan_slow(nL, ns, bool(frames[0].rec["pk3"])):
        rep.listed[ph.key] = ph.status
        if ph.status != CHECKED:
            continue
        li = ph.layer
        l = W.layers[li]
        e_launch = [int(f.rec["epoch"]) - 2 * EPOCH_STEP for f in frames]        # the slow launch of a frame: two launches back
        want = [tag16(e + li + (1 if ph.kind == "w2" else 0)) for e in e_launch]
        dx = None
        if ("embed",) in ph.src:
            er = A.embed_ref(FMT, X["emb"], X["cb_emb"], np.stack([f.toks_in for f in frames]), X["ncb"], X["cbsize"], X["sem_begin"],
                             X["sem_end"], X["scale"])
            x_in, dx = A.rch(er.ref, er.err, FMT)
        elif ph.kind in ("qkv", "wo"):
            x_in = _vals(_bits(frames, *ph.src[-1]))
        if ph.kind == "qkv":
            ref = A.gemv_ref(FMT, A.PRO_RMSNORM, A.EPI_STORE, x=x_in, W=l["wqkv"], gain=l["attn_norm"], bias=l["bqkv"], eps=eps, seed=seed, dx_in=dx)
            got = _bits(frames, *ph.dst)
        elif ph.kind == "attn":
            qkv = _vals(_bits(frames, "qkv", li & 1, 0))
            n = int(pos.max()) + 1
            kc = np.zeros((F_, Hkv, n, hd), dtype=np.uint16)
            vc = np.zeros_like(kc)
            for i, f in enumerate(frames):
                kc[i, :, :f.pos + 1], vc[i, :, :f.pos + 1] = f.caches[li]
            pr = A.decode_attn_ref(FMT, qkv, pos, l["qn"], l["kn"], kc, vc, W.rope, H, Hkv, hd, ns, eps, seed=seed)
            rows = np.arange(F_)
            vk = A.check(kc[rows, :, pos], pr.k.ref, pr.k.err, FMT)
            rep.note(Phase(-1, li, "append_k", CHECKED, (), None), vk, F_, " (the appended K row)", side=True)
            if not np.array_equal(vc[rows, :, pos], h16_bits(pr.v, FMT).reshape(F_, Hkv, hd)):
                rep.flagged.append(f"slow layer {li}: the appended V row is not the v part of the recorded q k v")
                rep.where.append(((-1, li, "append_v"), [], []))
            if ns > 1:
                part = np.stack([f.rec["part"][li & 1] for f in frames])                 # [F, H, ns, hd + 2]
                pv = A.check_parts(part[..., :hd], part[..., hd:], pr)
                ver = A.Verdict(pv.checked, pv.flagged, pv.worst, sorted({w[0] for w in pv.where}), sorted({w[1] for w in pv.where}))
                rep.note(ph, ver, F_, " (row, head, split) " + str(pv.where[:6]) if pv.flagged else "")
                for f, e in zip(frames, e_launch):
                    t = f.rec["part_tag"][li & 1]
                    rep.tag_units += t.size
                    if not bool((t == tag32(e + li)).all()):
                        rep.flagged.append(f"slow layer {li}: {int((t != tag32(e + li)).sum())} split-partial words carry another tag than {tag32(e + li):#x}")
                        rep.where.append(((-1, li, "attn", "tag"), [], []))
                continue
            raise AssertionError("one KV split (a 512-row cache without the XCD-local form): planned, no GPU case runs it yet")
        elif ph.kind == "merge":
            part = np.stack([f.rec["part"][li & 1] for f in frames])
            y, e, _, _ = A.merge_ref(part[..., :hd], part[..., hd:], FMT)
            ref = A.Ref(y, e, A.store(y, FMT))
            got = _bits(frames, *ph.dst)
        elif ph.kind == "wo":
            ref = A.gemv_ref(FMT, A.PRO_NONE, A.EPI_RESID, x=_vals(_bits(frames, *ph.src[0])), W=l["wo"], bias=l["bo"], resid=x_in, eps=eps, seed=seed)
            if dx is not None:
                ref = A.Ref(ref.ref, ref.err + dx, ref.rnd, ref.r_stage)
            got = _bits(frames, *ph.dst)
        elif ph.kind == "w13":
            ref = A.gemv_ref(FMT, A.PRO_RMSNORM, A.EPI_SWIGLU, x=_vals(_bits(frames, *ph.src[0])), W=l["w13"], gain=l["ffn_norm"], eps=eps, seed=seed)
            got = _bits(frames, *ph.dst)
        else:
            assert ph.kind == "w2", ph.kind
            ref = A.gemv_ref(FMT, A.PRO_NONE, A.EPI_RESID, x=_vals(_bits(frames, *ph.src[0])), W=l["w2"], resid=_vals(_bits(frames, *ph.src[1])),
                             eps=eps, seed=seed)
            got = _bits(frames, *ph.dst)
            if li == nL - 1 and frames[0].hid is not None:
                # the stack's output is also left as plain f32 (x_out: the head's and the loop's input): the same values
                hid = np.stack([f.hid for f in frames]).astype(np.float32)
                if not np.array_equal(h16_bits(torch.from_numpy(hid), FMT), got) or not np.array_equal(_vals(got).to(F32).numpy(), hid):
                    rep.flagged.append("the slow stack's plain f32 output differs from its last hand-off vector")
                    rep.where.append(((-1, li, "w2", "x_out"), [], []))
        rep.note(ph, A.check(got, ref.ref, ref.err, FMT), F_)
        _tags(rep, frames, ph, want)
    return rep


# ------------------------------------------------------------------------------------------------------ emulation
BUGS = ("swiglu_unrounded", "gain_other_layer", "pair_swapped", "hist_prev", "stale_code_head", "logit_shift", "two_ulp",
        "replica_stale", "tag_prev_step")


def _swiglu_f32(x, l, eps):
    """eng_gemv_rows' SwiGLU epilogue in float32 WITHOUT its last rounding (ar_ref.emulate_gemv's steps): the planted fault."""
    x32, W32 = x.to(F32), l["w13"].to(F32)
    K = x32.shape[1]
    NT, VEC = A.pick_nt(K, FMT), A.vec(FMT)
    xl = A._lanes(x32, NT, VEC)
    inv = 1.0 / torch.sqrt(A._chain_dot(xl, xl)[:, None] / float(K) + torch.tensor(eps, dtype=F32))
    xn = A._r32(A._r32(x32 * inv, FMT) * l["ffn_norm"].to(F32)[None, :], FMT)
    v = A._r32(A._chain_dot(A._lanes(W32, NT, VEC)[None], A._lanes(xn, NT, VEC)[:, None]), FMT)
    gate, up = v[:, 0::2], v[:, 1::2]
    return (A._r32(gate / (1.0 + torch.exp(-gate)), FMT) * up).to(F64)


def emulate_loop(cfg: LoopCfg, W: StackWeights, hid, toks, epoch: int, bug: Optional[str] = None, at: Optional[dict] = None,
                 resume=None, prev: Optional[LoopFrame] = None, copies: int = 2):
    """One fast_engine_kernel launch in float32 (ar_ref.emulate_gemv / emulate_fast_attn, teacher-forced on the codes toks[1:])
    -> (LoopFrame with the records the hook would return, the emulated launch-path K/V history in .hist; snapshots).
    epoch: the word the launch read.  prev: the launch before it on the same buffers (what a stale unit holds).
    bug / at {step, layer, unit, wg}: one planted fault of tests/test_engine_phase_ref_host.py.  resume = (step, snapshot of an
    honest run at that step): only the steps from there on are recomputed."""
    assert bug is None or bug in BUGS, bug
    at = at or {}
    nL, ncb, H, Hkv, hd, eps = cfg.n_layer, cfg.ncb, W.H, W.Hkv, W.hd, W.eps
    D, QKVN = W.layers[0]["wqkv"].shape[1], W.layers[0]["wqkv"].shape[0]
    Ff, V = W.layers[0]["w2"].shape[1], W.extra["fast_out"].shape[0]
    hid = torch.as_tensor(np.asarray(hid, dtype=np.float32)).to(F64).reshape(1, D)
    if resume is None:
        rec = dict(n_layer=nL, ncb=ncb, pair=int(cfg.pair), qkv0=int(cfg.qkv0), pk3=int(cfg.pk3), resident=int(cfg.resident), relay=int(copies > 1),
                   copies=copies, epoch=epoch + EPOCH_STEP, epoch_step=EPOCH_STEP, D=D, QKVN=QKVN, F=Ff, V=V, H=H, Hkv=Hkv, hd=hd, line=32, xl=0, nsplit=1,
                   code=np.zeros((copies, ncb, 32), dtype=np.uint32))
        for name, (layers, n) in dict(x=(nL + 1, D), qkv=(nL, QKVN), xb=(nL, D), g=(nL, Ff), g3=(nL, Ff), log=(1, V)).items():
            if name == "g3" and not cfg.pk3:
                continue
            for sfx in ("", "_tag"):
                rec[name + sfx] = prev.rec[name + sfx].copy() if prev is not None else np.zeros((copies, 2, layers, n), dtype=np.uint16)
        kc = np.zeros((nL, 1, Hkv, ncb, hd), dtype=np.uint16)
        vc, tabs, s0 = np.zeros_like(kc), {}, 0
    else:
        import copy
        s0, (rec, kc, vc, tabs) = resume[0], copy.deepcopy(resume[1])
    snaps = {}

    def put(name, par, li, v, tag):
        rec[name][:, par, li] = h16_bits(v, FMT).reshape(-1)
        rec[name + "_tag"][:, par, li] = tag

    def chain(s, x, kcs, vcs, record):
        """Step s from its layer-0 input x; record: write the hand-offs (False: a stale chain computed beside the launch)."""
        par, tag = s & 1, tag16(epoch + s)
        for li in range(nL):
            l = W.layers[li]
            here = record and at.get("step") == s and at.get("layer") == li
            qkv = A.emulate_gemv(FMT, A.PRO_RMSNORM, A.EPI_STORE, x, l["wqkv"], l["attn_norm"], l["bqkv"], eps=eps)
            if cfg.qkv0 and s >= 2 and li == 0:
                if record:
                    tabs[s] = h16_bits(qkv, FMT).reshape(-1)
            elif record:
                put("qkv", par, li, qkv, tag)
            kr, vr = kcs[li].copy(), vcs[li].copy()
            if here and bug == "hist_prev" and s >= 2:           # history position j - 1 read for j
                kr[:, :, 1:s], vr[:, :, 1:s] = kcs[li][:, :, 0:s - 1], vcs[li][:, :, 0:s - 1]
            y, k = A.emulate_fast_attn(FMT, qkv, s, l["qn"], l["kn"], kr, vr, W.rope, H, Hkv, hd, eps)
            kcs[li][0, :, s] = h16_bits(k, FMT).reshape(Hkv, hd)
            vcs[li][0, :, s] = h16_bits(qkv[:, (H + Hkv) * hd:], FMT).reshape(Hkv, hd)
            if cfg.pair and s == 0 and li == nL - 1:
                return None
            xb = A.emulate_gemv(FMT, A.PRO_NONE, A.EPI_RESID, y, l["wo"], bias=l["bo"], resid=x, eps=eps)
            g = A.emulate_gemv(FMT, A.PRO_RMSNORM, A.EPI_SWIGLU, xb, l["w13"], l["ffn_norm"], eps=eps)
            if here and bug in ("gain_other_layer", "pair_swapped"):
                alt = A.emulate_gemv(FMT, A.PRO_RMSNORM, A.EPI_SWIGLU, xb, l["w13"], W.layers[(li + 1) % nL]["ffn_norm"], eps=eps) \
                    if bug == "gain_other_layer" else A.emulate_gemv(FMT, A.PRO_RMSNORM, A.EPI_SWIGLU, xb, l["w13"], l["ffn_norm"], eps=eps, bug="swap_gate_up")
                g[:, at["unit"]] = alt[:, at["unit"]]
            g_in = _swiglu_f32(xb, l, eps) if here and bug == "swiglu_unrounded" else g
            x2 = A.emulate_gemv(FMT, A.PRO_NONE, A.EPI_RESID, g_in, l["w2"], resid=xb, eps=eps)
            if here and bug == "two_ulp":                        # one unit of the layer's output two bf16 steps off
                x2 = from_raw((h16_bits(x2, FMT) + np.where(np.arange(D) == at["unit"], 2, 0).astype(np.uint16)[None, :]), FMT).to(F64)
            if record:
                put("xb", par, li, xb, tag)
                put("g3" if cfg.pk3 and not (cfg.pair and s <= 1 and li < nL - 1) else "g", par, li, g, tag)
                put("x", par, li + 1, x2, tag)
            x = x2
        return x

    for s in range(s0, ncb):
        if s >= ncb - 2:
            import copy
            snaps[s] = copy.deepcopy((rec, kc, vc, tabs))
        x = hid if s == 0 else W.extra["fast_emb"][int(toks[s])][None, :]
        xs = chain(s, x, kc, vc, True)
        if s >= 1:
            par, tag = s & 1, tag16(epoch + s)
            log = A.emulate_gemv(FMT, A.PRO_RMSNORM, A.EPI_STORE, xs, W.extra["fast_out"], W.extra["fast_norm"], eps=eps)
            if at.get("step") == s and bug == "stale_code_head":
                # workgroup wg ran the step from the code before this one: its four head rows come from that chain
                stale = chain(s, W.extra["fast_emb"][int(toks[s - 1])][None, :], kc.copy(), vc.copy(), False)
                ls = A.emulate_gemv(FMT, A.PRO_RMSNORM, A.EPI_STORE, stale, W.extra["fast_out"], W.extra["fast_norm"], eps=eps)
                per = V // NB
                log[:, at["wg"] * per:(at["wg"] + 1) * per] = ls[:, at["wg"] * per:(at["wg"] + 1) * per]
            if at.get("step") == s and bug == "logit_shift":
                u = at["wg"] * (V // NB)
                log[:, u] = log[:, u - 1].clone()
            put("log", par, 0, log, tag)
    if bug in ("replica_stale", "tag_prev_step"):
        s, li, name = at["step"], at["layer"], at["name"]
        par = s & 1
        if bug == "tag_prev_step":
            rec[name + "_tag"][0, par, li, at["unit"]] = tag16(epoch + s - 1)
        else:
            p0 = at["unit"] // 256 * 256                                 # one 1 KiB piece of the XCD's replica: last launch's values, this one's tag
            rec[name][1, par, li, p0:p0 + 256] = prev.rec[name][1, par, li, p0:p0 + 256]
    fr = LoopFrame(rec, hid.to(F32).numpy().reshape(-1), np.asarray(toks), [(kc[li][0].copy(), vc[li][0].copy()) for li in range(nL)] if ncb > 2 else None, tabs)
    return fr, snaps
