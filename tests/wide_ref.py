"""Float64 reference of the lock-step batch kernels of csrc/wide_kernels.h and of the wide slow-stack attention, ONE
LAUNCH AT A TIME (host only; test infrastructure, the sibling of tests/codec_stage_ref.py, whose number-format helpers,
three-order `r_stage` measurement, MARGIN and op-by-op error terms it reuses).

The kernels are restated from oracle/ar.py (rms_norm, _mlp, _block, _attention, rope) as wide_kernels.h cites llama.py:

  linear_ref     RMSNorm (sum of squares, 1 / sqrt(ss / K + eps), round16(round16(x inv) gain)) fused in front of a
                 16-bit x 16-bit contraction with f32 accumulation, then one of three epilogues:
                     store     round16(acc + bias)
                     SwiGLU    round16(round16(silu(round16 gate)) * round16 up), weight rows (2i, 2i+1) = (gate, up) of column i
                     residual  round16(round16(acc + bias) + resid)            (no norm in front)
  attn_ref       q / k nn.RMSNorm (ONE rounding: F.rms_norm rounds (x inv) gain once), RoPE with the bf16 table and a
                 rounding, the K / V append at pos, f32 scores, an exact-maximum softmax over [0, pos], one rounding of y.

Each returns `ref`, the float64 value BEFORE the last rounding, `rnd`, that value rounded (what a chain feeds on), and `err`,
a bound on |device value before the last rounding - ref|.  `check` then demands, of EVERY element,

    |got - ref| <= half a ulp of the stored 16-bit format at max(|got|, |ref|) + err.

Error model (u = 2^-24; every f32 operation returns its exact result times (1 + d), |d| <= u):

  contraction.  16-bit x 16-bit is exact in f32 (8 + 8 or 11 + 11 significand bits), so the only error is the order of the
      f32 sums: E = min(MARGIN r_stage, K 2^-23) S, S = sum |xn| |w|, r_stage = the largest |f32 - f64| / S of the same
      sums in three f32 orders (codec_stage_ref.measure_r: one chain, per-32 blocks, pairwise) measured on THIS
      reference's operands only, never on device output.
  fused RMSNorm.  The sum of squares has non-negative terms; / K, + eps, 1 / sqrt and the product x inv: the device's
      t' = x inv is within d = (K / 512 + 10) u |t| of the float64 t (the RMSNorm term of codec_stage_ref.py).  t never
      leaves the registers, so which way round16(t') fell cannot be read back: where [t - d, t + d] holds a rounding
      boundary of the 16-bit format the device may hold EITHER neighbour a' of a = round16(t).  a gain is exact in f32
      (the same significand count), so xn' = round16(a' gain) is then known exactly for both candidates, and the
      operand's uncertainty is dx = max |round16(a' gain) - xn| over them: zero for an operand away from a boundary, and
      for one at a boundary the step the issue calls ulp16(xn) - computed, not assumed, because a one-step change of a
      is gain steps of a gain and lands 0, 1 or (gain > 1, or a binade edge) 2 steps away.  Such operands are counted per
      row (`amb`), and  sum_k |w_k| dx_k  goes into the element's bound.  Nothing else of the norm's error survives the
      rounding.
  every later INTERMEDIATE rounding (the gate, the up value, silu, acc + bias before the residual add; q, k after the
      norm and after the rotation).  The same rule, `reach`: with running error e at value v, the device rounds some
      v' in [v - e, v + e]; the error after the rounding is max(|round16(v - e) - round16(v)|, |round16(v + e) -
      round16(v)|): nothing where the interval holds no boundary, one step of that format where it holds one.
      (round16 goes through float32 first; the double rounding moves a boundary by at most 2^-29 relative, far inside e.)
  epilogue, op by op as in codec_stage_ref.py: v = acc + bias: e = E + u |v|.  silu (Lipschitz <= 1.1, expf to 2^-20
      relative): e = 1.1 e_gate + (2^-20 + 3 u) |silu|, then `reach`.  o = silu up: e = |up| e_s + |silu| e_up + e_s e_up + u |o|.
      Residual add: e = reach(e) + u |o|.
  q / k norm over hd: e = (hd / 512 + 10) u |v|, then `reach`.  RoPE: two products and one sum,
      e = |c| e_x0 + |s| e_x1 + 2 u (|x0 c| + |x1 s|) (and the twin); the appended K row is checked against this value,
      the scores use `reach` of it; V is a copy.
  attention over n = pos + 1 keys: a score is an hd-term sum times the scale.  The codec's worst-case chain term
      (hd + 2) u sum |q| |k| is several fp16 steps of y wide, so the order error of the two sums is measured like a
      contraction's: r_sc and r_pv = the largest |f32 - f64| / S of the q . k and the P V sums in the three f32 orders, on
      one seeded kv head per row, and ds = scale (e_q . |k| + |q| . e_k + e_q . e_k) + min(MARGIN r_sc, (hd + 2) u) scale
      sum |q| |k| + u |s|; the exponent s - max adds u |s - max|; an absolute error D in the exponent is a relative e^D - 1
      in the weight, expf adds 2^-20; numerator and denominator both carry it, the sum of the weights adds (n / 64 + 8) u,
      the products and the P V sum min(MARGIN r_pv, (n + 2) u) + 4 u:
          err = (2 (e^D - 1 + (1 + RS) 2^-20) + (min(MARGIN r_pv, (n + 2) u) + (n / 64 + 12 + 2 RS) u)) sum_j softmax_j |v_j|,
      D = max_j (ds_j + u |s_j - max|).  RS = 0 for the two-pass attn_wide_kernel.  The split fall-back (attn_decode_kernel
      + attn_combine_rows_kernel) keeps an online softmax per lane group: whenever a group's running maximum rises, what it
      gathered is rescaled by one more expf and product.  RS = the largest number of rises any (head, split, lane group)
      chain sees in the reference's own scores, + 2 for the merge of the lane groups and of the splits.

`emulate_*` restate the same launches in float32 with the device's work split (per-wave K slices summed in wave order,
per-32 k blocks, a two-pass softmax summed per lane-group slot) and 16-bit stores: an honest stand-in for the device
from which tests/test_wide_ref_host.py builds outputs with and without injected bugs.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from tests.codec_stage_ref import F32, F64, LIB, MARGIN, U, blocked32, f32_orders, from_raw, h16_bits, half_ulp, measure_r

STORE, SWIGLU, RESID = 0, 1, 2
FMT_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
OVERFLOW = {"bf16": float(2.0 ** 128 - 2.0 ** 119), "fp16": 65520.0}     # magnitudes from here on round to infinity
# the class ids ft_test_wide_linear reports (include/fishtts_hip_test.h)
ID_S11, ID_S12, ID_S22, ID_G12, ID_G22, ID_R11, ID_HEAD = range(7)


def round16(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """Round to nearest even into the 16-bit format, returned in the dtype of x (float64 or float32)."""
    return x.to(F32).to(FMT_DT[fmt]).to(x.dtype)


def reach(v: torch.Tensor, e: torch.Tensor, fmt: str):
    """round16(v) and how far the rounding of any value within e of v can land from it (zero away from a boundary)."""
    r = round16(v, fmt)
    lo, hi = round16(v - e, fmt), round16(v + e, fmt)
    return r, torch.maximum((lo - r).abs(), (hi - r).abs())


def values(bits, fmt: str) -> torch.Tensor:
    """uint16 patterns of fmt (or float32 values) -> float64 values."""
    return from_raw(np.asarray(bits), fmt).to(F64)


@dataclass
class Ref:
    ref: torch.Tensor                      # float64, before the last rounding
    err: torch.Tensor
    rnd: torch.Tensor                      # ref rounded to the format
    r_stage: Optional[float] = None
    amb: Optional[torch.Tensor] = None     # per row: operands the fused norm may have rounded either way


def rms_inv(x: torch.Tensor, eps: float) -> torch.Tensor:
    return 1.0 / torch.sqrt((x * x).mean(dim=-1, keepdim=True) + float(np.float32(eps)))


def linear_pre(fmt: str, epi: int, X, W, gain=None, eps: float = 1e-6, seed: int = 0):
    """The fused norm and the contraction of one wide Linear, shared by its runs with and without a bias:
    (acc [M, N] float64, E: the bound on the device's accumulator, r_stage, amb)."""
    X, W = X.to(F64), W.to(F64)
    M, K = X.shape
    amb = None
    if epi != RESID:
        g = gain.to(F64)[None, :]
        t = X * rms_inv(X, eps)
        d = (K / 512 + 10) * U * t.abs()
        a, alo, ahi = round16(t, fmt), round16(t - d, fmt), round16(t + d, fmt)
        xn = round16(a * g, fmt)
        dx = torch.maximum((round16(alo * g, fmt) - xn).abs(), (round16(ahi * g, fmt) - xn).abs())
        amb = (alo != ahi).sum(dim=-1)
    else:
        xn, dx = X, torch.zeros_like(X)
    Wt = W.t().contiguous()
    Wa = Wt.abs()
    r = measure_r(xn, Wt, seed=seed + 31 * M + W.shape[0])
    E = min(MARGIN * r, K * 2.0 ** -23) * ((xn.abs() + dx) @ Wa) + dx @ Wa
    return xn @ Wt, E, r, amb


def linear_ref(fmt: str, epi: int, X=None, W=None, gain=None, bias=None, resid=None, eps: float = 1e-6, seed: int = 0,
               pre=None, rows: Optional[int] = None) -> Ref:
    """One wide Linear.  X [M, K], W [N, K], gain [K], resid [M, N]: exact 16-bit values as tensors; bias [N] f32.
    pre: a linear_pre result to reuse; rows: only its first `rows` rows (the rows of a Linear do not depend on each other)."""
    v, err, r, amb = pre if pre is not None else linear_pre(fmt, epi, X, W, gain, eps, seed)
    if rows is not None:
        v, err, amb = v[:rows], err[:rows], None if amb is None else amb[:rows]
    if bias is not None:
        v = v + bias.to(F64)[None, :]
        err = err + U * v.abs()
    if epi == SWIGLU:
        gr, eg = reach(v[:, 0::2], err[:, 0::2], fmt)
        ur, eu = reach(v[:, 1::2], err[:, 1::2], fmt)
        s = gr / (1.0 + torch.exp(-gr))
        sr, es = reach(s, 1.1 * eg + (LIB + 3 * U) * s.abs(), fmt)
        v = sr * ur
        err = ur.abs() * es + sr.abs() * eu + es * eu + U * v.abs()
    elif epi == RESID:
        vr, ev = reach(v, err, fmt)
        v = vr + resid.to(F64)[:v.shape[0]]
        err = ev + U * v.abs()
    return Ref(v, err, round16(v, fmt), r, amb)


@dataclass
class Verdict:
    checked: int = 0
    flagged: int = 0
    worst: float = 0.0                                       # largest |got - ref| / bound
    rows: List[int] = field(default_factory=list)            # rows with a flagged element
    cols: List[int] = field(default_factory=list)
    bad: Optional[torch.Tensor] = None


def check(got, ref: torch.Tensor, err: torch.Tensor, fmt: str) -> Verdict:
    """Every element of got (uint16 patterns of fmt, or f32 values holding them) against ref: none is left out.  An
    element whose reference passes the format's overflow threshold by more than err must be that infinity, one that
    stays below it by more than err must be finite; NaN always flags."""
    g = values(got, fmt).reshape(ref.shape)
    ov = OVERFLOW[fmt]
    bound = half_ulp(torch.maximum(g.abs().clamp_max(ov), ref.abs().clamp_max(ov)), False, fmt) + err
    diff = (g - ref).abs()
    bad = ~(diff <= bound)
    inf = torch.isinf(g)
    bad = torch.where(inf, ~((ref.abs() + err >= ov) & (torch.sign(g) == torch.sign(ref))), bad)
    bad = bad | (~inf & (ref.abs() - err >= ov))
    ratio = torch.where(inf, bad.to(F64) * float("inf"), diff / bound).nan_to_num(nan=float("inf"))
    ratio = torch.where(inf & ~bad, torch.zeros_like(ratio), ratio)
    b2 = bad.reshape(bad.shape[0], -1)
    return Verdict(int(diff.numel()), int(bad.sum()), float(ratio.max()), torch.nonzero(b2.any(dim=1)).flatten().tolist(),
                   torch.nonzero(b2.any(dim=0)).flatten().tolist(), bad)


# ------------------------------------------------------------------------------------------------------ attention
def _norm_rope(x: torch.Tensor, gain, tab: torch.Tensor, eps: float, fmt: str, emulate: bool = False):
    """x [heads, hd] -> (value before the rotation's rounding, its error bound, the rounded value, its reach)."""
    hd = x.shape[-1]
    if gain is not None:
        t = (x * rms_inv(x, eps)) * gain[None, :]
        xr, e = reach(t, (hd / 512 + 10) * U * t.abs(), fmt)
    else:
        xr, e = x, torch.zeros_like(x)
    x0, x1, e0, e1 = xr[:, 0::2], xr[:, 1::2], e[:, 0::2], e[:, 1::2]
    c, s = tab[None, :, 0], tab[None, :, 1]
    re, im = x0 * c - x1 * s, x1 * c + x0 * s
    ere = c.abs() * e0 + s.abs() * e1 + 2 * U * ((x0 * c).abs() + (x1 * s).abs())
    eim = c.abs() * e1 + s.abs() * e0 + 2 * U * ((x1 * c).abs() + (x0 * s).abs())
    v = torch.stack([re, im], dim=-1).reshape(x.shape)
    ev = torch.stack([ere, eim], dim=-1).reshape(x.shape)
    r, er = reach(v, ev, fmt)
    return v, ev, r, er


@dataclass
class AttnRef:
    y: Ref
    k: Ref                # the appended K rows [M, Hkv, hd]
    v: torch.Tensor       # the appended V rows (copies of the inputs)


def _r3(X: torch.Tensor, Wm: torch.Tensor) -> float:
    """The largest |f32 - f64| / sum |x| |w| of X @ Wm summed in float32 in the three orders of codec_stage_ref.f32_orders."""
    ref, S = X @ Wm, X.abs() @ Wm.abs()
    ok = S > 0
    return max(float(((o.to(F64) - ref).abs()[ok] / S[ok]).max()) for o in f32_orders(X, Wm)) if bool(ok.any()) else 0.0


def _rescales(sc: torch.Tensor, splits: int) -> int:
    """The online softmax of the fall-back (attn_decode_kernel): split c walks positions [c chunk, (c + 1) chunk), lane
    group `slot` of 16 every 16th of them, rescaling by one more expf whenever its running maximum rises.  Returns the
    largest number of rises any (head, split, slot) chain sees, from the reference's scores sc [H, n]."""
    n = sc.shape[1]
    chunk = (n - 1 + splits) // splits
    worst = 0
    for lo in range(0, n, chunk):
        seq = sc[:, lo:min(lo + chunk, n)]
        pad = (-seq.shape[1]) % 16
        seq = torch.cat([seq, torch.full((seq.shape[0], pad), float("-inf"), dtype=seq.dtype)], dim=1).reshape(seq.shape[0], -1, 16)
        run = torch.cummax(seq, dim=1).values
        worst = max(worst, int((seq[:, 1:] > run[:, :-1]).sum(dim=1).max()) if seq.shape[1] > 1 else 0)
    return worst


def attn_ref(fmt: str, qkv, pos, qn, kn, kc, vc, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6, splits: int = 0,
             seed: int = 0) -> AttnRef:
    """qkv [M, (H + 2 Hkv) hd] (16-bit values), pos [M], qn / kn [hd] or None, kc / vc [M, Hkv, n_slots, hd] (rows < pos
    are read), tab [n_pos, hd / 2, 2]: the bf16-rounded rope table.  splits: 0 = the two-pass attn_wide_kernel, n >= 1 =
    the online-softmax fall-back over n KV splits (what ft_test_wide_attn reports): it sets the rescale count RS of the
    error model only, the reference value is the same."""
    qkv, tab = qkv.to(F64), tab.to(F64)
    qn = None if qn is None else qn.to(F64)
    kn = None if kn is None else kn.to(F64)
    M, G = qkv.shape[0], H // Hkv
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    gen = torch.Generator().manual_seed(seed)
    ys, es, ks, kes, vs, r_max = [], [], [], [], [], 0.0
    for m in range(M):
        p = int(pos[m])
        n = p + 1
        q = qkv[m, :H * hd].reshape(H, hd)
        k = qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd)
        v = qkv[m, (H + Hkv) * hd:].reshape(Hkv, hd)
        _, _, qr, eq = _norm_rope(q, qn, tab[p], eps, fmt)
        kv_, kev, kr, ek = _norm_rope(k, kn, tab[p], eps, fmt)
        K = torch.cat([values(kc[m, :, :p], fmt), kr[:, None, :]], dim=1).repeat_interleave(G, dim=0)       # [H, n, hd]
        V = torch.cat([values(vc[m, :, :p], fmt), v[:, None, :]], dim=1).repeat_interleave(G, dim=0)
        sc = torch.einsum("hd,hnd->hn", qr, K) * scale
        pw = torch.softmax(sc, dim=-1)
        # the two sums' order error, measured on one seeded kv head of the row (a maximum over fewer elements is smaller)
        h0 = int(torch.randint(0, Hkv, (1,), generator=gen)) * G
        r_sc, r_pv = _r3(qr[h0:h0 + G], K[h0].t().contiguous()), _r3(pw[h0:h0 + G], V[h0].contiguous())
        r_max = max(r_max, r_sc, r_pv)
        ds = scale * torch.einsum("hd,hnd->hn", eq, K.abs()) + U * sc.abs() \
            + min(MARGIN * r_sc, (hd + 2) * U) * scale * torch.einsum("hd,hnd->hn", qr.abs(), K.abs())
        ekh = ek.repeat_interleave(G, dim=0)
        ds[:, p] += scale * ((qr.abs() * ekh).sum(-1) + (eq * ekh).sum(-1))
        mx = sc.max(dim=-1, keepdim=True).values
        D = (ds + U * (sc - mx).abs()).max(dim=-1, keepdim=True).values
        RS = 0 if splits == 0 else _rescales(sc, splits) + 2                   # + the merge of the 16 slots, + the merge of the splits
        rel = 2 * (torch.expm1(D) + (1 + RS) * LIB) + (min(MARGIN * r_pv, (n + 2) * U) + (n / 64 + 12 + 2 * RS) * U)
        ys.append(torch.einsum("hn,hnd->hd", pw, V).reshape(-1))
        es.append((rel * torch.einsum("hn,hnd->hd", pw, V.abs())).reshape(-1))
        ks.append(kv_); kes.append(kev); vs.append(v)
    y, e, k, ke = torch.stack(ys), torch.stack(es), torch.stack(ks), torch.stack(kes)
    return AttnRef(Ref(y, e, round16(y, fmt), r_max), Ref(k, ke, round16(k, fmt)), torch.stack(vs))


# ------------------------------------------------------------------------------------------------------ emulation
def emulate_linear(fmt: str, epi: int, X, W, gain=None, bias=None, resid=None, eps: float = 1e-6, NW: int = 8, TS: int = 1,
                   bug: Optional[str] = None) -> torch.Tensor:
    """The launch in float32 as the device splits it: NW waves each own K / NW consecutive k (sum of squares and partial
    tile per wave, summed in wave order), per-32 k blocks inside a wave.  Returns the stored values (float64 tensor of
    exact 16-bit values).  bug: one of the emulated kernel faults of tests/test_wide_ref_host.py."""
    X32, W32 = X.to(F32), W.to(F32)
    M, K = X32.shape
    ks = K // NW
    if epi != RESID:
        ss = torch.zeros(M, 1, dtype=F32)
        for w in range(NW):
            xs = X32[:, w * ks:(w + 1) * ks]
            ss = ss + (xs * xs).sum(dim=-1, keepdim=True)
        if bug == "norm_neighbour":                                   # row m's statistic read from row m + 1
            ss = torch.roll(ss, -1, dims=0)
        inv = 1.0 / torch.sqrt(ss / K + torch.tensor(eps, dtype=F32))
        g32 = gain.to(F32)[None, :]
        xn = round16((X32 * inv) * g32, fmt) if bug == "single_round" else round16(round16(X32 * inv, fmt) * g32, fmt)
    else:
        xn = X32
    acc = torch.zeros(M, W32.shape[0], dtype=F32)
    for w in range(NW):
        if bug == "drop_wave" and w == NW - 3:
            continue
        acc = acc + blocked32(xn[:, w * ks:(w + 1) * ks].to(F64), W32[:, w * ks:(w + 1) * ks].t().to(F64))
    if bug == "ts2_rows" and TS == 2:                                 # the second 16-row tile of a TS = 2 workgroup repeats the first
        for m0 in range(0, M, 32):
            n2 = max(0, min(32, M - m0) - 16)
            acc[m0 + 16:m0 + 16 + n2] = acc[m0:m0 + n2]
    v = acc
    if bias is not None and bug != "drop_bias":
        v = v + bias.to(F32)[None, :]
    v = round16(v, fmt)
    if epi == SWIGLU:
        gate, up = (v[:, 1::2], v[:, 0::2]) if bug == "swap_gate_up" else (v[:, 0::2], v[:, 1::2])
        v = round16(round16(gate / (1.0 + torch.exp(-gate)), fmt) * up, fmt)
    elif epi == RESID:
        r32 = resid.to(F32)
        out = round16(v + r32, fmt)
        if bug == "resid_after_store":                               # aliased form: a quarter tile reads its residual after the store
            out[:, 8:12] = round16(v[:, 8:12] + out[:, 8:12], fmt)
        v = out
    return v.to(F64)


def emulate_attn(fmt: str, qkv, pos, qn, kn, kc, vc, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6,
                 bug: Optional[str] = None):
    """attn_wide_kernel in float32: scores of every position, the exact maximum, one exponential per position, the weighted
    V rows summed per lane-group slot (16 slots of positions j = slot mod 16) and the slots in order.  Returns (y, k rows)
    as float64 tensors of exact 16-bit values."""
    M, G = qkv.shape[0], H // Hkv
    scale = torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(hd), dtype=F32))
    tab = tab.to(F32)

    def nr(x, gain, t):
        if gain is not None:
            inv = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / hd + torch.tensor(eps, dtype=F32))
            x = round16((x * inv) * gain.to(F32)[None, :], fmt)
        x0, x1, c, s = x[:, 0::2], x[:, 1::2], t[None, :, 0], t[None, :, 1]
        return round16(torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1).reshape(x.shape), fmt)

    ys, ks = [], []
    for m in range(M):
        p = int(pos[m])
        q = qkv[m, :H * hd].reshape(H, hd).to(F32)
        k = qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd).to(F32)
        v = qkv[m, (H + Hkv) * hd:].reshape(Hkv, hd).to(F32)
        qr, kr = nr(q, qn, tab[p]), nr(k, kn, tab[p])
        K = torch.cat([values(kc[m, :, :p], fmt).to(F32), kr[:, None, :]], dim=1)
        V = torch.cat([values(vc[m, :, :p], fmt).to(F32), v[:, None, :]], dim=1)
        if bug == "stale_pos1":                                       # the walk runs one row past the new position
            K = torch.cat([K, values(kc[m, :, p + 1:p + 2], fmt).to(F32)], dim=1)
            V = torch.cat([V, values(vc[m, :, p + 1:p + 2], fmt).to(F32)], dim=1)
        keep = torch.ones(K.shape[1], dtype=torch.bool)
        if bug == "miss_pos" and p > 0:
            keep[p] = False
        if bug == "miss_128" and K.shape[1] > 128:
            keep[128] = False
        K, V = K[:, keep].repeat_interleave(G, dim=0), V[:, keep].repeat_interleave(G, dim=0)
        sc = torch.einsum("hd,hnd->hn", qr, K) * scale
        e = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        L = e.sum(dim=-1, keepdim=True)
        O = torch.zeros(H, hd, dtype=F32)
        for sl in range(16):
            O = O + torch.einsum("hn,hnd->hd", e[:, sl::16], V[:, sl::16])
        ys.append(round16(O / L, fmt).reshape(-1))
        ks.append(kr)
    return torch.stack(ys).to(F64), torch.stack(ks).to(F64)


# ------------------------------------------------------------------------------------------------------ test inputs
def seeded_linear_inputs(fmt: str, M: int, N: int, K: int, seed: int, w_std: float = 0.03, loud_row: int = 3):
    """The inputs of the GPU and host tests, rounded to the type first: X ~ N(0, 1) with one row scaled by 64 (a mixed-up
    row statistic then shows), W ~ N(0, w_std), gain = 1 + 0.1 N, bias = 0.1 N, resid ~ N(0, 1).  All rows distinct."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, K, generator=g)
    if M > loud_row:
        X[loud_row] *= 64.0
    W = w_std * torch.randn(N, K, generator=g)
    gain = 1.0 + 0.1 * torch.randn(K, generator=g)
    bias = (0.1 * torch.randn(N, generator=g)).to(F32)
    resid = torch.randn(M, N, generator=g)
    r = lambda t: round16(t.to(F32), fmt)
    return r(X), r(W), r(gain), bias, r(resid)


def interleave_w13(w1: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """[2 F, K]: rows (2i, 2i + 1) = (gate, up) of column i, the layout the SwiGLU epilogue reads."""
    return torch.stack([w1, w3], dim=1).reshape(-1, w1.shape[1])
