"""Float64 reference of the bf16 prompt pass (csrc/engine.hip: prefill_gemm), ONE LAUNCH AT A TIME (host only; test
infrastructure, the sibling of tests/codec_stage_ref.py and tests/wide_ref.py, whose number-format helpers, three-order
`r_stage` measurement, MARGIN, `reach`, `_norm_rope`, epilogue error terms, `check` and `Verdict` it reuses).

The launches are restated from oracle/ar.py (rms_norm, _mlp, _block, _attention, rope) as gemm_kernels.h / ar_kernels.h cite
llama.py:

  linear_ref   a bf16 x bf16 contraction with f32 accumulation, then one of the four forms prefill_gemm uses (epilogues of
               gemm_kernels.h: tapgemm_epilogue, tapgemm_epilogue_lds, skinny_gemm_kernel):
                   WQKV   round16(acc + bias), stored as f32
                   RESID  round16(round16(acc + bias) + resid), resid f32, stored as f32 (wo, w2; in place or two buffers)
                   W13    round16(round16(silu(round16 gate)) * round16 up), weight rows (2i, 2i + 1) = (gate, up), stored as bf16
  norm_ref     rmsnorm_llama_rows_kernel: round16(round16(x inv) gain), inv = 1 / sqrt(mean x^2 + eps)
  append_ref   prefill_rope_append_kernel: q / k nn.RMSNorm (ONE rounding of (x inv) gain), RoPE with the bf16 table and a
               rounding; the finished queries, the appended K rows, the appended V rows (copies)
  attn_ref     flash_prefill_kernel: a causal softmax of every row over cache positions [0, pos0 + row] of its sequence's
               slot, one rounding of y.  It reads the queries and the K / V rows THE DEVICE RETURNED (the codec trace's rule
               of recorded inputs): a boundary flip of the append is judged once, by append_ref, and does not count again here.
  The position-by-position path (fewer than 16 rows, FT_PREFILL_ATTN_V0) is attn_decode_kernel, whose reference and bound are
  wide_ref.attn_ref with splits = 1 (`decode_ref` lays the prompt out for it).

Each returns `ref`, the float64 value BEFORE the last rounding, and `err`, a bound on |device value before the last rounding -
ref|; `check` (wide_ref.check and, for f32 stores, that the stored value IS a bf16 value) demands of EVERY element

    |got - ref| <= half a ulp of bf16 at max(|got|, |ref|) + err.

Error model (u = 2^-24; every f32 operation returns its exact result times (1 + d), |d| <= u):

  contraction.  bf16 x bf16 is exact in f32, so the only error is the order of the f32 sums: E = min(MARGIN r_stage, K 2^-23) S,
      S = sum |x| |w|, r_stage = the largest |f32 - f64| / S of the same sums in three f32 orders (codec_stage_ref.measure_r:
      one chain, per-32 blocks, pairwise), measured on THIS reference's operands only, never on device output.  MARGIN = 4 is
      the project's factor; no other constant is chosen by hand.
  epilogues.  As wide_ref.linear_ref, op by op: v = acc + bias: e = E + u |v|; every intermediate rounding through `reach`
      (nothing where [v - e, v + e] holds no rounding boundary of bf16, one step where it holds one); silu: e = 1.1 e_gate +
      (2^-20 + 3 u) |silu|; the product and the residual add: one u each.  No norm sits in front of these products, so a
      gate can be large: from gate <= -88 on expf(-gate) overflows float32 and the device's silu is 0 where the float64 one
      is some 1e-37: there the whole |silu| (or its rounded value, if larger) joins the silu's error, (|up| + e_up) |silu| that of
      the product.
  norm.  t = x inv: the device's t' is within (D / 512 + 10) u |t| of it (the RMSNorm term of codec_stage_ref.py), `reach`
      gives the rounded a = round16(t) and how far the device's may lie; a gain is exact in f32 (8 + 8 significand bits), so
      err = reach |gain| and the last rounding is the checker's half ulp.
  append.  wide_ref._norm_rope: (hd / 512 + 10) u |v| and `reach` for the norm, two products and a sum for the rotation.
  attention of row i over n = pos0 + i + 1 keys, key tiles of 32 walked by NG groups (a group sees every NG-th tile) with an
  online softmax each, merged at the end:
      a score is an hd-term f32 sum of exact products times the scale:
          ds_j = min(MARGIN r_sc, (hd + 2) u) scale sum |q| |k_j| + u |s_j|,          r_sc measured like r_stage on q, K;
      exp in f32: its argument s_j - m (m a running maximum of visible scores) is rounded once, u (max s - min s) =: u R, and
          expf returns its value to 2^-20 relative (LIB, the project's figure for expf);
      the online rescaling: each time a group's maximum rises what it gathered is multiplied by one more expf of a rounded
          difference of two visible scores: (2^-20 + u) relative and u R in the exponent, at most once per key tile the group
          walks and once more in the merge: RS = 2 ceil(n_max / (64 NG)) + 1, n_max the keys of the sequence's last row (the
          kernel walks its tiles in pairs);
      so the weight of key j carries an absolute exponent error D = max_j ds_j + (1 + RS) u R, a relative e^D - 1, and
          (1 + RS) (2^-20 + u) from the exponentials, in the numerator and in the denominator alike;
      the split of P into two bf16 planes hi = bf16(p), lo = bf16(p - hi): p - hi is exact in f32 and at most 2^-9 p, lo is
          within 2^-9 of it, so hi + lo leaves at most 2^-18 p per probability (numerator only: l sums the f32 p), and
          hi v, lo v are exact in f32;
      the P V sum in f32: min(MARGIN r_pv, (n + 2) u), r_pv measured on softmax, V; the row sum l: (n / 64 + 8) u as in
          wide_ref; the division and the merge products: 4 u + 2 RS u;
          err = (2 (e^D - 1 + (1 + RS) (2^-20 + u)) + 2^-18 + min(MARGIN r_pv, (n + 2) u) + (n / 64 + 12 + 2 RS) u) sum_j softmax_j |v_j|.
      Then the one rounding of y: the checker's half ulp.

`emulate_*` restate the same launches in float32 with the device's work split (K in 64-steps of two 32-wide MFMA blocks,
row tiles, 32-key tiles in NG groups with an online softmax and the merge, P as two planes) and bf16 stores: an honest
stand-in for the device from which tests/test_pf_ref_host.py builds outputs with and without injected faults.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from tests import wide_ref as WR
from tests.codec_stage_ref import F32, F64, LIB, MARGIN, U, h16_bits, measure_r
from tests.wide_ref import Ref, Verdict, reach, round16, values

FMT = "bf16"
WQKV, RESID, W13 = 0, 1, 2
_WIDE_EPI = {WQKV: WR.STORE, RESID: WR.RESID, W13: WR.SWIGLU}
# the kernel class ids ft_test_pf_linear reports (include/fishtts_hip_test.h)
ID_SKINNY1, ID_SKINNY2, ID_SKINNY4, ID_LIN128, ID_LIN64, ID_TAP64_128, ID_TAP64_64, ID_TAP_128, ID_TAP_64 = range(9)
ID_NAMES = ("skinny<1>", "skinny<2>", "skinny<4>", "lingemm<128,128>", "lingemm<64,64>", "tapgemm64<128,128>", "tapgemm64<64,64>",
            "tapgemm<128,128>", "tapgemm<128,64>")
SENT16, SENT32 = 0xFFFE, 0xFFFFFFFE
P_SPLIT = 2.0 ** -18
EXP_OVERFLOW = -88.0        # expf(-gate) passes FLT_MAX = e^88.72 (from e^88 on it is within a factor 2.1 of it)


def want_id(mode: int, S: int, N: int, K: int) -> int:
    """pf_gemm's choice (engine.hip), restated: mode is FT_PREFILL_GEMM (2 by default)."""
    if mode >= 2 and S <= 128 and K % 128 == 0 and N % 2 == 0:
        return ID_SKINNY1 if S <= 16 else ID_SKINNY2 if S <= 32 else ID_SKINNY4
    if mode >= 1 and K % 64 == 0 and N % 128 == 0:
        if K % 256 == 0:
            return ID_LIN128 if S >= 512 and N > 1024 else ID_LIN64
        return ID_TAP64_128 if S >= 512 else ID_TAP64_64
    return ID_TAP_128 if N >= 128 else ID_TAP_64


# ------------------------------------------------------------------------------------------------------ linear, norm
def linear_pre(X: torch.Tensor, W: torch.Tensor, seed: int = 0):
    """The contraction of one product, shared by its forms, bias choices and row counts: (acc [S, N] float64, E: the bound
    on the device's accumulator, r_stage, None) - the `pre` tuple of wide_ref.linear_ref."""
    X, W = X.to(F64), W.to(F64)
    K = X.shape[1]
    Wt = W.t().contiguous()
    r = measure_r(X, Wt, seed=seed + 31 * X.shape[0] + W.shape[0])
    return X @ Wt, min(MARGIN * r, K * 2.0 ** -23) * (X.abs() @ Wt.abs()), r, None


def linear_ref(form: int, pre, bias=None, resid=None, rows: Optional[int] = None) -> Ref:
    """One product of the prompt pass from its linear_pre: the epilogue and its error terms are wide_ref.linear_ref's, plus
    the float32 range of expf for W13 (see the module docstring: no norm sits in front of these products)."""
    ref = WR.linear_ref(FMT, _WIDE_EPI[form], bias=bias, resid=resid, pre=pre, rows=rows)
    if form == W13:
        v, e = pre[0], pre[1]
        if rows is not None:
            v, e = v[:rows], e[:rows]
        if bias is not None:
            v = v + bias.to(F64)[None, :]
            e = e + U * v.abs()
        gr, _ = reach(v[:, 0::2], e[:, 0::2], FMT)
        ur, eu = reach(v[:, 1::2], e[:, 1::2], FMT)
        s = gr / (1.0 + torch.exp(-gr))
        ref.err = ref.err + torch.where(gr <= EXP_OVERFLOW, (ur.abs() + eu) * torch.maximum(s.abs(), round16(s, FMT).abs()), torch.zeros_like(s))
    return ref


def norm_ref(x: torch.Tensor, gain: torch.Tensor, eps: float) -> Ref:
    x, g = x.to(F64), gain.to(F64)[None, :]
    t = x * WR.rms_inv(x, eps)
    a, ea = reach(t, (x.shape[1] / 512 + 10) * U * t.abs(), FMT)
    v = a * g
    return Ref(v, ea * g.abs(), round16(v, FMT))


def check(got, ref: torch.Tensor, err: torch.Tensor) -> Verdict:
    """wide_ref.check on every element; a float32 store of the prompt pass holds bf16 VALUES (round_lin / round_f32_out), so an
    element of a float32 `got` that is no bf16 value is flagged whatever its distance (a rounding left out lands closer to the
    reference than the rounded value does)."""
    ver = WR.check(got, ref, err, FMT)
    g = np.asarray(got)
    if g.dtype == np.float32:
        v = torch.from_numpy(np.ascontiguousarray(g)).reshape(ref.shape)
        off = (v.to(torch.bfloat16).to(F32) != v) & ~torch.isnan(v)
        if bool(off.any()):
            bad = ver.bad | off
            b2 = bad.reshape(bad.shape[0], -1)
            ver = Verdict(ver.checked, int(bad.sum()), float("inf"), torch.nonzero(b2.any(dim=1)).flatten().tolist(),
                          torch.nonzero(b2.any(dim=0)).flatten().tolist(), bad)
    return ver


# ------------------------------------------------------------------------------------------------------ attention
@dataclass
class Seq:
    row0: int
    rows: int
    pos0: int
    slot: int


def as_seqs(seqs) -> List[Seq]:
    return [s if isinstance(s, Seq) else Seq(*[int(v) for v in s]) for s in seqs]


@dataclass
class AppendRef:
    q: Ref                # [S, H hd] the finished queries
    k: Ref                # [S, Hkv hd] the appended K rows
    v: torch.Tensor       # [S, Hkv hd] the appended V rows (copies)


def append_ref(qkv, pos: Sequence[int], qn, kn, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6) -> AppendRef:
    """qkv [S, (H + 2 Hkv) hd] f32 rows, pos [S]: the cache position of each row, qn / kn [hd], tab [n_pos, hd / 2, 2]."""
    qkv, tab, qn, kn = qkv.to(F64), tab.to(F64), qn.to(F64), kn.to(F64)
    qs, qe, ks, ke = [], [], [], []
    for m, p in enumerate(pos):
        v, e, _, _ = WR._norm_rope(qkv[m, :H * hd].reshape(H, hd), qn, tab[int(p)], eps, FMT)
        qs.append(v.reshape(-1)); qe.append(e.reshape(-1))
        v, e, _, _ = WR._norm_rope(qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd), kn, tab[int(p)], eps, FMT)
        ks.append(v.reshape(-1)); ke.append(e.reshape(-1))
    q, k = torch.stack(qs), torch.stack(ks)
    return AppendRef(Ref(q, torch.stack(qe), round16(q, FMT)), Ref(k, torch.stack(ke), round16(k, FMT)), qkv[:, (H + Hkv) * hd:].clone())


def rescales(n_max: int, NG: int) -> int:
    return 2 * math.ceil(n_max / (64 * NG)) + 1


def attn_ref(q, kc, vc, seqs, NG: int, H: int, Hkv: int, hd: int, seed: int = 0) -> Ref:
    """q [S, H hd] (bf16 patterns or values: the finished queries the device returned), kc / vc [max_batch, Hkv, n_slots, hd]
    (bf16 patterns: the caches as the device left them), seqs: {first row, rows, first cache position, slot} per sequence,
    NG: the key groups of the tiled kernel that ran (it sets the rescale count of the error model only)."""
    seqs = as_seqs(seqs)
    q = values(q, FMT) if not isinstance(q, torch.Tensor) else q.to(F64)
    S, G = q.shape[0], H // Hkv
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    y, err = torch.zeros(S, H * hd, dtype=F64), torch.zeros(S, H * hd, dtype=F64)
    gen = torch.Generator().manual_seed(seed)
    r_max = 0.0
    for sq in seqs:
        n = sq.pos0 + sq.rows
        Q = q[sq.row0:sq.row0 + sq.rows].reshape(sq.rows, H, hd)
        K, V = values(kc[sq.slot, :, :n], FMT), values(vc[sq.slot, :, :n], FMT)              # [Hkv, n, hd]
        vis = torch.arange(n)[None, :] <= (sq.pos0 + torch.arange(sq.rows))[:, None]          # [rows, n]
        n_i = (sq.pos0 + torch.arange(sq.rows) + 1).to(F64)[:, None]
        RS = rescales(n, NG)
        def head(h):
            sc = (Q[:, h] @ K[h // G].t()) * scale
            return sc, torch.softmax(sc.masked_fill(~vis, float("-inf")), dim=-1)

        # the two sums' order error, measured like a contraction's on two heads of the sequence (head 0 and a seeded one)
        r_s = r_p = 0.0
        for h in {0, int(torch.randint(0, H, (1,), generator=gen))}:
            r_s = max(r_s, measure_r(Q[:, h], K[h // G].t().contiguous(), seed=seed + h))
            r_p = max(r_p, measure_r(head(h)[1], V[h // G].contiguous(), seed=seed + h + 1))
        r_max = max(r_max, r_s, r_p)
        for h in range(H):
            Kh, Vh = K[h // G], V[h // G]
            sc, pw = head(h)
            ds = min(MARGIN * r_s, (hd + 2) * U) * scale * (Q[:, h].abs() @ Kh.abs().t()) + U * sc.abs()
            ds = ds.masked_fill(~vis, 0.0)
            R = (sc.masked_fill(~vis, float("-inf")).max(dim=-1).values - sc.masked_fill(~vis, float("inf")).min(dim=-1).values)[:, None]
            D = ds.max(dim=-1, keepdim=True).values + (1 + RS) * U * R
            rel = 2 * (torch.expm1(D) + (1 + RS) * (LIB + U)) + P_SPLIT + torch.clamp(n_i + 2, max=MARGIN * r_p / U) * U \
                + (n_i / 64 + 12 + 2 * RS) * U
            y[sq.row0:sq.row0 + sq.rows, h * hd:(h + 1) * hd] = pw @ Vh
            err[sq.row0:sq.row0 + sq.rows, h * hd:(h + 1) * hd] = rel * (pw @ Vh.abs())
    return Ref(y, err, round16(y, FMT), r_max)


def decode_ref(qkv, kc, vc, sq: Seq, qn, kn, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6) -> WR.AttnRef:
    """The position-by-position path (attn_decode_kernel, one split): wide_ref.attn_ref with row i at position pos0 + i reading
    the rows below it from the slot's cache as the device left it."""
    n = sq.pos0 + sq.rows                                             # row i reads cache rows [0, pos0 + i) only
    view = lambda c: np.ascontiguousarray(np.broadcast_to(c[sq.slot][None, :, :n], (sq.rows, Hkv, n, hd)))
    pos = [sq.pos0 + i for i in range(sq.rows)]
    return WR.attn_ref(FMT, qkv[sq.row0:sq.row0 + sq.rows].to(F64), pos, qn, kn, view(kc), view(vc), tab, H, Hkv, hd, eps, splits=1)


@dataclass
class CacheVerdict:
    k: Verdict                    # the appended K rows against append_ref
    v_equal: bool                 # the appended V rows are the copies
    untouched: bool               # every other row of both caches is bit-unchanged (the hook's NaN fill included)


def nan_fill(kc: np.ndarray, vc: np.ndarray, seqs) -> Tuple[np.ndarray, np.ndarray]:
    """The hook's fill, restated: NaN patterns in every cache row at or behind a sequence's pos0 + rows and in every slot no
    sequence names.  Returns copies."""
    kc, vc = kc.copy(), vc.copy()
    end = np.zeros(kc.shape[0], dtype=np.int64)
    for sq in as_seqs(seqs):
        end[sq.slot] = sq.pos0 + sq.rows
    for m in range(kc.shape[0]):
        kc[m, :, end[m]:] = SENT16
        vc[m, :, end[m]:] = SENT16
    return kc, vc


def check_cache(kc0, vc0, kc1, vc1, seqs, app: AppendRef, Hkv: int, hd: int) -> CacheVerdict:
    """kc0 / vc0: the caches the caller passed in, kc1 / vc1: what came back."""
    seqs = as_seqs(seqs)
    wk, wv = nan_fill(kc0, vc0, seqs)
    S = app.k.ref.shape[0]
    k_new, v_new = np.zeros((S, Hkv, hd), dtype=np.uint16), np.zeros((S, Hkv, hd), dtype=np.uint16)
    for sq in seqs:
        sl = slice(sq.pos0, sq.pos0 + sq.rows)
        k_new[sq.row0:sq.row0 + sq.rows] = kc1[sq.slot, :, sl].transpose(1, 0, 2)
        v_new[sq.row0:sq.row0 + sq.rows] = vc1[sq.slot, :, sl].transpose(1, 0, 2)
        wk[sq.slot, :, sl] = kc1[sq.slot, :, sl]
        wv[sq.slot, :, sl] = vc1[sq.slot, :, sl]
    vk = WR.check(k_new.reshape(S, -1), app.k.ref, app.k.err, FMT)
    return CacheVerdict(vk, bool(np.array_equal(v_new.reshape(S, -1), h16_bits(app.v, FMT))),
                        bool(np.array_equal(wk, kc1) and np.array_equal(wv, vc1)))


# ------------------------------------------------------------------------------------------------------ emulation
def emulate_linear(form: int, X, W, bias=None, resid=None, BM: int = 64, bug: Optional[str] = None) -> torch.Tensor:
    """The launch in float32 as the device splits it: K in 64-steps, each two 32-wide MFMA blocks (an exactly summed,
    once-rounded partial per block, added to the accumulator in order), row tiles of BM.  Returns the stored values as float64
    (exact bf16 values; for the float32 forms what the f32 store holds).  bug: an emulated fault of tests/test_pf_ref_host.py."""
    X, W = X.to(F64), W.to(F64)
    S, K = X.shape
    steps = list(range(K // 64))
    if bug == "drop_kstep":
        steps.remove(len(steps) // 2)
    if bug == "last_kstep_twice":
        steps.append(steps[-1])
    acc = torch.zeros(S, W.shape[0], dtype=F32)
    for st in steps:
        for b in range(2):
            k0 = st * 64 + b * 32
            acc += (X[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()).to(F32)
    if bug == "last_tile_stale" and S % BM and S > BM:                 # the last partial row tile holds the tile before it
        m0 = S // BM * BM
        acc[m0:] = acc[m0 - BM:m0 - BM + (S - m0)]
    v = acc
    if bias is not None and bug != "drop_bias":
        v = v + bias.to(F32)[None, :]
    v = round16(v, FMT)
    if form == W13:
        gate, up = (v[:, 1::2], v[:, 0::2]) if bug == "swap_gate_up" else (v[:, 0::2], v[:, 1::2])
        v = round16(round16(gate / (1.0 + torch.exp(-gate)), FMT) * up, FMT)
    elif form == RESID:
        r32 = resid.to(F32)
        v = round16(v, FMT) + r32 if bug == "resid_after_round" else round16(v + r32, FMT)
    return v.to(F64)


def emulate_norm(x, gain, eps: float) -> torch.Tensor:
    x32 = x.to(F32)
    ss = (x32 * x32).sum(dim=-1, keepdim=True)
    inv = 1.0 / torch.sqrt(ss / x32.shape[1] + torch.tensor(eps, dtype=F32))
    return round16(round16(x32 * inv, FMT) * gain.to(F32)[None, :], FMT).to(F64)


def emulate_append(qkv, kc: np.ndarray, vc: np.ndarray, seqs, qn, kn, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6,
                   bug: Optional[str] = None):
    """prefill_rope_append_kernel in float32 on the hook's NaN-filled caches.  Returns (q [S, H hd] float64 of bf16 values,
    kc, vc as bf16 patterns)."""
    seqs = as_seqs(seqs)
    kc, vc = nan_fill(kc, vc, seqs)
    tab = tab.to(F32)

    def nr(x, gain, t):
        inv = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / hd + torch.tensor(eps, dtype=F32))
        x = round16((x * inv) * gain.to(F32)[None, :], FMT)
        x0, x1, c, s = x[:, 0::2], x[:, 1::2], t[None, :, 0], t[None, :, 1]
        return round16(torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1).reshape(x.shape), FMT)

    q = torch.zeros(qkv.shape[0], H * hd, dtype=F32)
    for sq in seqs:
        for i in range(sq.rows):
            m, p = sq.row0 + i, sq.pos0 + i
            row = qkv[m].to(F32)
            q[m] = nr(row[:H * hd].reshape(H, hd), qn, tab[p]).reshape(-1)
            at = p + 1 if bug == "append_pos_plus_1" else p
            kc[sq.slot, :, at] = h16_bits(nr(row[H * hd:(H + Hkv) * hd].reshape(Hkv, hd), kn, tab[p]), FMT)
            vc[sq.slot, :, at] = h16_bits(row[(H + Hkv) * hd:].reshape(Hkv, hd), FMT)
    return q.to(F64), kc, vc


def emulate_attn(q, kc, vc, seqs, NG: int, H: int, Hkv: int, hd: int, bug: Optional[str] = None) -> torch.Tensor:
    """flash_prefill_kernel in float32: blocks of QROWS = 128 / NG query rows of one head; a step takes NG tiles of 32 keys, group
    g the g-th, steps in pairs up to the block's last visible key (keys past it re-read that key's row and are masked); an
    online softmax per group with P entering the second product as hi + lo bf16 planes; the groups merged at the end.
    Returns y [S, H hd] as float64 of bf16 values."""
    seqs = as_seqs(seqs)
    q = (values(q, FMT) if not isinstance(q, torch.Tensor) else q).to(F32)
    S, G, QR = q.shape[0], H // Hkv, 128 // NG
    scale = torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(hd), dtype=F32))
    ninf = float("-inf")
    y = torch.zeros(S, H * hd, dtype=F32)
    n_mb = kc.shape[0]
    for sq in seqs:
        slot = (sq.slot + 1) % n_mb if bug == "neighbour_slot" and len(seqs) > 1 else sq.slot
        for q0 in range(0, sq.rows, QR):
            nr = min(QR, sq.rows - q0)
            kmax = sq.pos0 + q0 + nr - 1
            Q = q[sq.row0 + q0:sq.row0 + q0 + nr].reshape(nr, H, hd).transpose(0, 1)                  # [H, nr, hd]
            qabs = (sq.pos0 + q0 + torch.arange(nr))[None, :, None]                                   # [1, nr, 1]
            if bug == "mask_without_pos0":
                qabs = qabs - sq.pos0
            m = torch.full((NG, H, nr), ninf, dtype=F32)
            l = torch.zeros(NG, H, nr, dtype=F32)
            O = torch.zeros(NG, H, nr, hd, dtype=F32)
            n_steps = 2 * ((kmax // (NG * 32)) // 2 + 1)
            for step in range(n_steps):
                for g in range(NG):
                    kt = (step * NG + g) * 32
                    j = torch.clamp(kt + torch.arange(32), max=kmax)
                    Kt = values(kc[slot][:, j], FMT).to(F32).repeat_interleave(G, dim=0)              # [H, 32, hd]
                    Vt = values(vc[slot][:, j], FMT).to(F32).repeat_interleave(G, dim=0)
                    s = torch.einsum("hqd,hkd->hqk", Q, Kt) * scale
                    key = (kt + torch.arange(32))[None, None, :]
                    hide = key >= qabs if bug == "mask_off_by_one" else key > qabs
                    if bug == "miss_key_128":
                        hide = hide | (key == sq.pos0 + 128)
                    s = s.masked_fill(hide, ninf)
                    mn = torch.maximum(m[g], s.max(dim=-1).values)
                    live = mn > ninf
                    safe = torch.where(live, mn, torch.zeros_like(mn))
                    corr = torch.where(live, torch.exp(m[g] - safe), torch.ones_like(mn))
                    p = torch.where(live[..., None], torch.exp(s - safe[..., None]), torch.zeros_like(s))
                    l[g] = l[g] * corr + p.sum(dim=-1)
                    hi = round16(p, FMT)
                    lo = round16(p - hi, FMT)
                    pv = torch.einsum("hqk,hkd->hqd", hi, Vt)
                    if bug != "drop_lo":
                        pv = pv + torch.einsum("hqk,hkd->hqd", lo, Vt)
                    O[g] = O[g] * corr[..., None] + pv
                    m[g] = mn
            groups = list(range(NG))
            if bug == "drop_group":
                groups.remove(NG - 1)
            mm = torch.stack([m[g] for g in groups]).max(dim=0).values
            lt, Ot = torch.zeros(H, nr, dtype=F32), torch.zeros(H, nr, hd, dtype=F32)
            for g in groups:
                c = torch.where(m[g] > ninf, torch.exp(m[g] - mm), torch.zeros_like(mm))
                lt = lt + l[g] * c
                Ot = Ot + O[g] * c[..., None]
            y[sq.row0 + q0:sq.row0 + q0 + nr] = round16(Ot / lt[..., None], FMT).transpose(0, 1).reshape(nr, H * hd)
    return y.to(F64)


# ------------------------------------------------------------------------------------------------------ test inputs
def seeded_linear_inputs(S: int, N: int, K: int, seed: int, w_std: float = 0.03, loud_row: int = 3):
    """X ~ N(0, 1) with one row scaled by 64, W ~ N(0, w_std), bias = 0.1 N (f32), resid ~ N(0, 1): all but the bias rounded to
    bf16 (the residual stream of the prompt pass holds bf16 values in f32).  All rows distinct."""
    X, W, _, bias, _ = WR.seeded_linear_inputs(FMT, S, N, K, seed, w_std, loud_row)
    resid = round16(torch.randn(S, N, generator=torch.Generator().manual_seed(seed + 1)), FMT)
    return X, W, bias, resid


def seeded_attn_inputs(S: int, H: int, Hkv: int, hd: int, n_slots: int, max_batch: int, seed: int, rope_base: float = 1e6):
    """qkv [S, (H + 2 Hkv) hd] bf16 values (one loud row), qn / kn, finite random caches [max_batch, Hkv, n_slots, hd] as bf16
    patterns (a stale read then shows as a wrong number, the hook's NaN fill as a NaN) and the bf16 rope table."""
    from oracle import ar as O
    g = torch.Generator().manual_seed(seed)
    r = lambda t: round16(t.to(F32), FMT)
    qkv = r(torch.randn(S, (H + 2 * Hkv) * hd, generator=g))
    if S > 3:
        qkv[3] = r(qkv[3] * 64.0)
    qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.0 + 0.1 * torch.randn(hd, generator=g))
    kc = h16_bits(torch.randn(max_batch, Hkv, n_slots, hd, generator=g), FMT)
    vc = h16_bits(torch.randn(max_batch, Hkv, n_slots, hd, generator=g), FMT)
    return qkv, qn, kn, kc, vc, O.rope_table(n_slots, hd, rope_base).to(F32)
