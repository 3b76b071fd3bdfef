"""Float64 reference of the decode launches of csrc/ar_kernels.h (1..max_batch rows), ONE LAUNCH AT A TIME (host only; test
infrastructure, the sibling of tests/codec_stage_ref.py, tests/wide_ref.py and tests/pf_ref.py, whose number-format helpers,
`reach`, `rms_inv`, `_norm_rope`, `attn_ref`, three-order `r_stage` measurement and MARGIN it reuses):

  gemv_ref        gemv_kernel / gemv_mb_kernel: optional RMSNorm rb(rb(x inv) g) fused in front of a W x contraction with f32
                  accumulation, then   store rb(acc + bias) | residual rb(resid + rb(acc + bias)) |
                  SwiGLU rb(rb(rb(a) / (1 + exp(-rb(a)))) rb(b)) on interleaved (gate, up) weight rows.
  decode_attn_ref attn_decode_kernel: q / k nn.RMSNorm (one rounding), RoPE, the K / V append at pos, and per KV split
                  s the triple (O_s, m_s, l_s) of the softmax over its own range [lo, hi), chunk = (pos + nsplit) / nsplit;
                  one split: the finished y (wide_ref.attn_ref).  merge_ref: gemv_attn_combine_kernel's y from RECORDED
                  partials, so a wrong partial is charged to the attention and a wrong merge to the Wo launch.
  fast_attn_ref   fast_attn_kernel, the explicit path: rb(rb(d) scale), exact maximum, expf, sequential f32 sum,
                  rb(p / sum), an fma chain over j <= c, rb(o).
  embed_ref       embed_kernel: rb(sum of the ncb codebook rows in order), rb(emb + vq), rb(x / (float)sqrt(ncb + 1)).

Formats: "bf16", "fp16" and "f32".  "f32" is the engine's RND_NONE: rb is the identity, so NO intermediate rounding exists
(`rch` passes value and error through) and the store is a float32: half a float32 ulp.  Each reference returns `ref` (float64,
before the last rounding), `err` (a bound on |device value before its last rounding - ref|) and `rnd`; `check` demands of
EVERY element  |got - ref| <= half a ulp of the stored format at max(|got|, |ref|) + err,  and of a 16-bit model's float32
store that it holds a value of the model's type (pf_ref's rule: a rounding left out lands CLOSER to the reference).

Error model (u = 2^-24; every f32 operation returns its exact result times (1 + d), |d| <= u; an fma rounds once):

  contraction.  A lane owns NT pieces of VEC = 16 bytes / element consecutive k: a chain of n_c = NT VEC fma, then the 64
      lanes are summed in 6 steps (row16_sum: 4, then 3 more additions counted as 2 levels): every term passes at most
      n_c + 6 roundings, so the worst case is (n_c + 7) u S, S = sum |w| |x|.  The bound used is the issue's
      E = min(MARGIN r_stage, (n_c + 7) u) S  (MARGIN = 4) with r_stage = the largest |f32 - f64| / S of the reference's own
      sums in three f32 orders (codec_stage_ref.measure_r).  A decode launch may have one row and one weight row: too
      few sums to measure on.  The sample is therefore the reference's own activation rows AND their rotations along k (the
      same operands paired with other weights: 64 rows in all; the first 64 rows of a larger launch), never device output.
  fused RMSNorm.  ss = sum x^2 goes through the same lane chain and wave sum: non-negative terms, relative error
      (n_c + 6) u; / K and + eps add one u each, the square root halves the sum and adds one, the reciprocal one, x inv one:
      t' = x inv is within d = (n_c / 2 + 8) u |t| of the float64 t (7 from the count, 1 for the second order).  16-bit
      models round twice, rb(rb(t) g): wherever [t - d, t + d] holds a rounding boundary BOTH neighbours a' are computed,
      a' g is exact in f32, and dx = max |rb(a' g) - xn| joins the bound as sum_k |w_k| dx_k (wide_ref's rule with this
      kernel's d).  f32 models: xn = t g carries d |g| + u |t g|.
  epilogue, op by op: v = acc + bias: + u |v|, then `rch` (the rounding: nothing where [v - e, v + e] holds no boundary, one
      step where it does).  Residual: rb(resid + rb(v)): + u |sum|.  SwiGLU: silu (Lipschitz <= 1.1, expf to 2^-20):
      e = 1.1 e_gate + (2^-20 + 3 u) |silu|, `rch`; the product: |up| e_s + |silu| e_up + e_s e_up + u |o|; from gate <= -88
      on expf(-gate) overflows float32 and the device's silu is 0: the whole |silu| joins its error (pf_ref's rule).
  decode attention.  q, k: wide_ref._norm_rope (kn / qn absent: identity); the appended K row is judged against it, V is a
      copy.  A score is judged directly here (m is recorded), and a row of one position gives two sums to measure an order
      error on, so the score's term is the worst case of its own chain instead of a measured r: a lane's 8 fma, log2(hd / 8)
      levels of the lane-group sum and the product with the scale, (10 + log2(hd / 8)) u scale sum |q| |k| (one u for the
      second order).  Weights and the P V sum carry wide_ref.attn_ref's terms over the split's own keys (r_pv measured on
      G x hd sums), with RS = the rises of the online softmax inside the range + 1 for the in-block merge of the lane groups;
      O / l is compared (O and l are float32 stores: 2 u more) and m against the largest score within its ds.  An empty
      range must be exactly (0, -inf, 0).
  merge of recorded partials: w_s = expf(m_s - M) (2^-20 + u |m_s - M|), sums of nsplit terms in chunks of 8 with one
      rescale of the running sums per later chunk (another expf and product, C = chunks - 1 of them).  Numerator and
      denominator each carry the weight's error and their sum's:  rel = 2 (2^-20 (1 + C) + u max |m_s - M|) + (nsplit + 2 C + 4) u,
      times sum_s |O_s| w_s / L.  y is rounded through `rch`, its reach joins the Wo product as dx.
  fast attention.  d = fma(q1, k1, q0 k0) per lane and a 6-step wave sum: 8 u sum |q| |k|.  rb(d), times scale (+ u), rb.
      The maximum is exact.  The exponent s_j - mx carries e_j + e_max + u |s_j - mx| = D_j absolutely: weight relative
      e^D_j - 1 + 2^-20; the sequential sum adds (c + 1) u and takes the largest weight error; p / sum adds u; `rch`.  The
      fma chain over j <= c: sum_j e_pj |v_j| + (c + 1) u sum_j |p_j v_j|.
  embedding.  The ncb rows are summed in codebook order in f32: (ncb - 1) u sum |e|; `rch`; emb + vq: u; `rch`; the divide by
      (float)sqrt(ncb + 1) - the float32 divisor is restated exactly - u; the stored value.  A text token is a copy: err 0.

`emulate_*` restate the launches in float32 with the device's work split (lanes of NT x VEC fma, a butterfly wave sum, MB
rows per tile over ceil(M / MB) groups - a tail group's dead rows load row M - 1 and store nothing -, nsplit ranges with the
in-block slot merge, the 8-split chunks of merge_splits4 on row m's own partials): an honest stand-in from which
tests/test_ar_ref_host.py builds outputs with and without injected faults.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from tests import wide_ref as WR
from tests.codec_stage_ref import F32, F64, LIB, MARGIN, U, f32_orders, from_raw, h16_bits, half_ulp, measure_r
from tests.wide_ref import Ref, Verdict, reach, rms_inv, round16

PRO_NONE, PRO_RMSNORM = 0, 1
EPI_STORE, EPI_RESID, EPI_SWIGLU = 0, 1, 2                   # ar_kernels.h
FMTS = ("bf16", "fp16", "f32")
SENT16, SENT32 = 0xFFFE, 0xFFFFFFFE
EXP_OVERFLOW = -88.0
NT_OPTS = (1, 2, 3, 4, 6, 8, 12)


# ------------------------------------------------------------------------------------------------------ formats
def vec(fmt: str) -> int:
    return 4 if fmt == "f32" else 8


def pick_nt(K: int, fmt: str) -> int:
    need = (K + 64 * vec(fmt) - 1) // (64 * vec(fmt))
    return next((o for o in NT_OPTS if o >= need), -1)


def rows_per_wave(N: int, M: int) -> int:
    return 4 if N * M >= 65536 else 2 if N * M >= 2048 else 1


def want_id(fmt: str, epi: int, M: int, N: int, K: int):
    """gemv's choice (engine.hip), restated: (MB, R, NT)."""
    nt, R = pick_nt(K, fmt), rows_per_wave(N, M)
    if epi == EPI_SWIGLU and R < 2:
        R = 2
    if fmt != "f32" and M >= 2 and nt in (1, 2, 4, 6):
        four = M >= 3 and nt <= 2 and R <= 2
        if R >= 4:
            return (2 if nt <= 2 else 0, 4, nt)
        return (4 if four else 2, R, nt)
    return (0, R, nt)


def rnd(v: torch.Tensor, fmt: str) -> torch.Tensor:
    """rb<ROUND>: round to the model's type; the identity in an f32 model."""
    return v if fmt == "f32" else round16(v, fmt)


def rch(v: torch.Tensor, e: torch.Tensor, fmt: str):
    """An intermediate rb: (rounded value, how far the device's rounded value may lie from it)."""
    return (v, e) if fmt == "f32" else reach(v, e, fmt)


def store(v: torch.Tensor, fmt: str) -> torch.Tensor:
    """The value a store holds: the model's type, or a float32."""
    return v.to(F32).to(v.dtype) if fmt == "f32" else round16(v, fmt)


def wvalues(a, fmt: str) -> torch.Tensor:
    """Patterns as they travel to a hook (uint16 of a 16-bit type, float32) or a tensor -> float64 values."""
    return a.to(F64) if isinstance(a, torch.Tensor) else from_raw(np.asarray(a), fmt).to(F64)


def wbits(t: torch.Tensor, fmt: str) -> np.ndarray:
    """Exact values -> what a hook takes: uint16 patterns of a 16-bit type, float32 in an f32 model."""
    return t.to(F32).contiguous().numpy() if fmt == "f32" else h16_bits(t, fmt)


def check(got, ref: torch.Tensor, err: torch.Tensor, fmt: str) -> Verdict:
    """Every element of got against ref; none is left out.  NaN and (f32) infinity always flag."""
    if fmt != "f32":
        ver = WR.check(got, ref, err, fmt)
        g = np.asarray(got) if not isinstance(got, torch.Tensor) else got.numpy()
        if g.dtype == np.float32:                                       # a float32 store of a 16-bit model holds 16-bit VALUES
            v = torch.from_numpy(np.ascontiguousarray(g)).reshape(ref.shape)
            off = (v.to(WR.FMT_DT[fmt]).to(F32) != v) & ~torch.isnan(v)
            if bool(off.any()):
                bad = ver.bad | off
                b2 = bad.reshape(bad.shape[0], -1)
                ver = Verdict(ver.checked, int(bad.sum()), float("inf"), torch.nonzero(b2.any(dim=1)).flatten().tolist(),
                              torch.nonzero(b2.any(dim=0)).flatten().tolist(), bad)
        return ver
    g = wvalues(got, fmt).reshape(ref.shape)
    bound = half_ulp(torch.maximum(g.abs(), ref.abs()).clamp_max(3e38), True) + err
    diff = (g - ref).abs()
    bad = ~(diff <= bound) | ~torch.isfinite(g)
    ratio = torch.where(torch.isfinite(g), diff / bound, torch.full_like(diff, float("inf"))).nan_to_num(nan=float("inf"))
    b2 = bad.reshape(bad.shape[0], -1)
    return Verdict(int(diff.numel()), int(bad.sum()), float(ratio.max()), torch.nonzero(b2.any(dim=1)).flatten().tolist(),
                   torch.nonzero(b2.any(dim=0)).flatten().tolist(), bad)


# ------------------------------------------------------------------------------------------------------ products
def _sample_rows(xn: torch.Tensor) -> torch.Tensor:
    """The activation rows and their rotations along k, 64 rows in all: the sums r_stage is measured on."""
    M, K = xn.shape
    rows = [xn]
    s = 1
    while sum(r.shape[0] for r in rows) < 64:
        rows.append(torch.roll(xn, shifts=(s * 37) % K, dims=1))
        s += 1
    return torch.cat(rows)[:64]


def gemv_pre(fmt: str, pro: int, x, W, gain=None, eps: float = 1e-6, seed: int = 0, dx_in=None):
    """The fused norm and the contraction, shared by the epilogues, bias choices and row counts of a case:
    (acc [M, N] float64, E: the bound on the device's accumulator, r_stage, amb).  dx_in: an uncertainty the activations
    arrive with (the reach of a rounded merge result)."""
    x, W = x.to(F64), W.to(F64)
    M, K = x.shape
    nc = pick_nt(K, fmt) * vec(fmt)
    amb = None
    if pro == PRO_RMSNORM:
        g = gain.to(F64)[None, :]
        t = x * rms_inv(x, eps)
        d = (nc / 2 + 8) * U * t.abs()
        if fmt == "f32":
            xn = t * g
            dx = d * g.abs() + U * xn.abs()
        else:
            a, alo, ahi = round16(t, fmt), round16(t - d, fmt), round16(t + d, fmt)
            xn = round16(a * g, fmt)
            dx = torch.maximum((round16(alo * g, fmt) - xn).abs(), (round16(ahi * g, fmt) - xn).abs())
            amb = (alo != ahi).sum(dim=-1)
    else:
        xn, dx = x, torch.zeros_like(x)
    if dx_in is not None:
        dx = dx + dx_in
    Wt = W.t().contiguous()
    Wa = Wt.abs()
    r = measure_r(_sample_rows(xn), Wt, seed=seed + 31 * M + W.shape[0])
    E = min(MARGIN * r, (nc + 7) * U) * ((xn.abs() + dx) @ Wa) + dx @ Wa
    return xn @ Wt, E, r, amb


def gemv_ref(fmt: str, pro: int, epi: int, x=None, W=None, gain=None, bias=None, resid=None, eps: float = 1e-6, seed: int = 0,
             pre=None, rows: Optional[int] = None, dx_in=None) -> Ref:
    """One product.  x [M, K] (exact f32 values), W [N, K], gain [K], bias [N], resid [M, N]."""
    v, err, r, amb = pre if pre is not None else gemv_pre(fmt, pro, x, W, gain, eps, seed, dx_in)
    if rows is not None:
        v, err, amb = v[:rows], err[:rows], None if amb is None else amb[:rows]
    if bias is not None:
        v = v + bias.to(F64)[None, :]
        err = err + U * v.abs()
    if epi == EPI_SWIGLU:
        gr, eg = rch(v[:, 0::2], err[:, 0::2], fmt)
        ur, eu = rch(v[:, 1::2], err[:, 1::2], fmt)
        s = gr / (1.0 + torch.exp(-gr))
        e_s = 1.1 * eg + (LIB + 3 * U) * s.abs()
        e_s = e_s + torch.where(gr <= EXP_OVERFLOW, torch.maximum(s.abs(), rnd(s, fmt).abs()), torch.zeros_like(s))
        sr, es = rch(s, e_s, fmt)
        v = sr * ur
        err = ur.abs() * es + sr.abs() * eu + es * eu + U * v.abs()
    elif epi == EPI_RESID:
        vr, ev = rch(v, err, fmt)
        v = vr + resid.to(F64)[:v.shape[0]]
        err = ev + U * v.abs()
    return Ref(v, err, store(v, fmt), r, amb)


def seeded_gemv_inputs(fmt: str, M: int, N: int, K: int, seed: int, w_std: float = 0.03):
    """x ~ N(0, 1) with row 1 scaled by 64 (a mixed-up row or row statistic then shows), W ~ N(0, w_std), gain = 1 + 0.1 N,
    bias = 0.1 N, resid ~ N(0, 1); x and resid exact in the model's type (what a decode launch reads), all rows distinct."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    if M > 1:
        x[1] *= 64.0
    W = w_std * torch.randn(N, K, generator=g)
    gain = 1.0 + 0.1 * torch.randn(K, generator=g)
    bias = 0.1 * torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    r = lambda t: store(t.to(F64), fmt).to(F32)
    return r(x), r(W), r(gain), r(bias), r(resid)


# --- emulation
def _r32(v: torch.Tensor, fmt: str) -> torch.Tensor:
    return v if fmt == "f32" else v.to(WR.FMT_DT[fmt]).to(F32)


def _fma(a, b, c):
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _wave_sum(v: torch.Tensor) -> torch.Tensor:
    """[..., 64] f32 -> [...]: a butterfly inside each row of 16 lanes, then ((r0 + r1) + r2) + r3."""
    v = v.reshape(*v.shape[:-1], 4, 16)
    idx = torch.arange(16)
    for s in (1, 2, 4, 8):
        v = v + v[..., idx ^ s]
    r = v[..., 0]
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def _lanes(a: torch.Tensor, NT: int, VEC: int) -> torch.Tensor:
    """[..., K] -> [..., 64, NT VEC]: lane l's chain, k = t 64 VEC + l VEC + j in (t, j) order; zeros past K."""
    K = a.shape[-1]
    p = torch.zeros(*a.shape[:-1], NT * 64 * VEC, dtype=a.dtype)
    p[..., :K] = a
    return p.reshape(*a.shape[:-1], NT, 64, VEC).transpose(-3, -2).reshape(*a.shape[:-1], 64, NT * VEC)


def _chain_dot(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """sum over the last axis as the device does: an fma chain per lane, then the wave sum.  A, B [..., 64, n]."""
    acc = torch.zeros(torch.broadcast_shapes(A.shape, B.shape)[:-1], dtype=F32)
    for i in range(A.shape[-1]):
        acc = _fma(A[..., i], B[..., i], acc)
    return _wave_sum(acc)


def tile_rows(M: int, MB: int, bug: Optional[str] = None):
    """gemv_mb_kernel's work split: grid.y = ceil(M / MB) groups of MB rows.  -> (src, dst): slot i of the padded launch loads
    activation row src[i] (m = min(m0 + mb, M - 1)) and stores output row dst[i], or nothing (-1: m0 + mb >= M).  MB = 0
    (gemv_kernel, grid.y = M): row m is its own block.  bug: the emulated faults of the split."""
    if MB == 0:
        return list(range(M)), list(range(M))
    src, dst = [], []
    for g in range((M + MB - 1) // MB):
        m0 = g * MB
        tail = m0 + MB > M
        for mb in range(MB):
            m = m0 + mb
            live = m < M
            s = min(m, M - 1)
            if bug == "tail_from_last" and tail:                          # a tail group's live rows computed from row M - 1's activation
                s = M - 1
            if bug == "group_prev" and g > 0:                             # group g reads group g - 1's rows
                s = min(m, M - 1) - MB
            src.append(s)
            dst.append(m if live or bug == "tail_store" else -1)          # the dead rows of a tail group stored
    return src, dst


def emulate_gemv(fmt: str, pro: int, epi: int, x, W, gain=None, bias=None, resid=None, eps: float = 1e-6, bug: Optional[str] = None,
                 bug_row: int = 2, tail: bool = False) -> torch.Tensor:
    """The launch in float32 with the device's work split.  Returns the stored values (float64) [M, columns]; tail: [M + 1,
    columns], the row behind row M - 1 included (NaN unless a fault stores it).  bug: an emulated fault of
    tests/test_ar_ref_host.py."""
    x32, W32 = x.to(F32).clone(), W.to(F32).clone()
    M, K = x32.shape
    N = W32.shape[0]
    NT, VEC = pick_nt(K, fmt), vec(fmt)
    MB, R, _ = want_id(fmt, epi, M, N, K)
    if bug == "mb_row":                                                   # row bug_row of an MB = 4 tile reads row M - 1's activation
        assert MB == 4 and M == 4
        x32[bug_row] = x32[M - 1]
    if bug in ("tail_store", "tail_from_last", "group_prev"):
        assert MB > 0, "a fault of gemv_mb_kernel's work split"
    src, dst = tile_rows(M, MB, bug if bug in ("tail_store", "tail_from_last", "group_prev") else None)
    x32 = x32[src]                                                        # the padded launch: one slot per (group, mb)
    if resid is not None:                                                 # the residual is read at the OUTPUT row (0 behind row M - 1: the hook's fill is a NaN pattern)
        r_all = torch.cat([resid.to(F32), torch.zeros(max(dst) + 1 - M if max(dst) >= M else 0, resid.shape[1])])
        resid = r_all[[d if d >= 0 else 0 for d in dst]]
    xl = _lanes(x32, NT, VEC)                                             # [M, 64, n]
    if pro == PRO_RMSNORM:
        ss = _chain_dot(xl, xl)[:, None]
        if bug == "norm_other_row":
            ss = torch.roll(ss, -1, dims=0)
        inv = 1.0 / torch.sqrt(ss / float(K) + torch.tensor(eps, dtype=F32))
        g32 = gain.to(F32)[None, :]
        xn = _r32((x32 * inv) * g32, fmt) if bug == "single_round" else _r32(_r32(x32 * inv, fmt) * g32, fmt)
        xl = _lanes(xn, NT, VEC)
    wl = _lanes(W32, NT, VEC)                                             # [N, 64, n]
    if bug in ("drop_piece", "twice_piece"):                              # the last 16-byte piece of K: lane, chain slots of k in [K - VEC, K)
        k0 = K - VEC
        t, l = k0 // (64 * VEC), (k0 % (64 * VEC)) // VEC
        wl[:, l, t * VEC:(t + 1) * VEC] *= 0.0 if bug == "drop_piece" else 2.0
    acc = _chain_dot(wl[None], xl[:, None])                               # [M, N]
    if bug == "last_wg":                                                  # the last (partial) workgroup of 4 R rows repeats the one before
        n0 = (N - 1) // (4 * R) * (4 * R)
        acc[:, n0:] = acc[:, n0 - 4 * R:n0 - 4 * R + (N - n0)]
    v = acc
    if bias is not None and bug != "drop_bias":
        v = v + bias.to(F32)[None, :]
    if epi == EPI_SWIGLU:
        v = _r32(v, fmt)
        gate, up = (v[:, 1::2], v[:, 0::2]) if bug == "swap_gate_up" else (v[:, 0::2], v[:, 1::2])
        v = _r32(_r32(gate / (1.0 + torch.exp(-gate)), fmt) * up, fmt)
    elif epi == EPI_RESID:
        r32 = resid.to(F32)
        out = _r32(r32 + v, fmt) if bug == "resid_before_round" else _r32(r32 + _r32(v, fmt), fmt)
        if bug == "resid_after_store":                                    # aliased: the last lanes' rows read their residual after the store
            out[:, -3:] = _r32(out[:, -3:] + _r32(v[:, -3:], fmt), fmt)
        v = out
    else:
        v = _r32(v, fmt)
    out = torch.full((M + 1, v.shape[1]), float("nan"), dtype=F64)
    for i, d in enumerate(dst):                                           # the stores, in launch order
        if 0 <= d <= M:
            out[d] = v[i].to(F64)
    return out if tail else out[:M]


# ------------------------------------------------------------------------------------------------------ decode attention
def norm_rope(x: torch.Tensor, gain, tab: torch.Tensor, eps: float, fmt: str):
    """x [heads, hd] -> (value before the rotation's rounding, its bound, the rounded value, its reach): wide_ref._norm_rope,
    and its f32 form (no rounding: the norm's (hd / 512 + 10) u and the gain product's u travel through the rotation)."""
    if fmt != "f32":
        return WR._norm_rope(x, gain, tab, eps, fmt)
    hd = x.shape[-1]
    if gain is not None:
        xr = (x * rms_inv(x, eps)) * gain[None, :]
        e = (hd / 512 + 11) * U * xr.abs()
    else:
        xr, e = x, torch.zeros_like(x)
    x0, x1, e0, e1 = xr[:, 0::2], xr[:, 1::2], e[:, 0::2], e[:, 1::2]
    c, s = tab[None, :, 0], tab[None, :, 1]
    re, im = x0 * c - x1 * s, x1 * c + x0 * s
    ere = c.abs() * e0 + s.abs() * e1 + 2 * U * ((x0 * c).abs() + (x1 * s).abs())
    eim = c.abs() * e1 + s.abs() * e0 + 2 * U * ((x1 * c).abs() + (x0 * s).abs())
    v = torch.stack([re, im], dim=-1).reshape(x.shape)
    ev = torch.stack([ere, eim], dim=-1).reshape(x.shape)
    return v, ev, v, ev


def split_ranges(pos: int, nsplit: int):
    chunk = (pos + nsplit) // nsplit
    return [(s * chunk, min(s * chunk + chunk, pos + 1)) for s in range(nsplit)]


@dataclass
class PartRef:
    on: torch.Tensor        # [M, H, nsplit] bool: the range is not empty
    y: torch.Tensor         # [M, H, nsplit, hd]: O / l of the range (0 where empty)
    y_err: torch.Tensor
    m: torch.Tensor         # [M, H, nsplit]: the largest score of the range
    m_err: torch.Tensor
    k: Ref                  # the appended K rows [M, Hkv, hd]
    v: torch.Tensor         # the appended V rows
    r_stage: float


def decode_attn_ref(fmt: str, qkv, pos, qn, kn, kc, vc, tab, H: int, Hkv: int, hd: int, nsplit: int, eps: float = 1e-6,
                    seed: int = 0) -> PartRef:
    """pos: the APPENDED row of each utterance (device position + pos_off).  kc / vc [M, Hkv, n_slots, hd]: rows < pos read."""
    qkv, tab = qkv.to(F64), tab.to(F64)
    qn = None if qn is None else qn.to(F64)
    kn = None if kn is None else kn.to(F64)
    M, G = qkv.shape[0], H // Hkv
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    gen = torch.Generator().manual_seed(seed)
    on = torch.zeros(M, H, nsplit, dtype=torch.bool)
    Y, YE = torch.zeros(M, H, nsplit, hd, dtype=F64), torch.zeros(M, H, nsplit, hd, dtype=F64)
    Mx, ME = torch.full((M, H, nsplit), float("-inf"), dtype=F64), torch.zeros(M, H, nsplit, dtype=F64)
    ks, kes, vs, r_max = [], [], [], 0.0
    for m in range(M):
        p = int(pos[m])
        q = qkv[m, :H * hd].reshape(H, hd)
        k = qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd)
        v = qkv[m, (H + Hkv) * hd:].reshape(Hkv, hd)
        _, _, qr, eq = norm_rope(q, qn, tab[p], eps, fmt)
        kv_, kev, kr, ek = norm_rope(k, kn, tab[p], eps, fmt)
        K = torch.cat([wvalues(kc[m, :, :p], fmt), kr[:, None, :]], dim=1).repeat_interleave(G, dim=0)       # [H, n, hd]
        V = torch.cat([wvalues(vc[m, :, :p], fmt), v[:, None, :]], dim=1).repeat_interleave(G, dim=0)
        sc = torch.einsum("hd,hnd->hn", qr, K) * scale
        h0 = int(torch.randint(0, Hkv, (1,), generator=gen)) * G
        ds = scale * torch.einsum("hd,hnd->hn", eq, K.abs()) + U * sc.abs() \
            + (10 + math.log2(hd // 8)) * U * scale * torch.einsum("hd,hnd->hn", qr.abs(), K.abs())
        ekh = ek.repeat_interleave(G, dim=0)
        ds[:, p] += scale * ((qr.abs() * ekh).sum(-1) + (eq * ekh).sum(-1))
        for s, (lo, hi) in enumerate(split_ranges(p, nsplit)):
            if lo >= hi:
                continue
            n = hi - lo
            scr, Vr = sc[:, lo:hi], V[:, lo:hi]
            pw = torch.softmax(scr, dim=-1)
            r_pv = WR._r3(pw[h0:h0 + G], Vr[h0].contiguous())
            r_max = max(r_max, r_pv)
            mx = scr.max(dim=-1, keepdim=True).values
            D = (ds[:, lo:hi] + U * (scr - mx).abs()).max(dim=-1, keepdim=True).values
            RS = WR._rescales(scr, 1) + 1
            rel = 2 * (torch.expm1(D) + (1 + RS) * LIB) + (min(MARGIN * r_pv, (n + 2) * U) + (n / 64 + 14 + 2 * RS) * U)
            on[m, :, s] = True
            Y[m, :, s] = torch.einsum("hn,hnd->hd", pw, Vr)
            YE[m, :, s] = rel * torch.einsum("hn,hnd->hd", pw, Vr.abs())
            Mx[m, :, s] = mx[:, 0]
            ME[m, :, s] = ds[:, lo:hi].max(dim=-1).values
        ks.append(kv_); kes.append(kev); vs.append(v)
    k, ke = torch.stack(ks), torch.stack(kes)
    return PartRef(on, Y, YE, Mx, ME, Ref(k, ke, store(k, fmt)), torch.stack(vs), r_max)


@dataclass
class PartVerdict:
    checked: int
    flagged: int
    worst: float
    where: List[tuple]      # (row, head, split) with a flagged element


def check_parts(part_o, part_ml, ref: PartRef) -> PartVerdict:
    """The recorded (O, m, l) of every (row, head, split): an empty range exactly (0, -inf, 0); else O / l and m within
    their bounds, l > 0, everything finite."""
    O = torch.from_numpy(np.ascontiguousarray(part_o)).to(F64)
    ml = torch.from_numpy(np.ascontiguousarray(part_ml)).to(F64)
    m, l = ml[..., 0], ml[..., 1]
    empty_ok = (O == 0).all(dim=-1) & (m == float("-inf")) & (l == 0)
    lpos = torch.isfinite(l) & (l > 0)
    y = O / torch.where(lpos, l, torch.ones_like(l))[..., None]
    yb = ref.y_err + 2 * U * ref.y.abs() + half_ulp(ref.y.abs(), True)
    mb = ref.m_err + half_ulp(ref.m.abs().clamp_max(3e38), True)
    ry = ((y - ref.y).abs() / yb).nan_to_num(nan=float("inf"))
    rm = ((m - torch.where(ref.on, ref.m, torch.zeros_like(m))).abs() / mb).nan_to_num(nan=float("inf"))
    full_bad = ~lpos | ~(ry <= 1).all(dim=-1) | ~(rm <= 1) | ~torch.isfinite(O).all(dim=-1)
    bad = torch.where(ref.on, full_bad, ~empty_ok)
    ratio = torch.where(ref.on, torch.maximum(ry.max(dim=-1).values, rm), (~empty_ok).to(F64) * float("inf")).nan_to_num(nan=0.0, posinf=float("inf"))
    ratio = torch.where(ref.on & ~lpos, torch.full_like(ratio, float("inf")), ratio)
    return PartVerdict(int(O.numel() + ml.numel()), int(bad.sum()), float(ratio.max()), [tuple(t) for t in torch.nonzero(bad).tolist()])


def merge_ref(part_o, part_ml, fmt: str):
    """gemv_attn_combine_kernel's y [M, H hd] from RECORDED partials: (y before rb, its bound, rb(y), its reach)."""
    O = torch.from_numpy(np.ascontiguousarray(part_o)).to(F64)                    # [M, H, ns, hd]
    ml = torch.from_numpy(np.ascontiguousarray(part_ml)).to(F64)
    m, l = ml[..., 0], ml[..., 1]
    ns = m.shape[-1]
    Mx = m.max(dim=-1, keepdim=True).values
    w = torch.where(torch.isfinite(m), torch.exp(m - Mx), torch.zeros_like(m))
    L = (l * w).sum(dim=-1, keepdim=True)
    y = (O * w[..., None]).sum(dim=-2) / L
    C = (ns + 7) // 8 - 1
    dm = torch.where(torch.isfinite(m), (m - Mx).abs(), torch.zeros_like(m)).max(dim=-1, keepdim=True).values
    rel = 2 * (LIB * (1 + C) + U * dm) + (ns + 2 * C + 4) * U
    e = rel * ((O.abs() * w[..., None]).sum(dim=-2) / L)
    Mr = y.shape[0]
    y, e = y.reshape(Mr, -1), e.reshape(Mr, -1)
    yr, er = rch(y, e, fmt)
    return y, e, yr, er


def check_cache(fmt: str, kc0, vc0, kc1, vc1, pos, k: Ref, v: torch.Tensor):
    """kc0 / vc0: what went in, kc1 / vc1 [M, Hkv, rows, hd]: what came back.  Returns (verdict of the appended K rows, the
    appended V rows are exact copies, every other row bit-unchanged)."""
    rows = np.arange(len(pos))
    p = np.asarray(pos)
    k_new, v_new = kc1[rows, :, p], vc1[rows, :, p]
    vk = check(k_new, k.ref, k.err, fmt)
    v_ok = bool(np.array_equal(np.asarray(v_new).view(np.uint8), np.asarray(wbits(v, fmt)).view(np.uint8)))
    same = True
    for got, was, new in ((kc1, kc0, k_new), (vc1, vc0, v_new)):
        was = np.array(was)
        was[rows, :, p] = new
        same = same and bool(np.array_equal(np.asarray(got).view(np.uint8), was.view(np.uint8)))
    return vk, v_ok, same


def emulate_decode_attn(fmt: str, qkv, pos, qn, kn, kc, vc, tab, H: int, Hkv: int, hd: int, nsplit: int, eps: float = 1e-6,
                        bug: Optional[str] = None):
    """attn_decode_kernel in float32: per split its range, positions dealt to NSLOT lane-group slots, a softmax per slot, the
    in-block merge of the slots.  Returns (part_o [M, H, ns, hd], part_ml [M, H, ns, 2], k rows, kc, vc after the append)."""
    M, G = qkv.shape[0], H // Hkv
    NSLOT = 4 * (64 // (hd // 8))
    scale = torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(hd), dtype=F32))
    tab = tab.to(F32)

    def nr(x, gain, t):
        if gain is not None:
            inv = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / hd + torch.tensor(eps, dtype=F32))
            x = _r32((x * inv) * gain.to(F32)[None, :], fmt)
        x0, x1, c, s = x[:, 0::2], x[:, 1::2], t[None, :, 0], t[None, :, 1]
        return _r32(torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1).reshape(x.shape), fmt)

    po = torch.zeros(M, H, nsplit, hd, dtype=F32)
    pml = torch.zeros(M, H, nsplit, 2, dtype=F32)
    pml[..., 0] = float("-inf")
    kc1, vc1, ks = np.array(kc), np.array(vc), []
    for m in range(M):
        p = int(pos[m])
        q = qkv[m, :H * hd].reshape(H, hd).to(F32)
        k = qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd).to(F32)
        v = qkv[m, (H + Hkv) * hd:].reshape(Hkv, hd).to(F32)
        qr, kr = nr(q, qn, tab[p]), nr(k, kn, tab[p])
        ks.append(kr)
        if bug != "append_wrong_split":                                  # the block whose range holds pos appends; a wrong range: nobody does
            kc1[m, :, p], vc1[m, :, p] = wbits(kr, fmt), wbits(v, fmt)
        K = torch.cat([wvalues(kc[m, :, :p], fmt).to(F32), kr[:, None, :], wvalues(kc[m, :, p + 1:p + 2], fmt).to(F32)], dim=1)
        V = torch.cat([wvalues(vc[m, :, :p], fmt).to(F32), v[:, None, :], wvalues(vc[m, :, p + 1:p + 2], fmt).to(F32)], dim=1)
        K, V = K.repeat_interleave(G, dim=0), V.repeat_interleave(G, dim=0)
        sc = torch.einsum("hd,hnd->hn", qr, K) * scale
        ranges = split_ranges(p, nsplit)
        last = max(s for s, (lo, hi) in enumerate(ranges) if lo < hi)
        for s, (lo, hi) in enumerate(ranges):
            if lo >= hi:
                if bug == "empty_m0":                                    # an empty range leaves m = 0: the merge sees it as visible
                    pml[m, :, s, 0] = 0.0
                continue
            idx = list(range(lo, hi))
            if bug == "miss_pos" and p in idx and p > 0:
                idx.remove(p)
            if bug == "stale_pos1" and s == last and K.shape[1] > p + 1:
                idx.append(p + 1)
            if not idx:
                continue
            ms, ls, os_ = [], [], []
            for sl in range(NSLOT):
                j = idx[sl::NSLOT]
                if not j:
                    continue
                scj = sc[:, j]
                mj = scj.max(dim=-1, keepdim=True).values
                e = torch.exp(scj - mj)
                ms.append(mj[:, 0]); ls.append(e.sum(dim=-1)); os_.append(torch.einsum("hn,hnd->hd", e, V[:, j]))
            ms, ls, os_ = torch.stack(ms, dim=1), torch.stack(ls, dim=1), torch.stack(os_, dim=1)
            Mb = ms.max(dim=1, keepdim=True).values
            w = torch.exp(ms - Mb)
            L, O = torch.zeros(H, dtype=F32), torch.zeros(H, hd, dtype=F32)
            for i in range(ms.shape[1]):
                L = L + ls[:, i] * w[:, i]
                O = O + os_[:, i] * w[:, i, None]
            po[m, :, s], pml[m, :, s, 0], pml[m, :, s, 1] = O, Mb[:, 0], L
    return po.numpy(), pml.numpy(), torch.stack(ks).to(F64), kc1, vc1


def emulate_merge(fmt: str, part_o, part_ml, bug: Optional[str] = None, bug_split: int = 1) -> torch.Tensor:
    """merge_splits4 in float32: chunks of 8 splits, the running sums rescaled per later chunk; returns rb(y) [M, H hd]."""
    O, ml = torch.from_numpy(np.ascontiguousarray(part_o)), torch.from_numpy(np.ascontiguousarray(part_ml))
    if bug == "row_mod4":                                                 # row m's partials read at row m mod 4's offset
        rows = torch.arange(O.shape[0]) % 4
        O, ml = O[rows], ml[rows]
    m, l = ml[..., 0], ml[..., 1]
    ns = m.shape[-1]
    Mr = torch.full(m.shape[:-1], float("-inf"), dtype=F32)
    L = torch.zeros_like(Mr)
    A = torch.zeros(*Mr.shape, O.shape[-1], dtype=F32)
    for c0 in range(0, ns, 8):
        mc = m[..., c0:c0 + 8]
        Mc = mc.max(dim=-1).values
        vis = Mc > float("-inf")
        Mn = torch.maximum(Mr, Mc)
        if c0 > 0:
            r = torch.where(vis & (Mr > float("-inf")), torch.exp(Mr - Mn), torch.ones_like(Mr))
            if bug == "chunk2_twice" and c0 == 8:
                r = r * r
            L, A = L * r, A * r[..., None]
        Mr = torch.where(vis, Mn, Mr)
        for s in range(mc.shape[-1]):
            w = torch.where(mc[..., s] > float("-inf"), torch.exp(mc[..., s] - Mr), torch.zeros_like(Mr))
            if bug == "weight_one" and c0 + s == bug_split:
                w = torch.where(mc[..., s] > float("-inf"), torch.ones_like(w), w)
            w = torch.where(vis, w, torch.zeros_like(w))
            L = L + l[..., c0 + s] * w
            A = A + O[..., c0 + s, :] * w[..., None]
    y = _r32(A / L[..., None], fmt)
    return y.reshape(y.shape[0], -1).to(F64)


# ------------------------------------------------------------------------------------------------------ fast attention
@dataclass
class FastRef:
    y: Ref                  # [M, H hd]
    k: Ref                  # the appended K rows [M, Hkv, hd]
    v: torch.Tensor


def fast_attn_ref(fmt: str, qkv, c: int, qn, kn, kc, vc, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6,
                  k_hist_err=None) -> FastRef:
    """One fast_attn_kernel launch at codebook position c: qkv [M, (H + 2 Hkv) hd], kc / vc [M, Hkv, ncb, hd] (rows < c read),
    tab [ncb, hd / 2, 2].  k_hist_err [M, Hkv, c, hd]: how far the K rows the device read may lie from kc's (rows that are
    themselves restated, not read back: the reach of their last rounding); it joins the scores as the new row's ek does."""
    qkv, tab = qkv.to(F64), tab.to(F64)
    qn = None if qn is None else qn.to(F64)
    kn = None if kn is None else kn.to(F64)
    M, G = qkv.shape[0], H // Hkv
    scale = float(np.float32(1.0 / math.sqrt(float(hd))))
    ys, es, ks, kes, vs = [], [], [], [], []
    for m in range(M):
        q = qkv[m, :H * hd].reshape(H, hd)
        k = qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd)
        v = qkv[m, (H + Hkv) * hd:].reshape(Hkv, hd)
        _, _, qr, eq = norm_rope(q, qn, tab[c], eps, fmt)
        kv_, kev, kr, ek = norm_rope(k, kn, tab[c], eps, fmt)
        K = torch.cat([wvalues(kc[m, :, :c], fmt), kr[:, None, :]], dim=1).repeat_interleave(G, dim=0)       # [H, c + 1, hd]
        V = torch.cat([wvalues(vc[m, :, :c], fmt), v[:, None, :]], dim=1).repeat_interleave(G, dim=0)
        d = torch.einsum("hd,hnd->hn", qr, K)
        ed = torch.einsum("hd,hnd->hn", eq, K.abs()) + 8 * U * torch.einsum("hd,hnd->hn", qr.abs(), K.abs())
        ekh = ek.repeat_interleave(G, dim=0)
        ed[:, c] += (qr.abs() * ekh).sum(-1) + (eq * ekh).sum(-1)
        if k_hist_err is not None and c > 0:
            eh = k_hist_err[m].to(F64).repeat_interleave(G, dim=0)                                           # [H, c, hd]
            ed[:, :c] += torch.einsum("hd,hnd->hn", qr.abs() + eq, eh)
        dr, e1 = rch(d, ed, fmt)
        s = dr * scale
        sr, e_s = rch(s, scale * e1 + U * s.abs(), fmt)
        mx, imx = sr.max(dim=-1, keepdim=True)
        D = e_s + e_s.gather(1, imx) + U * (sr - mx).abs()
        w = torch.exp(sr - mx)
        rw = torch.expm1(D) + LIB
        pj = w / w.sum(dim=-1, keepdim=True)
        rp = rw + rw.max(dim=-1, keepdim=True).values + (c + 3) * U
        pr, ep = rch(pj, rp * pj, fmt)
        o = torch.einsum("hn,hnd->hd", pr, V)
        eo = torch.einsum("hn,hnd->hd", ep, V.abs()) + (c + 1) * U * torch.einsum("hn,hnd->hd", pr, V.abs())
        ys.append(o.reshape(-1)); es.append(eo.reshape(-1)); ks.append(kv_); kes.append(kev); vs.append(v)
    y, e, k, ke = torch.stack(ys), torch.stack(es), torch.stack(ks), torch.stack(kes)
    return FastRef(Ref(y, e, store(y, fmt)), Ref(k, ke, store(k, fmt)), torch.stack(vs))


def emulate_fast_attn(fmt: str, qkv, c: int, qn, kn, kc, vc, tab, H: int, Hkv: int, hd: int, eps: float = 1e-6,
                      bug: Optional[str] = None, k0_from=None):
    """fast_attn_kernel in float32.  k0_from: the paired pass's position-1 block (c = 1): qkv rows of position 0, from which
    it rebuilds cache row 0 instead of reading it.  Returns (y [M, H hd], the appended k rows), float64 of exact values."""
    M, G = qkv.shape[0], H // Hkv
    scale = torch.tensor(1.0 / math.sqrt(float(hd)), dtype=F32)
    tab = tab.to(F32)

    def nr(x, gain, t):
        if gain is not None:
            inv = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / hd + torch.tensor(eps, dtype=F32))
            x = _r32((x * inv) * gain.to(F32)[None, :], fmt)
        x0, x1, cs, sn = x[:, 0::2], x[:, 1::2], t[None, :, 0], t[None, :, 1]
        return _r32(torch.stack([x0 * cs - x1 * sn, x1 * cs + x0 * sn], dim=-1).reshape(x.shape), fmt)

    ys, ks = [], []
    for m in range(M):
        q = qkv[m, :H * hd].reshape(H, hd).to(F32)
        k = qkv[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd).to(F32)
        v = qkv[m, (H + Hkv) * hd:].reshape(Hkv, hd).to(F32)
        tq = tab[c - 1] if bug == "rot_prev" and c > 0 else tab[c]
        qr, kr = nr(q, qn, tq), nr(k, kn, tq)
        Kc, Vc = wvalues(kc[m, :, :c], fmt).to(F32), wvalues(vc[m, :, :c], fmt).to(F32)
        if k0_from is not None:
            k0 = k0_from[m, H * hd:(H + Hkv) * hd].reshape(Hkv, hd).to(F32)
            Kc[:, 0] = nr(k0, None if bug == "pair_no_kn" else kn, tab[0])
            Vc[:, 0] = k0_from[m, (H + Hkv) * hd:].reshape(Hkv, hd).to(F32)
        K = torch.cat([Kc, kr[:, None, :]], dim=1).repeat_interleave(G, dim=0)
        V = torch.cat([Vc, v[:, None, :]], dim=1).repeat_interleave(G, dim=0)
        d = torch.einsum("hd,hnd->hn", qr, K)
        s = _r32((d if bug == "no_rb_d" else _r32(d, fmt)) * scale, fmt)
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        tot = torch.zeros(H, dtype=F32)
        for j in range(c + 1):
            tot = tot + e[:, j]
        pj = _r32(e / tot[:, None], fmt)
        o = torch.zeros(H, hd, dtype=F32)
        for j in range(c + 1):
            o = _fma(pj[:, j, None], V[:, j], o)
        ys.append(_r32(o, fmt).reshape(-1))
        ks.append(kr)
    return torch.stack(ys).to(F64), torch.stack(ks).to(F64)


# ------------------------------------------------------------------------------------------------------ embedding
def embed_ref(fmt: str, emb, cb_emb, toks, ncb: int, cbsize: int, sem_begin: int, sem_end: int, scale: bool) -> Ref:
    """toks [M, ncb + 1] (token, then the codes); emb [vocab, D], cb_emb [ncb cbsize, D]: exact values of the model's type."""
    emb, cbe = emb.to(F64), cb_emb.to(F64)
    toks = np.asarray(toks).reshape(-1, ncb + 1)
    vocab = emb.shape[0]
    div = float(np.float32(math.sqrt(ncb + 1)))
    vs, es = [], []
    for row in toks:
        t0 = int(row[0])
        is_vq = sem_begin <= t0 <= sem_end
        e0 = emb[min(max(t0, 0), vocab - 1)]
        if not is_vq:
            vs.append(e0); es.append(torch.zeros_like(e0))
            continue
        rows = torch.stack([cbe[min(max(int(row[i + 1]), 0), cbsize - 1) + i * cbsize] for i in range(ncb)])
        vq, evq = rch(rows.sum(dim=0), (ncb - 1) * U * rows.abs().sum(dim=0), fmt)
        x = e0 + vq
        e = evq + U * x.abs()
        if scale:
            xr, e = rch(x, e, fmt)
            x = xr / div
            e = e / div + U * x.abs()
        vs.append(x); es.append(e)
    v, e = torch.stack(vs), torch.stack(es)
    return Ref(v, e, store(v, fmt))


def emulate_embed(fmt: str, emb, cb_emb, toks, ncb: int, cbsize: int, sem_begin: int, sem_end: int, scale: bool,
                  bug: Optional[str] = None) -> torch.Tensor:
    emb, cbe = emb.to(F32), cb_emb.to(F32)
    toks = np.asarray(toks).reshape(-1, ncb + 1)
    vocab = emb.shape[0]
    div = torch.tensor(float(np.float32(math.sqrt(ncb + 1))), dtype=F32)
    out = []
    for row in toks:
        t0 = int(row[0])
        is_vq = sem_begin <= t0 <= (sem_end + 1 if bug == "vq_past_end" else sem_end)
        x = emb[min(max(t0, 0), vocab - 1)]
        if is_vq:
            vq = torch.zeros_like(x)
            for i in range(ncb):
                vq = vq + cbe[min(max(int(row[i + 1]), 0), cbsize - 1) + i * cbsize]
            x = _r32(x + _r32(vq, fmt), fmt)
        if scale and (is_vq or bug == "scale_text"):
            x = _r32(x / div, fmt)
        out.append(x)
    return torch.stack(out).to(F64)


def xo_rows(xo: np.ndarray, M: int, D: int) -> np.ndarray:
    """The octet-major copy Xo[D / 8][ldm][8] -> rows [M, D]."""
    return np.ascontiguousarray(xo[:, :M, :].transpose(1, 0, 2).reshape(M, -1)[:, :D])
