"""The draw launches (csrc/ar_kernels.h: sample_small_kernel, sample_block_kernel, samp_cut / samp_count / samp_race /
samp_finish_kernel, finish_draw) restated: float64 where the draw is arithmetic, exact where it is integer.  The restatement
is built on oracle.ar.logits_to_probs (golden-pinned to the reference's inference.py:30-80), and returns per row everything
the hook ft_test_draw returns, so a launch is judged field by field (judge()).

Penalty (inference.py:38-46, window rule 187-191).  nf = 0: none.  cb = 0: the R ids of history column ws + 1; cb >= 1: the 16
ids of history row cb + 1 from column ws + 1; ws = 0 below 17 frames, else nf - 17.  Gather all, then scatter: a duplicate id
writes the same value twice; ids outside [0, V) are ignored.  ban_eos writes -inf at im_end, at cb = 0 only, after the penalty.
The values are torch's own in the model's type (the same gather / where / scatter as the oracle; test_draw_ref_host.py pins
them to oracle.ar.logits_to_probs), so the row a launch leaves behind must equal them bit for bit.

The kept set as a band.  Ranks are the descending order of the penalised logits, ties in index order.  p[r] are the reference's
own rounded probabilities (softmax of the sorted row in the model's type), c64[r] their inclusive float64 cumulative sum.  The
comparison `rb(cum) > rb(top_p)` flips at X: in f32 rb is the identity and X = top_p (as f32); in a 16-bit type rb(cum) exceeds
rb(top_p) once cum passes the midpoint between rb(top_p) and the next value of the type above it.  The reference sums
sequentially in float32, the device in another order (per lane, per wave, per class with one fma per class), so neither holds
c64: e = MARGIN (4) x the largest |f32 - f64| over all ranks of the cumulative sums of p taken in float32 in three orders (one
chain; per-32 blocks; pairwise), the r_stage convention of tests/codec_stage_ref.py.  Rank r MUST be kept if c64[r] < X - e,
MUST be dropped if c64[r] > X + e, rank 0 is always kept, ranks in between are free: the kept count n satisfies lo <= n <= hi.
Where the total mass lies within e of X (top_p = 1.0), the reference itself depends on the order of summation and only the
must-keep side is judged (hi = V).  MAX_BAND = 8 free ranks at most, otherwise the INPUT is bad (BandTooWide); it is never
widened.  Inside an exactly tied class the count kept is specified by the same band and the members are the lowest indices
(the kernel's stated rule; the reference's sort is unstable there), which is what "ties in index order" above says.

Probes.  The winner is argmax(p / q) over the kept set, so a noise row that is 2^lo_e at j and 2^hi_e elsewhere turns the winner
into a membership test for j: j kept -> j wins; j dropped -> the reference's argmax wins (or a member of its exact tie class).
(lo_e, hi_e) = (-60, 60) in bf16 and f32, whose exponent range holds both powers and every p 2^60 and p 2^-60 exactly.  fp16
cannot hold 2^60 (largest finite value 65504: it would become inf and every other ratio 0, so a dropped j would lose to index 0,
not to the argmax), so there (lo_e, hi_e) = (-24, 3): 2^-24 is fp16's smallest subnormal and exact, p / 8 is a normal number
down to p = 2^-11, and p 2^24 is either exact or overflows to +inf, which still wins; were 2^-24 flushed to 0 a kept j would
give +inf and a dropped one 0 / 0 = NaN, which never wins: the probe's answer is the same.  A probe is valid only if the reference's own
post-temperature probability of j - over the reference's kept set, j added if it was dropped - is non-zero as rounded and
p_j 2^(hi_e - lo_e) > 4 x the largest kept probability (a factor 4 above every rounding of p, q and p / q, each below 2^-8
relative); invalid probes are left out and counted.

Philox.  philox4 / philox_word / draw_noise4 / exp1_from_word in numpy integers; u = ((w >> 8) + 1) 2^-24 is exact, q =
max(-log u, 1e-30) is taken in float64 and rounded once to f32.  The device's logf is within 2 ulp of its own result, so its q
is within 2 x 2^-23 relative of ours (the error is relative to -log u at every u, also near u = 1 where -log u is tiny), then q
is rounded once to the model's type (u_t = 2^-9 bf16, 2^-11 fp16, 0 in f32, relative) and p / q once more (f32: 2^-24 each).  So
a device winner w differing from the reference's w* is accepted if ratio64(w) >= ratio64(w*) (1 - RATIO_TOL[fmt]) with
RATIO_TOL = 2 x (2 x 2^-23 + 2 u_t + 2^-23): both competitors, each with its q error, its two roundings and one f32 division.
Such draws are counted (the GPU test caps them at 2 %).

Bookkeeping (finish_draw) is integer and copies: exact.  Everything a launch must not write holds the caller's sentinel or
the hook's 0xFF fill afterwards."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ar as O

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
MARGIN = 4.0
MAX_BAND = 8
PROBE_EXP = {"bf16": (-60, 60), "f32": (-60, 60), "fp16": (-24, 3)}
U_T = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -11, "f32": 0.0}
RATIO_TOL = {f: 2.0 * (2 * 2.0 ** -23 + 2 * u + 2.0 ** -23) for f, u in U_T.items()}
SENT = 0x7E5A5A5A                     # ARHipEngine.DRAW_SENTINEL
FILL32, FILL16 = 0xFFFFFFFF, 0xFFFF   # the hook's 0xFF fill


class BandTooWide(AssertionError):
    """The free band of an input holds more than MAX_BAND ranks: a bad input, not a finding."""


class NormaliserTooClose(BandTooWide):
    """The reference's own classification of a rank next to the band changes with the float32 error of its softmax
    normaliser (see _normaliser_reach): a bad input, like a band that is too wide."""


def rb(x, fmt):
    """float array -> float32 values rounded once to `fmt` (nearest even)."""
    a = np.asarray(x, dtype=np.float32)
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    return t.to(DT[fmt]).to(torch.float32).numpy().reshape(a.shape)[()]


def bits16(x, fmt):
    """float32 values exact in the 16-bit `fmt` -> their bit patterns."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DT[fmt]).contiguous()
    return t.view(torch.int16).numpy().view(np.uint16)


def order_key(f32):
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------ Philox
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays (broadcast) -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & 0xFFFFFFFF for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & np.uint64(0xFFFFFFFF), n2, p0 & np.uint64(0xFFFFFFFF)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def philox_word(c0, c1, c2, c3, k0, k1):
    c0 = np.asarray(c0, dtype=np.uint32)
    w = np.stack(philox4(c0 >> np.uint32(2), c1, c2, c3, k0, k1), axis=-1)
    return np.take_along_axis(w, (c0 & np.uint32(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def exp1_from_word(w):
    """-> (q float32, u float64): u = ((w >> 8) + 1) / 2^24 in (0, 1], q = max(-log u, 1e-30) rounded once to f32."""
    u = ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    return np.maximum((-np.log(u)).astype(np.float32), np.float32(1e-30)), u


def draw_noise(V, cb, nf, seed, *, slot=0, fault=None):
    """The V draws of (seed, frame nf, codebook cb): element 4 g + e is word e of the call with counter (g, cb, nf, 0) and key
    (seed low, seed high).  fault: an emulated mistake (test_draw_ref_host.py)."""
    g = np.arange((V + 3) // 4, dtype=np.uint32)
    c1, c3 = (0 if fault == "philox_no_cb" else cb), (slot if fault == "philox_slot" else 0)
    k1 = 0 if fault == "philox_no_hi" else (seed >> 32)
    w = np.stack(philox4(g, c1, nf, c3, seed & 0xFFFFFFFF, k1), axis=-1)
    if fault == "philox_perm":
        w = w[:, [1, 0, 3, 2]]
    return exp1_from_word(w.reshape(-1)[:V])[0]


# ------------------------------------------------------------------------------------------------------------ inputs
@dataclass
class DrawModel:
    """What a draw launch knows of its context."""
    fmt: str
    V: int                 # vocab_size
    fastV: int
    ncb: int
    cap: int
    sem_begin: int
    im_end: int
    cbsize: int
    fast_emb: np.ndarray   # [cbsize][Df] float32, values exact in fmt
    MB: int = 1
    xo_pair: int = 0       # 0: no lock-step path
    qkv0_tab: Optional[np.ndarray] = None   # [fastV][n] uint16

    @property
    def R(self):
        return self.ncb + 1

    def width(self, cb):
        return self.V if cb == 0 else self.fastV


@dataclass
class Ctl:
    top_p: float
    temperature: float
    rep: float
    ban_eos: bool = False
    seed: int = 0


@dataclass
class Row:
    logits: np.ndarray           # (V,) float32, exact in fmt
    ctl: Ctl
    nf: int
    hist: np.ndarray             # (R, cap) int32
    pos: int = 0
    done: int = 0
    probe: Optional[int] = None  # probe noise at this index ...
    noise: Optional[np.ndarray] = None   # ... or an explicit noise row, or neither: the counter-based generator
    strict: bool = False         # explicit noise built so that no tolerance applies: the winner is the reference's, ties to the lowest index
    tag: str = ""
    ref: Optional["RowRef"] = None


def window_ids(hist, cb, nf, *, fault=None):
    """The ids the penalty reads (None: no penalty)."""
    if nf <= 0:
        return None
    it = nf - 1
    ws = 0 if it < 16 else it - 16
    if fault == "window_early":
        ws -= 1
    if cb == 0:
        return np.asarray(hist[:, ws + 1], dtype=np.int64)
    n = 15 if fault == "window15" else 16
    return np.asarray(hist[cb if fault == "window_row" else cb + 1, ws + 1: ws + 1 + n], dtype=np.int64)


def hist_for(model: DrawModel, cb, nf, ids, filler):
    """A history block whose window at (cb, nf) holds `ids` (R ids at cb = 0, 16 otherwise); everything else `filler` (R, cap)."""
    h = np.array(filler, dtype=np.int32).reshape(model.R, model.cap).copy()
    if nf > 0:
        it = nf - 1
        ws = 0 if it < 16 else it - 16
        if cb == 0:
            h[:, ws + 1] = ids
        else:
            h[cb + 1, ws + 1: ws + 17] = ids
    return h


def penalised(model: DrawModel, cb, row: Row):
    """The row after the penalty and the ban, as a tensor of the model's type."""
    V = model.width(cb)
    lg = torch.from_numpy(np.ascontiguousarray(row.logits, dtype=np.float32)).to(DT[model.fmt]).clone()
    ids = window_ids(row.hist, cb, row.nf)
    if ids is not None:
        ids = ids[(ids >= 0) & (ids < V)]
        if len(ids):
            idx = torch.from_numpy(ids)
            rep = torch.tensor(row.ctl.rep)
            s = torch.gather(lg, dim=-1, index=idx)
            s = torch.where(s < 0, s * rep, s / rep)
            lg.scatter_(dim=-1, index=idx, src=s)
    if cb == 0 and row.ctl.ban_eos and model.im_end < V:
        lg[model.im_end] = -float("inf")
    return lg


def _cum_orders(p32):
    """Inclusive cumulative sums of p32 in float32 in three orders: one chain, per-32 blocks, pairwise."""
    n = len(p32)
    chain = np.cumsum(p32, dtype=np.float32)
    nb = (n + 31) // 32
    pp = np.zeros(nb * 32, dtype=np.float32)
    pp[:n] = p32
    inner = np.cumsum(pp.reshape(nb, 32), axis=1, dtype=np.float32)
    base = np.concatenate([[np.float32(0)], np.cumsum(inner[:, -1], dtype=np.float32)[:-1]]).astype(np.float32)
    blocked = (inner + base[:, None]).astype(np.float32).reshape(-1)[:n]
    P = 1 << max(0, (n - 1).bit_length())
    pw = np.zeros(P, dtype=np.float32)
    pw[:n] = p32
    levels = [pw]
    while len(levels[-1]) > 1:
        a = levels[-1]
        levels.append((a[0::2] + a[1::2]).astype(np.float32))
    pre = np.zeros(1, dtype=np.float32)                                   # exclusive prefix of each node, root downwards
    for a in reversed(levels[:-1]):
        nxt = np.empty(len(a), dtype=np.float32)
        nxt[0::2] = pre
        nxt[1::2] = (pre + a[0::2]).astype(np.float32)
        pre = nxt
    pair = (pre + pw).astype(np.float32)[:n]
    return chain, blocked, pair


def _normaliser_reach(srt, order_hi, fmt):
    """A second condition on the INPUT, found on the MI355X (fp16, V = 155776, spread 0.3: every probability is an fp16
    subnormal, a multiple of 2^-24, so every float32 sum of them is exact and e = 0).  The probabilities are exp(l - max) / Z
    ROUNDED to the type, and Z is itself a float32 sum of V exponentials: its relative error r_Z moves every quotient the
    same way, and each element whose quotient lies within it of a rounding midpoint lands on the other neighbour - in the
    reference (torch's order) as well as on the device (its order).  reach = the summed steps of those elements among ranks
    <= hi, with r_Z = MARGIN x (the largest |f32 - f64| / Z of the normaliser in the three float32 orders + 2 ulp of expf).  A
    rank next to the band whose distance from X -+ e is within reach is not classified by the reference itself."""
    ex = torch.exp(srt.to(torch.float64) - float(srt[0])).numpy()
    Z = ex.sum()
    rz = MARGIN * (max(abs(float(o[-1]) - Z) for o in _cum_orders(ex.astype(np.float32))) / Z + 2.0 ** -22)
    v = (ex / Z)[: order_hi + 1]
    if fmt == "f32":
        r = v.astype(np.float32)
        up, dn = np.nextafter(r, np.float32(np.inf)).astype(np.float64), np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
        r = r.astype(np.float64)
    else:
        t = torch.from_numpy(v).to(DT[fmt])
        b = t.view(torch.int16)
        up = (b + 1).view(DT[fmt]).to(torch.float64).numpy()
        dn = torch.where(b > 0, b - 1, b).view(DT[fmt]).to(torch.float64).numpy()
        r = t.to(torch.float64).numpy()
    other = np.where(v >= r, up, dn)
    flips = np.abs(v - (r + other) / 2) <= rz * v
    return float(np.abs(other - r)[flips].sum())


@dataclass
class RowRef:
    after: np.ndarray          # (V,) float32: the row after penalty and ban
    order: np.ndarray          # rank -> index
    rank_of: np.ndarray        # index -> rank
    c64: np.ndarray
    X: float
    e: float
    lo: int                    # kept count n: lo <= n <= hi
    hi: int
    one_sided: bool
    probs: np.ndarray          # (V,) float64: the reference's final probabilities, the kept members of a tied class by index
    n_ref: int                 # ranks the reference keeps
    ref_probs: np.ndarray      # (V,) float64: as oracle.ar.logits_to_probs returned them
    p_if_kept: np.ndarray      # (V,) float64: the post-temperature probability of every index were it kept (rounded to fmt)
    pmax: float
    argmax_class: np.ndarray   # indices that may win a race of equal noise: the largest probability, inside the band
    Lmax: float
    Tc: np.float32
    Mt: np.float32

    @property
    def band(self):
        return 0 if self.one_sided else self.hi - self.lo


def reference(model: DrawModel, cb, row: Row) -> RowRef:
    fmt, dt = model.fmt, DT[model.fmt]
    lg = penalised(model, cb, row)
    after = lg.to(torch.float32).numpy().copy()
    V = len(after)
    srt, order = torch.sort(lg, descending=True, stable=True)
    p = F.softmax(srt, dim=-1)                                            # the reference's own rounded probabilities
    p64 = p.to(torch.float64).numpy()
    c64 = np.cumsum(p64)
    e = MARGIN * max(float(np.abs(o.astype(np.float64) - c64).max()) for o in _cum_orders(p64.astype(np.float32)))
    tp = torch.tensor(row.ctl.top_p, dtype=torch.float32)
    if fmt == "f32":
        X = float(tp)
    else:
        t = tp.to(dt)
        up = (t.view(torch.int16) + 1).view(dt)                            # top_p > 0: the next pattern is the next value
        X = (float(t) + float(up)) / 2
    one_sided = abs(c64[-1] - X) <= e
    lo = max(1, int((c64 < X - e).sum()))
    hi = V if one_sided else max(lo, int((c64 <= X + e).sum()))
    if not one_sided and hi - lo > MAX_BAND:
        raise BandTooWide(f"free band of {hi - lo} ranks ({row.tag})")
    if not one_sided:
        reach = _normaliser_reach(srt, order_hi=hi, fmt=fmt)
        if (lo >= 2 and X - e - c64[lo - 1] <= reach) or (hi < V and c64[hi] - (X + e) <= reach):
            raise NormaliserTooClose(f"the cut lies within {reach:.3g} of a must-keep / must-drop rank ({row.tag})")
    order = order.numpy()
    rank_of = np.empty(V, dtype=np.int64)
    rank_of[order] = np.arange(V)
    probs = O.logits_to_probs(lg.clone(), torch.tensor(row.ctl.temperature), torch.tensor(row.ctl.top_p), torch.tensor(1.0), None)
    probs = probs.to(torch.float64).numpy()
    Tc = np.float32(max(np.float32(row.ctl.temperature), np.float32(1e-5)))
    lt = (lg / torch.clip(torch.tensor(row.ctl.temperature), min=1e-5)).to(torch.float64).numpy()   # rb(l / Tc), torch's own
    # the reference's own cut (inference.py:50-53 as oracle.ar.logits_to_probs states it; the host test pins this count to the
    # oracle's probs > 0 at T = 1, where no kept probability underflows)
    drop_sorted = torch.cumsum(p, dim=-1) > torch.tensor(row.ctl.top_p)
    drop_sorted[0] = False
    n_ref = int((~drop_sorted).sum())
    # the reference's sort is unstable: inside a tied class it keeps SOME members; the rule keeps the lowest indices.  Tied
    # members have equal probabilities, so the kept probabilities in rank order are the reference's, sorted.
    keep = rank_of < n_ref
    mt = lt[order[0]]
    ex = np.exp(np.where(np.isfinite(lt), lt - mt, -np.inf))
    Z2 = ex[keep].sum()
    if cb == 0 and row.ctl.ban_eos and model.im_end < V:                  # the banned token's probe asks what it would hold unbanned
        nb = penalised(model, cb, Row(row.logits, Ctl(row.ctl.top_p, row.ctl.temperature, row.ctl.rep, False), row.nf, row.hist))
        ex[model.im_end] = np.exp(float((nb[model.im_end] / torch.clip(torch.tensor(row.ctl.temperature), min=1e-5)).to(torch.float64)) - mt)
    p_all = rb(ex / (Z2 + ex), fmt).astype(np.float64)
    rule = np.zeros(V, dtype=np.float64)
    rule[order[:n_ref]] = np.sort(probs)[::-1][:n_ref]
    p_all[order[:n_ref]] = rule[order[:n_ref]]
    pm = rule.max()
    top = np.flatnonzero((p_all == pm) & (rank_of < hi))
    return RowRef(after=after, order=order, rank_of=rank_of, c64=c64, X=X, e=e, lo=lo, hi=hi, one_sided=one_sided, probs=rule, n_ref=n_ref,
                  ref_probs=probs, p_if_kept=p_all, pmax=float(pm), argmax_class=top, Lmax=float(after[order[0]]),
                  Tc=Tc, Mt=np.float32(rb(np.float32(after[order[0]]) / Tc, fmt)))


def cut_class(ref: RowRef, fmt):
    """(indices of the tied class that holds rank lo - 1 ... the class the cut falls in, in index order)."""
    r = min(ref.lo, len(ref.order) - 1)                                   # the first rank that may be dropped
    v = ref.after[ref.order[r]]
    return np.flatnonzero(ref.after == v)


def probe_noise(model: DrawModel, V, j):
    lo_e, hi_e = PROBE_EXP[model.fmt]
    q = np.full(V, 2.0 ** hi_e, dtype=np.float32)
    q[j] = 2.0 ** lo_e
    return q


def probe_valid(model: DrawModel, ref: RowRef, j):
    lo_e, hi_e = PROBE_EXP[model.fmt]
    pj = ref.p_if_kept[j]
    return pj > 0 and pj * 2.0 ** (hi_e - lo_e) > 4 * ref.pmax


def probe_list(model: DrawModel, ref: RowRef, row: Row, cb):
    """[(kind, index)] of the probes of one row configuration (see the module docstring), duplicates removed."""
    V, out = len(ref.after), []
    if ref.lo >= 1:
        out.append(("last must-keep", int(ref.order[ref.lo - 1])))
    if ref.hi < V:
        out.append(("first must-drop", int(ref.order[ref.hi])))
        cls = cut_class(ref, model.fmt)
        rk = ref.rank_of[cls]
        keep, drop = cls[rk < ref.lo], cls[rk >= ref.hi]
        if len(keep):
            out.append(("cut class, last must-keep member", int(keep.max())))
        if len(drop):
            out.append(("cut class, first must-drop member", int(drop.min())))
            out.append(("cut class, highest member", int(drop.max())))
    out.append(("argmax", int(ref.order[0])))
    ids = window_ids(row.hist, cb, row.nf)
    if ids is not None:
        out += [("penalised id", int(i)) for i in np.unique(ids[(ids >= 0) & (ids < V)])]
    if cb == 0 and row.ctl.ban_eos and model.im_end < V:
        out.append(("banned im_end", model.im_end))
    seen, res = set(), []
    for k, j in out:
        if j not in seen:
            seen.add(j)
            res.append((k, j))
    return res


def noise_of(model: DrawModel, cb, row: Row):
    V = model.width(cb)
    if row.probe is not None:
        return probe_noise(model, V, row.probe)
    if row.noise is not None:
        return np.asarray(row.noise, dtype=np.float32)
    return draw_noise(V, cb, row.nf, row.ctl.seed)


def noise_block(model: DrawModel, cb, rows: List[Row]):
    """The (rows, row_len) block in the layout enqueue_sample indexes, or None when no row injects noise (all rows must agree)."""
    inj = [r.probe is not None or r.noise is not None for r in rows]
    if not any(inj):
        return None
    assert all(inj) and len({r.nf for r in rows}) == len(rows), "one launch: all rows inject, nf distinct"
    V = model.width(cb)
    row_len = model.V + (model.ncb - 1) * model.fastV
    off = 0 if cb == 0 else model.V + (cb - 1) * model.fastV
    q = np.full((max(r.nf for r in rows) + 1, row_len), np.float32(1.0), dtype=np.float32)
    for r in rows:
        q[r.nf, off: off + V] = noise_of(model, cb, r)
    return q


# ------------------------------------------------------------------------------------------------------------ judging
@dataclass
class Flag:
    row: int
    field: str
    msg: str

    def __str__(self):
        return f"row {self.row} {self.field}: {self.msg}"


@dataclass
class Tally:
    probes: int = 0
    left_out: int = 0
    widest_band: int = 0
    draws: int = 0
    allowed: int = 0
    kinds: dict = field(default_factory=dict)


def expect_winner(model: DrawModel, cb, row: Row, got, tally: Tally):
    """None if `got` is an acceptable winner, else the reason."""
    ref, fmt = row.ref, model.fmt
    V = len(ref.after)
    if not 0 <= got < V:
        return f"winner {got} outside [0, {V})"
    if row.probe is not None:
        j, r = row.probe, int(ref.rank_of[row.probe])
        must_keep = r < ref.lo and np.isfinite(ref.after[j])
        must_drop = r >= ref.hi or not np.isfinite(ref.after[j])
        if must_keep and got != j:
            return f"probe {j} (rank {r}, class {ref.after[j]!r}) must be kept (lo {ref.lo}, hi {ref.hi}) but {got} won"
        if must_drop and got == j:
            return f"probe {j} (rank {r}, class {ref.after[j]!r}) must be dropped (lo {ref.lo}, hi {ref.hi}) but won"
        if got != j and got not in ref.argmax_class:
            return f"probe {j} lost to {got}, which is not the reference's argmax {ref.argmax_class[:4]}"
        return None
    q = torch.from_numpy(noise_of(model, cb, row)).to(DT[fmt])
    p = torch.from_numpy(ref.probs).to(DT[fmt])                           # exact: they are values of the type
    ratio = p / q
    want = int(torch.argmax(ratio))
    if row.strict:
        return None if got == want else f"winner {got}, the reference draws {want} (exact case: ties go to the lowest index)"
    tally.draws += 1
    if got == want or float(ratio[got]) == float(ratio[want]):
        return None
    r64 = ref.probs / q.to(torch.float64).numpy()
    free = ref.lo <= ref.rank_of[got] < ref.hi                            # a free-band member the reference happened to drop
    if free:
        r64 = r64.copy()
        r64[got] = ref.p_if_kept[got] / float(q[got])
    if r64[got] >= r64[want] * (1 - RATIO_TOL[fmt]):
        tally.allowed += 1
        return None
    return f"winner {got} (ratio {r64[got]:.6g}), the reference draws {want} (ratio {r64[want]:.6g})"


def judge(model: DrawModel, cb, last, rows: List[Row], got, tally: Optional[Tally] = None) -> List[Flag]:
    """Every field of a launch of len(rows) rows against the restatement.  got: the dict ARHipEngine.test_draw returns."""
    tally = tally or Tally()
    fl: List[Flag] = []
    M, R, cap, MB, fmt = len(rows), model.R, model.cap, model.MB, model.fmt
    V = model.width(cb)
    what, path = got["what"], got["what"] & 3
    want_path = 0 if V <= 1024 else 2 if fmt == "bf16" else 1
    if path != want_path:
        fl.append(Flag(-1, "path", f"path {path}, expected {want_path}"))
    fe = model.fast_emb
    Df = fe.shape[1]
    col = 0 if cb == 0 else cb + 1
    for m, row in enumerate(rows):
        ref = row.ref
        add = lambda f, msg: fl.append(Flag(m, f, msg))
        # ---- the winner
        tokn = got["tokn"][m]
        w = int(tokn[col])
        why = expect_winner(model, cb, row, w, tally)
        if why:
            add("winner", why)
        w = min(max(w, 0), V - 1)
        # ---- the frame under construction
        code = w
        want_tokn = np.full(R, SENT, dtype=np.int64)
        if cb == 0:
            code = min(max(w - model.sem_begin, 0), model.cbsize - 1)
            want_tokn[0], want_tokn[1] = w, code
        else:
            want_tokn[cb + 1] = w
        if not np.array_equal(tokn, want_tokn):
            add("tokn", f"{tokn.tolist()} expected {want_tokn.tolist()}")
        # ---- the logits row left behind
        if path != 0 and not np.array_equal(got["logits"][m].view(np.uint32), ref.after.view(np.uint32)):
            bad = np.flatnonzero(got["logits"][m].view(np.uint32) != ref.after.view(np.uint32))
            add("logits", f"{len(bad)} logits differ from the penalised row, first at {bad[:6].tolist()}")
        if path == 0 and not np.array_equal(got["logits"][m].view(np.uint32), np.asarray(row.logits, dtype=np.float32).view(np.uint32)):
            add("logits", "sample_small_kernel wrote its logits row")
        # ---- embedding row and its 16-bit copy
        if not np.array_equal(got["femb"][m].view(np.uint32), fe[code].view(np.uint32)):
            add("femb", f"not the embedding row of code {code}")
        if what & 12:
            xo = got["xo_x" if what & 8 else "xo_femb"]
            r0 = m + (model.xo_pair if what & 8 else 0)
            if not np.array_equal(xo[:, r0, :].reshape(-1)[:Df], bits16(fe[code], fmt)):
                add("xo", f"octet-major row {r0} is not the 16-bit pattern of the embedding row of code {code}")
        # ---- the table row
        if what & 16:
            n = model.qkv0_tab.shape[1]
            want_q = torch.from_numpy(model.qkv0_tab[code].view(np.int16).copy()).view(DT[fmt]).to(torch.float32).numpy()
            if not np.array_equal(got["qkvf"].reshape(-1)[m * n:(m + 1) * n].view(np.uint32), want_q.view(np.uint32)):
                add("qkv0", f"not table row {code}")
        # ---- frame finalisation
        frozen = row.done != 0
        want_tok = want_tokn if last else np.full(R, SENT, dtype=np.int64)
        if not np.array_equal(got["tok"][m], want_tok):
            add("tok", f"{got['tok'][m].tolist()} expected {want_tok.tolist()}")
        want_seq = np.array(row.hist, dtype=np.int64).reshape(R, cap)
        adv = last and not frozen
        if adv and row.nf < cap:
            want_seq[:, row.nf] = want_tokn
        if not np.array_equal(got["seq"][m], want_seq):
            cols = np.flatnonzero((got["seq"][m] != want_seq).any(axis=0))
            add("seq", f"history columns {cols[:6].tolist()} differ (nf {row.nf}, cap {cap})")
        want_done = 1 if adv and int(want_tokn[0]) == model.im_end else row.done
        for name, wv in (("pos", row.pos + (1 if adv else 0)), ("nf", row.nf + (1 if adv else 0)), ("done", want_done)):
            if int(got[name][m]) != wv:
                add(name, f"{int(got[name][m])} expected {wv}")
        # ---- the large draw's record
        if path == 2:
            nchunk = (V + 1023) // 1024
            cw = got["cut"][m]
            kstar, nk, all_kept = int(cw[0]), int(cw[1].view(np.int32)), int(cw[2].view(np.int32))
            Lmax, Mt, Tc = (float(cw[i:i + 1].view(np.float32)[0]) for i in (4, 5, 7))
            k16 = (order_key(ref.after) >> np.uint32(16)).astype(np.int64)
            cc = got["chunk_cnt"][m * nchunk:(m + 1) * nchunk]
            if all_kept:
                n_kept, members = V, 0
            else:
                members = int((k16 == kstar).sum())
                n_kept = int((k16 > kstar).sum()) + nk
                if members == 0 or not 0 <= nk <= members:
                    add("cut", f"class {kstar:#x} holds {members} logits, nk {nk}")
            if not ref.lo <= n_kept <= ref.hi:
                add("cut", f"keeps {n_kept} ranks (class {kstar:#x}, nk {nk}, all_kept {all_kept}); the band is {ref.lo}..{ref.hi}")
            if int(cc.sum()) != (int((k16 == kstar).sum())):
                add("chunk_cnt", f"sums to {int(cc.sum())}, class {kstar:#x} holds {int((k16 == kstar).sum())}")
            if Lmax != ref.Lmax or np.float32(Mt) != ref.Mt or np.float32(Tc) != ref.Tc:
                add("cut", f"Lmax {Lmax} Mt {Mt} Tc {Tc}, expected {ref.Lmax} {ref.Mt} {ref.Tc}")
        tally.widest_band = max(tally.widest_band, ref.band)
    # ---- nothing else was written
    def intact(name, a, fill):
        a = np.asarray(a)
        if a.size and not bool((a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16) == fill).all()):
            fl.append(Flag(-1, "sentinel:" + name, "written outside the launch's rows"))
    for name in ("tokn", "tok", "seq", "pos", "nf", "done"):
        intact(name, got[name][M:], SENT)
    intact("femb", got["femb"][M:], FILL32)
    intact("logits", got["logits"][M:], FILL32)
    if got.get("xo_femb") is not None:
        for name, used, r0 in (("xo_femb", what & 4, 0), ("xo_x", what & 8, model.xo_pair)):
            a = got[name].copy()
            if used:
                a[: (Df + 7) // 8, r0: r0 + M, :] = FILL16
            intact(name, a, FILL16)
    q = got["qkvf"].reshape(-1).view(np.uint32).copy()
    if what & 16:
        q[: M * model.qkv0_tab.shape[1]] = FILL32
    intact("qkvf", q, FILL32)
    if path == 2:
        nchunk = (V + 1023) // 1024
        intact("cut", got["cut"][M:], FILL32)
        intact("chunk_cnt", got["chunk_cnt"][M * nchunk:], FILL32)
        intact("part_idx", got["part_idx"][M * nchunk:], FILL32)
    else:
        for name in ("cut", "chunk_cnt", "part_idx"):
            intact(name, got[name], FILL32)
    return fl


# ------------------------------------------------------------------------------------------------------------ input families
SPREADS = (0.3, 1.0, 3.0, 8.0)
CONTROLS = ((0.8, 0.7, 1.1), (0.2, 1.0, 1.5), (0.95, 0.1, 1.1), (1e-6, 0.7, 1.2), (1.0, 1.3, 1.0))      # (top_p, T, rep)


def family_logits(fmt, V, spread, seed, variant="plain", top_p=0.8):
    """Seeded logits of one family, values exact in fmt.  variant: "plain"; "top3": three exact ties at the top; "cut40": 40
    equal logits where the top-p cut of `top_p` falls; "big": one class of more than 65535 members far below every cut."""
    g = torch.Generator().manual_seed(seed)
    lg = (spread * torch.randn(V, generator=g)).to(DT[fmt])
    if variant == "top3" and V >= 8:
        lg[torch.randperm(V, generator=g)[:3]] = lg.max()
    if variant == "big":
        lg[:70000] = lg.min() - 1
    if variant == "cut40" and V >= 64:
        srt, _ = torch.sort(lg, descending=True)
        c = np.cumsum(F.softmax(srt.to(torch.float64), dim=-1).numpy())
        r = min(int((c <= top_p).sum()), V - 1)
        lg[torch.randperm(V, generator=g)[:40]] = srt[r]
    return lg.to(torch.float32).numpy()


def random_hist(model: DrawModel, seed):
    """A history block of plausible ids: row 0 vocabulary ids, rows 1.. codes below 1024, some outside the fast vocabulary."""
    g = np.random.default_rng(seed)
    h = g.integers(0, 1024, size=(model.R, model.cap)).astype(np.int32)
    h[0] = g.integers(0, model.V, size=model.cap)
    return h


def pick_ids(logits, n_ids, top_p, g, V=None):
    """Window ids that matter: ids among the 32 likeliest tokens, one random id twice, and at the END the last (up to three) tokens the unpenalised row
    would keep, which the penalty moves across the cut (a positive logit shrinks, a negative one grows in size)."""
    V = len(logits) if V is None else V
    order = np.lexsort((np.arange(len(logits)), -logits.astype(np.float64)))
    ex = np.exp(logits[order].astype(np.float64) - float(logits[order[0]]))
    n = max(1, int((np.cumsum(ex / ex.sum()) <= top_p).sum()))
    cross = order[max(n - 3, 0):n]
    near = order[: min(32, len(order))]                                   # likely tokens (a history holds drawn tokens): their
    ids = near[g.integers(0, len(near), size=n_ids)]                       # probes stay valid at a low temperature and in fp16
    ids[0] = ids[1] = g.integers(0, V)                                     # an unlikely token, twice
    ids[n_ids - len(cross):] = cross
    return ids
