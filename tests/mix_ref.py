"""The mix stage restated in numpy (include/fishtts_hip.h: "Mix"), from the timeline onward: the bed arrives as an array at
the output rate, so everything behind the bed's preparation is compared bit for bit.  Integers for D_k, float32 operations
one at a time for the sample rule (numpy rounds every float32 operation on its own), float64 for T and sg.

`knock` takes one rule out, so that tests/test_mix_ref_host.py can show each is caught:
  "behind"    the behind term counts from k instead of k - 1 (the off-by-one)
  "fma"       u and the sum contracted into one multiply-add (one rounding instead of two)
  "ceiling"   the ceiling applied when pk == c too"""
from typing import NamedTuple, Optional

import numpy as np

MAX_DEPTH = 6000
CEILING = 10.0 ** (-1.0 / 20.0)


class Params(NamedTuple):
    depth: int = 1200
    threshold: float = 10.0 ** (-45.0 / 20.0)
    attack: int = 15
    release: int = 40
    lead: int = 0
    tail: int = 0
    fade_in: int = 0
    fade_out: int = 0
    offset: int = 0
    loop: int = 1


class Mixed(NamedTuple):
    y: np.ndarray          # float32 [N]
    D: np.ndarray          # int32 [Nh + 1]
    act: np.ndarray        # bool [Nh]
    N: int
    Nh: int
    H: int
    dmax: int
    pk: np.float32
    sg: np.float32
    capped: bool
    m: np.ndarray          # the samples before the ceiling
    gd: np.ndarray         # the interpolated gain per sample


def hop(rate: int) -> int:
    return rate // 50


def gains() -> np.ndarray:
    """T[d] = (float) 10^(-d / 2000): a float64 power rounded once."""
    return np.power(10.0, -np.arange(MAX_DEPTH + 1, dtype=np.float64) / 2000.0).astype(np.float32)


def duck(act, depth: int, Wa: int, Wr: int, knock: Optional[str] = None) -> np.ndarray:
    """D_k, k = 0 .. Nh, by the stated rule as it is written: every active hop of either window, python integers."""
    act = np.asarray(act, dtype=bool)
    Nh = len(act)
    D = np.zeros(Nh + 1, dtype=np.int32)
    shift = 0 if knock == "behind" else 1
    for k in range(Nh + 1):
        d = 0
        for h in range(max(0, k), min(Nh, k + Wa)):
            if act[h]:
                d = max(d, depth * (Wa - (h - k)) // Wa)
        for h in range(max(0, k - Wr), min(Nh, k - shift + 1)):
            if act[h]:
                d = max(d, depth * (Wr - (k - shift - h)) // Wr)
        D[k] = d
    return D


def timeline(x, bed, p: Params):
    """(s, b): the programme and the bed over the N samples of the timeline."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    bed = np.asarray(bed, dtype=np.float32).reshape(-1)
    n, nb = len(x), len(bed)
    assert n >= 1 and nb >= 1
    N = p.lead + n + p.tail
    s = np.zeros(N, dtype=np.float32)
    s[p.lead:p.lead + n] = x
    j = np.arange(N, dtype=np.int64) + p.offset
    if p.loop:
        b = bed[j % nb]
    else:
        b = np.where(j < nb, bed[np.minimum(j, nb - 1)], np.float32(0.0)).astype(np.float32)
    return s, b


def activity(s, H: int, threshold) -> np.ndarray:
    """act_h: some sample of the hop reaches the threshold, compared in float32; a NaN never does."""
    thr = np.float32(threshold)
    N = len(s)
    Nh = -(-N // H)
    with np.errstate(invalid="ignore"):
        loud = np.abs(s) >= thr
    pad = np.zeros(Nh * H, dtype=bool)
    pad[:N] = loud
    return pad.reshape(Nh, H).any(axis=1)


def ramp(j, f: int) -> np.ndarray:
    return ((2.0 * np.asarray(j, dtype=np.float64) + 1.0) / (2.0 * float(f))).astype(np.float32)


def fmaf32(a, b, c) -> np.ndarray:
    """fmaf on float32 arrays: a b + c rounded once.  The product of two float32 values is exact in float64; the float64 sum
    s rounds once more, with the exact error e from the two-sum.  Rounding s to float32 then gives the fused result unless s
    lies exactly half-way between two float32 values while e is not zero: there e decides the side (a half-way point is a
    float64, and rounding to float64 is monotonic, so in every other case s lies on the exact value's side of it)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    y = s.astype(np.float32)
    y64 = y.astype(np.float64)
    other = np.nextafter(y, np.where(s > y64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tie = (s != y64) & (np.abs(s - y64) == np.abs(other - s)) & (e != 0)
        up = np.maximum(y64, other).astype(np.float32)
        dn = np.minimum(y64, other).astype(np.float32)
    return np.where(tie, np.where(e > 0, up, dn), y).astype(np.float32)


def mix(x, bed, rate: int, p: Params, knock: Optional[str] = None, ceiling: float = CEILING) -> Mixed:
    """The stage.  `ceiling`: c, for the host test alone - 10^(-1/20) is no float32, so pk == c needs a c that is one."""
    s, b = timeline(x, bed, p)
    N, H = len(s), hop(rate)
    Nh = -(-N // H)
    act = activity(s, H, p.threshold)
    D = duck(act, p.depth, p.attack, p.release, knock)
    g = gains()[D]
    i = np.arange(N, dtype=np.int64)
    k, j = i // H, i % H
    r = j.astype(np.float32) / np.float32(H)
    gd = fmaf32(r, (g[k + 1] - g[k]).astype(np.float32), g[k])
    t = b.copy()
    f_in, f_out = min(p.fade_in, N // 2), min(p.fade_out, N // 2)
    if f_in > 0:
        t[:f_in] = t[:f_in] * ramp(i[:f_in], f_in)
    if f_out > 0:
        t[N - f_out:] = t[N - f_out:] * ramp(N - 1 - i[N - f_out:], f_out)
    with np.errstate(invalid="ignore", over="ignore"):
        if knock == "fma":
            m = fmaf32(t, gd, s)
        else:
            u = (t * gd).astype(np.float32)
            m = (s + u).astype(np.float32)
        a = np.abs(m)
    a = a[~np.isnan(a)]
    pk = np.float32(a.max()) if len(a) else np.float32(0.0)
    capped = float(pk) >= ceiling if knock == "ceiling" else float(pk) > ceiling
    sg = np.float32(ceiling / float(pk)) if capped else np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (m * sg).astype(np.float32) if capped else m
    return Mixed(y, D, act, N, Nh, H, int(D.max()), pk, sg, bool(capped), m, gd)
