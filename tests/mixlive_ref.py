"""The live mix stage restated in numpy (include/fishtts_hip.h: "Live mix") on top of tests/mix_ref.py: the timeline, the
activity, the duck, the table and the ramps are Mix's and are imported; the fades without Mix's N / 2 clamps, the hop peaks,
need_h, the limiter nodes L_k, the output and what a stream has emitted after n_in samples are written here.  Integers for
need and L_k, float32 operations one at a time for the samples.

`knock` takes one rule out, so that tests/test_mixlive_ref_host.py can show each is caught:
  "need"      need_h found with < for <=
  "behind"    the release cone counts from k instead of k - 1 (the off-by-one)
  "nearest"   only the nearest hop of a window that needs anything counts, as in the duck
  "fade"      Mix's N / 2 clamp on both fades kept"""
from typing import NamedTuple, Optional

import numpy as np

from tests.mix_ref import Params, activity, duck, fmaf32, gains, hop, ramp, timeline

LA, LR = 5, 25
MAX_FADE = 1 << 30
CF = np.float32(10.0 ** (-1.0 / 20.0))


class Live(NamedTuple):
    y: np.ndarray          # float32 [N]
    m: np.ndarray          # the samples before the limiter
    D: np.ndarray          # int32 [Nh + 1]
    L: np.ndarray          # int32 [Nh + 1]
    act: np.ndarray        # bool [Nh]
    need: np.ndarray       # int32 [Nh]
    Q: np.ndarray          # float32 [Nh]
    N: int
    Nh: int
    H: int


def lay(x, bed, p: Params):
    """mix_ref.timeline, and an empty programme too (b(i) does not depend on the programme)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if len(x):
        return timeline(x, bed, p)
    N = p.lead + p.tail
    return np.zeros(N, dtype=np.float32), timeline(np.zeros(1, dtype=np.float32), bed, p)[1][:N]


def premix(x, bed, rate: int, p: Params, knock: Optional[str] = None):
    """(m, D, act): Mix's sample rule up to its ceiling, with the live stage's fades."""
    s, b = lay(x, bed, p)
    N, H = len(s), hop(rate)
    act = activity(s, H, p.threshold)
    D = duck(act, p.depth, p.attack, p.release)
    g = gains()[D]
    i = np.arange(N, dtype=np.int64)
    k, j = i // H, i % H
    r = j.astype(np.float32) / np.float32(H)
    gd = fmaf32(r, (g[k + 1] - g[k]).astype(np.float32), g[k])
    t = b.copy()
    f_in, f_out = min(p.fade_in, MAX_FADE), min(p.fade_out, MAX_FADE)
    if knock == "fade":
        f_in, f_out = min(p.fade_in, N // 2), min(p.fade_out, N // 2)
    a = i < f_in
    t[a] = t[a] * ramp(i[a], max(f_in, 1))
    z = i >= N - f_out
    t[z] = t[z] * ramp(N - 1 - i[z], max(f_out, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        u = (t * gd).astype(np.float32)
        m = (s + u).astype(np.float32)
    return m, D, act


def hop_peaks(m, H: int) -> np.ndarray:
    """Q_h: the largest |m| of the hop that is not a NaN, 0 for a hop of NaNs."""
    N = len(m)
    Nh = -(-N // H)
    a = np.abs(m)
    a[np.isnan(a)] = 0.0
    pad = np.zeros(Nh * H, dtype=np.float32)
    pad[:N] = a
    return pad.reshape(Nh, H).max(axis=1) if Nh else np.zeros(0, dtype=np.float32)


def needs(Q, knock: Optional[str] = None) -> np.ndarray:
    """need_h: the smallest d with T[d] Q_h <= cf in float32, 6000 where there is none."""
    T = gains()
    out = np.zeros(len(Q), dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h, q in enumerate(np.asarray(Q, dtype=np.float32)):
            prod = (T * q).astype(np.float32)
            ok = prod < CF if knock == "need" else prod <= CF
            out[h] = int(np.argmax(ok)) if ok.any() else len(T) - 1
    return out


def limit(need, knock: Optional[str] = None) -> np.ndarray:
    """L_k, k = 0 .. Nh, by the stated rule as it is written: every hop of either window, python integers."""
    need = [int(v) for v in need]
    Nh = len(need)
    L = np.zeros(Nh + 1, dtype=np.int32)
    shift = 0 if knock == "behind" else 1
    for k in range(Nh + 1):
        ahead = list(range(max(0, k), min(Nh, k + LA)))
        behind = list(range(min(Nh, k - shift + 1) - 1, max(0, k - LR) - 1, -1))
        if knock == "nearest":
            ahead = [h for h in ahead if need[h] > 0][:1]
            behind = [h for h in behind if need[h] > 0][:1]
        l = 0
        for h in ahead:
            l = max(l, need[h] * (LA - (h - k)) // LA)
        for h in behind:
            l = max(l, need[h] * (LR - (k - shift - h)) // LR)
        L[k] = l
    return L


def live(x, bed, rate: int, p: Params, knock: Optional[str] = None) -> Live:
    """The stage over a whole programme: what any cutting of it into pushes gives."""
    m, D, act = premix(x, bed, rate, p, knock)
    N, H = len(m), hop(rate)
    Nh = -(-N // H)
    Q = hop_peaks(m, H)
    need = needs(Q, knock)
    L = limit(need, knock)
    l = gains()[L]
    i = np.arange(N, dtype=np.int64)
    k, j = i // H, i % H
    r = j.astype(np.float32) / np.float32(H)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (m * fmaf32(r, (l[k + 1] - l[k]).astype(np.float32), l[k])).astype(np.float32)
    return Live(y, m, D, L, act, need, Q, N, Nh, H)


def emitted(n_in: int, final: bool, rate: int, p: Params) -> int:
    """The samples a stream has emitted after n_in programme samples ("Emission")."""
    H = hop(rate)
    F = p.lead + n_in
    if final:
        return F + p.tail
    W = F // H
    E = F + p.tail - min(p.fade_out, MAX_FADE)
    Wm = min(max(0, W - p.attack), max(0, E) // H)
    return max(0, Wm - LA) * H


def held_bound(rate: int, p: Params) -> int:
    """The stage holds back fewer than this many samples of lead + n_in."""
    return (p.attack + LA + 2) * hop(rate) + max(0, min(p.fade_out, MAX_FADE) - p.tail)
