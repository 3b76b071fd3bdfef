"""The live stereo mix stage restated in numpy (include/fishtts_hip.h: "Live stereo mix") on top of tests/mixlive_ref.py -
premix (for the activity and the duck of the mono programme), hop_peaks, needs, limit, emitted - and tests/stereo_ref.py -
pan_gains, region_pans.  A stream is a list of pushes (x, regions), the regions relative to their push; what the stage gives
does not depend on the cutting, so the restatement lays the pushes end to end, finds q per programme sample, and runs the
sample rule per channel, the linked limiter over both.

`knock` takes one rule out, so that tests/test_stereolive_ref_host.py can show each is caught:
  "left"      Q_h from the left channel alone
  "unlinked"  a limiter per channel: need_h and L_k from each channel's own peaks
  "carry"     the pan of a carried sample lost: a programme sample not yet mixed when its push ends sits at 0 afterwards
  "swap"      left and right swapped
  "stream"    the regions of a push taken in the stream's coordinates instead of the push's"""
from typing import NamedTuple, Optional

import numpy as np

from tests import mix_ref as MR
from tests import mixlive_ref as ML
from tests import stereo_ref as SR


class LiveStereo(NamedTuple):
    y: np.ndarray          # float32 [N, 2]
    m: np.ndarray          # [N, 2] before the limiter
    D: np.ndarray          # int32 [Nh + 1]
    L: np.ndarray          # int32 [Nh + 1]
    act: np.ndarray        # bool [Nh]
    need: np.ndarray       # int32 [Nh]
    Q: np.ndarray          # float32 [Nh]
    q: np.ndarray          # int64 [n]: the pan of every programme sample
    N: int
    Nh: int
    H: int


def carried_from(n_in: int, rate: int, p: MR.Params) -> int:
    """The first programme sample a stream still carries, not yet mixed, after n_in samples (not final)."""
    H = MR.hop(rate)
    F = p.lead + n_in
    W = F // H
    E = F + p.tail - min(p.fade_out, ML.MAX_FADE)
    Wm = min(max(0, W - p.attack), max(0, E) // H)                        # ("Emission": the hops that have their m)
    return min(max(Wm * H, p.lead), F) - p.lead


def pans_of(pushes, rate: int, p: MR.Params, knock: Optional[str] = None) -> np.ndarray:
    """q over the concatenated programme."""
    n = sum(len(x) for x, _ in pushes)
    q = np.zeros(n, dtype=np.int64)
    at = 0
    for j, (x, regions) in enumerate(pushes):
        k = len(x)
        if knock == "stream":
            for a, e, pan in regions:
                q[min(a, n):min(e, n)] = pan
        else:
            q[at:at + k] = SR.region_pans(regions, k)
        at += k
        if knock == "carry" and j < len(pushes) - 1:
            q[carried_from(at, rate, p):at] = 0
    return q


def live(pushes, bed0, bed1, rate: int, p: MR.Params, knock: Optional[str] = None) -> LiveStereo:
    """The stage over a stream.  bed0, bed1: the two sides at the output rate (the same array where they are one), or None,
    None."""
    pushes = [(np.asarray(x, dtype=np.float32).reshape(-1), [tuple(r) for r in regions]) for x, regions in pushes]
    x = np.concatenate([x for x, _ in pushes] + [np.zeros(0, dtype=np.float32)])
    n, H = len(x), MR.hop(rate)
    q = pans_of(pushes, rate, p, knock)
    left, right = SR.gains_of(q)
    if knock == "swap":
        left, right = right, left
    zero = np.zeros(1, dtype=np.float32)
    _, D, act = ML.premix(x, zero if bed0 is None else bed0, rate, p)
    N = p.lead + n + p.tail
    Nh = -(-N // H)
    beds = [np.zeros(N, dtype=np.float32)] * 2 if bed0 is None else [ML.lay(x, b, p)[1] for b in (bed0, bed1)]
    g = MR.gains()[D]
    i = np.arange(N, dtype=np.int64)
    k, j = i // H, i % H
    r = j.astype(np.float32) / np.float32(H)
    gd = MR.fmaf32(r, (g[k + 1] - g[k]).astype(np.float32), g[k]) if N else np.zeros(0, dtype=np.float32)
    f_in, f_out = min(p.fade_in, ML.MAX_FADE), min(p.fade_out, ML.MAX_FADE)
    a, z = i < f_in, i >= N - f_out
    m = np.zeros((N, 2), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, pc in enumerate((left, right)):
            s = np.zeros(N, dtype=np.float32)
            s[p.lead:p.lead + n] = (x * pc).astype(np.float32)
            t = beds[c].copy()
            t[a] = t[a] * MR.ramp(i[a], max(f_in, 1))
            t[z] = t[z] * MR.ramp(N - 1 - i[z], max(f_out, 1))
            u = (t * gd).astype(np.float32)
            m[:, c] = (s + u).astype(np.float32)
    Qc = [ML.hop_peaks(m[:, c], H) for c in (0, 1)]
    Q = Qc[0] if knock == "left" else np.maximum(Qc[0], Qc[1])
    need = ML.needs(Q)
    L = ML.limit(need)
    T = MR.gains()
    y = np.zeros((N, 2), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in (0, 1):
            l = T[ML.limit(ML.needs(Qc[c]))] if knock == "unlinked" else T[L]
            y[:, c] = (m[:, c] * MR.fmaf32(r, (l[k + 1] - l[k]).astype(np.float32), l[k])).astype(np.float32) if N else 0
    return LiveStereo(y, m, D, L, act, need, Q, q, N, Nh, H)


def piece(x, regions, at: int, k: int):
    """The push (x[at : at + k], its regions): every region of the programme that meets the push, clipped to it and shifted to
    its coordinates."""
    return x[at:at + k], [(max(a, at) - at, min(e, at + k) - at, pan) for a, e, pan in regions if max(a, at) < min(e, at + k)]


def cut(x, regions, sizes):
    """The programme x with regions (a, e, pan) over it, as pushes of the given sizes."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    assert sum(sizes) == len(x)
    out, at = [], 0
    for k in sizes:
        out.append(piece(x, regions, at, k))
        at += k
    return out
