"""The stereo mix stage restated in numpy (include/fishtts_hip.h: "Stereo mix"), on tests/mix_ref.py, tests/level_ref.py and
tests/intake_ref.py: the pan table, the region lookup, the side selection, the pair measure over two sides at 44.1 kHz, and
the stage from the timeline onward - the two sides arrive as arrays at the output rate, so everything behind the bed's
preparation is compared bit for bit.  The activity, D_k and g_k come from the mono programme through mix_ref's own functions;
the sample rule is mix_ref.mix's, written once more because it runs per channel over a panned programme with the mono duck."""
from typing import NamedTuple, Optional

import numpy as np

from tests import level_ref as LR
from tests import mix_ref as MR

MAX_PAN = 100
MAX_REGIONS = 4096


def pan_gains() -> np.ndarray:
    """U[j] = (float) min(1, sqrt(2) sin(j pi / 400)), j = 0 .. 200: float64 rounded once; U[0] = 0, U[j] = 1 from 100 on."""
    j = np.arange(2 * MAX_PAN + 1, dtype=np.float64)
    U = np.minimum(1.0, np.sqrt(2.0) * np.sin(j * np.pi / 400.0)).astype(np.float32)
    U[0] = 0.0
    U[MAX_PAN:] = 1.0
    return U


def gains_of(q):
    """(left, right) gains of pans q (hundredths, -100 hard left): U[100 - q], U[100 + q]."""
    q = np.asarray(q, dtype=np.int64)
    U = pan_gains()
    return U[MAX_PAN - q], U[MAX_PAN + q]


def check_regions(regions, n: int) -> Optional[str]:
    """None, or why the table is refused - in the stage's order."""
    if not 0 <= len(regions) <= MAX_REGIONS:
        return "R"
    at = 0
    for a, e, pan in regions:
        if a < at or a >= e or e > n:
            return "place"
        if not -MAX_PAN <= pan <= MAX_PAN:
            return "pan"
        at = e
    return None


def region_pans(regions, n: int) -> np.ndarray:
    """q over the programme's samples 0 .. n - 1: the pan of the region that holds the sample, 0 where none does."""
    assert check_regions(regions, n) is None
    q = np.zeros(n, dtype=np.int64)
    for a, e, pan in regions:
        q[a:e] = pan
    return q


def sides(channel: int, channels: int):
    """The channels of the bed's two sides: channel = -1 takes 0 and 1 (a mono file: 0 twice), channel = k takes k twice."""
    if channel == -1:
        return 0, (1 if channels >= 2 else 0)
    return channel, channel


def pair_measure(s0, s1, target: int = 0, rate: int = 44100) -> LR.Ref:
    """The pair level over two sides of equal length: e_h = e_h(side 0) + e_h(side 1), p the larger peak, then level_ref's
    blocks, gates and gain as for one item of that length."""
    s0, s1 = (np.asarray(s, dtype=np.float32).reshape(-1) for s in (s0, s1))
    assert len(s0) == len(s1)
    H = LR.hop(rate)
    e = LR.hop_sums(LR.kweight(s0, rate), H) + LR.hop_sums(LR.kweight(s1, rate), H)
    r = LR.gate(e, len(s0), H)
    p = np.float32(max(np.max(np.abs(s0)), np.max(np.abs(s1)))) if len(s0) else np.float32(0)
    g, capped = LR.gain(r.L, p, target)
    return LR.Ref(r.L, p, g, r.blocks, r.gated, capped, r.margin, e)


class Stereo(NamedTuple):
    y: np.ndarray          # float32 [N, 2]
    D: np.ndarray          # int32 [Nh + 1]
    act: np.ndarray        # bool [Nh]
    N: int
    Nh: int
    H: int
    dmax: int
    pk: np.float32
    sg: np.float32
    capped: bool
    m: np.ndarray          # [N, 2] before the ceiling
    s: np.ndarray          # [N, 2] the panned programme on the timeline


def mix(x, bed0, bed1, regions, rate: int, p: MR.Params, ceiling: float = MR.CEILING) -> Stereo:
    """The stage.  bed0, bed1: the two sides at the output rate (the same array where they are one), or None, None."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = len(x)
    N, H = p.lead + n + p.tail, MR.hop(rate)
    Nh = -(-N // H)
    left, right = gains_of(region_pans(regions, n))
    one = np.float32(1.0)
    if bed0 is None:
        mono, _ = MR.timeline(x, [one], p)
        beds = [np.zeros(N, dtype=np.float32)] * 2
    else:
        mono, b0 = MR.timeline(x, bed0, p)
        beds = [b0, MR.timeline(x, bed1, p)[1]]
    act = MR.activity(mono, H, p.threshold)
    D = MR.duck(act, p.depth, p.attack, p.release)
    g = MR.gains()[D]
    i = np.arange(N, dtype=np.int64)
    k, j = i // H, i % H
    r = j.astype(np.float32) / np.float32(H)
    gd = MR.fmaf32(r, (g[k + 1] - g[k]).astype(np.float32), g[k])
    f_in, f_out = min(p.fade_in, N // 2), min(p.fade_out, N // 2)
    s = np.zeros((N, 2), dtype=np.float32)
    m = np.zeros((N, 2), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, pc in enumerate((left, right)):
            s[p.lead:p.lead + n, c] = (x * pc).astype(np.float32)
            t = beds[c].copy()
            if f_in > 0:
                t[:f_in] = t[:f_in] * MR.ramp(i[:f_in], f_in)
            if f_out > 0:
                t[N - f_out:] = t[N - f_out:] * MR.ramp(N - 1 - i[N - f_out:], f_out)
            u = (t * gd).astype(np.float32)
            m[:, c] = (s[:, c] + u).astype(np.float32)
        a = np.abs(m)
    a = a[~np.isnan(a)]
    pk = np.float32(a.max()) if len(a) else np.float32(0.0)
    capped = float(pk) > ceiling
    sg = np.float32(ceiling / float(pk)) if capped else np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (m * sg).astype(np.float32) if capped else m
    return Stereo(y, D, act, N, Nh, H, int(D.max()), pk, sg, bool(capped), m, s)
