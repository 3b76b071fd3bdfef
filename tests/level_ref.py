"""The level stage (include/fishtts_hip.h: "Level") restated in float64 on the host: the K-weighting design at any rate, the
plain serial recursion from zero state at sample 0, the hop sums, the 400 ms blocks, the two gates and the gain.  measure()
also returns the gate margin - the smallest distance of any block's loudness from either gate - so that a test can require
inputs whose blocks cannot change sides through rounding."""
from dataclasses import dataclass

import numpy as np

SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416)     # f0, G (dB), Q, the exponent of Vb
HIGHPASS = (38.13547087602444, 0.5003270373238773)                                         # f0, Q
CEILING = 10.0 ** (-1.0 / 20.0)      # -1 dBFS on the sample peak
ABS_GATE = -70.0
RATES = (8000, 11025, 16000, 44100, 48000)

# ITU-R BS.1770-4, table 1 and table 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def design(rate: int) -> np.ndarray:
    """The ten coefficients at `rate`: the shelf's b0 b1 b2 a1 a2, then the high-pass's."""
    f0, G, Q, vbe = SHELF
    K = np.tan(np.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** vbe
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = HIGHPASS
    K = np.tan(np.pi * f0 / rate)
    d = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]
    return np.array(shelf + hp, dtype=np.float64)


def hop(rate: int) -> int:
    return rate // 10


def _biquad(x: np.ndarray, c) -> np.ndarray:
    """y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2], serially, from zero state."""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    try:
        from scipy.signal import lfilter          # the same recursion (transposed direct form II, float64), compiled
        return lfilter([b0, b1, b2], [1.0, a1, a2], x)
    except ImportError:
        y = np.zeros(len(x), dtype=np.float64)
        s1 = s2 = 0.0
        for i, v in enumerate(x.tolist()):
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            y[i] = o
        return y


def kweight(x: np.ndarray, rate: int) -> np.ndarray:
    c = design(rate)
    return _biquad(_biquad(np.asarray(x, dtype=np.float64), c[:5]), c[5:])


def hop_sums(z: np.ndarray, H: int) -> np.ndarray:
    """e_h over [h H, min((h + 1) H, n)), h < ceil(n / H): the whole hops, then what is left of the item."""
    n = len(z)
    return np.array([float(np.sum(z[h * H:min((h + 1) * H, n)] ** 2)) for h in range((n + H - 1) // H)], dtype=np.float64)


def lufs(E):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(E)


@dataclass
class Gated:
    L: float            # integrated loudness, -inf when nothing was measured
    blocks: int
    gated: int
    margin: float       # smallest |l_j - (-70)| and |l_j - Gamma| over all blocks (inf without blocks / without a Gamma)


def gate(e: np.ndarray, n: int, H: int) -> Gated:
    """Blocks and gates over the hop sums e (hop_sums' layout) of an item of n samples."""
    if n < 1:
        return Gated(-np.inf, 0, 0, np.inf)
    whole = n // H
    if whole < 4:
        E = np.array([np.sum(e) / n], dtype=np.float64)
    else:
        E = np.array([(e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * H) for j in range(whole - 3)], dtype=np.float64)
    l = lufs(E)
    margin = float(np.min(np.abs(l - ABS_GATE)))
    keep = l > ABS_GATE
    if not np.all(np.isfinite(E)) or not keep.any():
        return Gated(-np.inf, len(E), 0, margin)
    gamma = float(lufs(np.mean(E[keep]))) - 10.0
    margin = min(margin, float(np.min(np.abs(l - gamma))))
    keep2 = keep & (l > gamma)
    if not keep2.any():
        return Gated(-np.inf, len(E), 0, margin)
    return Gated(float(lufs(np.mean(E[keep2]))), len(E), int(keep2.sum()), margin)


def gain(L: float, p: float, target: int):
    """(g as float32, whether the ceiling bound it) for loudness L, peak p and a target in hundredths of a LUFS (0: none)."""
    if target == 0 or not np.isfinite(L):
        return np.float32(1.0), False
    g = 10.0 ** ((target / 100.0 - L) / 20.0)
    capped = bool(p > 0 and CEILING / float(p) < g)
    if capped:
        g = CEILING / float(p)
    return np.float32(g), capped


@dataclass
class Ref:
    L: float
    p: np.float32
    g: np.float32
    blocks: int
    gated: int
    capped: bool
    margin: float
    e: np.ndarray


def measure(x: np.ndarray, rate: int, target: int = 0) -> Ref:
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    H = hop(rate)
    e = hop_sums(kweight(x, rate), H)
    r = gate(e, len(x), H)
    p = np.float32(np.max(np.abs(x))) if len(x) else np.float32(0)
    g, capped = gain(r.L, p, target)
    return Ref(r.L, p, g, r.blocks, r.gated, capped, r.margin, e)
