"""numpy restatement of the join stage (include/fishtts_hip.h: ft_codec_decode_join): edges by loud windows, the kept
margin, linear fades computed through float64 and applied as one float32 multiply, pieces laid out behind their gaps.
Every operation is the header's, in its order, so the device result has to equal this one bit for bit."""
import numpy as np


def edges(x, threshold, hop, keep):
    """(a, e) of one item: the cut positions, (0, 0) when no window is loud."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    with np.errstate(invalid="ignore"):
        loud = np.abs(x) >= np.float32(threshold)          # float32 compare; False for a NaN
    idx = np.flatnonzero(loud)
    if len(idx) == 0:
        return 0, 0
    first, last = int(idx[0]) // hop, int(idx[-1]) // hop
    return max(0, first * hop - keep), min(n, (last + 1) * hop + keep)


def piece(x, a, e, fade):
    """x[a:e] with the two ramps of f = min(fade, (e - a) // 2) samples."""
    y = np.array(np.asarray(x, dtype=np.float32)[a:e], dtype=np.float32)
    m = e - a
    f = min(int(fade), m // 2)
    if f > 0:
        j = np.arange(f, dtype=np.int64)
        ramp = ((2 * j + 1).astype(np.float64) / np.float64(2 * f)).astype(np.float32)
        y[:f] = y[:f] * ramp                     # i < f: ramp(i)
        y[m - f:] = y[m - f:] * ramp[::-1]       # i >= m - f: ramp(m - 1 - i)
    return y


def join(items, threshold, hop, keep, fade, gaps, started=0):
    """items: float32 arrays; gaps: one per item.  Returns (audio float32, cuts (B, 2) int64, started afterwards)."""
    out, cuts, s = [], np.zeros((len(items), 2), dtype=np.int64), bool(started)
    for b, x in enumerate(items):
        a, e = edges(x, threshold, hop, keep)
        cuts[b] = (a, e)
        if e - a == 0:
            continue
        if s:
            out.append(np.zeros(int(gaps[b]), dtype=np.float32))
        out.append(piece(x, a, e, fade))
        s = True
    audio = np.concatenate(out) if out else np.zeros(0, dtype=np.float32)
    return audio.astype(np.float32, copy=False), cuts, int(s)
