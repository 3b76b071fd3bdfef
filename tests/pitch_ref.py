"""Helpers of the pitch tests, restated from include/fishtts_hip.h (Pitch): the pitch stage in float64 on the library's
float32 table with the float32 summation bound of its kernel, and the time-scale stage of tests/test_timescale_host.py at a
rational rate num / den.  No test in here; no GPU."""
import ctypes as CT

import numpy as np

from tests.test_timescale_host import D, HS, N, WIN, _LPAD, _padded

SHIFT, PHASES, FRAC = 20, 512, 2048


def _lib():
    from fish_tts_amd import _lib as L
    return L.load()


def pitch_table(cents):
    """(S, K, w) through ft_pitch_filter: the step, the tap count and the float32 table w[513][K]."""
    lib = _lib()
    step, K = CT.c_int64(0), CT.c_int32(0)
    assert lib.ft_pitch_filter(int(cents), CT.byref(step), CT.byref(K), None) == 0, cents
    w = np.zeros((PHASES + 1, K.value), dtype=np.float32)
    assert lib.ft_pitch_filter(int(cents), None, None, w.ctypes.data_as(CT.c_void_p)) == 0
    return step.value, K.value, w


def rate_of(pct, cents):
    """(num, den) of the time-scale stage under a pitch shift: pct 2^20 / (100 S)."""
    return pct << SHIFT, 100 * pitch_table(cents)[0]


def pitch_coefs(w, u):
    """The interpolated coefficients of positions u (n S, 20 fractional bits) in float64: (i0, c[len(u)][K])."""
    u = np.asarray(u, dtype=np.int64)
    p = (u >> 11) & (PHASES - 1)
    f = ((u & (FRAC - 1)) / float(FRAC))[:, None]
    w64 = w.astype(np.float64)
    return u >> SHIFT, (1.0 - f) * w64[p] + f * w64[p + 1]


def pitch_ref(x, cents, n_out):
    """Outputs [0, n_out) of the pitch stage over x (zero outside) in float64 on the float32 table, and the per-sample
    bound of the kernel's float32 sum: (K + 4) 2^-24 sum_t |w_t x_t| + 1e-7 - a K-term float32 sum's bound with the
    interpolated coefficient's extra roundings (two products, one sum, the product with x)."""
    S, K, w = pitch_table(cents)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    last = ((n_out - 1) * S >> SHIFT) + K // 2 if n_out else 0
    xp = np.concatenate([np.zeros(K), x, np.zeros(max(0, last + 1 - len(x)))])
    y, bound = np.zeros(n_out), np.zeros(n_out)
    taps = np.arange(K)
    for a in range(0, n_out, 8192):
        n = np.arange(a, min(n_out, a + 8192), dtype=np.int64)
        i0, c = pitch_coefs(w, n * S)
        prod = c * xp[K + (i0 - K // 2 + 1)[:, None] + taps]
        y[a:a + len(n)] = prod.sum(axis=1)
        bound[a:a + len(n)] = (K + 4) * 2.0 ** -24 * np.abs(prod).sum(axis=1) + 1e-7
    return y, bound


def n_out_q(n, num, den):
    return -(-n * den // num)


def n_frames_q(n, num, den):
    return -(-n_out_q(n, num, den) // HS) + 1


def frame_scores_q(x, num, den, deltas):
    """test_timescale_host.frame_scores at the rate num / den."""
    xp = _padded(x)
    out = []
    s_prev = -HS + int(deltas[0])
    for k in range(1, len(deltas)):
        a = k * HS * num // den
        tpl = xp[_LPAD + s_prev + HS:_LPAD + s_prev + HS + N]
        reg = xp[_LPAD + a - HS - D:_LPAD + a + HS + D]
        out.append((np.correlate(reg, tpl, "valid"), np.correlate(np.abs(reg), np.abs(tpl), "valid")))
        s_prev = a - HS + int(deltas[k])
    return out


def timescale_ref_q(x, num, den, deltas=None, return_deltas=False):
    """test_timescale_host.timescale_ref at the rational rate num / den: a_k = floor(k HS num / den), ceil(len(x) den /
    num) samples."""
    n = len(x)
    n_out, K = n_out_q(n, num, den), n_frames_q(n, num, den)
    xp = _padded(x)
    y = np.zeros((K + 1) * HS)                 # position p lives at y[p + HS]
    ds = np.zeros(K, dtype=np.int64)
    s_prev = 0
    for k in range(K):
        a = k * HS * num // den
        if deltas is not None:
            d = int(deltas[k])
        elif k == 0:
            d = 0
        else:
            tpl = xp[_LPAD + s_prev + HS:_LPAD + s_prev + HS + N]
            reg = xp[_LPAD + a - HS - D:_LPAD + a + HS + D]
            d = int(np.argmax(np.correlate(reg, tpl, "valid"))) - D      # argmax: the first, so the lowest d
        assert -D <= d <= D and (k > 0 or d == 0)
        ds[k] = d
        s = a - HS + d
        y[k * HS:k * HS + N] += WIN * xp[_LPAD + s:_LPAD + s + N]
        s_prev = s
    y = y[HS:HS + n_out]
    return (y, ds) if return_deltas else y
