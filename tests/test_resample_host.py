"""Host checks of the resampler behind sample_rate= (include/fishtts_hip.h, ft_resample_filter / ft_resampled_len): rate
validation and L / M reduction, the designed filter's quality at every accepted rate, and a float64 numpy restatement of
the kernel's arithmetic (resample_ref, used by the GPU tests) checked against scipy.signal.resample_poly.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

FI = 44100
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 48000)


def _lib():
    from fish_tts_amd import _lib as L
    return L.load()


def filter_table(rate):
    """(L, M, K, w[L][K] float32) of ft_resample_filter; K = 0 (no table) at the codec's own rate."""
    lib = _lib()
    L, M, K = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.ft_resample_filter(rate, C.byref(L), C.byref(M), C.byref(K), None) == 0, rate
    w = np.zeros((L.value, max(K.value, 1)), dtype=np.float32)
    assert lib.ft_resample_filter(rate, None, None, None, w.ctypes.data_as(C.c_void_p)) == 0
    return L.value, M.value, K.value, w[:, :K.value]


def resample_ref(x, rate, table=None):
    """What the kernel computes, in float64: output n (u = n M, i0 = u // L, p = u % L) is
    sum_t w[p][t] x[i0 - K/2 + 1 + t], the input zero outside [0, len(x)); ceil(len(x) L / M) outputs."""
    L, M, K, w = table or filter_table(rate)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if K == 0:
        return x.copy()
    n_out = -(-len(x) * L // M)
    xp = np.concatenate([np.zeros(K), x, np.zeros(K)])
    w = w.astype(np.float64)
    out = np.empty(n_out)
    taps = np.arange(K)
    for a in range(0, n_out, 8192):
        n = np.arange(a, min(n_out, a + 8192), dtype=np.int64)
        u = n * M
        i0, p = u // L, u % L
        out[a:a + len(n)] = (w[p] * xp[(i0 - K // 2 + 1 + K)[:, None] + taps[None, :]]).sum(1)
    return out


def test_rate_reduction_and_lengths():
    lib = _lib()
    for rate in RATES + (FI,):
        L, M, K, w = filter_table(rate)
        g = math.gcd(rate, FI)
        assert (L, M) == (rate // g, FI // g)
        assert (K == 0) == (rate == FI) and K % 2 == 0
        for n in (0, 1, 2047, 2048, 215 * 2048):
            assert lib.ft_resampled_len(rate, n) == -(-n * L // M)
    assert lib.ft_resampled_len(16000, 215 * 2048) == 159754


@pytest.mark.parametrize("rate", [7999, 48001, 44099, 0, -16000, 1 << 20])
def test_refused_rates(rate):
    lib = _lib()
    L = C.c_int32(-5)
    assert lib.ft_resample_filter(rate, C.byref(L), None, None, None) == 1      # FT_ERR_ARG
    assert L.value == -5
    assert lib.ft_resampled_len(rate, 2048) == -1


@pytest.mark.parametrize("rate", RATES)
def test_filter_quality(rate):
    """The prototype rebuilt from the table (tap t of phase p sits at p + (K/2 - 1 - t) L): >= 70 dB stop band from
    0.5 Fmin, <= 0.01 dB pass band ripple up to 0.43 Fmin, measured on a dense grid."""
    L, M, K, w = filter_table(rate)
    proto = np.zeros(L * K)
    for t in range(K):
        proto[np.arange(L) + (K // 2 - 1 - t) * L + (K // 2) * L] = w[:, t]
    proto /= L                                  # gain L: the zero-stuffed input
    nf = 1 << int(math.ceil(math.log2(len(proto) * 64)))
    H = np.abs(np.fft.rfft(proto, nf))
    f = np.arange(len(H)) * (L * FI) / nf
    fmin = min(rate, FI)
    pb, sb = H[f <= 0.43 * fmin], H[f >= 0.5 * fmin]
    assert np.max(np.abs(20 * np.log10(pb))) <= 0.01, (rate, 20 * np.log10(pb.min()), 20 * np.log10(pb.max()))
    assert -20 * np.log10(sb.max()) >= 70.0, (rate, -20 * np.log10(sb.max()))


@pytest.mark.parametrize("rate", RATES)
def test_restatement_matches_resample_poly(rate):
    """Alignment (zero phase) and gain against an independent polyphase resampler, on tones at or below 0.25 Fmin."""
    from scipy.signal import resample_poly
    L, M, K, w = tab = filter_table(rate)
    n = 8192
    t = np.arange(n) / FI
    fmin = min(rate, FI)
    x = sum(0.3 * np.sin(2 * np.pi * f * t + ph) for f, ph in ((0.25 * fmin, 0.1), (0.11 * fmin, 1.3), (517.0, 2.0)))
    got = resample_ref(x, rate, tab)
    want = resample_poly(x, L, M)
    assert len(got) == len(want) == -(-n * L // M)
    edge = int(0.05 * len(got)) + K
    err = np.max(np.abs(got[edge:-edge] - want[edge:-edge]))
    assert err <= 5e-3, (rate, err)
