"""Host checks of the time-scale stage behind speed= (include/fishtts_hip.h, ft_timescaled_len): a float64 numpy
restatement of the algorithm stated there (timescale_ref, used by the GPU tests) checked on its own - lengths, tones,
exact ties - and the validation of speed values through the host-only calls.  No GPU."""
import math

import numpy as np
import pytest

FI = 44100
N, HS, D = 1024, 512, 384
PCTS = (50, 99, 101, 125, 200)
WIN = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N) / N))
_LPAD, _RPAD = HS + D + N, 4 * N + 2 * D


def _lib():
    from fish_tts_amd import _lib as L
    return L.load()


def n_out_of(n, pct):
    return -(-100 * n // pct)


def n_frames_of(n, pct):
    return -(-n_out_of(n, pct) // HS) + 1


def _padded(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return np.concatenate([np.zeros(_LPAD), x, np.zeros(_RPAD)])


def frame_scores(x, pct, deltas):
    """For every frame k >= 1, following the given d_k: (c, cabs), c[j] = sum_i x[a_k - HS + d + i] x[s_{k-1} + HS + i]
    for d = j - D in float64, cabs the same sum over the products' absolute values."""
    xp = _padded(x)
    out = []
    s_prev = -HS + int(deltas[0])
    for k in range(1, len(deltas)):
        a = k * HS * pct // 100
        tpl = xp[_LPAD + s_prev + HS:_LPAD + s_prev + HS + N]
        reg = xp[_LPAD + a - HS - D:_LPAD + a + HS + D]
        out.append((np.correlate(reg, tpl, "valid"), np.correlate(np.abs(reg), np.abs(tpl), "valid")))
        s_prev = a - HS + int(deltas[k])
    return out


def timescale_ref(x, pct, deltas=None, return_deltas=False):
    """The algorithm of fishtts_hip.h in float64: x at the codec rate (zero outside), speed pct / 100 ->
    ceil(100 len(x) / pct) samples.  It chooses the d_k itself (the lowest d of the largest correlation), or takes them."""
    n = len(x)
    n_out, K = n_out_of(n, pct), n_frames_of(n, pct)
    xp = _padded(x)
    y = np.zeros((K + 1) * HS)                 # position p lives at y[p + HS]
    ds = np.zeros(K, dtype=np.int64)
    s_prev = 0
    for k in range(K):
        a = k * HS * pct // 100
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


def impulse_train(n):
    x = np.zeros(n, dtype=np.float32)
    x[::64] = 1.0
    return x


def test_window_sums_to_one():
    assert np.max(np.abs(WIN[:HS] + WIN[HS:] - 1.0)) <= 1e-15


@pytest.mark.parametrize("pct", PCTS)
def test_lengths(pct):
    rng = np.random.default_rng(pct)
    for n in (1, 31, 512, 1023, 1024, 1025, 6880, 100000):
        y = timescale_ref(rng.uniform(-1, 1, n), pct)
        assert len(y) == math.ceil(100 * n / pct) == n_out_of(n, pct), (n, pct)


@pytest.mark.parametrize("freq", (110, 200, 1000))
def test_tones_keep_level_and_pitch(freq):
    n = 4 * FI
    x = 0.5 * np.sin(2 * np.pi * freq * np.arange(n) / FI)
    rms_in = np.sqrt(np.mean(x ** 2))
    for pct in (50, 75, 90, 125, 150, 200):
        y = timescale_ref(x, pct)[2 * N:-2 * N]
        ratio = np.sqrt(np.mean(y ** 2)) / rms_in
        assert abs(ratio - 1.0) <= 1e-3, (freq, pct, ratio)
        spec = np.abs(np.fft.rfft(y))
        assert int(np.argmax(spec)) == int(round(freq * len(y) / FI)), (freq, pct)


@pytest.mark.parametrize("pct", PCTS)
def test_exact_ties_take_the_lowest_delta(pct):
    """An impulse train of 1.0 every 64 samples: every product is 0 or 1, every sum exact, and the candidates 64 apart
    tie.  The restatement picks the lowest of them."""
    x = impulse_train(6880)
    y, ds = timescale_ref(x, pct, return_deltas=True)
    tied_frames = 0
    for k, (c, _) in enumerate(frame_scores(x, pct, ds), start=1):
        assert np.array_equal(c, np.round(c))
        best = np.flatnonzero(c == c.max())
        assert ds[k] == best[0] - D, (pct, k)
        tied_frames += len(best) > 1
    assert tied_frames >= len(ds) // 2


def test_given_deltas_reproduce():
    x = np.random.default_rng(3).uniform(-1, 1, 6880)
    y, ds = timescale_ref(x, 125, return_deltas=True)
    assert np.array_equal(timescale_ref(x, 125, deltas=ds), y)
    assert len(ds) == n_frames_of(len(x), 125)


def test_speed_validation():
    from fish_tts_amd.codec_engine import output_speed, timescaled_len
    assert output_speed(None) is None
    assert output_speed(1) is None and output_speed(1.0) is None and output_speed(1.004) is None
    assert output_speed(0.5) == 50 and output_speed(2.0) == 200 and output_speed(1.25) == 125
    assert output_speed(np.float32(0.8)) == 80
    for bad in (0.49, 2.01, 0, -1, "1", True, float("nan")):
        with pytest.raises(ValueError):
            output_speed(bad)
    assert timescaled_len(None, 1000) == 1000 and timescaled_len(1.0, 1000) == 1000
    assert timescaled_len(0.8, 1000) == 1250


def test_timescaled_len_host_call():
    lib = _lib()
    for pct in PCTS + (50, 75, 150):
        for n in (0, 1, 31, 512, 1023, 1024, 1025, 6880, 100000, 1 << 33):
            assert lib.ft_timescaled_len(pct, n) == -(-100 * n // pct), (pct, n)
    assert lib.ft_timescaled_len(49, 1000) == -1
    assert lib.ft_timescaled_len(201, 1000) == -1
    assert lib.ft_timescaled_len(100, -1) == -1
