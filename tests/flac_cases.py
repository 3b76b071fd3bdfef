"""The inputs of the FLAC stage's tests (tests/test_flac_gpu.py runs them on the device, tests/test_flac_ref_host.py through the
reference and its decoder): every length at which the stage takes another path, the contents that reach every subframe kind,
order, channel assignment and partition order, and the float values the quantiser treats specially.  A case is (name, x, rate,
B): x float32 or int16, (n,) or (n, 2).  reference(name) encodes a case once with tests/flac_ref.py and keeps the result."""
from __future__ import annotations

import functools

import numpy as np

from tests import flac_ref as R


def _noise(n, amp, seed):
    return np.random.default_rng(seed).integers(-amp, amp + 1, n).astype(np.int16)


def speech(n: int, rate: int = 44100, seed: int = 3) -> np.ndarray:
    """A speech-like sum of enveloped harmonics, float32 in (-1, 1): a 140 Hz pitch with vibrato, twelve harmonics under a
    formant-like tilt, a syllable envelope, a breath of noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    f0 = 140.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * t))
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(n)
    for h in range(1, 13):
        x += np.sin(h * ph + rng.uniform(0, 6.28)) / (1.0 + ((h * 140.0 - 700.0) / 500.0) ** 2) / h ** 0.5
    env = 0.5 * (1.0 - np.cos(2 * np.pi * 3.1 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t))
    x = 0.35 * x / np.abs(x).max() * env + 0.0015 * rng.standard_normal(n)
    return x.astype(np.float32)


def _ramp(n, degree):
    i = np.arange(n, dtype=np.int64)
    v = {1: 7 * i - 900, 2: 3 * (i - n // 2) ** 2 // 8 - 4000, 3: (i - n // 2) ** 3 // 900}[degree]
    assert np.abs(v).max() < 32768
    return v.astype(np.int16)


def _sine(n, amp=30000, period=60):
    return np.round(amp * np.sin(2 * np.pi * np.arange(n) / period)).astype(np.int16)


def _cases():
    out = []

    def add(name, x, rate=44100, B=256):
        out.append((name, x, rate, B))

    # ---- lengths (B = 256 unless said otherwise)
    add("n1_mono", _noise(1, 900, 1))
    add("n1_stereo", np.stack([_noise(1, 900, 2), _noise(1, 900, 3)], 1), 48000)
    for n in (255, 256, 257, 2 * 256 + 255):
        add(f"n{n}", _noise(n, 300, n), 22050)
    add("last4", _noise(256 + 4, 40, 5), 16000)                        # the order limit o < bs binds: orders 0..3
    add("last5", np.cumsum(np.cumsum(_noise(256 + 5, 3, 6).astype(np.int64))).astype(np.int16), 8000)
    add("last4_sine", _sine(256 + 4), 24000)                            # a content whose full frames take o = 4
    add("last5_sine", _sine(256 + 5), 24000)
    add("B1024_last257", speech(1024 + 257, seed=7), 32000, 1024)       # the 16-bit blocksize extra
    add("B1024_last700", speech(1024 + 700, seed=8), 11025, 1024)       # ... and a rate outside the table: the 16-bit rate extra
    add("B1024_last256", speech(1024 + 256, seed=9), 44100, 1024)       # a short last frame of 256 takes the 8-bit extra
    add("frames130", _noise(130 * 256, 25, 9), 44100)                   # the 2-byte frame number
    big = np.zeros(2050 * 256, dtype=np.int16)                          # the 3-byte frame number; zeros except a few frames
    for f in (0, 127, 128, 2047, 2048, 2049):
        big[f * 256:(f + 1) * 256] = _noise(256, 1000, f)
    add("frames2050", big, 44100)
    # ---- mono content
    add("zeros", np.zeros(700, dtype=np.int16))
    add("constant", np.full(700, -1234, dtype=np.int16))
    add("ramp_linear", _ramp(600, 1))
    add("ramp_quadratic", _ramp(600, 2))
    add("ramp_cubic", _ramp(600, 3))
    add("sine_fast", _sine(700))                                        # the fourth difference is the smallest: FIXED 4
    add("walk", np.clip(np.cumsum(_noise(1500, 60, 11).astype(np.int64)), -32768, 32767).astype(np.int16))
    add("white_full", np.random.default_rng(12).integers(-32768, 32768, 1000).astype(np.int16))
    add("noise_low", _noise(1000, 3, 13))
    spike = np.zeros(600, dtype=np.int16)
    spike[300] = 32767
    add("spike_full", spike)
    spike2 = np.zeros(1024 + 257, dtype=np.int16)                       # one partition of 257: the unary run of 300 crosses words
    spike2[1024 + 100] = 300
    add("spike_long_run", spike2, 44100, 1024)
    sp = speech(3 * 4096 + 17)
    for B in R.BLOCKSIZES:
        add(f"speech_B{B}", sp, 44100, B)
    # ---- stereo content
    a = _noise(1000, 12000, 20)
    add("st_equal", np.stack([a, a], 1))
    add("st_opposite", np.stack([a, -a], 1), 48000)
    add("st_independent", np.stack([_noise(1000, 500, 21), _noise(1000, 500, 22)], 1), 24000)
    loud = speech(2000, seed=23)
    add("st_quiet_right", np.stack([loud, 0.002 * speech(2000, seed=24)], 1), 44100, 512)
    add("st_quiet_left", np.stack([0.002 * speech(2000, seed=25), loud], 1), 44100, 512)
    add("st_speech_pair", np.stack([speech(5000, seed=26), 0.8 * speech(5000, seed=26) + 0.01 * speech(5000, seed=27)], 1), 32000, 2048)
    add("st_extremes", np.stack([np.full(700, 32767, dtype=np.int16), np.full(700, -32767, dtype=np.int16)], 1))
    wide = np.stack([_noise(600, 32767, 28), _noise(600, 32767, 29)], 1)
    add("st_white_full", wide)
    # ---- float edge cases: +-1, beyond +-1, NaN, -0.0, 1 - 2^-24, infinities, the smallest steps around a quantiser edge
    edge = np.array([1.0, -1.0, 1.5, -1.5, np.nan, -0.0, 0.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), np.inf, -np.inf, 1e-30, -1e-30,
                     1.0 / 32767.0, np.nextafter(np.float32(1.0 / 32767.0), np.float32(0)), 0.5, -0.5, 3.0517578e-05, 0.99996948,
                     np.nextafter(np.float32(1.0), np.float32(2.0)), 1e38, -1e38], dtype=np.float32)
    add("float_edges", np.concatenate([edge, 0.3 * speech(300, seed=30), edge[::-1]]).astype(np.float32))
    add("float_edges_stereo", np.stack([np.resize(edge, 300), np.resize(edge[::-1], 300)], 1).astype(np.float32), 48000)
    return out


CASES = _cases()
BY_NAME = {c[0]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(stream bytes, flac_ref.Census, the quantised samples) of a case, computed once."""
    _, x, rate, B = BY_NAME[name]
    pcm = R.quantise(x)
    data, census = R.encode(pcm, rate, B, census=True)
    return data, census, pcm
