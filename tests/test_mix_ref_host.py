"""CPU: the mix stage's checker (tests/mix_ref.py) pinned on cases computed by hand from the statement in
include/fishtts_hip.h ("Mix"), each rule knocked out once to show the cases catch it, and the gain table."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import mix_ref as R

RATE = 8000
H = 160


def test_one_active_hop_in_silence():
    act = np.zeros(10, dtype=bool)
    act[5] = True
    # ahead: 1200 (4 - (5 - k)) / 4 for k = 2 .. 5; behind: 1200 (2 - (k - 6)) / 2 for k = 6, 7
    want = [0, 0, 300, 600, 900, 1200, 1200, 600, 0, 0, 0]
    assert R.duck(act, 1200, 4, 2).tolist() == want
    assert R.duck(act, 1200, 4, 2, knock="behind").tolist() != want          # the off-by-one is caught
    # integer division: 1000 2 / 3 = 666, 1000 1 / 3 = 333
    assert R.duck(act, 1000, 3, 3).tolist() == [0, 0, 0, 333, 666, 1000, 1000, 666, 333, 0, 0]


def test_two_runs_closer_than_both_windows():
    act = np.zeros(8, dtype=bool)
    act[[2, 5]] = True
    # node 3: behind hop 2 at full depth beats the cone of hop 5 (600); node 4: 900 ahead of hop 5 beats 600 behind hop 2
    assert R.duck(act, 1200, 4, 2).tolist() == [600, 900, 1200, 1200, 900, 1200, 1200, 600, 0]


def test_first_hop_and_last_partial_hop():
    n = 3 * H + 5
    x = np.zeros(n, dtype=np.float32)
    x[0] = x[n - 1] = 0.5
    m = R.mix(x, np.zeros(7, dtype=np.float32), RATE, R.Params(depth=1200, attack=2, release=2))
    assert (m.N, m.Nh, m.H) == (n, 4, H)
    assert m.act.tolist() == [True, False, False, True]
    assert m.D.tolist() == [1200, 1200, 600, 1200, 1200] and m.dmax == 1200
    assert np.array_equal(m.y.view(np.uint32), x.view(np.uint32))           # a bed of zeros: the programme, bit for bit


def test_windows_longer_than_the_timeline():
    assert R.duck([False, True, False], 6000, 500, 500).tolist() == [5988, 6000, 6000, 5988]
    assert R.duck([False, False], 6000, 500, 500).tolist() == [0, 0, 0]
    assert R.duck([True], 0, 500, 500).tolist() == [0, 0]                   # depth 0


def test_threshold_nan_lead_and_wrap():
    thr = np.float32(0.1)
    x = np.zeros(2 * H, dtype=np.float32)
    x[3] = thr                                     # exactly at the threshold: active
    x[H + 3] = np.nextafter(thr, np.float32(0))    # one step below: not
    x[H + 9] = np.nan                              # never loud, never the peak
    bed = np.arange(1, 6, dtype=np.float32) / 16
    p = R.Params(depth=0, threshold=float(thr), lead=7, tail=3, offset=13, loop=1)
    m = R.mix(x, bed, RATE, p)
    assert m.N == 2 * H + 10 and m.Nh == 3 and m.act.tolist() == [True, False, False]
    s, b = R.timeline(x, bed, p)
    assert b[:4].tolist() == [bed[3], bed[4], bed[0], bed[1]] and s[7 + 3] == thr and s[:7].tolist() == [0.0] * 7
    assert np.all(m.gd == 1.0) and np.isnan(m.y[7 + H + 9]) and m.pk == np.float32(thr + bed[3]) and not m.capped
    s, b = R.timeline(x, bed, p._replace(loop=0, offset=2))
    assert b[:5].tolist() == [bed[2], bed[3], bed[4], 0.0, 0.0]


def test_sample_rule_closed_form_and_fades():
    # one active hop at full depth 2000 (g = 0.1 as float32), bed 0.25: inside the hop u = 0.25 T[2000]
    n = 4 * H
    x = np.zeros(n, dtype=np.float32)
    x[H:2 * H] = 0.5
    p = R.Params(depth=2000, attack=1, release=1, fade_in=4, fade_out=10 * n)
    m = R.mix(x, np.full(3, 0.25, dtype=np.float32), RATE, p)
    T = R.gains()
    assert m.D.tolist() == [0, 2000, 2000, 0, 0] and T[2000] == np.float32(0.1)
    want = np.float32(0.5) + np.float32(0.25) * T[2000]
    assert np.all(m.m[H:2 * H] == want)
    # the ramp over the first 4 samples: (2 j + 1) / 8, node 0 at gain 1 falling toward T[2000] over the hop
    r1 = np.float32(1) / np.float32(H)
    gd1 = np.float32(float(Fraction(float(r1)) * Fraction(float(T[2000] - T[0])) + 1))       # fmaf, exact then rounded once
    assert m.gd[1] == gd1
    assert m.m[1] == np.float32(np.float32(np.float32(0.25) * np.float32(3 / 8)) * gd1)
    # fade_out longer than the piece: f_out = N / 2, the last sample carries ramp(0) = 1 / N
    assert m.m[n - 1] == np.float32(np.float32(0.25) * np.float32(1.0 / n)) * m.gd[n - 1]
    assert m.m[n // 2] == np.float32(np.float32(0.25) * np.float32((2 * (n // 2 - 1) + 1) / n)) * m.gd[n // 2]
    assert m.m[n // 2 - 1] == np.float32(0.5) + np.float32(0.25) * m.gd[n // 2 - 1]     # the sample before the fade: no ramp


def test_fmaf32_is_fused():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(np.float32)
    # (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46: the float64 sum lands half-way between two float32 values, the remainder decides
    one, tiny = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24) * np.float32(1 - 2.0 ** -23)
    a = np.append(a, [one, one]).astype(np.float32)
    b = np.append(b, [tiny, -tiny]).astype(np.float32)
    c = np.append(c, [one, one]).astype(np.float32)
    assert R.fmaf32(a[-2:], b[-2:], c[-2:]).tolist() == [one, one]          # (rounding the float64 sum would give the even neighbours)
    got = R.fmaf32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(exact))                    # (float(Fraction) rounds once to float64, then once more: not used alone)
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert g == best, (x, y, z)


def test_contracted_multiply_add_is_caught():
    rng = np.random.default_rng(11)
    x = (0.3 * rng.standard_normal(40 * H)).astype(np.float32)
    bed = (0.2 * rng.standard_normal(977)).astype(np.float32)
    p = R.Params(depth=1200, attack=4, release=6)
    a, b = R.mix(x, bed, RATE, p), R.mix(x, bed, RATE, p, knock="fma")
    assert np.array_equal(a.D, b.D) and np.any(a.m.view(np.uint32) != b.m.view(np.uint32))


def test_ceiling_binds_only_above_it():
    x = np.full(2 * H, 0.5, dtype=np.float32)
    zero = np.zeros(4, dtype=np.float32)
    m = R.mix(x, zero, RATE, R.Params(), ceiling=0.5)
    assert m.pk == np.float32(0.5) and not m.capped and m.sg == 1.0                  # pk == c: untouched
    assert R.mix(x, zero, RATE, R.Params(), knock="ceiling", ceiling=0.5).capped      # the knocked-out rule is caught
    x[5] = np.nextafter(np.float32(0.5), np.float32(1))
    m = R.mix(x, zero, RATE, R.Params(), ceiling=0.5)
    assert m.capped and m.sg == np.float32(0.5 / float(x[5])) and np.array_equal(m.y, m.m * m.sg)
    # the stage's own ceiling is no float32: a peak at the float32 just under it passes, the next one up is scaled
    under = np.float32(R.CEILING)
    under = under if float(under) < R.CEILING else np.nextafter(under, np.float32(0))
    x[:] = 0.1
    x[5] = under
    assert not R.mix(x, zero, RATE, R.Params()).capped
    x[5] = np.nextafter(under, np.float32(1))
    m = R.mix(x, zero, RATE, R.Params())
    assert m.capped and m.sg == np.float32(R.CEILING / float(x[5]))


def test_gain_table():
    T = R.gains()
    assert len(T) == 6001 and T.dtype == np.float32 and T[0] == 1.0 and T[6000] == np.float32(1e-3)
    assert np.all(np.diff(T.astype(np.float64)) <= 0) and np.all(T > 0)
    from fish_tts_amd import _lib
    if not __import__("os").path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    got = np.zeros(6001, dtype=np.float32)
    assert lib.ft_mix_gains(got.ctypes.data_as(C.c_void_p)) == _lib.FT_OK
    assert lib.ft_mix_gains(None) == _lib.FT_ERR_ARG
    # both are a float64 power rounded once; two correctly-working pow()s differ by at most an ulp64, so by one float32 step
    assert got[0] == 1.0 and np.all(np.abs(got.view(np.int32).astype(np.int64) - T.view(np.int32)) <= 1)


@pytest.mark.parametrize("args,want", [((8000, 1, 0, 0), (1, 160, 2)), ((8000, 160, 0, 0), (160, 160, 2)),
                                       ((8000, 161, 0, 0), (161, 160, 3)), ((44100, 1000, 441, 441), (1882, 882, 4)),
                                       ((48000, 1 << 28, 0, 0), (1 << 28, 960, (1 << 28) // 960 + 2))])
def test_plan(args, want):
    from fish_tts_amd import _lib
    lib = _lib.load()
    N, hop, nodes = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    assert lib.ft_mix_plan(*args, C.byref(N), C.byref(hop), C.byref(nodes)) == _lib.FT_OK
    assert (N.value, hop.value, nodes.value) == want
    assert lib.ft_mix_plan(*args, None, None, None) == _lib.FT_OK
    for bad, st in [((7999, 1, 0, 0), _lib.FT_ERR_ARG), ((8000, 0, 0, 0), _lib.FT_ERR_ARG), ((8000, 1, -1, 0), _lib.FT_ERR_ARG),
                    ((8000, 1, 0, -1), _lib.FT_ERR_ARG), ((8000, 1 << 28, 1, 0), _lib.FT_ERR_TOO_LONG),
                    ((8000, 1, 0, (1 << 28)), _lib.FT_ERR_TOO_LONG)]:
        assert lib.ft_mix_plan(*bad, C.byref(N), C.byref(hop), C.byref(nodes)) == st
        assert (N.value, hop.value, nodes.value) == want
