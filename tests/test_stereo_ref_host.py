"""CPU: the stereo mix stage's restatement tests/stereo_ref.py pinned - the pan table (against the library's host-only
ft_pan_gains, bit for bit), the region lookup at every edge, the side selection, q = 0 reproducing tests/mix_ref.py on both
channels, and the pair measure against the closed form for two sines."""
import ctypes as C

import numpy as np
import pytest

from tests import level_ref as LR
from tests import mix_ref as MR
from tests import stereo_ref as SR


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def test_pan_table():
    U = SR.pan_gains()
    assert U.dtype == np.float32 and len(U) == 201
    assert U[0] == 0.0 and U[100] == 1.0 and U[200] == 1.0 and np.all(U[100:] == 1.0)
    assert np.all(np.diff(U[:101]) > 0) and np.all(U <= 1.0)
    assert U[50] == np.float32(np.sqrt(2.0) * np.sin(np.pi / 8.0))
    for q in range(-100, 101):                             # the left gain of q is the right gain of -q
        (l, r), (l2, r2) = SR.gains_of(q), SR.gains_of(-q)
        assert l == r2 and r == l2 and l == U[100 - q] and r == U[100 + q]
    assert SR.gains_of(-100) == (1.0, 0.0) and SR.gains_of(100) == (0.0, 1.0) and SR.gains_of(0) == (1.0, 1.0)
    j = np.arange(1, 100)                                  # constant power below the clamp: sin^2 + cos^2
    assert np.allclose(U[j].astype(np.float64) ** 2 + 2.0 * np.cos(j * np.pi / 400.0) ** 2, 2.0, atol=1e-6)
    from fish_tts_amd import _lib as L
    got = np.full(201, -1.0, dtype=np.float32)
    assert L.load().ft_pan_gains(got.ctypes.data_as(C.c_void_p)) == 0 and L.load().ft_pan_gains(None) == L.FT_ERR_ARG
    assert np.array_equal(bits(got), bits(U))


def test_region_lookup_at_every_edge():
    n = 40
    regions = [(0, 1, -100), (1, 5, 37), (5, 6, 1), (9, 10, 100), (10, 39, -37)]       # one frame; touching; a hole; up to n - 1
    q = SR.region_pans(regions, n)
    want = np.zeros(n, dtype=np.int64)
    want[0], want[1:5], want[5], want[9], want[10:39] = -100, 37, 1, 100, -37
    assert q.tolist() == want.tolist() and q[6] == q[8] == q[39] == 0
    assert SR.region_pans([], 3).tolist() == [0, 0, 0]
    assert SR.region_pans([(0, 3, 5)], 3).tolist() == [5, 5, 5]
    assert SR.check_regions([(0, 3, 5)], 3) is None and SR.check_regions([(i, i + 1, 0) for i in range(4096)], 4096) is None
    assert SR.check_regions([(i, i + 1, 0) for i in range(4097)], 5000) == "R"
    for bad in ([(0, 4, 0)], [(-1, 2, 0)], [(2, 2, 0)], [(0, 2, 0), (1, 3, 0)], [(2, 3, 0), (0, 1, 0)]):
        assert SR.check_regions(bad, 3) == "place", bad
    assert SR.check_regions([(0, 1, 101)], 3) == "pan" and SR.check_regions([(0, 1, -101)], 3) == "pan"
    assert SR.check_regions([(0, 4, 101)], 3) == "place"                               # the place is judged first


def test_sides():
    assert SR.sides(-1, 2) == (0, 1) and SR.sides(-1, 6) == (0, 1) and SR.sides(-1, 1) == (0, 0)
    assert SR.sides(4, 6) == (4, 4) and SR.sides(0, 2) == (0, 0) and SR.sides(1, 2) == (1, 1)


@pytest.mark.parametrize("lead,tail", [(0, 0), (37, 9)])
def test_centre_and_one_bed_is_the_mono_stage_twice(lead, tail):
    rate, H = 8000, 160
    x = noise(9 * H + 13, 1, 0.3)
    x[2 * H:4 * H] = 0.0
    x[700] = np.nan
    bed = noise(908, 2)
    p = MR.Params(depth=900, attack=3, release=4, lead=lead, tail=tail, fade_in=50, fade_out=120, offset=11)
    want = MR.mix(x, bed, rate, p)
    for regions in ([], [(0, len(x), 0)], [(5, 9, 0), (9, 200, 0)]):
        got = SR.mix(x, bed, bed, regions, rate, p)
        assert np.array_equal(bits(got.y[:, 0]), bits(want.y)) and np.array_equal(bits(got.y[:, 1]), bits(want.y))
        assert np.array_equal(got.D, want.D) and (got.pk, got.sg, got.capped) == (want.pk, want.sg, want.capped)
        assert np.isnan(got.y[lead + 700]).all()
    # panned: hard left leaves the right channel the bed alone; the duck still follows the mono programme
    got = SR.mix(x, bed, bed, [(0, len(x), -100)], rate, p)
    assert np.array_equal(got.D, want.D) and np.array_equal(bits(got.m[:, 0]), bits(want.m))
    silent = np.ones(want.N, dtype=bool)
    silent[lead:lead + len(x)] = x == 0
    z = bits(got.s[:, 1]).copy()
    z[lead + 700] = 0                                                     # (the NaN stays one under a gain of 0)
    assert not (z & 0x7FFFFFFF).any() and np.isnan(got.s[lead + 700, 1]) and silent.sum() >= 2 * H      # a zero everywhere else
    assert np.array_equal(bits(got.m[silent, 1]), bits(want.m[silent])) and not np.array_equal(got.m[~silent, 1], want.m[~silent])
    # without a bed: the panned programme, lead and tail zeros
    got = SR.mix(x[:600] * np.float32(0.5), None, None, [(0, 300, -37)], rate, p)
    l, r = SR.gains_of(-37)
    assert not got.capped and np.array_equal(bits(got.y[lead:lead + 300, 0]), bits(x[:300] * np.float32(0.5) * l))
    assert np.array_equal(bits(got.y[lead:lead + 300, 1]), bits(x[:300] * np.float32(0.5) * r))
    assert np.array_equal(bits(got.y[lead + 300:lead + 600, 0]), bits(x[300:600] * np.float32(0.5)))
    assert not got.y[:lead].any() and not got.y[lead + 600:].any() and got.N == lead + 600 + tail


def test_ceiling_binds_on_one_channel_and_scales_both():
    rate, H = 8000, 160
    x = noise(5 * H, 3, 0.05)
    x[333] = 0.95
    got = SR.mix(x, np.zeros(10, np.float32), np.zeros(10, np.float32), [(300, 400, 100)], rate, MR.Params())
    assert got.capped and got.pk == np.float32(0.95) and got.sg == np.float32(MR.CEILING / float(np.float32(0.95)))
    assert np.all(got.y[300:400, 0] == 0) and np.array_equal(bits(got.y[:300, 0]), bits(x[:300] * got.sg))
    assert np.array_equal(bits(got.y[:, 1]), bits(x * got.sg))


def _response(rate, f):
    """|H(f)|^2 of the two K-weighting biquads, from the design's coefficients."""
    c = LR.design(rate)
    z = np.exp(-2j * np.pi * f / rate)
    h = 1.0
    for b0, b1, b2, a1, a2 in (c[:5], c[5:]):
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return float(abs(h) ** 2)


def test_pair_measure_on_two_sines_against_the_closed_form():
    rate, n = 44100, 5 * 44100
    t = np.arange(n) / rate
    a0, f0, a1, f1 = 0.25, 997.0, 0.1, 3000.0
    s0, s1 = (a0 * np.sin(2 * np.pi * f0 * t)).astype(np.float32), (a1 * np.sin(2 * np.pi * f1 * t)).astype(np.float32)
    got = SR.pair_measure(s0, s1, -2300)
    closed = -0.691 + 10.0 * np.log10(a0 * a0 / 2.0 * _response(rate, f0) + a1 * a1 / 2.0 * _response(rate, f1))
    assert abs(got.L - closed) < 0.01, (got.L, closed)     # (the filters' transient and the float32 samples)
    assert abs(-0.691 + 10 * np.log10(_response(rate, 997.0) / 2.0) + 3.01) < 0.01     # a full-scale 997 Hz sine: -3.01 LUFS
    assert got.p == np.float32(max(np.abs(s0).max(), np.abs(s1).max())) and got.blocks == 50 - 3
    assert got.g == np.float32(10.0 ** ((-23.0 - got.L) / 20.0)) and not got.capped
    m0, m1 = LR.measure(s0, rate), LR.measure(s1, rate)
    assert np.array_equal(got.e, m0.e + m1.e)
    assert abs(got.L - LR.lufs(10 ** ((m0.L + 0.691) / 10) + 10 ** ((m1.L + 0.691) / 10))) < 1e-9      # energies add
    twice = SR.pair_measure(s0, s0)
    assert abs(twice.L - (m0.L + 10.0 * np.log10(2.0))) < 1e-9 and twice.g == 1.0 and twice.p == m0.p
    spike = s1.copy()
    spike[1234] = -0.9
    loud = SR.pair_measure(s0, spike, -500)                # the ceiling binds on the larger of the two peaks: side 1's
    assert loud.capped and loud.p == np.float32(0.9) and loud.g == np.float32(LR.CEILING / float(np.float32(0.9)))
