"""CPU: the level stage's restatement (tests/level_ref.py) pinned to ITU-R BS.1770-4 and EBU Tech 3341, the host design of the
library (ft_level_filter) pinned to the restatement, and what OutputFx.of accepts as a loudness."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import level_ref as R


def test_design_at_48k_is_the_bs1770_table():
    assert np.max(np.abs(R.design(48000) - np.array(R.BS1770_48K))) <= 1e-9
    assert abs(R.design(48000)[0] - 1.53512485958697) <= 1e-9 and abs(R.design(48000)[8] - -1.99004745483398) <= 1e-9


@pytest.mark.parametrize("rate", R.RATES)
def test_full_scale_997hz_sine_reads_minus_3(rate):
    """A 997 Hz sine of amplitude 1.0 reads -3.01 LUFS (BS.1770's calibration), within EBU Tech 3341's +-0.1 LU, at every rate."""
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * rate) / rate)
    got = R.measure(x, rate).L
    print(f"rate {rate}: {got:.4f} LUFS")
    assert abs(got - -3.01) <= 0.1


def _energy(l):
    return 10.0 ** ((l + 0.691) / 10.0)


H = 4800


def test_absolute_gate():
    e = np.full(12, _energy(-80.0) * H)
    e[4:8] = _energy(-20.0) * H
    r = R.gate(e, 12 * H, H)
    assert r.blocks == 9 and r.gated == 7          # the two blocks of quiet hops alone are below -70
    assert abs(r.L - (-20.0 + 10.0 * math.log10(16.0 / 28.0))) <= 1e-4


def test_relative_gate():
    e = np.full(16, _energy(-20.0) * H)
    e[8:] = _energy(-35.0) * H
    r = R.gate(e, 16 * H, H)
    ungated = R.lufs(np.mean([(e[j:j + 4].sum()) / (4.0 * H) for j in range(13)]))
    assert r.blocks == 13 and 5 <= r.gated < 13
    assert r.L > ungated + 0.5 and r.L <= -20.0 + 1e-9      # the passage 15 dB down was cut


def test_short_item_is_one_block():
    n = 3 * H + 17
    r = R.gate(np.array([1.0, 2.0, 3.0, 0.5]), n, H)
    assert r.blocks == 1 and r.gated == 1 and abs(r.L - R.lufs(6.5 / n)) <= 1e-12
    r = R.gate(np.array([0.25]), 1, H)
    assert r.blocks == 1 and abs(r.L - R.lufs(0.25)) <= 1e-12
    # four whole hops and a rest: one block of the four, the rest counts for nothing
    r = R.gate(np.array([1.0, 1.0, 1.0, 1.0, 50.0]), 4 * H + 1, H)
    assert r.blocks == 1 and abs(r.L - R.lufs(4.0 / (4.0 * H))) <= 1e-12


def test_nothing_measured_gives_gain_one():
    for e, n in ((np.zeros(8), 8 * H), (np.zeros(0), 0), (np.full(8, _energy(-90.0) * H), 8 * H)):
        r = R.gate(e, n, H)
        assert r.L == -np.inf and r.gated == 0
        g, capped = R.gain(r.L, 0.5, -1600)
        assert g == np.float32(1.0) and not capped
    bad = np.full(8, _energy(-20.0) * H)
    bad[3] = np.nan
    assert R.gate(bad, 8 * H, H).L == -np.inf
    bad[3] = np.inf
    assert R.gate(bad, 8 * H, H).L == -np.inf


def test_gain_and_ceiling():
    g, capped = R.gain(-23.0, 0.1, -1600)
    assert not capped and g == np.float32(10.0 ** (7.0 / 20.0))
    g, capped = R.gain(-30.0, np.float32(0.9), -1000)
    assert capped and g == np.float32(R.CEILING / float(np.float32(0.9)))
    assert float(g) * 0.9 <= R.CEILING * (1 + 2.0 ** -23)
    g, capped = R.gain(-30.0, 0.9, -4000)
    assert not capped and abs(float(g) - 10.0 ** -0.5) <= 1e-7
    g, capped = R.gain(-30.0, 0.0, -1000)
    assert not capped and abs(float(g) - 10.0) <= 1e-5
    assert R.gain(-30.0, 0.9, 0) == (np.float32(1.0), False)


def test_measure_margin_reports_the_nearest_gate():
    rate = 8000
    rng = np.random.default_rng(5)
    x = 0.1 * rng.standard_normal(2 * rate)
    r = R.measure(x, rate, -2000)
    assert r.blocks == 2 * 10 - 3 and r.gated == r.blocks and np.isfinite(r.margin) and r.margin > 1.0
    assert len(r.e) == 20 and r.p == np.float32(np.max(np.abs(x.astype(np.float32))))


@pytest.mark.parametrize("rate", R.RATES + (12000, 22050, 24000, 32000))
def test_ft_level_filter_is_the_python_design(rate):
    from fish_tts_amd import _lib as L
    lib = L.load()
    c, h = (C.c_double * 10)(), C.c_int32(0)
    assert lib.ft_level_filter(rate, c, C.byref(h)) == L.FT_OK
    assert h.value == rate // 10
    assert np.max(np.abs(np.array(c) / R.design(rate) - 1.0)) <= 1e-12
    assert lib.ft_level_filter(rate, None, None) == L.FT_OK


def test_ft_level_filter_refuses_a_bad_rate():
    from fish_tts_amd import _lib as L
    lib = L.load()
    c, h = (C.c_double * 10)(*([7.0] * 10)), C.c_int32(-1)
    for rate in (0, 7999, 48001, 44101):
        assert lib.ft_level_filter(rate, c, C.byref(h)) == L.FT_ERR_ARG
    assert list(c) == [7.0] * 10 and h.value == -1


def test_output_fx_loudness():
    from fish_tts_amd.codec_engine import OutputFx
    fx = OutputFx.of(loudness=-16)
    assert fx.level == -1600 and fx.rate is None and fx.pct is None and fx.cents is None
    assert bool(fx) and fx.native == (44100, 100, 0) and fx.native_level == -1600 and fx.kw == {"fx": fx}
    assert OutputFx.of(loudness=-23.456).level == -2346
    assert OutputFx.of(loudness=-50).level == -5000 and OutputFx.of(loudness=-5.0).level == -500
    assert OutputFx.of(loudness=np.float32(-20)).level == -2000
    plain = OutputFx.of()
    assert plain.level is None and not plain and plain.native_level == 0 and plain == OutputFx.of(loudness=None)
    assert OutputFx.of(16000, 1.25, 3, -20) == OutputFx(16000, 125, 300, -2000)
    assert OutputFx.of(16000, 1.25, 3).native == OutputFx.of(16000, 1.25, 3, -20).native
    for bad in (-50.01, -4.99, 0, 16, float("nan"), float("inf"), True, "loud", [-16]):
        with pytest.raises(ValueError):
            OutputFx.of(loudness=bad)
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        fx.no_level("a stream")
    assert plain.no_level("a stream") is plain
