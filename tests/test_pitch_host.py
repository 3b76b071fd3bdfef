"""Host checks of the pitch stage behind pitch= (include/fishtts_hip.h, Pitch): the step and tap count of every cents
value, the quality of the filter through the interpolated coefficients, a tone through the float64 restatement
(tests/pitch_ref.py), the accepted speed / pitch combinations, the rational-rate time-scale restatement against the
percentage one, and the validation of pitch values.  No GPU."""
import ctypes as CT
import math

import numpy as np
import pytest

from tests.pitch_ref import PHASES, SHIFT, pitch_coefs, pitch_ref, pitch_table, timescale_ref_q
from tests.test_timescale_host import PCTS, timescale_ref

CENTS = (-1200, -700, -1, 1, 100, 700, 1200)


def _lib():
    from fish_tts_amd import _lib as L
    return L.load()


def test_step_and_taps_of_every_cents_value():
    lib = _lib()
    step, K = CT.c_int64(0), CT.c_int32(0)
    for c in range(-1200, 1201):
        assert lib.ft_pitch_filter(c, CT.byref(step), CT.byref(K), None) == 0
        assert step.value == round(2 ** 20 * 2 ** (c / 1200)), c
        r = step.value / 2 ** 20
        assert abs(r / 2 ** (c / 1200) - 1) <= 2.0 ** -20, c        # half a step of 2^-20 over r >= 0.5
        if c == 0:
            assert K.value == 0
            continue
        k = math.ceil((75 - 7.95) / (2.285 * 2 * math.pi * 0.07) * max(1.0, r))
        assert K.value == k + (k & 1) and K.value % 2 == 0, (c, K.value)
    assert pitch_table(-1200)[1] == 68 and pitch_table(-1)[1] == 68 and pitch_table(1200)[1] == 134
    for bad in (-1201, 1201):
        step.value, K.value = 77, 78
        assert lib.ft_pitch_filter(bad, CT.byref(step), CT.byref(K), None) == 1
        assert (step.value, K.value) == (77, 78)


def test_row_512_is_row_0_one_tap_on():
    for c in (-700, 1200):
        _, K, w = pitch_table(c)
        assert np.array_equal(w[PHASES, 1:], w[0, :-1])


@pytest.mark.parametrize("cents", CENTS)
def test_filter_quality_through_interpolated_coefficients(cents):
    """Pass band <= 0.01 dB to 0.43 min(1, 1 / r), stop band >= 70 dB from 0.5 / r, at fractional phases that are not table
    rows.  Per phase: the coefficient set is a discrete filter whose ideal is the pure advance by the fraction - its
    complex deviation from that (level and delay together) stays within the 0.01 dB ratio over the pass band, and above
    0.5 / r (where that lies below the input's half rate) it passes less than -70 dB.  As one kernel: the phases midway
    between all rows sample the continuous prototype at 1 / 512; its response is within 0.01 dB over the pass band and
    below -70 dB from 0.5 / r to 3 cycles per input sample (the images a slower read would fold back)."""
    S, K, w = pitch_table(cents)
    r = S / 2 ** SHIFT
    tol = 10 ** (0.01 / 20) - 1
    stop = 10 ** (-70 / 20)
    fp, fs = 0.43 * min(1.0, 1.0 / r), 0.5 / r
    off = np.arange(K) - K // 2 + 1                       # tap t reads x[i0 + off[t]]
    fracs = np.array([1023, 1 << 10, 3 * 2048 + 5, 123457, 524288 + 1024, 777777, (1 << SHIFT) - 1], dtype=np.int64)
    assert np.all(fracs & 2047)                           # none of them a table row
    _, c = pitch_coefs(w, fracs)
    nu_p = np.linspace(0, fp, 200)
    for q, cq in zip(fracs / 2.0 ** SHIFT, c):
        H = (cq[None, :] * np.exp(2j * np.pi * nu_p[:, None] * (off[None, :] - q))).sum(axis=1)
        assert np.max(np.abs(H - 1)) <= tol, (cents, q, np.max(np.abs(H - 1)))
        if fs < 0.5:
            nu_s = np.linspace(fs, 0.5, 200)
            Hs = (cq[None, :] * np.exp(2j * np.pi * nu_s[:, None] * off[None, :])).sum(axis=1)
            assert np.max(np.abs(Hs)) <= stop, (cents, q, np.max(np.abs(Hs)))
    mid = (np.arange(PHASES, dtype=np.int64) << 11) + 1024
    _, cm = pitch_coefs(w, mid)                           # [512][K]: the prototype at tau = (p + 0.5) / 512 - off[t]
    tau = (mid / 2.0 ** SHIFT)[:, None] - off[None, :]
    for nus, lim, centre in ((nu_p, tol, 1.0), (np.linspace(fs, 3.0, 400), stop, 0.0)):
        Hc = np.array([(cm * np.exp(-2j * np.pi * nu * tau)).sum() for nu in nus]) / PHASES
        assert np.max(np.abs(np.abs(Hc) - centre)) <= lim, (cents, centre, np.max(np.abs(np.abs(Hc) - centre)))


@pytest.mark.parametrize("cents", CENTS)
def test_tone_comes_out_at_r_times_the_frequency(cents):
    S, K, _ = pitch_table(cents)
    r = S / 2 ** SHIFT
    nu = 0.2 * min(1.0, 1.0 / r)
    n_in = 6000
    x = np.sin(2 * np.pi * nu * np.arange(n_in))
    n_out = int((n_in - 2) / r)
    y, bound = pitch_ref(x.astype(np.float32), cents, n_out)
    want = np.sin(2 * np.pi * nu * r * np.arange(n_out))
    edge = int(K / r) + 2
    assert np.max(np.abs(y - want)[edge:-edge]) <= 1e-3, cents
    assert np.all(bound > 0)


def test_accepted_combinations():
    lib = _lib()
    for pct, c in ((100, 1200), (100, -1200), (200, 1200), (50, -1200), (125, 300), (80, -500), (100, 0), (125, 0)):
        assert lib.ft_pitch_ok(pct, c) == 0, (pct, c)
    for pct, c in ((200, -100), (50, 100), (100, 1201), (100, -1201), (49, 0), (201, 1200)):
        assert lib.ft_pitch_ok(pct, c) == 1, (pct, c)


@pytest.mark.parametrize("pct", PCTS)
def test_rational_restatement_equals_the_percentage_one(pct):
    rng = np.random.default_rng(pct)
    for n in (1, 1025, 6880):
        x = rng.uniform(-1, 1, n)
        y, d = timescale_ref(x, pct, return_deltas=True)
        yq, dq = timescale_ref_q(x, pct, 100, return_deltas=True)
        assert np.array_equal(y, yq) and np.array_equal(d, dq)
        assert np.array_equal(timescale_ref_q(x, 7 * pct, 700, deltas=d), y)


def test_pitch_validation():
    from fish_tts_amd.codec_engine import output_fx, output_pitch
    assert output_pitch(None) is None
    assert output_pitch(0) is None and output_pitch(0.0) is None and output_pitch(0.004) is None and output_pitch(-0.004) is None
    assert output_pitch(12) == 1200 and output_pitch(-12) == -1200 and output_pitch(7) == 700
    assert output_pitch(np.float32(-2.5)) == -250 and output_pitch(0.01) == 1
    for bad in (12.01, -12.01, float("nan"), True, "1"):
        with pytest.raises(ValueError):
            output_pitch(bad)
    assert output_fx(None, None) == (None, None) and output_fx(1.0, 0) == (None, None)
    assert output_fx(1.25, 3) == (125, 300) and output_fx(0.8, -5) == (80, -500)
    assert output_fx(2.0, 12) == (200, 1200) and output_fx(0.5, -12) == (50, -1200)
    assert output_fx(None, 12) == (None, 1200) and output_fx(2.0, None) == (200, None)
    for speed, pitch in ((2.0, -1), (0.5, 1), (1.0, 12.01), (2.01, 0), (None, float("nan")), (None, True), (None, "1")):
        with pytest.raises(ValueError):
            output_fx(speed, pitch)
    with pytest.raises(ValueError, match=r"speed / 2\^\(pitch / 12\)"):
        output_fx(2.0, -1)
