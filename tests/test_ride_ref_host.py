"""CPU: the float64 restatement of the ride stage (tests/ride_ref.py) pinned - a stationary tone lands on the target, silence
comes back untouched, the slew and the ceiling hold, the node and output counts at every border of the emission rule - and
each rule knocked out in turn to show that ride_ref.check, which the GPU tests use, notices it."""
import numpy as np
import pytest

from tests import level_ref as R
from tests import ride_ref as RR

TARGET = -2300


@pytest.mark.parametrize("rate", R.RATES)
def test_a_stationary_tone_lands_on_the_target(rate):
    x = (0.1 * np.sin(2.0 * np.pi * 997.0 * np.arange(4 * rate) / rate)).astype(np.float32)
    r = RR.ride(x, rate, TARGET)
    H = RR.hop(rate)
    # past the first blocks the measure is the tone's, every node sits on target - L, and the output measures at the target
    assert np.max(np.abs(np.diff(r.v))) <= RR.SLEW + 1e-12
    out = R.measure(r.y[6 * H:], rate)
    assert abs(out.L - TARGET / 100.0) <= 1e-4, (rate, out.L)
    assert r.capped == 0 and np.isfinite(r.margin)


@pytest.mark.parametrize("rate", R.RATES)
def test_silence_and_what_stays_below_the_gates_come_back_untouched(rate):
    H = RR.hop(rate)
    for x in (np.zeros(13 * H + 3, dtype=np.float32), (1e-5 * np.random.default_rng(1).standard_normal(13 * H)).astype(np.float32)):
        r = RR.ride(x, rate, TARGET)
        assert np.all(r.g == np.float32(1.0)) and np.array_equal(r.y.view(np.uint32), x.view(np.uint32))
        assert np.all(r.v == 0.0) and np.all(r.L == -np.inf)


@pytest.mark.parametrize("rate", R.RATES)
def test_slew_ceiling_and_capped_nodes_on_the_step_signal(rate):
    x = RR.step_signal(rate, seed=rate)
    r = RR.ride(x, rate, -1600)            # a target loud enough for the click and the step's peaks to meet the guard
    assert np.max(np.abs(np.diff(r.v))) <= RR.SLEW + 1e-12
    assert abs(np.max(np.abs(np.diff(r.v))) - RR.SLEW) <= 1e-12            # the step makes the slew bind
    assert np.max(np.abs(r.y)) <= RR.CEILING * (1 + 2.0 ** -22)
    assert r.capped >= 2 and r.margin >= 1e-6, (r.capped, r.margin)
    assert RR.check(r.g, r.y, r) == []
    # cumulative measure: the output settles toward the programme loudness so far and does not reach the target at once
    assert R.measure(RR.ride(x, rate, TARGET).y, rate).L > TARGET / 100.0


@pytest.mark.parametrize("rate", R.RATES)
def test_counts_at_the_borders(rate):
    H, A = RR.hop(rate), RR.A
    rng = np.random.default_rng(3)
    for n in (0, 1, H - 1, H, 4 * H - 1, 4 * H, (A + 1) * H - 1, (A + 1) * H, (A + 1) * H + 1):
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        r = RR.ride(x, rate, TARGET)
        W, nh, nn = RR.counts(n, H)
        assert (W, nh, nn) == (n // H, -(-n // H), -(-n // H) + 1)
        assert len(r.g) == len(r.v) == nn and len(r.y) == n
        assert RR.plan(n, H, True) == (nn, n)
        k, out = RR.plan(n, H, False)
        assert (k, out) == ((W - A + 1, (W - A) * H) if W >= A else (0, 0)) and n - out < (A + 1) * H
        if k:
            # the nodes that are final before the end are those of the whole stream: they see A whole hops ahead either way
            more = np.concatenate([x, (0.3 * rng.standard_normal(5 * H)).astype(np.float32)])
            assert np.array_equal(RR.ride(more, rate, TARGET).g[:k], r.g[:k])
        if n and W < 1:
            assert np.all(r.L == -np.inf)


@pytest.mark.parametrize("knock", ["slew", "guard", "look", "interp"])
def test_check_notices_each_rule_knocked_out(knock):
    rate = 16000
    x = RR.step_signal(rate, seed=rate)
    ref = RR.ride(x, rate, -1600)
    bad = RR.ride(x, rate, -1600, knock=knock)
    assert RR.check(ref.g, ref.y, ref) == []
    assert RR.check(bad.g, bad.y, ref) != [], knock
    if knock == "slew":
        assert np.max(np.abs(np.diff(bad.v))) > RR.SLEW + 0.1
    if knock == "guard":
        assert np.max(np.abs(bad.y)) > RR.CEILING * (1 + 2.0 ** -22)
    if knock == "interp":
        assert np.array_equal(bad.g, ref.g) and not np.array_equal(bad.y, ref.y)
    with pytest.raises(AssertionError):
        assert RR.check(bad.g[:-1], bad.y, ref) == []
