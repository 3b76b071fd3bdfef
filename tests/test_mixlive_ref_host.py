"""CPU: the live mix stage's restatement (tests/mixlive_ref.py) pinned - against Mix's restatement where the two must agree,
against its own knock-outs, against the ceiling it promises and against the emission rule's own consequences."""
import numpy as np
import pytest

from tests import mix_ref as R
from tests import mixlive_ref as ML

RATES = [8000, 16000, 44100, 48000]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sine_bed(n, amp=0.5, period=37.0):
    return (amp * np.sin(2.0 * np.pi * np.arange(n) / period)).astype(np.float32)


def capped_cases():
    """Four rates, six random lengths up to 40 H each: a 0.97 spike (and some loud noise) over a 0.5 sine bed."""
    rng = np.random.default_rng(20240917)
    out = []
    for rate in RATES:
        H = R.hop(rate)
        for c in range(6):
            n = int(rng.integers(1, 40 * H + 1))
            x = (0.05 * rng.standard_normal(n)).astype(np.float32)
            x[int(rng.integers(0, n))] = 0.97 if c % 2 == 0 else -0.97
            if c >= 3 and n > 2 * H:
                a = int(rng.integers(0, n - H))
                x[a:a + H] = (0.6 * rng.standard_normal(H)).astype(np.float32)
            p = R.Params(depth=[0, 600, 1200][c % 3], attack=1 + c, release=2 + 3 * c, lead=(c % 2) * (H + 3), tail=(c % 3) * 50,
                         fade_in=7 * c, fade_out=11 * c, offset=c, threshold=0.02)
            out.append((rate, x, sine_bed(300 + 17 * c), p))
    return out


CAPPED = capped_cases()


def uncapped_cases():
    rng = np.random.default_rng(7)
    out = []
    for rate in RATES:
        H = R.hop(rate)
        for c in range(3):
            n = int(rng.integers(2 * H, 30 * H))
            x = (0.1 * rng.standard_normal(n)).astype(np.float32)
            x[n // 3:n // 2] = 0.0
            fade = [0, 40, n // 2][c]
            p = R.Params(depth=1200, attack=2 + c, release=3 + 2 * c, lead=c * 31, tail=c * (H + 1), fade_in=fade, fade_out=fade // 2,
                         offset=5 * c, threshold=0.01)
            out.append((rate, x, sine_bed(500 + c, 0.3), p))
    return out


def test_uncapped_inputs_are_mix_bit_for_bit():
    for rate, x, bed, p in uncapped_cases():
        got, want = ML.live(x, bed, rate, p), R.mix(x, bed, rate, p)
        assert want.N >= 2 * max(p.fade_in, p.fade_out) and not want.capped
        assert not got.L.any() and np.array_equal(got.D, want.D)
        assert np.array_equal(bits(got.y), bits(want.y))


@pytest.mark.parametrize("knock", ["need", "behind", "nearest", "fade"])
def test_every_knock_out_changes_some_bit(knock):
    cases = list(CAPPED)
    # need: a peak whose product with some T[d] is cf exactly - T[0] = 1 and Q = cf
    rate, H = 8000, 160
    x = np.zeros(12 * H, dtype=np.float32)
    x[5 * H + 3] = ML.CF
    cases.append((rate, x, np.zeros(64, dtype=np.float32), R.Params(depth=0, attack=2, release=3)))
    # fade: fades longer than N / 2
    cases.append((rate, (0.1 * np.ones(3 * H)).astype(np.float32), sine_bed(200), R.Params(attack=1, release=1, fade_in=2 * H,
                                                                                           fade_out=5 * H)))
    changed = 0
    for rate, x, bed, p in cases:
        a, b = ML.live(x, bed, rate, p), ML.live(x, bed, rate, p, knock=knock)
        changed += int(not np.array_equal(bits(a.y), bits(b.y)) or not np.array_equal(a.L, b.L))
    assert changed > 0


def test_the_limiter_holds_the_ceiling():
    worst, engaged = 0.0, 0
    for rate, x, bed, p in CAPPED:
        r = ML.live(x, bed, rate, p)
        worst = max(worst, float(np.abs(r.y).max()))
        engaged += int(r.L.any())
        for h in range(r.Nh):                       # both nodes of a hop sit at need_h or deeper
            assert r.L[h] >= r.need[h] and r.L[h + 1] >= r.need[h]
    assert engaged >= len(CAPPED) // 2           # (a spike can meet the bed at its trough)
    assert worst <= float(ML.CF) * (1.0 + 2.0 ** -22), worst


def test_emission_is_monotone_complete_and_bounded():
    rng = np.random.default_rng(3)
    for rate in RATES:
        H = R.hop(rate)
        for c in range(40):
            p = R.Params(attack=int(rng.integers(1, 30)), release=4, lead=int(rng.integers(0, 3)) * int(rng.integers(0, 20 * H)),
                         tail=int(rng.integers(0, 3 * H)), fade_out=int(rng.integers(0, 4 * H)))
            n = int(rng.integers(0, 60 * H))
            last, at = 0, 0
            while at < n:
                at = min(n, at + int(rng.integers(0, 3 * H)))
                e = ML.emitted(at, False, rate, p)
                assert e >= last and e % H == 0
                assert p.lead + at - e < ML.held_bound(rate, p)
                last = e
            assert ML.emitted(n, True, rate, p) == p.lead + n + p.tail >= last
    # the default attack (0.3 s = 15 hops): 22 hops, 0.44 s, held back at most
    assert ML.held_bound(44100, R.Params(attack=15)) == 22 * 882
