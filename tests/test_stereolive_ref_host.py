"""CPU: the live stereo mix stage's restatement tests/stereolive_ref.py pinned - identity (a) against mixlive_ref.live and
identity (b) against stereo_ref.mix on seeded inputs, a case small enough to be written out by hand, cutting-independence of
the restatement itself, and every `knock` changing at least one output bit on an input named here."""
import numpy as np
import pytest

from tests import mix_ref as MR
from tests import mixlive_ref as ML
from tests import stereo_ref as SR
from tests import stereolive_ref as SL

RATE, H = 8000, 160


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def P(**kw):
    base = dict(depth=1200, threshold=0.01, attack=2, release=3)
    base.update(kw)
    return MR.Params(**base)


def loud(n, seed):
    """A programme that exceeds the ceiling here and there, with a quiet stretch."""
    x = (0.9 * np.sign(noise(n, seed))).astype(np.float32)
    x[:2 * H] = 0.0
    x[7 * H:9 * H] *= 0.1
    return x


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_identity_a_every_pan_zero_is_the_mono_stage_twice(seed):
    n = 13 * H + 5 + seed
    x, bed = loud(n, seed), noise(907, 70 + seed, 0.4)
    p = P(lead=H + 3, tail=2 * H + 1, fade_in=20, fade_out=H, offset=11)
    want = ML.live(x, bed, RATE, p)
    for pushes in ([(x, [])], [(x, [(0, n, 0)])], SL.cut(x, [(5, n - 1, 0)], [0, 3 * H + 1, n - 3 * H - 1])):
        got = SL.live(pushes, bed, bed, RATE, p)
        assert np.array_equal(bits(got.y[:, 0]), bits(want.y)) and np.array_equal(bits(got.y[:, 1]), bits(want.y))
        assert np.array_equal(got.D, want.D) and np.array_equal(got.L, want.L) and np.array_equal(got.need, want.need)
        assert np.array_equal(bits(got.Q), bits(want.Q)) and (got.N, got.Nh) == (want.N, want.Nh) and want.L.any()


@pytest.mark.parametrize("seed", [4, 5])
def test_identity_b_below_the_ceiling_it_is_the_stereo_mix_stage(seed):
    n = 11 * H + 7
    x, b0, b1 = noise(n, seed, 0.05), noise(800, 80 + seed, 0.1), noise(800, 90 + seed, 0.1)
    regions = [(0, 3 * H + 1, -100), (3 * H + 1, 5 * H, 40), (6 * H - 2, n, 100)]
    p = P(lead=37, tail=H + 2, fade_in=9, fade_out=2 * H)
    want = SR.mix(x, b0, b1, regions, RATE, p)
    assert not want.capped and want.N >= 2 * max(p.fade_in, p.fade_out)
    for sizes in ([n], [3 * H + 2, 2 * H, n - 5 * H - 2], [1] * 3 + [n - 3]):
        got = SL.live(SL.cut(x, regions, sizes), b0, b1, RATE, p)
        assert not got.L.any() and np.array_equal(bits(got.y), bits(want.y)) and np.array_equal(got.D, want.D)
    none = SL.live(SL.cut(x, regions, [n]), None, None, RATE, p)
    assert np.array_equal(bits(none.y), bits(SR.mix(x, None, None, regions, RATE, p).y))


def test_a_case_written_out_by_hand():
    """H = 160, no bed, no duck to speak of: two samples of 1.0, the first hard left, the second at pan 50.  The left channel
    peaks at 1 > cf, so need_0 is the smallest d with T[d] <= cf: 10^(-d / 2000) <= 10^(-1 / 20) from d = 100 on, and the
    float32 T[100] rounds to cf itself.  One hop: L_0 = need_0 = 100, L_1 = need_0 (25 - 0) / 25 = 100, so f = T[100] = cf on
    every sample and the right channel, which never reached the ceiling, is turned down by the same factor."""
    T, U = MR.gains(), SR.pan_gains()
    assert T[100] == ML.CF and T[99] > ML.CF
    x = np.array([1.0, 1.0], dtype=np.float32)
    got = SL.live([(x, [(0, 1, -100), (1, 2, 50)])], None, None, RATE, P(depth=0))
    assert (got.N, got.Nh) == (2, 1) and got.q.tolist() == [-100, 50]
    assert got.m.tolist() == [[1.0, 0.0], [float(U[50]), 1.0]]
    assert got.Q.tolist() == [1.0] and got.need.tolist() == [100] and got.L.tolist() == [100, 100]
    want = np.array([[ML.CF, 0.0], [np.float32(U[50] * ML.CF), ML.CF]], dtype=np.float32)
    assert np.array_equal(bits(got.y), bits(want))
    assert U[50] == np.float32(np.sqrt(2.0) * np.sin(np.pi / 8.0))
    # the same two samples in two pushes, the second region relative to its own push
    two = SL.live([(x[:1], [(0, 1, -100)]), (x[1:], [(0, 1, 50)])], None, None, RATE, P(depth=0))
    assert np.array_equal(bits(two.y), bits(got.y))


def knock_case():
    """The input every knock is shown on: hard-left speech over the ceiling in hop 4 and beyond, a region that crosses the
    cut, a second push whose own region does not begin at its first sample."""
    n = 14 * H + 9
    x = loud(n, 6)
    regions = [(2 * H, 9 * H + 40, -100), (9 * H + 40, n, 30)]
    sizes = [9 * H + 3, n - 9 * H - 3]
    return x, regions, sizes, noise(907, 60, 0.3), noise(907, 61, 0.3), P(lead=5, tail=H, fade_out=H // 2)


def test_the_restatement_does_not_depend_on_the_cutting():
    x, regions, sizes, b0, b1, p = knock_case()
    one = SL.live(SL.cut(x, regions, [len(x)]), b0, b1, RATE, p)
    for cutting in (sizes, [0, 7, len(x) - 7, 0], [H] * 14 + [9]):
        got = SL.live(SL.cut(x, regions, cutting), b0, b1, RATE, p)
        assert np.array_equal(bits(got.y), bits(one.y)) and np.array_equal(got.L, one.L) and got.q.tolist() == one.q.tolist()
    assert one.L.any()
    # (d): under the ceiling on both channels, up to one rounding
    assert float(np.abs(one.y).max()) <= float(ML.CF) * (1.0 + 2.0 ** -22)


@pytest.mark.parametrize("knock", ["left", "unlinked", "carry", "swap", "stream"])
def test_every_knock_changes_a_bit(knock):
    x, regions, sizes, b0, b1, p = knock_case()
    if knock == "left":                                    # the right channel alone over the ceiling
        regions = [(a, e, -pan) for a, e, pan in regions]
    pushes = SL.cut(x, regions, sizes)
    good, bad = SL.live(pushes, b0, b1, RATE, p), SL.live(pushes, b0, b1, RATE, p, knock=knock)
    assert good.y.shape == bad.y.shape and (bits(good.y) != bits(bad.y)).any(), knock
    if knock == "carry":                                   # exactly the samples the stream carried over the cut
        first = SL.carried_from(sizes[0], RATE, p)
        assert 0 < first < sizes[0] and (bad.q[first:sizes[0]] == 0).all() and (good.q[first:sizes[0]] == -100).all()
        assert bad.q[:first].tolist() == good.q[:first].tolist() and bad.q[sizes[0]:].tolist() == good.q[sizes[0]:].tolist()
    if knock == "stream":
        assert bad.q[:sizes[0]].tolist() != good.q[:sizes[0]].tolist() or bad.q[sizes[0]:].tolist() != good.q[sizes[0]:].tolist()


def test_cut_clips_and_shifts():
    x = np.zeros(10, dtype=np.float32)
    pushes = SL.cut(x, [(1, 4, 7), (4, 9, -7)], [3, 0, 3, 4])
    assert [r for _, r in pushes] == [[(1, 3, 7)], [], [(0, 1, 7), (1, 3, -7)], [(0, 3, -7)]]
