"""CPU: tests/room_ref.py, the numpy restatement of the room stage, pinned without a GPU: against a float64 convolution within
the chain's own error bound, its stated identities, and every `knock` - a rule taken out - caught by a comparison of bits."""
import numpy as np
import pytest

from tests import room_ref as R
from tests.mix_ref import gains


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def decay(n, seed):
    return (noise(n, seed, 0.5) * np.exp(-np.arange(n) / (0.25 * n))).astype(np.float32)


@pytest.mark.parametrize("L,n,predelay", [(1, 50, 0), (33, 400, 0), (257, 700, 3), (600, 300, 40)])
def test_the_chain_against_a_float64_convolution(L, n, predelay):
    """A chain of L fused multiply-adds: each step rounds once, relative error 2^-24 of a partial sum that is at most
    sum |h| |x| over the terms so far - so L 2^-24 sum |h| |x| bounds the whole."""
    xs, hn = noise(n, L), decay(L, n)
    N = n + predelay + L - 1
    c = R.chain(xs, hn, predelay, N)
    want = np.concatenate([np.zeros(predelay), np.convolve(xs.astype(np.float64), hn.astype(np.float64))])
    bound = L * 2.0 ** -24 * np.concatenate([np.zeros(predelay), np.convolve(np.abs(xs).astype(np.float64), np.abs(hn).astype(np.float64))])
    assert len(c) == N and np.all(np.abs(c.astype(np.float64) - want) <= bound)
    assert np.array_equal(bits(R.chain(xs, hn, predelay, n)), bits(c[:n]))          # a shorter N cuts, nothing else


def test_the_energy_in_its_block_order():
    t = decay(700, 1)
    E = R.energy(t)
    t64 = t.astype(np.float64)
    assert abs(E - float(np.sum(t64 * t64))) <= 1e-12 * E
    blocks = [float(np.cumsum(t64[b:b + 256] ** 2)[-1]) for b in range(0, 700, 256)]      # cumsum adds in order
    assert E == (blocks[0] + blocks[1]) + blocks[2]
    assert R.energy(np.ones(1, dtype=np.float32)) == 1.0


def test_taps_fade_and_plan():
    ir = decay(500, 2)
    t, raw = R.taps(ir, R.Params(offset=100, length=300, fade=50))
    assert len(t) == 300 and np.array_equal(raw, ir[100:400]) and np.array_equal(t[:250], raw[:250])
    assert t[299] == raw[299] * np.float32(1.0 / 100.0) and t[250] == raw[250] * np.float32(99.0 / 100.0)
    assert R.plan(1000, 500, R.Params(offset=100, length=300, predelay=7)) == (300, 1000 + 7 + 299)
    assert R.plan(1000, 500, R.Params(length=10 ** 9, fade=10 ** 9)) == (500, 1499)
    assert R.plan(1000, 500, R.Params(tail=0)) == (500, 1000) and R.plan(1, 1, R.Params()) == (1, 1)
    t, raw = R.taps(ir, R.Params(fade=10 ** 9))                                     # f = L: the whole response under the ramp
    assert t[0] == raw[0] * np.float32(999.0 / 1000.0)


def test_identities():
    x = noise(600, 3, 0.3)
    x[5] = -0.0
    one = np.ones(1, dtype=np.float32)
    r = R.room(x, one, (), R.Params(wet=0, dry=-1, ceiling=0))
    assert np.array_equal(bits(r.y), bits(x + np.float32(0.0))) and not np.signbit(r.y[5]) and r.N == 600    # pass-through
    ir = decay(200, 4)
    T = gains()
    r = R.room(x, ir, [(0, 600, -1)], R.Params(dry=300, predelay=9, ceiling=0))                               # dry only
    assert np.array_equal(bits(r.y), bits(np.concatenate([(T[300] * x).astype(np.float32) + np.float32(0.0), np.zeros(208, np.float32)])))
    a = R.room(x, ir, (), R.Params(dry=-1, ceiling=0, predelay=2))
    b = R.room(x, ir, (), R.Params(dry=-1, ceiling=0, predelay=2 + 31))                                       # the shift
    assert np.array_equal(bits(b.y), bits(np.concatenate([np.zeros(31, np.float32), a.y])))
    assert np.array_equal(bits(R.room(x, ir, (), R.Params()).y), bits(R.room(x, ir, (), R.Params()).y))
    n = R.room(x, ir, (), R.Params(normalize=1, ceiling=0))
    assert n.gn == np.float32(1.0 / np.sqrt(n.E)) and abs(R.energy(n.hn) - 1.0) < 1e-5
    assert R.room(x, ir, (), R.Params(normalize=0)).gn == 1.0


def test_sends():
    x = noise(100, 5)
    T = gains()
    xs = R.sent(x, [(10, 20, 600), (20, 30, -1)], 250)
    assert np.array_equal(xs[:10], (x[:10] * T[250]).astype(np.float32)) and np.array_equal(xs[10:20], (x[10:20] * T[600]).astype(np.float32))
    assert not xs[20:30].any() and not np.signbit(xs[20:30]).any() and np.array_equal(xs[30:], (x[30:] * T[250]).astype(np.float32))
    assert np.array_equal(R.sent(x, (), 0), x)


@pytest.mark.parametrize("knock", ["descending", "wetfold", "predelay", "energy"])
def test_every_knock_is_caught(knock):
    x, ir = noise(900, 6, 0.1), decay(300, 7)
    p = R.Params(wet=700, fade=60, predelay=5, ceiling=0)
    good, bad = R.room(x, ir, [(100, 200, 900)], p), R.room(x, ir, [(100, 200, 900)], p, knock=knock)
    assert len(good.y) == len(bad.y) and not np.array_equal(bits(good.y), bits(bad.y))
    if knock in ("descending", "wetfold"):                # a rounding moved, not a different signal
        assert np.allclose(good.y, bad.y, rtol=0, atol=1e-5)


def test_the_ceiling_knock_is_caught():
    """pk == c exactly: c = 0.5 is a float32 (10^(-1/20) is not), the stated rule leaves the piece, the knock scales it."""
    x = np.zeros(50, dtype=np.float32)
    x[7] = 0.5
    one = np.ones(1, dtype=np.float32)
    p = R.Params(wet=0, dry=-1)
    good, bad = R.room(x, one, (), p, ceiling=0.5), R.room(x, one, (), p, knock="ceiling", ceiling=0.5)
    assert good.pk == 0.5 and not good.capped and good.sg == 1.0 and bad.capped
    x[7] = np.nextafter(np.float32(0.5), np.float32(1))
    over = R.room(x, one, (), p, ceiling=0.5)
    assert over.capped and over.sg == np.float32(0.5 / float(x[7])) and np.array_equal(bits(over.y), bits((x * over.sg).astype(np.float32)))
    assert not R.room(x, one, (), p._replace(ceiling=0), ceiling=0.5).capped       # ceiling = 0: reported, never applied
