"""GPU: the room stage through the C ABI (include/fishtts_hip.h: "Room"; ft_test_room_conv, ft_codec_room,
CodecHipEngine.room) against its restatement tests/room_ref.py.  The convolution launches are compared on taps the test
gives; the whole stage with the impulse response at the output rate taken from the existing calls - intake(), then the
resampler hook - so everything behind the response's preparation is compared, and every comparison is exact: every sample's
bits, E, gn, pk, sg.

TILE is what one wave of room_conv_kernel covers, SPAN one workgroup, STAGE the chain terms of one LDS stage, LAUNCH the
outputs of one launch (room_kernels.h: RM_TILE, RM_SPAN, RM_DC, RM_LAUNCH)."""
import ctypes as C

import numpy as np
import pytest

from tests import intake_ref as IR
from tests import room_ref as R
from tests.test_codec_gpu import encode_shape, make_codec

pytestmark = pytest.mark.gpu
TILE, SPAN, STAGE, LAUNCH = 1024, 4096, 1024, 1 << 22
RAGGED = 2 * STAGE + 452                     # L + 31 terms: two whole stages and a ragged third of 483 (an odd count)


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(encode_shape(), max_frames=1024)       # 65 536 samples through the resampler hook
    yield e
    e.close()


def clip(v, fmt="f32", rate=44100, **kw):
    from fish_tts_amd.wavfile import parse_wav
    b = IR.wav_bytes(v, fmt, rate, **kw)
    return b, parse_wav(b)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    same = bits(got) == bits(want)
    assert len(got) == len(want) and same.all(), (int((~same).sum()), int(np.argmin(same)))


def noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ---- the convolution launches alone
_CHAINS = {}


def chain0(L, n):
    """(xs, hn, c) with predelay 0 and the full tail, computed once per (L, n): random float32 of every sign and scale."""
    if (L, n) not in _CHAINS:
        rng = np.random.default_rng(1000 * L + n)
        xs = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32)
        hn = (rng.standard_normal(L) * np.exp(rng.uniform(-8, 0, L))).astype(np.float32)
        _CHAINS[(L, n)] = (xs, hn, R.chain(xs, hn, 0, n + L - 1))
    return _CHAINS[(L, n)]


@pytest.mark.parametrize("n", [1, 31, 1023, 1024, 1025, 3 * SPAN + 7])
@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 1025, RAGGED])
def test_conv_bit_for_bit(eng, L, n):
    """Every L x n, each with the predelays 0, 1 and 777 and N at n, at a partial tail and at the full tail.  One
    reference per (L, n): the chain of output i under predelay p is term for term the chain of output i - p under predelay 0,
    and for i < p every term is a product with +0.0, which leaves +0.0 - so c_p is c_0 shifted, and a shorter N cuts it."""
    xs, hn, c0 = chain0(L, n)
    for p in (0, 1, 777):
        full = n + p + L - 1
        want = np.concatenate([np.zeros(p, dtype=np.float32), c0])
        for N in sorted({n, n + (p + L - 1) // 2, full}):
            same_bits(eng.test_room_conv(xs, hn, p, N), want[:N])


def test_conv_shift_is_the_reference_too(eng):
    """The shift rule the cases above lean on, against the restatement itself at one shape."""
    xs, hn, c0 = chain0(33, 1025)
    want = R.chain(xs, hn, 777, 1025 + 777 + 32)
    assert np.array_equal(bits(want), bits(np.concatenate([np.zeros(777, dtype=np.float32), c0])))
    same_bits(eng.test_room_conv(xs, hn, 777, len(want)), want)


@pytest.mark.parametrize("L,n,predelay", [(R.MAX_L, 3000, 5), (4096, (1 << 20) + 5, 0), (64, LAUNCH + 5, 3)])
def test_conv_exact_integers(eng, L, n, predelay):
    """x integers in [-64, 64], hn in {-1, 0, 1}: every partial sum is an integer below 2^24 (64 L <= 2^23), so c is the int64
    convolution whatever the order - a wrong index at the cap, at a stage border or across the launches (the third case has
    more outputs than one launch takes) shows."""
    rng = np.random.default_rng(L)
    x = rng.integers(-64, 65, n)
    h = rng.integers(-1, 2, L)
    h[0], h[-1] = 1, -1
    N = n + predelay + L - 1
    # np.convolve on int64 is exact
    want = np.concatenate([np.zeros(predelay, dtype=np.int64), np.convolve(x, h)])
    assert np.abs(want).max() < 1 << 24
    got = eng.test_room_conv(x.astype(np.float32), h.astype(np.float32), predelay, N)
    same_bits(got, want.astype(np.float32) + np.float32(0.0))


def test_conv_keeps_subnormals_and_states_negative_zero(eng):
    tiny = np.float32(2.0 ** -140)
    xs = np.array([tiny, -tiny, 0.0, -0.0, 1.0], dtype=np.float32)
    hn = np.array([1.0, 0.5], dtype=np.float32)
    want = R.chain(xs, hn, 0, 6)
    assert want[0] == tiny and want[1] == -tiny / 2 and want[1] != 0
    same_bits(eng.test_room_conv(xs, hn, 0, 6), want)
    # a chain that ends at -0.0: x = -tiny under a tap so small that the product rounds to -0.0
    hn2 = np.array([2.0 ** -20], dtype=np.float32)
    got = eng.test_room_conv(np.array([-tiny], dtype=np.float32), hn2, 0, 1)
    assert got[0] == 0 and not np.signbit(got[0])
    same_bits(got, R.chain(np.array([-tiny], dtype=np.float32), hn2, 0, 1))


# ---- the whole stage
_IRS = {}


def ir_at(eng, c, rate, channel=None):
    """The impulse response at the output rate by the existing calls, computed once per clip."""
    key = (c[0], rate, channel)
    if key not in _IRS:
        pieces, reps = eng.intake([c], channel=channel)
        i44 = pieces[0].copy()
        _IRS[key] = (i44 if rate == 44100 else eng.test_resample(i44, rate).copy(), reps[0])
    return _IRS[key]


def native(p: R.Params, channel=-1):
    from fish_tts_amd.room import RoomParams
    return RoomParams(channel, p.normalize, p.wet, p.dry, p.send, p.offset, p.length, p.fade, p.predelay, p.tail)


def check(eng, x, c, p: R.Params, regions=(), rate=44100, channel=None):
    """One call against the restatement, everything exact.  Returns (got y, report, reference)."""
    irF, irep = ir_at(eng, c, rate, channel)
    want = R.room(x, irF, regions, p)
    y, rep = eng.room(x, c, regions, sample_rate=rate, params=native(p, -1 if channel is None else channel), ceiling=bool(p.ceiling))
    assert (rep.n, rep.ir_len, rep.taps) == (want.N, len(irF), want.L)
    assert rep.energy == want.E and np.float32(rep.norm) == want.gn
    assert np.float32(rep.peak) == want.pk and np.float32(rep.gain) == want.sg and rep.capped == want.capped
    assert rep.ir == irep
    same_bits(y, want.y)
    return y, rep, want


def decay(n, seed, tau=0.25):
    """A room-like response: noise under an exponential decay."""
    return (noise(n, seed, 0.5) * np.exp(-np.arange(n) / (tau * n))).astype(np.float32)


_CLIPS = {}


def ir_clip(kind="mono"):
    if kind not in _CLIPS:
        if kind == "mono":
            _CLIPS[kind] = clip(decay(700, 5), "f32", 44100)
        elif kind == "48k":
            _CLIPS[kind] = clip(decay(1500, 6), "f32", 48000)
        elif kind == "stereo":
            k = np.clip(np.round(np.stack([decay(600, 7), decay(600, 8)], 1) * 32768), -32767, 32767).astype(np.int64)
            _CLIPS[kind] = clip(k, "s16", 44100)
        elif kind == "one":
            _CLIPS[kind] = clip(np.ones(1, dtype=np.float32), "f32", 44100)
    return _CLIPS[kind]


@pytest.mark.parametrize("rate,kind", [(44100, "mono"), (24000, "mono"), (16000, "48k")])
def test_rates(eng, rate, kind):
    x = noise(2 * SPAN + 77, rate, 0.1)
    y, rep, want = check(eng, x, ir_clip(kind), R.Params(wet=600, fade=40, predelay=13), rate=rate)
    assert (rep.ir_len == 700) == (rate == 44100) and rep.n == len(x) + 13 + rep.ir_len - 1


@pytest.mark.parametrize("channel", [None, 1])
def test_two_channel_response(eng, channel):
    x = noise(3000, 3, 0.1)
    check(eng, x, ir_clip("stereo"), R.Params(wet=900, fade=30), channel=channel)
    a, b = ir_at(eng, ir_clip("stereo"), 44100, None)[0], ir_at(eng, ir_clip("stereo"), 44100, 1)[0]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("p", [R.Params(offset=100), R.Params(offset=699), R.Params(length=1), R.Params(length=300, fade=300),
                               R.Params(offset=50, length=10 ** 6, fade=10 ** 6), R.Params(length=257, fade=1),
                               R.Params(normalize=0, wet=0), R.Params(normalize=0, length=256, fade=17, dry=-1),
                               R.Params(predelay=44100, length=5), R.Params(tail=0), R.Params(tail=350, predelay=3),
                               R.Params(tail=699 + 9, predelay=9)],
                         ids=lambda p: "-".join(f"{k}{v}" for k, v in p._asdict().items() if v != getattr(R.Params(), k)) or "default")
def test_response_shapes_and_tails(eng, p):
    x = noise(1500, 11, 0.1)
    y, rep, want = check(eng, x, ir_clip(), p)
    if p.length == 1:
        assert rep.taps == 1 and rep.n == 1500


def test_regions_sends_and_no_dry(eng):
    x = noise(5000, 21, 0.1)
    regions = [(0, 100, 600), (100, 1000, -1), (1500, 1501, 6000), (2000, 4999, 0), (4999, 5000, -1)]
    check(eng, x, ir_clip(), R.Params(send=300, fade=20), regions)
    check(eng, x, ir_clip(), R.Params(send=-1, dry=-1, fade=20), regions)
    check(eng, x, ir_clip(), R.Params(send=0, dry=1234), regions[:1])
    check(eng, x, ir_clip(), R.Params(send=777))                       # a send without regions: the send pass runs


def test_ceiling_binds_and_does_not(eng):
    x = noise(3000, 31, 0.1)
    y, rep, want = check(eng, x, ir_clip(), R.Params(wet=1200))
    assert not rep.capped and rep.gain == 1.0
    loud = noise(3000, 32, 0.6)
    y, rep, want = check(eng, loud, ir_clip(), R.Params(wet=0))
    assert rep.capped and float(np.abs(y).max()) <= R.CEILING * (1 + 2.0 ** -23)
    y0, rep0, want0 = check(eng, loud, ir_clip(), R.Params(wet=0, ceiling=0))
    assert not rep0.capped and rep0.gain == 1.0 and rep0.peak == rep.peak and rep0.peak > R.CEILING
    same_bits(y, (y0 * np.float32(rep.gain)).astype(np.float32))


def test_pass_through(eng):
    x = noise(SPAN + 5, 41, 0.3)
    x[7], x[8] = -0.0, 0.0
    y, rep, want = check(eng, x, ir_clip("one"), R.Params(wet=0, dry=-1, ceiling=0))
    assert rep.taps == 1 and rep.n == len(x) and rep.energy == 1.0 and rep.norm == 1.0
    same_bits(y, x + np.float32(0.0))                                  # y = x, the -0.0 a +0.0
    assert not np.signbit(y[7])


def test_dry_only_when_every_send_is_muted(eng):
    x = noise(2000, 42, 0.1)
    T = R.gains()
    y, rep, want = check(eng, x, ir_clip(), R.Params(send=-1, dry=250, predelay=4))
    assert rep.n == 2000 + 4 + 699
    same_bits(y, np.concatenate([(T[250] * x).astype(np.float32) + np.float32(0.0), np.zeros(4 + 699, dtype=np.float32)]))
    y2, _, _ = check(eng, x, ir_clip(), R.Params(dry=250, predelay=4), [(0, 2000, -1)])
    same_bits(y2, y)


def test_predelay_shifts_the_wet_signal(eng):
    x = noise(2500, 43, 0.1)
    a, _, _ = check(eng, x, ir_clip(), R.Params(dry=-1, ceiling=0, predelay=10))
    b, _, _ = check(eng, x, ir_clip(), R.Params(dry=-1, ceiling=0, predelay=10 + 321))
    same_bits(b, np.concatenate([np.zeros(321, dtype=np.float32), a]))


def test_calls_repeat_and_buffers_regrow(eng):
    small, big = noise(300, 50, 0.1), noise(5 * SPAN + 1, 51, 0.1)
    p = R.Params(fade=100, predelay=2)
    a1, _, _ = check(eng, small, ir_clip(), p, [(10, 20, 500)])
    b1, _, _ = check(eng, big, ir_clip("48k"), p)
    a2, _, _ = check(eng, small, ir_clip(), p, [(10, 20, 500)])
    b2, _, _ = check(eng, big, ir_clip("48k"), p)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))


def test_a_nan_stays_in_its_range(eng):
    x = noise(3 * SPAN, 60, 0.1)
    p = R.Params(fade=30, predelay=17, ceiling=0)
    clean, rep, _ = check(eng, x, ir_clip(), p)
    j = SPAN + 321
    bad = x.copy()
    bad[j] = np.nan
    y, rep2 = eng.room(bad, ir_clip(), (), params=native(p), ceiling=False)
    lo, hi = max(0, j - 1024), j + 17 + rep.taps + 1024
    outside = np.ones(len(y), dtype=bool)
    outside[lo:hi] = False
    assert np.array_equal(bits(y[outside]), bits(clean[outside])) and np.isnan(y[j]) and np.isfinite(rep2.peak)


# ---- refusals, in the header's order: each refused call leaves the next good call's result as it was
def _raw(eng, x, c, rp_kw=None, rate=44100, item_kw=None, null=None, cap=None, n=None, regions=None, R_=None):
    from fish_tts_amd import _lib as L
    from fish_tts_amd.wavfile import FORMATS
    data, info = c
    buf = np.frombuffer(data, dtype=np.uint8)
    item = dict(data=buf.ctypes.data + info.data_offset, n_frames=info.n_frames, rate=info.rate, channels=info.channels,
                fmt=FORMATS.index(info.fmt), channel=-1)
    item.update(item_kw or {})
    rp = dict(channel=-1, normalize=1, wet=600, dry=0, send=0, ceiling=1, offset=0, length=0, fade=10, predelay=5, tail=-1)
    rp.update(rp_kw or {})
    it, r = L.ft_intake_item(**item), L.ft_room_params(**rp)
    regions = [(3, 9, 100)] if regions is None else regions
    reg = (L.ft_send_region * max(len(regions), 1))(*[L.ft_send_region(a, e, s, 0) for a, e, s in regions])
    n = len(x) if n is None else n
    N = len(x) + 5 + 699
    y = np.full(N, 7.0, dtype=np.float32)
    total, out = C.c_int64(-7), L.ft_room_info()
    args = dict(x=x.ctypes.data_as(C.c_void_p), ir=C.byref(it), rp=C.byref(r), y=y.ctypes.data_as(C.c_void_p), total=C.byref(total),
                info=C.byref(out), regions=reg)
    if null:
        args[null] = None
    st = eng.lib.ft_codec_room(eng._h, args["x"], n, rate, args["regions"], len(regions) if R_ is None else R_, args["ir"],
                               args["rp"], args["y"], N if cap is None else cap, args["total"], args["info"])
    return st, y, total.value, buf


REFUSALS = [
    ("x", dict(null="x")), ("ir", dict(null="ir")), ("rp", dict(null="rp")), ("y", dict(null="y")), ("total", dict(null="total")),
    ("info", dict(null="info")),
    ("rate", dict(rate=7999)), ("rate-L", dict(rate=44101)),
    ("n", dict(n=0)),
    ("regions-null", dict(null="regions")), ("R", dict(R_=4097)), ("R-neg", dict(R_=-1)),
    ("region-order", dict(regions=[(5, 9, 0), (8, 12, 0)])), ("region-empty", dict(regions=[(5, 5, 0)])),
    ("region-outside", dict(regions=[(5, 1 << 20, 0)])), ("region-send", dict(regions=[(5, 9, 6001)])),
    ("region-send-low", dict(regions=[(5, 9, -2)])),
    ("channel", dict(rp_kw=dict(channel=1))), ("channel-low", dict(rp_kw=dict(channel=-2))),
    ("normalize", dict(rp_kw=dict(normalize=2))),
    ("wet", dict(rp_kw=dict(wet=6001))), ("wet-neg", dict(rp_kw=dict(wet=-1))),
    ("dry", dict(rp_kw=dict(dry=6001))), ("dry-low", dict(rp_kw=dict(dry=-2))),
    ("send", dict(rp_kw=dict(send=6001))), ("send-low", dict(rp_kw=dict(send=-2))),
    ("ceiling", dict(rp_kw=dict(ceiling=-1))),
    ("offset", dict(rp_kw=dict(offset=-1))), ("length", dict(rp_kw=dict(length=-1))), ("fade", dict(rp_kw=dict(fade=-1))),
    ("predelay", dict(rp_kw=dict(predelay=-1))), ("predelay-high", dict(rp_kw=dict(predelay=44101))),
    ("tail-low", dict(rp_kw=dict(tail=-2))),
    ("n-long", dict(n=(1 << 28) + 1, regions=[], too_long=True)),
    ("offset-all", dict(rp_kw=dict(offset=700))),
    ("L", dict(item_kw=dict(n_frames=R.MAX_L + 1), too_long=True)),
    ("tail", dict(rp_kw=dict(tail=5 + 699 + 1))),
    ("N", dict(n=(1 << 28) - 100, regions=[], too_long=True)),
    ("capacity", dict(cap=10)),
    ("ir-frames", dict(item_kw=dict(n_frames=0))), ("ir-data", dict(item_kw=dict(data=None))),
    ("ir-fmt", dict(item_kw=dict(fmt=5))), ("ir-channels", dict(item_kw=dict(channels=9))),
    ("ir-rate", dict(item_kw=dict(rate=7000))),
    ("ir-length", dict(item_kw=dict(n_frames=1 << 29), rp_kw=dict(length=100), cap=1 << 40, too_long=True)),
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(eng, name, kw):
    from fish_tts_amd import _lib as L
    kw = dict(kw)
    want_st = L.FT_ERR_TOO_LONG if kw.pop("too_long", False) else L.FT_ERR_ARG
    x = noise(300, 70, 0.1)
    c = ir_clip()
    st, y0, t0, _ = _raw(eng, x, c)
    assert st == L.FT_OK and t0 == len(x) + 5 + 699
    st, y, t, _ = _raw(eng, x, c, **kw)
    assert st == want_st, (name, st, eng.lib.ft_last_error(eng._h))
    assert np.all(y == 7.0) and t == -7                              # nothing written
    st, y1, t1, _ = _raw(eng, x, c)
    assert st == L.FT_OK and t1 == t0 and np.array_equal(bits(y1), bits(y0))


def test_a_silent_response_is_refused_after_the_launches(eng):
    from fish_tts_amd import _lib as L
    x = noise(300, 71, 0.1)
    zeros = clip(np.zeros(50, dtype=np.float32), "f32", 44100)
    st, y, t, _ = _raw(eng, x, zeros, rp_kw=dict(predelay=0))
    assert st == L.FT_ERR_ARG and "energy" in eng.lib.ft_last_error(eng._h).decode() and np.all(y == 7.0) and t == -7
    st, y, t, _ = _raw(eng, x, zeros, rp_kw=dict(normalize=0, predelay=0))        # without normalize it is a room of silence
    assert st == L.FT_OK and t == 300 + 49 and np.array_equal(bits(y[:300]), bits(x + np.float32(0.0)))


def test_the_earlier_reason_wins(eng):
    """The order of the checks: a call wrong in two ways is refused for the earlier one (the message names it)."""
    from fish_tts_amd import _lib as L
    x = noise(200, 72, 0.1)
    order = [("sample rate", dict(rate=7999)), ("n must", dict(n=0)), ("send region", dict(regions=[(5, 5, 0)])),
             ("channel", dict(rp_kw=dict(channel=3))), ("normalize", dict(rp_kw=dict(normalize=-1))),
             ("wet", dict(rp_kw=dict(wet=-1))), ("dry", dict(rp_kw=dict(dry=-2))), ("send neither", dict(rp_kw=dict(send=-2))),
             ("ceiling", dict(rp_kw=dict(ceiling=2))), ("offset must", dict(rp_kw=dict(offset=-1))),
             ("length", dict(rp_kw=dict(length=-1))), ("fade", dict(rp_kw=dict(fade=-1))), ("predelay", dict(rp_kw=dict(predelay=-1))),
             ("tail must", dict(rp_kw=dict(tail=-2))), ("capacity", dict(cap=1)), ("fmt", dict(item_kw=dict(fmt=9)))]
    for (w1, k1), (w2, k2) in zip(order, order[1:]):
        kw = {}
        for k in (k2, k1):
            for key, v in k.items():
                kw[key] = {**kw.get(key, {}), **v} if isinstance(v, dict) else v
        st, *_ = _raw(eng, x, ir_clip(), **kw)
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and w1 in msg and w2 not in msg.replace(w1, ""), (w1, w2, msg)
