"""GPU: the live room stage through the C ABI (include/fishtts_hip.h: "Live room"; ft_codec_room_stream_*, ft_codec_room_live,
CodecHipEngine.room_stream / room_live) against the room stage's restatement tests/room_ref.py on the whole programme with every
push's regions moved to the timeline - every sample's bits, E, gn, pk, L and N, whatever the cutting - and the bare limiter
(ft_codec_mix_stream_begin_bare) against the limiter of tests/mixlive_ref.py on m = x + 0.0.

TILE, SPAN, STAGE and LAUNCH are room_kernels.h's RM_TILE, RM_SPAN, RM_DC and RM_LAUNCH, as in tests/test_room_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import mix_ref as MR
from tests import mixlive_ref as ML
from tests import room_ref as R
from tests.test_codec_gpu import encode_shape, make_codec
from tests.test_mix_gpu import native as mix_native
from tests.test_room_gpu import LAUNCH, RAGGED, SPAN, bits, clip, decay, ir_at, ir_clip, native, noise, same_bits

pytestmark = pytest.mark.gpu
N_PROG = 3 * SPAN + 7


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(encode_shape(), max_frames=1024)
    yield e
    e.close()


def split_regions(regions, at, k):
    """The regions of the timeline that fall into the push [at, at + k), relative to it."""
    return [(max(a, at) - at, min(e, at + k) - at, s) for a, e, s in regions if max(a, at) < min(e, at + k)]


def stream(eng, x, c, p: R.Params, sizes, regions=(), rate=44100, channel=None):
    """x through a room stream in pushes of `sizes` (the last one final) -> (y, the report behind the last push, the counts)."""
    chunks, counts, at = [], [], 0
    with eng.room_stream(c, sample_rate=rate, params=native(p, -1 if channel is None else channel)) as rs:
        for j, k in enumerate(sizes):
            got = rs.push(x[at:at + k], split_regions(regions, at, k), final=j == len(sizes) - 1)
            chunks.append(got.copy())
            counts.append(len(got))
            at += k
            assert rs.report().n == sum(counts)
        rep = rs.report()
    assert at == len(x)
    return np.concatenate(chunks), rep, counts


def agree(rep, want, irF):
    assert (rep.n, rep.ir_len, rep.taps) == (want.N, len(irF), want.L)
    assert rep.energy == want.E and np.float32(rep.norm) == want.gn and np.float32(rep.peak) == want.pk
    assert rep.gain == 1.0 and not rep.capped


def cuttings(n, hist, seed):
    rng = np.random.default_rng(seed)
    out = {"one": [n], "small-then-rest": [1, 31, 1024, 4097, n - 1 - 31 - 1024 - 4097],
           "empties": [0, 0, 500, 0, n - 500, 0]}
    cuts = np.sort(rng.integers(0, n + 1, 12))
    out["random"] = [int(v) for v in np.diff(np.concatenate([[0], cuts, [n]]))]
    first = min(n, hist + 1000)
    rest, at = [first], first
    while at < n:
        k = min(n - at, int(rng.integers(1, 32)))
        rest.append(k)
        at += k
    out["long-then-tiny"] = rest
    assert all(sum(v) == n for v in out.values())
    return out


# ---- the chain's shapes: one reference per shape, five cuttings each
_SHAPES = {}


def shape(eng, L, predelay):
    if (L, predelay) not in _SHAPES:
        c = clip(decay(L, 100 + L), "f32", 44100)
        irF, _ = ir_at(eng, c, 44100)
        x = noise(N_PROG, 7 * L + predelay, 0.1)
        p = R.Params(wet=600, fade=min(40, L), predelay=predelay, ceiling=0)
        _SHAPES[(L, predelay)] = (c, irF, x, p, R.room(x, irF, (), p))
    return _SHAPES[(L, predelay)]


@pytest.mark.parametrize("predelay", [0, 777])
@pytest.mark.parametrize("L", [1, 33, 1025, RAGGED])
def test_any_cutting_gives_the_whole_call(eng, L, predelay):
    c, irF, x, p, want = shape(eng, L, predelay)
    assert want.L == L and want.N == N_PROG + predelay + L - 1
    for name, sizes in cuttings(N_PROG, predelay + L - 1, L + predelay).items():
        y, rep, counts = stream(eng, x, c, p, sizes)
        assert counts[:-1] == sizes[:-1] and counts[-1] == sizes[-1] + predelay + L - 1, name      # nothing is held back
        same_bits(y, want.y)
        agree(rep, want, irF)
    y, rep = eng.room_live(x, c, params=native(p))
    same_bits(y, want.y)
    agree(rep, want, irF)


@pytest.mark.parametrize("L,n,predelay,sizes", [(R.MAX_L, 3000, 5, [1000, 1, 1999]), (64, LAUNCH + 5, 3, [9, LAUNCH - 4])])
def test_exact_integers(eng, L, n, predelay, sizes):
    """x integers in [-64, 64], the response in {-1, 0, 1}: every partial sum is an integer below 2^24, so the wet signal is
    the int64 convolution whatever the order - a wrong index at the cap of L, in a carry shorter than the history, or in the
    second launch of a push that spans two, shows."""
    rng = np.random.default_rng(L)
    x = rng.integers(-64, 65, n)
    h = rng.integers(-1, 2, L)
    h[0], h[-1] = 1, -1
    want = np.concatenate([np.zeros(predelay, dtype=np.int64), np.convolve(x, h)])
    assert np.abs(want).max() < 1 << 24 and sum(sizes) == n and (n < LAUNCH or sizes[1] + predelay + L - 1 > LAUNCH)
    c = clip(h.astype(np.float32), "f32", 44100)
    p = R.Params(normalize=0, wet=0, dry=-1, predelay=predelay, ceiling=0)
    y, rep, _ = stream(eng, x.astype(np.float32), c, p, sizes)
    same_bits(y, want.astype(np.float32) + np.float32(0.0))
    assert rep.taps == L and rep.n == n + predelay + L - 1 and rep.peak == float(np.abs(want).max())


# ---- regions
@pytest.mark.parametrize("p", [R.Params(send=300, fade=20, ceiling=0), R.Params(send=-1, dry=-1, fade=20, ceiling=0),
                               R.Params(send=0, dry=1234, predelay=9, ceiling=0)], ids=["send", "muted-no-dry", "plain"])
def test_regions_move_to_the_timeline(eng, p):
    """Sends that change inside a push, at a push border (the region ends one push and another begins the next), across a
    4096 border, a muted region, and a line that crosses a cut as two regions of equal send."""
    n = 2 * SPAN + 300
    x = noise(n, 21, 0.1)
    regions = [(0, 100, 600), (100, 1000, -1), (1500, 1501, 6000), (2000, 3000, 0), (3000, SPAN + 50, 250), (SPAN + 50, SPAN + 900, -1),
               (SPAN + 2000, n, 1200)]
    sizes = [1500, 1500, 1000, SPAN - 4000 + 50, 2000, n - SPAN - 2050]
    irF, _ = ir_at(eng, ir_clip(), 44100)
    want = R.room(x, irF, regions, p)
    y, rep, _ = stream(eng, x, ir_clip(), p, sizes, regions)
    same_bits(y, want.y)
    agree(rep, want, irF)
    y1, rep1 = eng.room_live(x, ir_clip(), regions, params=native(p))
    same_bits(y1, want.y)
    y2, _ = eng.room(x, ir_clip(), regions, params=native(p), ceiling=False)
    same_bits(y, y2)


@pytest.mark.parametrize("rate,kind", [(44100, "mono"), (24000, "mono"), (16000, "48k")])
def test_equals_room_without_its_ceiling(eng, rate, kind):
    x = noise(SPAN + 77, rate, 0.4)
    p = R.Params(wet=300, fade=40, predelay=13, ceiling=0)
    whole, wrep = eng.room(x, ir_clip(kind), (), sample_rate=rate, params=native(p), ceiling=False)
    y, rep, _ = stream(eng, x, ir_clip(kind), p, [700, 0, 3000, len(x) - 3700], rate=rate)
    same_bits(y, whole)
    assert (rep.n, rep.ir_len, rep.taps, rep.energy, rep.norm, rep.peak, rep.ir) == \
           (wrep.n, wrep.ir_len, wrep.taps, wrep.energy, wrep.norm, wrep.peak, wrep.ir)


def test_two_streams_interleaved(eng):
    xa, xb = noise(5000, 81, 0.1), noise(7000, 82, 0.2)
    pa, pb = R.Params(fade=30, predelay=5, ceiling=0), R.Params(wet=0, dry=-1, send=500, ceiling=0)
    wa, _ = eng.room(xa, ir_clip(), (), params=native(pa), ceiling=False)
    wb, _ = eng.room(xb, ir_clip("48k"), (), params=native(pb), ceiling=False)
    sa = eng.room_stream(ir_clip(), params=native(pa))
    sb = eng.room_stream(ir_clip("48k"), params=native(pb))
    ga, gb, ia, ib = [], [], 0, 0
    rng = np.random.default_rng(99)
    while ia < len(xa) or ib < len(xb):
        ka, kb = int(rng.integers(0, 900)), int(rng.integers(0, 1300))
        ga.append(sa.push(xa[ia:ia + ka]).copy())
        gb.append(sb.push(xb[ib:ib + kb]).copy())
        ia, ib = ia + ka, ib + kb
    gb.append(sb.push(None, final=True).copy())
    ga.append(sa.push(None, final=True).copy())
    sa.close()
    sb.close()
    same_bits(np.concatenate(ga), wa)
    same_bits(np.concatenate(gb), wb)


def test_an_empty_programme(eng):
    p = R.Params(predelay=17, ceiling=0)
    with eng.room_stream(ir_clip(), params=native(p)) as rs:
        assert len(rs.push(None)) == 0
        tail = rs.push(None, final=True)
        rep = rs.report()
    assert len(tail) == 17 + 699 and not bits(tail).any() and rep.n == len(tail) and rep.peak == 0.0
    y, rep = eng.room_live(np.zeros(0, dtype=np.float32), ir_clip(), params=native(p))
    assert len(y) == 17 + 699 and not bits(y).any()
    y, rep = eng.room_live(np.zeros(0, dtype=np.float32), ir_clip(), params=native(p._replace(tail=0)))
    assert len(y) == 0 and rep.n == 0


@pytest.mark.parametrize("cut", [SPAN + 321, SPAN + 322, SPAN + 200, 3 * SPAN])
def test_a_nan_stays_in_rooms_range(eng, cut):
    """The NaN as the last sample of a push, the first of the next, in the middle of one, and in a one-push stream."""
    x = noise(3 * SPAN, 60, 0.1)
    p = R.Params(fade=30, predelay=17, ceiling=0)
    clean, _ = eng.room(x, ir_clip(), (), params=native(p), ceiling=False)
    j = SPAN + 321
    bad = x.copy()
    bad[j] = np.nan
    y, rep, _ = stream(eng, bad, ir_clip(), p, [cut, len(x) - cut])
    lo, hi = max(0, j - 1024), j + 17 + rep.taps + 1024
    outside = np.ones(len(y), dtype=bool)
    outside[lo:hi] = False
    assert np.array_equal(bits(y[outside]), bits(clean[outside])) and np.isnan(y[j]) and np.isfinite(rep.peak)


# ---- refusals
def _item(c, **kw):
    from fish_tts_amd import _lib as L
    from fish_tts_amd.wavfile import FORMATS
    data, info = c
    buf = np.frombuffer(data, dtype=np.uint8)
    item = dict(data=buf.ctypes.data + info.data_offset, n_frames=info.n_frames, rate=info.rate, channels=info.channels,
                fmt=FORMATS.index(info.fmt), channel=-1)
    item.update(kw)
    return L.ft_intake_item(**item), buf


def _begin(eng, c=None, rp_kw=None, rate=44100, item_kw=None, null=None):
    from fish_tts_amd import _lib as L
    rp = dict(channel=-1, normalize=1, wet=600, dry=0, send=0, ceiling=0, offset=0, length=0, fade=10, predelay=5, tail=-1)
    rp.update(rp_kw or {})
    it, keep = _item(c or ir_clip(), **(item_kw or {}))
    r = L.ft_room_params(**rp)
    h = C.c_void_p()
    args = dict(ir=C.byref(it), rp=C.byref(r), out=C.byref(h))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_room_stream_begin(eng._h, rate, args["ir"], args["rp"], args["out"])
    del keep
    return st, h


BEGIN_REFUSALS = [
    ("ir", dict(null="ir")), ("rp", dict(null="rp")), ("out", dict(null="out")),
    ("rate", dict(rate=7999)), ("rate-L", dict(rate=44101)),
    ("channel", dict(rp_kw=dict(channel=1))), ("channel-low", dict(rp_kw=dict(channel=-2))),
    ("normalize", dict(rp_kw=dict(normalize=2))), ("wet", dict(rp_kw=dict(wet=6001))), ("dry-low", dict(rp_kw=dict(dry=-2))),
    ("send", dict(rp_kw=dict(send=6001))), ("ceiling", dict(rp_kw=dict(ceiling=1))), ("ceiling-2", dict(rp_kw=dict(ceiling=2))),
    ("offset", dict(rp_kw=dict(offset=-1))), ("length", dict(rp_kw=dict(length=-1))), ("fade", dict(rp_kw=dict(fade=-1))),
    ("predelay", dict(rp_kw=dict(predelay=-1))), ("predelay-high", dict(rp_kw=dict(predelay=44101))),
    ("tail-low", dict(rp_kw=dict(tail=-2))), ("offset-all", dict(rp_kw=dict(offset=700))),
    ("L", dict(item_kw=dict(n_frames=R.MAX_L + 1), too_long=True)), ("tail", dict(rp_kw=dict(tail=5 + 699 + 1))),
    ("ir-frames", dict(item_kw=dict(n_frames=0))), ("ir-data", dict(item_kw=dict(data=None))), ("ir-fmt", dict(item_kw=dict(fmt=5))),
    ("ir-rate", dict(item_kw=dict(rate=7000))),
]


@pytest.mark.parametrize("name,kw", BEGIN_REFUSALS, ids=[r[0] for r in BEGIN_REFUSALS])
def test_begin_refusals(eng, name, kw):
    from fish_tts_amd import _lib as L
    kw = dict(kw)
    want = L.FT_ERR_TOO_LONG if kw.pop("too_long", False) else L.FT_ERR_ARG
    st, h = _begin(eng, **kw)
    assert st == want and not h.value, (name, st, eng.lib.ft_last_error(eng._h))


def test_begin_the_earlier_reason_wins(eng):
    from fish_tts_amd import _lib as L
    order = [("sample rate", dict(rate=7999)), ("channel", dict(rp_kw=dict(channel=3))), ("normalize", dict(rp_kw=dict(normalize=-1))),
             ("wet", dict(rp_kw=dict(wet=-1))), ("dry", dict(rp_kw=dict(dry=-2))), ("send neither", dict(rp_kw=dict(send=-2))),
             ("ceiling", dict(rp_kw=dict(ceiling=1))), ("offset must", dict(rp_kw=dict(offset=-1))),
             ("length", dict(rp_kw=dict(length=-1))), ("fade", dict(rp_kw=dict(fade=-1))), ("predelay", dict(rp_kw=dict(predelay=-1))),
             ("tail must", dict(rp_kw=dict(tail=-2))), ("fmt", dict(item_kw=dict(fmt=9)))]
    for (w1, k1), (w2, k2) in zip(order, order[1:]):
        kw = {}
        for k in (k2, k1):
            for key, v in k.items():
                kw[key] = {**kw.get(key, {}), **v} if isinstance(v, dict) else v
        st, h = _begin(eng, **kw)
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and not h.value and w1 in msg and w2 not in msg.replace(w1, ""), (w1, w2, msg)


def test_a_silent_response_is_refused_at_begin(eng):
    from fish_tts_amd import _lib as L
    zeros = clip(np.zeros(50, dtype=np.float32), "f32", 44100)
    st, h = _begin(eng, zeros, rp_kw=dict(predelay=0))
    assert st == L.FT_ERR_ARG and not h.value and "energy" in eng.lib.ft_last_error(eng._h).decode()
    st, h = _begin(eng, zeros, rp_kw=dict(normalize=0, predelay=0))       # without normalize it is a room of silence
    assert st == L.FT_OK and h.value
    eng.lib.ft_codec_room_stream_end(h)
    x = noise(300, 71, 0.1)                                              # ... and the context serves the next stream
    y, _, _ = stream(eng, x, zeros, R.Params(normalize=0, ceiling=0), [100, 200])
    same_bits(y, np.concatenate([x + np.float32(0.0), np.zeros(49, dtype=np.float32)]))


def _push(eng, h, x, n=None, regions=(), R_=None, final=0, cap=None, null=None):
    from fish_tts_amd import _lib as L
    reg = (L.ft_send_region * max(len(regions), 1))(*[L.ft_send_region(a, e, s, 0) for a, e, s in regions])
    n = len(x) if n is None else n
    size = len(x) + 5 + 699
    y = np.full(size, 7.0, dtype=np.float32)
    n_out = C.c_int64(-7)
    args = dict(x=x.ctypes.data_as(C.c_void_p), regions=reg, y=y.ctypes.data_as(C.c_void_p), n_out=C.byref(n_out))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_room_stream_push(h, args["x"], n, args["regions"], len(regions) if R_ is None else R_, final, args["y"],
                                           size if cap is None else cap, args["n_out"])
    return st, y, n_out.value


PUSH_REFUSALS = [
    ("n", dict(n=-1)), ("x", dict(null="x")), ("n_out", dict(null="n_out")),
    ("regions-null", dict(null="regions", regions=[(3, 9, 100)])), ("R", dict(R_=4097)), ("R-neg", dict(R_=-1)),
    ("region-order", dict(regions=[(5, 9, 0), (8, 12, 0)])), ("region-empty", dict(regions=[(5, 5, 0)])),
    ("region-outside", dict(regions=[(5, 301, 0)])), ("region-send", dict(regions=[(5, 9, 6001)])),
    ("region-send-low", dict(regions=[(5, 9, -2)])),
    ("long", dict(n=(1 << 28) - 1000, too_long=True)), ("long-one", dict(n=(1 << 28) + 1, too_long=True)),
    ("capacity", dict(cap=299)), ("capacity-final", dict(final=1, cap=300 + 5 + 699 - 1)), ("y", dict(null="y")),
]


@pytest.mark.parametrize("name,kw", PUSH_REFUSALS, ids=[r[0] for r in PUSH_REFUSALS])
def test_a_refused_push_leaves_its_stream_as_it_was(eng, name, kw):
    """Two good pushes, the refused one between them (nothing written, no counter moved), the final one: the whole call's bits."""
    from fish_tts_amd import _lib as L
    kw = dict(kw)
    want_st = L.FT_ERR_TOO_LONG if kw.pop("too_long", False) else L.FT_ERR_ARG
    x = noise(900, 70, 0.1)
    whole, _ = eng.room(x, ir_clip(), [(603, 609, 100)], params=native(R.Params(wet=600, fade=10, predelay=5, ceiling=0)), ceiling=False)
    st, h = _begin(eng)
    assert st == L.FT_OK
    try:
        st, y0, k0 = _push(eng, h, np.ascontiguousarray(x[:300]))
        assert st == L.FT_OK and k0 == 300
        mid = np.ascontiguousarray(x[300:600])
        st, y, k = _push(eng, h, mid, **kw)
        assert st == want_st, (name, st, eng.lib.ft_last_error(eng._h))
        assert np.all(y == 7.0) and k == -7
        info = L.ft_room_info()
        assert eng.lib.ft_codec_room_stream_info(h, C.byref(info)) == L.FT_OK and info.N == 300
        st, y1, k1 = _push(eng, h, mid)
        assert st == L.FT_OK and k1 == 300
        st, y2, k2 = _push(eng, h, np.ascontiguousarray(x[600:]), regions=[(3, 9, 100)], final=1)
        assert st == L.FT_OK and k2 == 300 + 5 + 699
        same_bits(np.concatenate([y0[:k0], y1[:k1], y2[:k2]]), whole)
        st, y3, k3 = _push(eng, h, mid)                                   # behind the final push
        assert st == L.FT_ERR_STATE and np.all(y3 == 7.0) and k3 == -7
        st, _, _ = _push(eng, h, mid, n=-1, regions=[(5, 5, 0)])          # ... whatever else is wrong with it
        assert st == L.FT_ERR_STATE
    finally:
        eng.lib.ft_codec_room_stream_end(h)


def test_push_the_earlier_reason_wins(eng):
    from fish_tts_amd import _lib as L
    x = noise(300, 72, 0.1)
    st, h = _begin(eng)
    assert st == L.FT_OK
    try:
        order = [("n must", L.FT_ERR_ARG, dict(n=-1)), ("send region", L.FT_ERR_ARG, dict(regions=[(5, 5, 0)])),
                 ("2^28", L.FT_ERR_TOO_LONG, dict(n=(1 << 28) + 1)), ("capacity", L.FT_ERR_ARG, dict(cap=1))]
        for (w1, s1, k1), (w2, s2, k2) in zip(order, order[1:]):
            if "n" in k1 and "n" in k2:
                continue
            kw = {**k2, **k1}
            if "regions" in kw and kw.get("n", 300) > 300:
                kw["regions"] = [(5, 5, 0)]
            st, _, _ = _push(eng, h, x, **kw)
            msg = eng.lib.ft_last_error(eng._h).decode()
            assert st == s1 and w1 in msg and w2 not in msg, (w1, w2, msg)
        st, _, _ = _push(eng, h, x, n=(1 << 28) + 1, cap=1)
        assert st == L.FT_ERR_TOO_LONG
    finally:
        eng.lib.ft_codec_room_stream_end(h)


def test_python_refusals(eng):
    with pytest.raises(ValueError, match="RoomParams"):
        eng.room_stream(ir_clip(), params=(1, 2))
    with eng.room_stream(ir_clip(), params=native(R.Params(ceiling=0))) as rs:
        with pytest.raises(ValueError, match="region"):
            rs.push(noise(10, 1), [(0, 11, 0)])
        with pytest.raises(ValueError, match="region"):
            rs.push(noise(10, 1), [(0, 5, 6001)])
    with pytest.raises(RuntimeError, match="closed"):
        rs.push(None)
    with pytest.raises(RuntimeError, match="closed"):
        rs.report()
    rs.close()                                                            # twice: nothing happens


# ---- the bare limiter: Live mix with the bed term +0.0
def bare_ref(x, rate, p: MR.Params):
    """m = s + 0.0 on Live mix's timeline, then its limiter by tests/mixlive_ref.py's own functions."""
    s = np.concatenate([np.zeros(p.lead, dtype=np.float32), np.asarray(x, dtype=np.float32), np.zeros(p.tail, dtype=np.float32)])
    m = (s + np.float32(0.0)).astype(np.float32)
    H = MR.hop(rate)
    N = len(m)
    need = ML.needs(ML.hop_peaks(m, H))
    Lk = ML.limit(need)
    l = MR.gains()[Lk]
    i = np.arange(N, dtype=np.int64)
    k, j = i // H, i % H
    r = j.astype(np.float32) / np.float32(H)
    y = (m * MR.fmaf32(r, (l[k + 1] - l[k]).astype(np.float32), l[k])).astype(np.float32)
    return y, m, Lk


def bare_stream(eng, x, rate, p, sizes):
    mp = mix_native(p)
    chunks, at, total = [], 0, 0
    with eng.mix_stream(None, sample_rate=rate, params=mp, bedless=True) as ms:
        for j, k in enumerate(sizes):
            final = j == len(sizes) - 1
            got = ms.push(x[at:at + k], final=final)
            at += k
            total += len(got)
            assert total == ML.emitted(at, final, rate, p)
            chunks.append(got.copy())
    return np.concatenate(chunks)


@pytest.mark.parametrize("rate,p", [(16000, MR.Params(attack=2, release=3, loop=0)),
                                   (44100, MR.Params(attack=2, release=3, lead=700, tail=333, loop=0))], ids=["16k", "44k-lead-tail"])
def test_the_bare_limiter(eng, rate, p):
    H = rate // 50
    n = 40 * H + 123
    x = noise(n, rate, 0.1)
    x[0] = -0.0
    for a, e, amp in [(5 * H + 3, 6 * H, 1.4), (17 * H, 17 * H + 40, 2.5), (30 * H - 9, 31 * H + 9, 0.95)]:
        x[a:e] = noise(e - a, a, amp)
    want, m, Lk = bare_ref(x, rate, p)
    assert Lk.max() > 0 and float(np.abs(m).max()) > float(ML.CF) and float(np.abs(want).max()) <= float(ML.CF) * (1 + 1e-6)
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.integers(0, n + 1, 9))
    for sizes in ([n], [1, H - 1, 7 * H, n - 8 * H], [0, 3 * H + 1, 0, n - 3 * H - 1, 0],
                  [int(v) for v in np.diff(np.concatenate([[0], cuts, [n]]))]):
        same_bits(bare_stream(eng, x, rate, p, sizes), want)
    quiet = noise(n, 3, 0.05)
    quiet[1] = -0.0
    got = bare_stream(eng, quiet, rate, p, [n // 3, n - n // 3])
    same_bits(got, np.concatenate([np.zeros(p.lead, dtype=np.float32), quiet + np.float32(0.0), np.zeros(p.tail, dtype=np.float32)]))


def test_bare_is_asked_for_by_name(eng):
    from fish_tts_amd import _lib as L
    with pytest.raises(ValueError, match="bedless"):
        eng.mix_stream(ir_clip(), bedless=True)
    with pytest.raises(ValueError, match="bedless"):
        eng.mix_stream(None, stereo=True, bedless=True)
    mp = eng._mix_params(mix_native(MR.Params()))
    h = C.c_void_p()
    assert eng.lib.ft_codec_mix_stream_begin(eng._h, 44100, None, C.byref(mp), C.byref(h)) == L.FT_ERR_ARG and not h.value
    assert eng.lib.ft_codec_mix_stream_begin_bare(eng._h, 44100, None, C.byref(h)) == L.FT_ERR_ARG and not h.value
    bad = eng._mix_params(mix_native(MR.Params(attack=0)))
    assert eng.lib.ft_codec_mix_stream_begin_bare(eng._h, 44100, C.byref(bad), C.byref(h)) == L.FT_ERR_ARG and not h.value
