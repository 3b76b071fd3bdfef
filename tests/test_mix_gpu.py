"""GPU: the mix stage through the C ABI (include/fishtts_hip.h: "Mix"; ft_codec_mix, CodecHipEngine.mix) against its
restatement tests/mix_ref.py.  The bed at the output rate comes from the existing calls - intake(), then the resampler hook -
so the stage is compared from the timeline onward, and every comparison is exact: D_k, N, the counts, every sample's bits,
pk, sg.  Fo = 8000 (H = 160) unless a rate is the point.

SPAN is what one workgroup of mix_kernel covers: 256 lanes x 4 samples x 4 steps (stage_kernels.h: MX_SPAN)."""
import ctypes as C

import numpy as np
import pytest

from tests import intake_ref as IR
from tests import mix_ref as R
from tests.test_codec_gpu import encode_shape, make_codec

pytestmark = pytest.mark.gpu
FO = 8000
H = 160
SPAN = 256 * 4 * 4


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


def noise(n, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def speech(n, seed=0, amp=0.3, quiet=()):
    """Noise with silent stretches [a, b)."""
    x = noise(n, seed, amp)
    for a, b in quiet:
        x[a:b] = 0.0
    return x


_BEDS = {}


def bed_at(eng, c, rate, loudness=None, channel=None):
    """The bed at the output rate by the existing calls, computed once per clip."""
    key = (c[0], rate, loudness, channel)
    if key not in _BEDS:
        pieces, reps = eng.intake([c], loudness=loudness, channel=channel)
        b44 = pieces[0].copy()
        _BEDS[key] = (b44 if rate == 44100 else eng.test_resample(b44, rate).copy(), reps[0])
    return _BEDS[key]


def native(p: R.Params, bed_loudness=0, channel=-1):
    from fish_tts_amd.mix import MixParams
    return MixParams(bed_loudness, channel, p.depth, p.threshold, p.attack, p.release, p.lead, p.tail, p.fade_in, p.fade_out,
                     p.offset, p.loop)


def check(eng, x, c, p: R.Params, rate=FO, loudness=None, channel=None):
    """One call against the restatement, everything exact.  Returns (got y, report, reference)."""
    bed, brep = bed_at(eng, c, rate, loudness, channel)
    want = R.mix(x, bed, rate, p)
    y, rep, D = eng.mix(x, c, sample_rate=rate, nodes=True,
                        params=native(p, 0 if loudness is None else int(round(100 * loudness)), -1 if channel is None else channel))
    assert (rep.n, rep.bed_len, rep.hops, rep.active) == (want.N, len(bed), want.Nh, int(want.act.sum()))
    assert np.array_equal(D, want.D) and rep.duck_max == want.dmax / 100.0
    assert np.float32(rep.peak) == want.pk and np.float32(rep.gain) == want.sg and rep.capped == want.capped
    assert rep.bed == brep
    same = bits(y) == bits(want.y)
    assert len(y) == want.N and same.all(), (int((~same).sum()), int(np.argmin(same)))
    return y, rep, want


BED = None


def bed_clip():
    global BED
    if BED is None:
        BED = clip(noise(5000, 77), "f32", 44100)          # 908 samples at 8 kHz
    return BED


@pytest.mark.parametrize("N", [1, H - 1, H, H + 1, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 3])
def test_sizes(eng, N):
    x = speech(N, seed=N, quiet=[(N // 3, N // 2)])
    check(eng, x, bed_clip(), R.Params(depth=1200, attack=3, release=5, fade_in=50, fade_out=120, offset=11))


@pytest.mark.parametrize("lead,tail", [(0, 0), (37, 501), (4 * 41, 8)])
@pytest.mark.parametrize("where", ["first", "last"])
def test_loud_at_the_edges_with_lead_and_tail(eng, where, lead, tail):
    n = 23 * H + 71                                       # the last hop is partial
    x = np.zeros(n, dtype=np.float32)
    if where == "first":
        x[:H // 2] = noise(H // 2, 3)
    else:
        x[n - 40:] = noise(40, 4)
    y, rep, want = check(eng, x, bed_clip(), R.Params(depth=1800, attack=4, release=6, lead=lead, tail=tail))
    assert rep.active >= 1 and rep.duck_max == 18.0


@pytest.mark.parametrize("Wa,Wr,depth", [(1, 1, 1200), (500, 500, 1200), (15, 40, 0), (15, 40, 6000), (7, 3, 1000)])
def test_windows_and_depths(eng, Wa, Wr, depth):
    n = 40 * H                                            # a 40-hop timeline
    x = speech(n, seed=Wa, quiet=[(0, 9 * H), (12 * H, 20 * H + 5), (31 * H, n)])
    y, rep, want = check(eng, x, bed_clip(), R.Params(depth=depth, attack=Wa, release=Wr))
    if depth == 0:
        assert not want.D.any() and np.all(want.gd == 1.0)
        s, b = R.timeline(x, bed_at(eng, bed_clip(), FO)[0], R.Params())
        assert np.array_equal(bits(y), bits(s + b)) or rep.capped
    else:
        assert rep.duck_max == depth / 100.0


def test_threshold_edge_and_nan(eng):
    thr = np.float32(0.0123)
    x = np.zeros(6 * H, dtype=np.float32)
    x[H + 5] = -thr                                       # exactly at the threshold: active
    x[3 * H + 9] = np.nextafter(thr, np.float32(0))       # one float32 step below: not
    x[5 * H + 1] = np.nan                                 # a NaN: its hop is not active, and it is not the peak
    y, rep, want = check(eng, x, bed_clip(), R.Params(depth=1200, threshold=float(thr), attack=2, release=2))
    assert want.act.tolist() == [False, True, False, False, False, False] and rep.active == 1
    assert np.isnan(y[5 * H + 1]) and np.isfinite(rep.peak)


def test_bed_shapes(eng):
    x = speech(9 * H + 13, seed=21, quiet=[(2 * H, 4 * H)])
    base = R.Params(depth=900, attack=3, release=4)
    nb = len(bed_at(eng, bed_clip(), FO)[0])
    assert nb == 908 and nb < len(x)
    check(eng, x, bed_clip(), base)                                            # several wraps
    check(eng, x, bed_clip(), base._replace(offset=3 * nb + 5))                # offset >= nb
    check(eng, x, bed_clip(), base._replace(offset=4 * nb))                    # ... landing on the bed's first sample
    y, rep, want = check(eng, x, bed_clip(), base._replace(loop=0, offset=100))     # cut: zeros past the bed's end
    assert np.array_equal(bits(want.m[nb - 100:]), bits(x[nb - 100:]))          # (before the ceiling, which binds here)
    check(eng, x, bed_clip(), base._replace(loop=0, offset=nb + 7))            # nothing of the bed is left
    longer = clip(noise(20000, 5), "f32", 44100)                              # 3629 samples at 8 kHz
    check(eng, x[:5 * H], longer, base._replace(loop=0, offset=2))             # a bed longer than N
    four = clip(noise(20, 6), "f32", 44100)                                   # ceil(20 80 / 441) = 4 samples
    assert len(bed_at(eng, four, FO)[0]) == 4
    check(eng, x, four, base._replace(offset=1))
    zeros = clip(np.zeros(3000, dtype=np.float32), "f32", 44100)
    p = base._replace(lead=33, tail=77)
    quiet = x * np.float32(0.5)                                                # (under the ceiling: nothing scales it)
    y, rep, want = check(eng, quiet, zeros, p)
    padded = np.concatenate([np.zeros(33, np.float32), quiet, np.zeros(77, np.float32)])
    assert not rep.capped and np.array_equal(bits(y), bits(padded))            # the padded programme, bit for bit


def test_constant_bed_at_the_native_rate(eng):
    """A float32 WAV holding 0.25 at 44 100 Hz with Fo = 44 100: nothing is resampled, so y - s is 0.25 gd in closed form."""
    Hn = 882
    n = 12 * Hn + 100
    x = np.zeros(n, dtype=np.float32)
    x[5 * Hn:7 * Hn] = 0.5                                 # exact sums: 0.5 + 0.25 gd has no rounding to speak of below
    c = clip(np.full(4000, 0.25, dtype=np.float32), "f32", 44100)
    p = R.Params(depth=2000, attack=3, release=2)
    y, rep, want = check(eng, x, c, p, rate=44100)
    assert rep.bed_len == 4000 and np.all(bed_at(eng, c, 44100)[0] == np.float32(0.25))
    T = R.gains()
    D = np.zeros(14, dtype=np.int64)
    D[3:9] = [666, 1333, 2000, 2000, 2000, 1000]         # 2000 (3 - d) / 3 ahead of hop 5; behind hop 6: 2000, 2000 / 2
    assert want.D.tolist() == D.tolist()
    i = np.arange(n)
    k, j = i // Hn, i % Hn
    g = T[D]
    gd = R.fmaf32(j.astype(np.float32) / np.float32(Hn), g[k + 1] - g[k], g[k])
    assert np.array_equal(bits(y), bits(x + np.float32(0.25) * gd))
    assert np.all(y[5 * Hn:7 * Hn] == np.float32(0.5) + np.float32(0.25) * T[2000])


def test_stereo_48k_bed_levelled(eng):
    """A 48 kHz stereo 16-bit bed to 8000 Hz with bed_loudness = -3000; its ft_intake_info is intake()'s (in check)."""
    rng = np.random.default_rng(9)
    t = np.arange(24000)
    left = 0.3 * np.sin(2 * np.pi * 330.0 * t / 48000) + 0.05 * rng.standard_normal(24000)
    right = 0.2 * np.sin(2 * np.pi * 495.0 * t / 48000) + 0.05 * rng.standard_normal(24000)
    k = np.clip(np.round(np.stack([left, right], 1) * 32768), -32767, 32767).astype(np.int64)
    c = clip(k, "s16", 48000)
    x = speech(30 * H + 7, seed=8, quiet=[(10 * H, 18 * H)])
    y, rep, want = check(eng, x, c, R.Params(), loudness=-30.0)
    assert rep.bed.n44 == 22050 and rep.bed_len == 4000 and rep.bed.level.gain != 1.0
    check(eng, x, c, R.Params(), loudness=-30.0, channel=1)


def test_fades_longer_than_the_piece(eng):
    N = 5 * H + 3
    x = speech(N, seed=2)
    y, rep, want = check(eng, x, bed_clip(), R.Params(depth=600, fade_in=N, fade_out=10 * N))     # f_in = f_out = N / 2
    check(eng, x, bed_clip(), R.Params(depth=600, fade_in=N // 2 + 40, fade_out=N // 2 + 1, lead=9))
    check(eng, x[:1], bed_clip(), R.Params(fade_in=5, fade_out=5))                                 # N = 1: no fade at all


def test_ceiling(eng):
    zeros = clip(np.zeros(3000, dtype=np.float32), "f32", 44100)
    under = np.float32(R.CEILING)
    under = under if float(under) < R.CEILING else np.nextafter(under, np.float32(0))
    x = speech(7 * H + 5, seed=12, amp=0.1)
    x[400] = -under
    y, rep, want = check(eng, x, zeros, R.Params())
    assert not rep.capped and rep.gain == 1.0 and np.float32(rep.peak) == under
    assert np.array_equal(bits(y), bits(x))                # mix_scale_kernel did not run: the samples are the programme's
    x[400] = np.nextafter(under, np.float32(1))
    y, rep, want = check(eng, x, zeros, R.Params())
    assert rep.capped and np.float32(rep.gain) == np.float32(R.CEILING / float(x[400])) and np.array_equal(bits(y), bits(x * want.sg))
    loud = speech(2 * SPAN + 9, seed=13, amp=0.5)
    y, rep, want = check(eng, loud, bed_clip(), R.Params(depth=300))
    assert rep.capped and float(np.abs(y).max()) <= R.CEILING * (1 + 2.0 ** -23)


def test_buffers_regrow_and_calls_repeat(eng):
    small, big = speech(3 * H, seed=30), speech(5 * SPAN + 1, seed=31, quiet=[(SPAN, 2 * SPAN)])
    big_bed = clip(noise(60000, 32), "f32", 44100)
    p = R.Params(depth=1500, attack=5, release=9, lead=3, tail=2, fade_out=300)
    a1, _, _ = check(eng, small, bed_clip(), p)
    b1, _, _ = check(eng, big, big_bed, p)
    a2, _, _ = check(eng, small, bed_clip(), p)
    b2, _, _ = check(eng, big, big_bed, p)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))


# ---- refusals, in the header's order: each refused call leaves the next good call's result as it was
def _raw(eng, x, c, mp_kw=None, rate=FO, item_kw=None, null=None, cap=None, n=None):
    from fish_tts_amd import _lib as L
    from fish_tts_amd.wavfile import FORMATS
    data, info = c
    buf = np.frombuffer(data, dtype=np.uint8)
    item = dict(data=buf.ctypes.data + info.data_offset, n_frames=info.n_frames, rate=info.rate, channels=info.channels,
                fmt=FORMATS.index(info.fmt), channel=-1)
    item.update(item_kw or {})
    mp = dict(bed_loudness=0, channel=-1, depth=1200, threshold=0.01, attack=15, release=40, lead=5, tail=6, fade_in=0,
              fade_out=100, offset=0, loop=1, reserved=0)
    mp.update(mp_kw or {})
    it, m = L.ft_intake_item(**item), L.ft_mix_params(**mp)
    n = len(x) if n is None else n
    N = max(1, len(x) + 5 + 6)
    y = np.full(N, 7.0, dtype=np.float32)
    D = np.full(N // H + 3, -7, dtype=np.int32)
    total, out = C.c_int64(-7), L.ft_mix_info()
    args = dict(x=x.ctypes.data_as(C.c_void_p), bed=C.byref(it), mp=C.byref(m), y=y.ctypes.data_as(C.c_void_p), total=C.byref(total),
                info=C.byref(out))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_mix(eng._h, args["x"], n, rate, args["bed"], args["mp"], args["y"], N if cap is None else cap,
                              args["total"], D.ctypes.data_as(C.c_void_p), args["info"])
    return st, y, D, total.value, buf


REFUSALS = [
    ("x", dict(null="x")), ("bed", dict(null="bed")), ("mp", dict(null="mp")), ("y", dict(null="y")), ("total", dict(null="total")),
    ("info", dict(null="info")),
    ("rate", dict(rate=7999)), ("rate-L", dict(rate=44101)),
    ("n", dict(n=0)),
    ("bed_loudness", dict(mp_kw=dict(bed_loudness=-499))), ("bed_loudness-low", dict(mp_kw=dict(bed_loudness=-5001))),
    ("depth", dict(mp_kw=dict(depth=6001))), ("depth-neg", dict(mp_kw=dict(depth=-1))),
    ("threshold", dict(mp_kw=dict(threshold=-0.5))), ("threshold-nan", dict(mp_kw=dict(threshold=float("nan")))),
    ("attack", dict(mp_kw=dict(attack=0))), ("attack-high", dict(mp_kw=dict(attack=501))),
    ("release", dict(mp_kw=dict(release=0))), ("release-high", dict(mp_kw=dict(release=501))),
    ("lead", dict(mp_kw=dict(lead=-1))), ("tail", dict(mp_kw=dict(tail=-1))),
    ("fade_in", dict(mp_kw=dict(fade_in=-1))), ("fade_out", dict(mp_kw=dict(fade_out=-1))),
    ("offset", dict(mp_kw=dict(offset=-1))), ("loop", dict(mp_kw=dict(loop=2))),
    ("N", dict(mp_kw=dict(tail=1 << 28), too_long=True)),
    ("capacity", dict(cap=10)),
    ("bed-frames", dict(item_kw=dict(n_frames=0))), ("bed-data", dict(item_kw=dict(data=None))),
    ("bed-fmt", dict(item_kw=dict(fmt=5))), ("bed-channels", dict(item_kw=dict(channels=9))),
    ("bed-channel", dict(mp_kw=dict(channel=1))), ("bed-rate", dict(item_kw=dict(rate=7000))),
    ("bed-length", dict(item_kw=dict(n_frames=1 << 29), too_long=True)),
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(eng, name, kw):
    from fish_tts_amd import _lib as L
    kw = dict(kw)
    want_st = L.FT_ERR_TOO_LONG if kw.pop("too_long", False) else L.FT_ERR_ARG
    x = speech(4 * H + 3, seed=40)
    c = bed_clip()
    st, y0, D0, t0, _ = _raw(eng, x, c)
    assert st == L.FT_OK and t0 == len(x) + 11
    st, y, D, t, _ = _raw(eng, x, c, **kw)
    assert st == want_st, (name, st, eng.lib.ft_last_error(eng._h))
    assert np.all(y == 7.0) and np.all(D == -7) and t == -7          # nothing written
    st, y1, D1, t1, _ = _raw(eng, x, c)
    assert st == L.FT_OK and t1 == t0 and np.array_equal(bits(y1), bits(y0)) and np.array_equal(D1, D0)


def test_the_earlier_reason_wins(eng):
    """The order of the checks: a call wrong in two ways is refused for the earlier one (the message names it)."""
    from fish_tts_amd import _lib as L
    x = speech(2 * H, seed=41)
    order = [("sample rate", dict(rate=7999)), ("n must", dict(n=0)), ("bed_loudness", dict(mp_kw=dict(bed_loudness=-1))),
             ("depth", dict(mp_kw=dict(depth=-1))), ("threshold", dict(mp_kw=dict(threshold=-1.0))),
             ("attack", dict(mp_kw=dict(attack=0))), ("release", dict(mp_kw=dict(release=0))), ("lead", dict(mp_kw=dict(lead=-1))),
             ("tail", dict(mp_kw=dict(tail=-1))), ("fade_in", dict(mp_kw=dict(fade_in=-1))), ("fade_out", dict(mp_kw=dict(fade_out=-1))),
             ("offset", dict(mp_kw=dict(offset=-1))), ("loop", dict(mp_kw=dict(loop=3))), ("capacity", dict(cap=1)),
             ("fmt", dict(item_kw=dict(fmt=9)))]
    for (w1, k1), (w2, k2) in zip(order, order[1:]):
        kw = {}
        for k in (k2, k1):
            for key, v in k.items():
                kw[key] = {**kw.get(key, {}), **v} if isinstance(v, dict) else v
        st, *_ = _raw(eng, x, bed_clip(), **kw)
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and w1 in msg and w2 not in msg.replace(w1, ""), (w1, w2, msg)
