"""GPU: the live mix stage through the C ABI (include/fishtts_hip.h: "Live mix"; ft_codec_mix_live, ft_codec_mix_stream_*,
ft_mix_live_plan) against its restatement tests/mixlive_ref.py.  The bed at the output rate comes from the existing calls -
intake(), then the resampler hook - as in tests/test_mix_gpu.py, so the stage is compared from the timeline onward and every
comparison is exact: every sample's bits, D_k, L_k, the counts, the largest hop peak.  Every input then goes through a stream
in several cuttings, each of which must give the one-shot call's bits and, push by push, ft_mix_live_plan's count.

Wa = 2 and Wr = 3 unless the windows are the point; with La = 5 the stage then holds back (Wa + La) = 7 whole hops."""
import ctypes as C

import numpy as np
import pytest

from tests import mix_ref as R
from tests import mixlive_ref as ML
from tests.test_codec_gpu import encode_shape, make_codec
from tests.test_mix_gpu import bed_at, bits, clip, native, noise, speech

pytestmark = pytest.mark.gpu
RATES = [8000, 16000, 44100, 48000]
WA, WR = 2, 3


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(encode_shape(), max_frames=1024)
    yield e
    e.close()


_CLIPS = {}


def the_clip(kind):
    if kind not in _CLIPS:
        if kind == "noise":
            _CLIPS[kind] = clip(noise(5000, 77), "f32", 44100)            # 908 samples at 8 kHz
        elif kind == "half":                                              # +-0.5, for the limiter
            _CLIPS[kind] = clip((0.5 * np.sign(np.sin(np.arange(6000) / 9.0))).astype(np.float32), "f32", 44100)
        elif kind == "short":                                             # shorter than one hop at any rate
            _CLIPS[kind] = clip(noise(120, 5, 0.3), "f32", 44100)
        elif kind == "soft":                                              # peaks near 0.4: nothing for the limiter to do
            _CLIPS[kind] = clip(noise(5000, 78, 0.1), "f32", 44100)
        elif kind == "zeros":
            _CLIPS[kind] = clip(np.zeros(2000, dtype=np.float32), "f32", 44100)
    return _CLIPS[kind]


def P(**kw):
    base = dict(depth=1200, threshold=0.01, attack=WA, release=WR)
    base.update(kw)
    return R.Params(**base)


def cases():
    """(id, rate, x, clip kind, Params) of every input; the clips themselves are built when first asked for."""
    out = []
    H = 160
    hold = (WA + ML.LA + 1) * H
    for n in (1, H - 1, H, H + 1, hold - 1, hold, hold + 1):
        out.append((f"n{n}", 8000, speech(n, seed=n, quiet=[(n // 3, n // 2)]), "noise", P(fade_in=20, fade_out=50, offset=11)))
    out.append(("w1", 8000, speech(20 * H + 7, seed=2, quiet=[(3 * H, 9 * H)]), "noise", P(attack=1, release=1)))
    out.append(("w500", 8000, speech(24000, seed=3, quiet=[(2000, 9000), (15000, 21000)]), "noise", P(attack=500, release=500)))
    for lead, tail in ((0, 0), (37, 501), (12 * H + 3, 11 * H + 5), (0, 10 * H + 1), (9 * H + 2, 0)):
        out.append((f"lead{lead}-tail{tail}", 8000, speech(11 * H + 9, seed=lead + 1, quiet=[(2 * H, 6 * H)]), "noise",
                    P(lead=lead, tail=tail, fade_out=30)))
    out.append(("short-bed", 8000, speech(9 * H + 1, seed=4), "short", P()))
    out.append(("bed-ends", 8000, speech(12 * H, seed=5, quiet=[(H, 4 * H)]), "noise", P(loop=0, offset=100)))
    out.append(("offset", 8000, speech(10 * H + 2, seed=6), "noise", P(offset=907 + 1000)))
    out.append(("long-fades", 8000, speech(6 * H + 3, seed=7), "noise", P(fade_in=20 * H, fade_out=25 * H, lead=H // 2, tail=H)))
    out.append(("tail<fade", 8000, speech(15 * H, seed=8), "noise", P(tail=H + 3, fade_out=4 * H + 1)))
    out.append(("tail>fade", 8000, speech(15 * H, seed=9), "noise", P(tail=4 * H + 1, fade_out=H + 3)))
    for rate in RATES:
        h = rate // 50
        x = (0.9 * np.sign(noise(14 * h + 5, 10 + rate))).astype(np.float32)
        x[:3 * h] = 0.0
        x[8 * h:10 * h + 1] *= 0.1
        out.append((f"limited-{rate}", rate, x, "half", P(depth=600, lead=h + 3, tail=2 * h + 1, fade_out=h)))
        out.append((f"quiet-{rate}", rate, speech(9 * h + 3, seed=rate, amp=0.05, quiet=[(h, 3 * h)]), "soft",
                    P(lead=5, tail=h + 2, fade_in=9, fade_out=2 * h)))
    for where in ("first", "last"):
        x = noise(16 * H, 12, 0.02)
        x[6 * H if where == "first" else 7 * H - 1] = 0.97
        out.append((f"spike-{where}", 8000, x, "half", P(depth=2000)))
    x = speech(10 * H + 4, seed=13)
    x[3 * H + 7] = np.nan
    x[5 * H:6 * H] = np.nan                                               # a whole hop of NaNs: Q = 0
    out.append(("nan", 8000, x, "noise", P()))
    out.append(("n0", 8000, np.zeros(0, dtype=np.float32), "noise", P(lead=3 * H + 1, tail=9 * H + 2, fade_out=2 * H)))
    out.append(("n0-short", 8000, np.zeros(0, dtype=np.float32), "half", P(lead=5, tail=0)))
    out.append(("n0-empty", 8000, np.zeros(0, dtype=np.float32), "half", P()))            # N = 0: one node, no sample
    out.append(("silent-bed", 8000, speech(9 * H, seed=14, amp=0.1), "zeros", P(lead=33, tail=20)))
    out.append(("w500-quiet", 8000, speech(24000, seed=15, amp=0.05, quiet=[(2000, 9000), (15000, 21000)]), "soft",
                P(attack=500, release=500, tail=77)))
    return out


CASES = cases()
_REF, _ONE = {}, {}


def ref_of(eng, case):
    cid, rate, x, kind, p = case
    if cid not in _REF:
        bed, brep = bed_at(eng, the_clip(kind), rate)
        _REF[cid] = (ML.live(x, bed, rate, p), len(bed), brep)
    return _REF[cid]


def one_shot(eng, case):
    cid, rate, x, kind, p = case
    if cid not in _ONE:
        _ONE[cid] = eng.mix_live(x, the_clip(kind), sample_rate=rate, params=native(p), nodes=True)
    return _ONE[cid]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_shot_against_the_restatement(eng, case):
    want, nb, brep = ref_of(eng, case)
    y, rep, D, Lk = one_shot(eng, case)
    qmax = np.float32(want.Q.max()) if want.Nh else np.float32(0.0)
    print(case[0], "N", want.N, "Nh", want.Nh, "active", int(want.act.sum()), "dmax", int(want.D.max()), "lmax", int(want.L.max()),
          "qmax", float(qmax), "got", rep)
    assert (rep.n, rep.bed_len, rep.hops, rep.active) == (want.N, nb, want.Nh, int(want.act.sum()))
    assert np.array_equal(D, want.D) and rep.duck_max == int(want.D.max()) / 100.0
    assert np.array_equal(Lk, want.L) and rep.limit_max == int(want.L.max()) / 100.0
    assert np.float32(rep.peak) == qmax
    assert rep.bed == brep
    same = bits(y) == bits(want.y)
    assert len(y) == want.N and same.all(), (int((~same).sum()), int(np.argmin(same)))


def cuttings(case):
    """Push sizes of the streams an input goes through: (name, sizes, the last push is the final one)."""
    cid, rate, x, kind, p = case
    n, H = len(x), rate // 50
    rng = np.random.default_rng(len(cid) + n)
    out = [("one", [n], True)]
    aligned, at = [], 0
    first = (-p.lead) % H or H                                            # the pushes end on hop borders of the timeline
    while at < n:
        k = min(n - at, first if not aligned else H * int(rng.integers(1, 4)))
        aligned.append(k)
        at += k
    out.append(("aligned", aligned or [0], True))
    rand, at = [0], 0                                                     # an empty first push
    while at < n:
        k = min(n - at, int(rng.choice([0, 1, 3, H // 2, H, H + 1, 3 * H - 1])))
        rand.append(k)
        at += k
    out.append(("random", rand + [0], True))                              # ... and an empty final one
    rand2 = [int(k) for k in rng.integers(0, 2 * H + 2, size=4 * (n // H + 1))]
    cut, at = [], 0
    for k in rand2:
        if at >= n:
            break
        cut.append(min(k, n - at))
        at += cut[-1]
    cut.append(n - at)
    out.append(("random2", cut, True))
    if n < 2 * H:
        out.append(("single", [1] * n or [0], True))
    return out


def run_stream(eng, case, sizes):
    """The chunks of one stream, each push's count checked against ft_mix_live_plan."""
    cid, rate, x, kind, p = case
    mp = native(p)
    chunks, at, total = [], 0, 0
    with eng.mix_stream(the_clip(kind), sample_rate=rate, params=mp) as ms:
        for j, k in enumerate(sizes):
            final = j == len(sizes) - 1
            got = ms.push(x[at:at + k], final=final)
            at += k
            total += len(got)
            assert total == eng.mix_live_plan(rate, mp, at, final)[0] == ML.emitted(at, final, rate, p), (cid, j, k, total)
            chunks.append(got.copy())
    assert at == len(x)
    return chunks


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_cutting_gives_the_one_shot_bits(eng, case):
    y = one_shot(eng, case)[0]
    cuts = cuttings(case)
    assert len(cuts) >= 4
    for name, sizes, _ in cuts:
        got = np.concatenate(run_stream(eng, case, sizes) + [np.zeros(0, dtype=np.float32)])
        same = bits(got) == bits(y) if len(got) == len(y) else np.zeros(1, dtype=bool)
        assert same.all(), (case[0], name, len(got), len(y), int(np.argmin(same)))


def test_a_lead_goes_out_before_any_programme(eng):
    case = next(c for c in CASES if c[0].startswith("lead1923"))
    cid, rate, x, kind, p = case
    chunks = run_stream(eng, case, [0, len(x)])
    assert len(chunks[0]) == ML.emitted(0, False, rate, p) == (12 - WA - ML.LA) * 160 > 0
    assert np.array_equal(bits(chunks[0]), bits(one_shot(eng, case)[0][:len(chunks[0])]))


def test_two_streams_interleaved_do_not_disturb_each_other(eng):
    a, b = next(c for c in CASES if c[0] == "limited-8000"), next(c for c in CASES if c[0] == "w1")
    ya, yb = one_shot(eng, a)[0], one_shot(eng, b)[0]
    sa = eng.mix_stream(the_clip(a[3]), sample_rate=a[1], params=native(a[4]))
    sb = eng.mix_stream(the_clip(b[3]), sample_rate=b[1], params=native(b[4]))
    ga, gb, ia, ib = [], [], 0, 0
    rng = np.random.default_rng(99)
    while ia < len(a[2]) or ib < len(b[2]):
        ka, kb = int(rng.integers(0, 400)), int(rng.integers(0, 700))
        ga.append(sa.push(a[2][ia:ia + ka]).copy())
        gb.append(sb.push(b[2][ib:ib + kb]).copy())
        ia, ib = ia + ka, ib + kb
    gb.append(sb.push(None, final=True).copy())
    ga.append(sa.push(None, final=True).copy())
    sa.close()
    sb.close()
    assert np.array_equal(bits(np.concatenate(ga)), bits(ya)) and np.array_equal(bits(np.concatenate(gb)), bits(yb))


@pytest.mark.parametrize("cid", ["quiet-8000", "quiet-16000", "quiet-44100", "quiet-48000", "w500-quiet", "silent-bed"])
def test_uncapped_inputs_equal_ft_codec_mix(eng, cid):
    case = next(c for c in CASES if c[0] == cid)
    _, rate, x, kind, p = case
    want = ref_of(eng, case)[0]
    assert not want.L.any() and want.N >= 2 * max(p.fade_in, p.fade_out)
    y, rep, D, Lk = one_shot(eng, case)
    ym, mrep, Dm = eng.mix(x, the_clip(kind), sample_rate=rate, params=native(p), nodes=True)
    assert not mrep.capped and rep.limit_max == 0.0 and not Lk.any()
    assert np.array_equal(D, Dm) and np.array_equal(bits(y), bits(ym))
    assert np.float32(rep.peak) == np.float32(mrep.peak)


def test_the_limiter_holds_the_ceiling_on_the_device(eng):
    worst = 0.0
    for case in CASES:
        if case[0].startswith("limited") or case[0].startswith("spike"):
            y, rep, _, Lk = one_shot(eng, case)
            assert Lk.any() and rep.limit_max > 0.0
            worst = max(worst, float(np.abs(y).max()))
    print("largest |y| of the limited cases", worst, "cf", float(ML.CF))
    assert worst <= float(ML.CF) * (1.0 + 2.0 ** -22)


# ---- refusals
def _raw(eng, x, c, rate=8000, n=None, cap=None, null=None, item_kw=None, mp_kw=None):
    """ft_codec_mix_live with any argument bent.  Returns (status, y, D, Lk, total)."""
    from fish_tts_amd import _lib as L
    from fish_tts_amd.wavfile import FORMATS
    data, info = c
    buf = np.frombuffer(data, dtype=np.uint8)
    item = dict(data=buf.ctypes.data + info.data_offset, n_frames=info.n_frames, rate=info.rate, channels=info.channels,
                fmt=FORMATS.index(info.fmt), channel=-1)
    item.update(item_kw or {})
    mp = dict(bed_loudness=0, channel=-1, depth=1200, threshold=0.01, attack=2, release=3, lead=5, tail=6, fade_in=0,
              fade_out=100, offset=0, loop=1, reserved=0)
    mp.update(mp_kw or {})
    it, m = L.ft_intake_item(**item), L.ft_mix_params(**mp)
    n = len(x) if n is None else n
    N = max(1, len(x) + 5 + 6)
    y = np.full(N, 7.0, dtype=np.float32)
    D = np.full(N // 160 + 3, -7, dtype=np.int32)
    Lk = np.full(N // 160 + 3, -7, dtype=np.int32)
    total, out = C.c_int64(-7), L.ft_mix_live_info()
    args = dict(x=x.ctypes.data_as(C.c_void_p), bed=C.byref(it), mp=C.byref(m), y=y.ctypes.data_as(C.c_void_p), total=C.byref(total),
                info=C.byref(out))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_mix_live(eng._h, args["x"], n, rate, args["bed"], args["mp"], args["y"], N if cap is None else cap,
                                   args["total"], D.ctypes.data_as(C.c_void_p), Lk.ctypes.data_as(C.c_void_p), args["info"])
    return st, y, D, Lk, total.value


REFUSALS = [
    ("x", dict(null="x")), ("bed", dict(null="bed")), ("mp", dict(null="mp")), ("y", dict(null="y")), ("total", dict(null="total")),
    ("info", dict(null="info")), ("rate", dict(rate=7999)), ("n", dict(n=-1)),
    ("bed_loudness", dict(mp_kw=dict(bed_loudness=-499))), ("depth", dict(mp_kw=dict(depth=6001))),
    ("threshold-nan", dict(mp_kw=dict(threshold=float("nan")))), ("attack", dict(mp_kw=dict(attack=0))),
    ("release", dict(mp_kw=dict(release=501))), ("lead", dict(mp_kw=dict(lead=-1))), ("tail", dict(mp_kw=dict(tail=-1))),
    ("fade_in", dict(mp_kw=dict(fade_in=-1))), ("fade_out", dict(mp_kw=dict(fade_out=-1))), ("offset", dict(mp_kw=dict(offset=-1))),
    ("loop", dict(mp_kw=dict(loop=2))), ("N", dict(mp_kw=dict(tail=1 << 28), too_long=True)), ("capacity", dict(cap=10)),
    ("bed-frames", dict(item_kw=dict(n_frames=0))), ("bed-fmt", dict(item_kw=dict(fmt=5))),
    ("bed-channel", dict(mp_kw=dict(channel=1))), ("bed-rate", dict(item_kw=dict(rate=7000))),
    ("bed-length", dict(item_kw=dict(n_frames=1 << 29), too_long=True)),
]


def test_refusals_change_nothing(eng):
    from fish_tts_amd import _lib as L
    x = speech(4 * 160 + 3, seed=40)
    c = the_clip("noise")
    st, y0, D0, L0, t0 = _raw(eng, x, c)
    assert st == L.FT_OK and t0 == len(x) + 11
    for name, kw in REFUSALS:
        kw = dict(kw)
        want_st = L.FT_ERR_TOO_LONG if kw.pop("too_long", False) else L.FT_ERR_ARG
        st, y, D, Lk, t = _raw(eng, x, c, **kw)
        assert st == want_st, (name, st, eng.lib.ft_last_error(eng._h))
        assert np.all(y == 7.0) and np.all(D == -7) and np.all(Lk == -7) and t == -7, name          # nothing written
    st, y1, D1, L1, t1 = _raw(eng, x, c)
    assert st == L.FT_OK and t1 == t0 and np.array_equal(bits(y1), bits(y0)) and np.array_equal(D1, D0) and np.array_equal(L1, L0)


def test_the_earlier_reason_wins(eng):
    """The order of the checks is ft_codec_mix's: a call wrong in two ways is refused for the earlier one."""
    from fish_tts_amd import _lib as L
    x = speech(2 * 160, seed=41)
    order = [("sample rate", dict(rate=7999)), ("n must", dict(n=-1)), ("bed_loudness", dict(mp_kw=dict(bed_loudness=-1))),
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
        st, *_ = _raw(eng, x, the_clip("noise"), **kw)
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and w1 in msg and w2 not in msg.replace(w1, ""), (w1, w2, msg)


def test_stream_refusals_and_the_push_after_final(eng):
    from fish_tts_amd import _lib as L
    case = next(c for c in CASES if c[0] == "limited-8000")
    _, rate, x, kind, p = case
    y = one_shot(eng, case)[0]
    # begin: the same checks, in the same order, before any device work
    data, info = the_clip(kind)
    buf = np.frombuffer(data, dtype=np.uint8)
    from fish_tts_amd.wavfile import FORMATS
    it = L.ft_intake_item(data=buf.ctypes.data + info.data_offset, n_frames=info.n_frames, rate=info.rate, channels=info.channels,
                          fmt=FORMATS.index(info.fmt), channel=-1)
    ok = dict(bed_loudness=0, channel=-1, depth=1200, threshold=0.01, attack=2, release=3, lead=0, tail=0, fade_in=0, fade_out=0,
              offset=0, loop=1, reserved=0)
    h = C.c_void_p()
    for bad, st_want in ((dict(depth=-1), L.FT_ERR_ARG), (dict(attack=501), L.FT_ERR_ARG), (dict(lead=(1 << 28) + 1), L.FT_ERR_TOO_LONG),
                         (dict(channel=3), L.FT_ERR_ARG)):
        mp = L.ft_mix_params(**{**ok, **bad})
        assert eng.lib.ft_codec_mix_stream_begin(eng._h, rate, C.byref(it), C.byref(mp), C.byref(h)) == st_want and not h.value, bad
    assert eng.lib.ft_codec_mix_stream_begin(eng._h, 7999, C.byref(it), C.byref(L.ft_mix_params(**ok)), C.byref(h)) == L.FT_ERR_ARG
    assert eng.lib.ft_codec_mix_stream_begin(eng._h, rate, None, C.byref(L.ft_mix_params(**ok)), C.byref(h)) == L.FT_ERR_ARG
    # pushes: a refused one leaves the stream able to continue
    ms = eng.mix_stream(the_clip(kind), sample_rate=rate, params=native(p))
    cut = 9 * 160 + 17
    got = [ms.push(x[:cut]).copy()]
    assert len(got[0]) > 0
    out = np.full(len(y), 7.0, dtype=np.float32)
    n_out = C.c_int64(-7)
    rest = np.ascontiguousarray(x[cut:])
    args = (rest.ctypes.data_as(C.c_void_p), len(rest), 1, out.ctypes.data_as(C.c_void_p))
    assert eng.lib.ft_codec_mix_stream_push(ms._h, args[0], len(rest), 1, args[3], 3, C.byref(n_out)) == L.FT_ERR_ARG      # capacity
    assert eng.lib.ft_codec_mix_stream_push(ms._h, None, len(rest), 1, args[3], len(y), C.byref(n_out)) == L.FT_ERR_ARG   # null x
    assert eng.lib.ft_codec_mix_stream_push(ms._h, args[0], -1, 1, args[3], len(y), C.byref(n_out)) == L.FT_ERR_ARG
    assert eng.lib.ft_codec_mix_stream_push(ms._h, args[0], 1 << 28, 0, args[3], len(y), C.byref(n_out)) == L.FT_ERR_TOO_LONG
    assert n_out.value == -7 and np.all(out == 7.0)
    got.append(ms.push(rest, final=True).copy())
    assert np.array_equal(bits(np.concatenate(got)), bits(y))
    assert eng.lib.ft_codec_mix_stream_push(ms._h, None, 0, 0, args[3], len(y), C.byref(n_out)) == L.FT_ERR_STATE
    assert eng.lib.ft_codec_mix_stream_push(ms._h, None, 0, 1, args[3], len(y), C.byref(n_out)) == L.FT_ERR_STATE
    ms.close()
    with pytest.raises(RuntimeError, match="closed"):
        ms.push(None)
    # the plan refuses what the calls refuse
    assert eng.lib.ft_mix_live_plan(rate, None, 0, 0, None, None) == L.FT_ERR_ARG
    assert eng.lib.ft_mix_live_plan(rate, C.byref(L.ft_mix_params(**ok)), -1, 0, None, None) == L.FT_ERR_ARG
    assert eng.lib.ft_mix_live_plan(rate, C.byref(L.ft_mix_params(**ok)), (1 << 28) + 1, 0, None, None) == L.FT_ERR_TOO_LONG
