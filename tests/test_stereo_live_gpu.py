"""GPU: the live stereo mix stage through the C ABI (include/fishtts_hip.h: "Live stereo mix"; ft_codec_mix_live_stereo,
ft_codec_mix_stream_begin_stereo, ft_codec_mix_stream_push_stereo) against its restatement tests/stereolive_ref.py.  The two
sides of the bed at the output rate come from the existing calls - intake() per channel, then the resampler hook - as in
tests/test_stereo_mix_gpu.py, so the stage is compared from the timeline onward and every comparison is exact: every bit of
both channels, D_k, L_k, the counts, the largest hop peak.  Every input then goes through a stream in several cuttings, the
regions clipped to each push and shifted to its coordinates; each must give the one-shot call's bits and, push by push,
ft_mix_live_plan's count.

Shapes as tests/test_mix_live_gpu.py: 8 kHz (H = 160), Wa = 2, Wr = 3; with La = 5 the stage holds back 7 whole hops."""
import ctypes as C

import numpy as np
import pytest

from tests import mix_ref as R
from tests import mixlive_ref as ML
from tests import stereo_ref as SR
from tests import stereolive_ref as SL
from tests.test_codec_gpu import encode_shape, make_codec
from tests.test_mix_gpu import bits, native, noise, speech
from tests.test_stereo_mix_gpu import made, sides_at

pytestmark = pytest.mark.gpu
RATES = [8000, 16000, 44100, 48000]
WA, WR = 2, 3
H = 160
PANS = (-100, -37, 0, 1, 100)


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(encode_shape(), max_frames=1024)
    yield e
    e.close()


def P(**kw):
    base = dict(depth=1200, threshold=0.01, attack=WA, release=WR)
    base.update(kw)
    return R.Params(**base)


def spread(n, h=H, step=97):
    """Regions over n samples: touching pairs of different pans, single samples, holes, all five pans, an edge on a hop
    border and edges inside groups of four; the last region ends on the last sample."""
    regions, at, k = [], 0, 0
    while at < n:
        e = min(n, at + (1 if k % 5 == 2 else 2 if k % 5 == 3 else step + k))
        if at < 3 * h < e:
            e = 3 * h                                          # an edge on a hop border (of the programme: with lead = 0, the timeline's)
        regions.append((at, e, PANS[k % 5]))
        at = e if k % 3 else e + (k % 7)
        k += 1
    if regions[-1][1] < n:
        regions.append((n - 1, n, 100))
    return regions


class Case:
    def __init__(self, cid, x, regions, p, bed="stereo", rate=8000, channel=None, loudness=None):
        self.id, self.x, self.regions, self.p, self.bed, self.rate = cid, np.asarray(x, dtype=np.float32), regions, p, bed, rate
        self.channel, self.loudness = channel, loudness
        assert SR.check_regions(regions, len(self.x)) is None, cid

    @property
    def clip(self):
        return None if self.bed is None else made(self.bed)

    @property
    def params(self):
        return native(self.p, 0 if self.loudness is None else int(round(100 * self.loudness)), -1 if self.channel is None else self.channel)


def cases():
    out = []
    hold = (WA + ML.LA + 1) * H
    for n in (1, H - 1, H, H + 1, hold - 1, hold, hold + 1):
        out.append(Case(f"n{n}", speech(n, seed=n, quiet=[(n // 3, n // 2)]), spread(n, step=41), P(fade_in=20, fade_out=50, offset=11)))
    for lead, tail in ((37, 501), (12 * H + 3, 11 * H + 5), (0, 10 * H + 1), (9 * H + 2, 0)):
        n = 11 * H + 9
        out.append(Case(f"lead{lead}-tail{tail}", speech(n, seed=lead + 1, quiet=[(2 * H, 6 * H)]), spread(n),
                        P(lead=lead, tail=tail, fade_out=30)))
    out.append(Case("long-fades", speech(6 * H + 3, seed=7), spread(6 * H + 3), P(fade_in=20 * H, fade_out=25 * H, lead=H // 2, tail=H)))
    out.append(Case("tail<fade", speech(15 * H, seed=8), spread(15 * H), P(tail=H + 3, fade_out=4 * H + 1)))
    out.append(Case("tail>fade", speech(15 * H, seed=9), spread(15 * H), P(tail=4 * H + 1, fade_out=H + 3)))
    n = 10 * H + 6
    x = speech(n, seed=21, amp=0.15, quiet=[(2 * H, 4 * H)])
    some = [(0, 500, -100), (500, 900, 37), (1000, n, 100)]
    for bed, channel in (("mono", None), ("stereo", None), (None, None), ("stereo", 1), ("six", None), ("six", 4)):
        out.append(Case(f"bed-{bed}-{channel}", x, some, P(lead=8, tail=5, offset=3, loop=1 if bed else 0), bed=bed, channel=channel))
    out.append(Case("bed-ends", x, some, P(loop=0, offset=100)))
    out.append(Case("pair-level", speech(30 * H + 7, seed=8, amp=0.1, quiet=[(10 * H, 18 * H)]), [(0, 10 * H, -37)], P(), bed="long",
                    loudness=-30.0))
    n = 12 * H + 2
    x = speech(n, seed=22, quiet=[(5 * H, 7 * H)])
    shapes = {
        "none": [],
        "one-over-everything": [(0, n, -37)],
        "one-sample": [(3 * H + 1, 3 * H + 2, 100), (7 * H, 7 * H + 1, -100), (n - 1, n, 37)],
        "touching": [(100, 200, -37), (200, 300, 37), (300, 301, -37), (301, 9 * H, 1)],
        "last-sample": [(5, n, -100)],
        "hard-and-centre": [(0, 2 * H, -100), (2 * H, 4 * H, 0), (4 * H, 6 * H, 100)],
        "edge-inside-a-group": [(0, 6, 100), (6, 7, -100), (9, 4 * H + 1, 1), (4 * H + 3, n - 1, -37)],
        "edge-on-a-hop": [(H, 2 * H, -100), (2 * H, 5 * H, 100), (8 * H, 9 * H, 37)],
    }
    for name, regions in shapes.items():
        out.append(Case(f"regions-{name}", x, regions, P(tail=3)))
    out.append(Case("regions-lead-3", x, shapes["edge-on-a-hop"], P(lead=3, tail=H)))       # ... and the same off every border
    for rate in RATES:
        h = rate // 50
        x = (0.95 * np.sign(noise(14 * h + 5, 10 + rate))).astype(np.float32)
        x[:3 * h] = 0.0
        x[8 * h:10 * h + 1] *= 0.1
        # hard left from hop 3 on: the left channel exceeds the ceiling, the right one holds the quiet bed alone
        out.append(Case(f"limited-{rate}", x, [(3 * h - 5, 12 * h + 1, -100), (12 * h + 1, len(x), -100)],
                        P(depth=600, lead=h + 3, tail=2 * h + 1, fade_out=h), rate=rate))
    x = speech(10 * H + 4, seed=13)
    x[3 * H + 7] = np.nan
    x[5 * H:6 * H] = np.nan                                               # a whole hop of NaNs: Q = 0
    out.append(Case("nan", x, [(3 * H, 3 * H + 9, 100), (5 * H - 3, 6 * H + 3, -37)], P()))
    none = np.zeros(0, dtype=np.float32)
    out.append(Case("n0", none, [], P(lead=3 * H + 1, tail=9 * H + 2, fade_out=2 * H)))
    out.append(Case("n0-empty", none, [], P()))                           # N = 0: one node, no frame
    return out


CASES = cases()
IDS = [c.id for c in CASES]
_REF, _ONE = {}, {}


def one_shot(eng, case):
    if case.id not in _ONE:
        _ONE[case.id] = eng.mix_live_stereo(case.x, case.clip, case.regions, sample_rate=case.rate, params=case.params, nodes=True)
    return _ONE[case.id]


def ref_of(eng, case):
    if case.id not in _REF:
        rep = one_shot(eng, case)[1]
        if case.clip is None:
            b0 = b1 = brep = None
        else:
            b0, b1, brep = sides_at(eng, case.clip, case.rate, case.loudness, case.channel, rep)
        _REF[case.id] = (SL.live([(case.x, case.regions)], b0, b1, case.rate, case.p), 0 if b0 is None else len(b0), brep)
    return _REF[case.id]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_shot_against_the_restatement(eng, case):
    y, rep, D, Lk = one_shot(eng, case)
    want, nb, brep = ref_of(eng, case)
    qmax = np.float32(want.Q.max()) if want.Nh else np.float32(0.0)
    print(case.id, "N", want.N, "Nh", want.Nh, "active", int(want.act.sum()), "dmax", int(want.D.max()), "lmax", int(want.L.max()),
          "qmax", float(qmax), "got", rep)
    assert (rep.n, rep.bed_len, rep.hops, rep.active) == (want.N, nb, want.Nh, int(want.act.sum()))
    assert np.array_equal(D, want.D) and rep.duck_max == int(want.D.max()) / 100.0
    assert np.array_equal(Lk, want.L) and rep.limit_max == int(want.L.max()) / 100.0
    assert np.float32(rep.peak) == qmax
    if case.clip is None:
        assert rep.bed.n44 == 0 and rep.bed.level.blocks == 0 and rep.bed.level.gain == 0.0        # zeroed
    elif brep is not None:
        assert rep.bed == brep
    same = bits(y) == bits(want.y)
    assert y.shape == (want.N, 2) and same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())


def cuttings(case):
    """Push sizes of the streams an input goes through."""
    n, h = len(case.x), case.rate // 50
    rng = np.random.default_rng(len(case.id) + n)
    edges = sorted({v for a, e, _ in case.regions for v in (a, e) if 0 < v < n})
    inside = sorted({v for a, e, _ in case.regions for v in (a + 1, e - 1) if 0 < v < n})

    def sizes(cuts):
        pts = [0] + list(cuts) + [n]
        return [b - a for a, b in zip(pts, pts[1:])]

    out = [("one", [n]), ("edges", sizes(edges)), ("inside", sizes(inside))]
    hops, at = [], 0
    while at < n:
        hops += [min(h, n - at), 0]
        at += h
    out.append(("hops", [0] + hops))                                      # an empty first push, empty ones between
    rand, at = [], 0
    while at < n:
        rand.append(min(n - at, int(rng.choice([0, 1, 3, h // 2, h, h + 1, 3 * h - 1]))))
        at += rand[-1]
    out.append(("random", rand + [0]))                                    # ... and an empty final one
    if n <= 2 * h:
        out.append(("single", [1] * n or [0]))
    return out


def run_stream(eng, case, sizes):
    """The chunks of one stream, each push's count checked against ft_mix_live_plan."""
    assert sum(sizes) == len(case.x)
    chunks, at, total = [], 0, 0
    pushes = SL.cut(case.x, case.regions, sizes)
    with eng.mix_stream(case.clip, sample_rate=case.rate, params=case.params, stereo=True) as ms:
        for j, (xk, regions) in enumerate(pushes):
            final = j == len(pushes) - 1
            got = ms.push(xk, regions, final=final)
            at += len(xk)
            total += len(got)
            assert total == eng.mix_live_plan(case.rate, case.params, at, final)[0] == ML.emitted(at, final, case.rate, case.p), \
                (case.id, j, len(xk), total)
            assert got.shape == (len(got), 2)
            chunks.append(got.copy())
    return chunks


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_cutting_gives_the_one_shot_bits(eng, case):
    y = one_shot(eng, case)[0]
    cuts = cuttings(case)
    assert len(cuts) >= 4
    for name, sizes in cuts:
        got = np.concatenate(run_stream(eng, case, sizes) + [np.zeros((0, 2), dtype=np.float32)])
        same = bits(got) == bits(y) if got.shape == y.shape else np.zeros(1, dtype=bool)
        assert same.all(), (case.id, name, got.shape, y.shape, np.argwhere(~same)[:4].tolist())


def case_of(cid):
    return next(c for c in CASES if c.id == cid)


@pytest.mark.parametrize("bed,channel", [("mono", None), ("six", 4), ("stereo", 1)])
def test_identity_a_centred_and_one_side_is_the_live_mix_stage_twice(eng, bed, channel):
    base = case_of("limited-8000")
    params = native(base.p, 0, -1 if channel is None else channel)
    m, mrep, mD, mL = eng.mix_live(base.x, made(bed), sample_rate=8000, params=params, nodes=True)
    assert mL.any()
    for regions in ([], [(0, len(base.x), 0)], [(3, 4, 0), (4, 9 * H, 0)]):
        y, rep, D, Lk = eng.mix_live_stereo(base.x, made(bed), regions, sample_rate=8000, params=params, nodes=True)
        assert np.array_equal(bits(y[:, 0]), bits(m)) and np.array_equal(bits(y[:, 1]), bits(m))
        assert rep == mrep and np.array_equal(D, mD) and np.array_equal(Lk, mL)


@pytest.mark.parametrize("cid", ["regions-touching", "bed-None-None", "bed-six-None", "regions-lead-3"])
def test_identity_b_below_the_ceiling_it_is_ft_codec_mix_stereo(eng, cid):
    case = case_of(cid)
    x = (case.x * np.float32(0.25)).astype(np.float32)                   # quiet enough for neither ceiling to bind
    p = case.p._replace(fade_in=9, fade_out=H)
    params = native(p, 0, -1 if case.channel is None else case.channel)
    y, rep, D, Lk = eng.mix_live_stereo(x, case.clip, case.regions, sample_rate=8000, params=params, nodes=True)
    ys, srep, sD = eng.mix_stereo(x, case.clip, case.regions, sample_rate=8000, params=params, nodes=True)
    assert not srep.capped and rep.limit_max == 0.0 and not Lk.any() and rep.n >= 2 * max(p.fade_in, p.fade_out)
    assert np.array_equal(D, sD) and np.array_equal(bits(y), bits(ys)) and np.float32(rep.peak) == np.float32(srep.peak)
    assert rep.bed == srep.bed


def test_identity_d_the_linked_limiter_holds_the_ceiling_on_the_device(eng):
    worst = 0.0
    for rate in RATES:
        case = case_of(f"limited-{rate}")
        y, rep, _, Lk = one_shot(eng, case)
        want = ref_of(eng, case)[0]
        assert Lk.any() and rep.limit_max > 0.0
        over = np.abs(want.m).max(axis=0)
        assert over[0] > float(ML.CF) > over[1]                          # the left channel alone exceeds the ceiling
        worst = max(worst, float(np.abs(y).max()))
        # the same factor on both channels: where the left channel was turned down, the right one was, by as much
        i = int(np.argmax(np.abs(want.m[:, 0])))
        k = i // want.H
        assert want.L[k] > 0 and abs(y[i, 1]) < abs(want.m[i, 1]) and y[i, 1] != 0.0
        f = float(y[i, 0]) / float(want.m[i, 0])                           # (each quotient is the factor up to one rounding)
        assert abs(float(y[i, 1]) / float(want.m[i, 1]) - f) <= 2.0 ** -22
    print("largest |y| of the limited cases", worst, "cf", float(ML.CF))
    assert worst <= float(ML.CF) * (1.0 + 2.0 ** -22)


def test_a_mono_and_a_stereo_stream_interleaved_do_not_disturb_each_other(eng):
    from tests.test_mix_live_gpu import CASES as MONO, the_clip
    a = case_of("limited-8000")
    b = next(c for c in MONO if c[0] == "w1")
    ya = one_shot(eng, a)[0]
    yb = eng.mix_live(b[2], the_clip(b[3]), sample_rate=b[1], params=native(b[4]))[0]
    sa = eng.mix_stream(a.clip, sample_rate=a.rate, params=a.params, stereo=True)
    sb = eng.mix_stream(the_clip(b[3]), sample_rate=b[1], params=native(b[4]))
    ga, gb, ia, ib = [], [], 0, 0
    rng = np.random.default_rng(99)
    while ia < len(a.x) or ib < len(b[2]):
        ka, kb = min(int(rng.integers(0, 400)), len(a.x) - ia), int(rng.integers(0, 700))
        ga.append(sa.push(*SL.piece(a.x, a.regions, ia, ka)).copy())
        gb.append(sb.push(b[2][ib:ib + kb]).copy())
        ia, ib = ia + ka, ib + kb
    gb.append(sb.push(None, final=True).copy())
    ga.append(sa.push(None, final=True).copy())
    sa.close()
    sb.close()
    assert np.array_equal(bits(np.concatenate(ga)), bits(ya)) and np.array_equal(bits(np.concatenate(gb)), bits(yb))


def test_a_lead_goes_out_in_stereo_before_any_programme(eng):
    case = case_of("lead1923-tail1765")
    chunks = run_stream(eng, case, [0, len(case.x)])
    assert len(chunks[0]) == ML.emitted(0, False, case.rate, case.p) == (12 - WA - ML.LA) * H > 0
    y = one_shot(eng, case)[0]
    assert np.array_equal(bits(chunks[0]), bits(y[:len(chunks[0])]))
    assert not np.array_equal(chunks[0][:, 0], chunks[0][:, 1])          # the bed alone, two different sides


# ---- refusals
def _item(c):
    from fish_tts_amd import _lib as L
    from fish_tts_amd.wavfile import FORMATS
    data, info = c
    buf = np.frombuffer(data, dtype=np.uint8)
    return buf, L.ft_intake_item(data=buf.ctypes.data + info.data_offset, n_frames=info.n_frames, rate=info.rate,
                                 channels=info.channels, fmt=FORMATS.index(info.fmt), channel=-1)


def _table(regions):
    from fish_tts_amd import _lib as L
    return (L.ft_pan_region * max(len(regions), 1))(*[L.ft_pan_region(a, e, q, 0) for a, e, q in regions])


OK_MP = dict(bed_loudness=0, channel=-1, depth=1200, threshold=0.01, attack=2, release=3, lead=5, tail=6, fade_in=0, fade_out=100,
             offset=0, loop=1, reserved=0)


def _raw(eng, x, regions, R=None, rate=8000, n=None, cap=None, null_table=False, mp_kw=None, bedless=False):
    """ft_codec_mix_live_stereo with any argument bent.  Returns (status, y, D, Lk, total)."""
    from fish_tts_amd import _lib as L
    keep, it = _item(made("stereo"))
    m = L.ft_mix_params(**{**OK_MP, **(mp_kw or {})})
    n = len(x) if n is None else n
    N = max(1, len(x) + 11)
    y = np.full((N, 2), 7.0, dtype=np.float32)
    D = np.full(N // 160 + 3, -7, dtype=np.int32)
    Lk = np.full(N // 160 + 3, -7, dtype=np.int32)
    total, out = C.c_int64(-7), L.ft_mix_live_info()
    st = eng.lib.ft_codec_mix_live_stereo(eng._h, x.ctypes.data_as(C.c_void_p), n, rate, None if null_table else _table(regions),
                                          len(regions) if R is None else R, None if bedless else C.byref(it), C.byref(m),
                                          y.ctypes.data_as(C.c_void_p), N if cap is None else cap, C.byref(total),
                                          D.ctypes.data_as(C.c_void_p), Lk.ctypes.data_as(C.c_void_p), C.byref(out))
    del keep
    return st, y, D, Lk, total.value


def test_one_shot_refusals_change_nothing_and_the_earlier_reason_wins(eng):
    from fish_tts_amd import _lib as L
    x = speech(4 * 160 + 3, seed=40)
    n = len(x)
    good = [(0, 100, -100), (100, n, 37)]
    st, y0, D0, L0, t0 = _raw(eng, x, good)
    assert st == L.FT_OK and t0 == n + 11
    many = [(i, i + 1, 0) for i in range(4097)]
    bad = [("null table", dict(null_table=True), "null"), ("R", dict(regions=many[:2], R=4097), "R outside"),
           ("R<0", dict(R=-1), "R outside"), ("outside", dict(regions=[(0, n + 1, 0)]), "out of order"), ("order", dict(regions=[(5, 9, 0), (8, 12, 0)]), "out of order"),
           ("empty", dict(regions=[(5, 5, 0)]), "out of order"), ("pan", dict(regions=[(0, 5, 101)]), "a pan outside"),
           ("n0-regions", dict(regions=[(0, 1, 0)], n=0), "out of order"), ("capacity", dict(cap=10), "capacity"),
           ("depth", dict(mp_kw=dict(depth=6001)), "depth"), ("rate", dict(rate=7999), "sample rate")]
    for name, kw, word in bad:
        kw = {"regions": good, **kw}
        st, y, D, Lk, t = _raw(eng, x, **kw)
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and word in msg, (name, st, msg)
        assert np.all(y == 7.0) and np.all(D == -7) and np.all(Lk == -7) and t == -7, name          # nothing written
    # the regions are judged behind the rate and n, before the mix parameters and the capacity
    for (w1, k1), (w2, k2) in ((("sample rate", dict(rate=7999)), ("out of order", dict(regions=[(0, n + 1, 0)]))),
                               (("n must", dict(n=-1)), ("a pan outside", dict(regions=[(0, 1, 101)]))),
                               (("out of order", dict(regions=[(0, n + 1, 0)])), ("bed_loudness", dict(mp_kw=dict(bed_loudness=-1)))),
                               (("a pan outside", dict(regions=[(0, 1, 101)])), ("capacity", dict(cap=1)))):
        st, *_ = _raw(eng, x, **{"regions": good, **k2, **k1})
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and w1 in msg and w2 not in msg, (w1, w2, msg)
    st, y1, D1, L1, t1 = _raw(eng, x, good)
    assert st == L.FT_OK and t1 == t0 and np.array_equal(bits(y1), bits(y0)) and np.array_equal(D1, D0) and np.array_equal(L1, L0)
    st, yb, *_ = _raw(eng, x, good, bedless=True)                         # no bed: allowed
    assert st == L.FT_OK and not yb[:5].any()


def test_stream_refusals_leave_the_stream_as_it_was(eng):
    from fish_tts_amd import _lib as L
    case = case_of("limited-8000")
    x, y = case.x, one_shot(eng, case)[0]
    keep, it = _item(case.clip)
    h = C.c_void_p()
    for bad, st_want in ((dict(depth=-1), L.FT_ERR_ARG), (dict(lead=(1 << 28) + 1), L.FT_ERR_TOO_LONG), (dict(channel=3), L.FT_ERR_ARG)):
        mp = L.ft_mix_params(**{**OK_MP, **bad})
        assert eng.lib.ft_codec_mix_stream_begin_stereo(eng._h, 8000, C.byref(it), C.byref(mp), C.byref(h)) == st_want and not h.value, bad
    ok = L.ft_mix_params(**OK_MP)
    assert eng.lib.ft_codec_mix_stream_begin_stereo(eng._h, 7999, C.byref(it), C.byref(ok), C.byref(h)) == L.FT_ERR_ARG
    assert eng.lib.ft_codec_mix_stream_begin_stereo(eng._h, 8000, C.byref(it), None, C.byref(h)) == L.FT_ERR_ARG
    ms = eng.mix_stream(case.clip, sample_rate=8000, params=case.params, stereo=True)
    mono = eng.mix_stream(case.clip, sample_rate=8000, params=case.params)
    cut = 9 * 160 + 17
    first, rest = SL.cut(x, case.regions, [cut, len(x) - cut])
    got = [ms.push(*first).copy()]
    assert len(got[0]) > 0
    out = np.full((len(y), 2), 7.0, dtype=np.float32)
    n_out = C.c_int64(-7)
    xr = np.ascontiguousarray(rest[0])
    xp, yp, nr = xr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(xr)
    push = eng.lib.ft_codec_mix_stream_push_stereo
    good = _table(rest[1])
    R = len(rest[1])
    assert push(ms._h, xp, nr, _table([(0, nr + 1, 0)]), 1, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_ARG       # outside its push
    assert push(ms._h, xp, nr, _table([(0, 1, 0)]), 4097, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_ARG           # R > 4096
    assert "R outside" in eng.lib.ft_last_error(eng._h).decode()
    assert push(ms._h, None, 0, _table([(0, 1, 0)]), 1, 0, yp, len(y), C.byref(n_out)) == L.FT_ERR_ARG            # regions with n = 0
    assert push(ms._h, xp, nr, None, 1, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_ARG                            # a null table
    assert push(ms._h, xp, nr, _table([(0, 1, -101)]), 1, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_ARG
    assert push(ms._h, xp, nr, good, R, 1, yp, 3, C.byref(n_out)) == L.FT_ERR_ARG                                 # capacity
    assert "capacity" in eng.lib.ft_last_error(eng._h).decode()
    assert push(ms._h, xp, nr, _table([(0, nr + 1, 0)]), 1, 1, yp, 3, C.byref(n_out)) == L.FT_ERR_ARG             # the earlier reason
    assert "out of order" in eng.lib.ft_last_error(eng._h).decode()
    assert push(ms._h, xp, -1, good, R, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_ARG
    assert push(ms._h, xp, 1 << 28, None, 0, 0, yp, len(y), C.byref(n_out)) == L.FT_ERR_TOO_LONG
    # a push of the wrong kind, either way
    assert eng.lib.ft_codec_mix_stream_push(ms._h, xp, nr, 1, yp, 2 * len(y), C.byref(n_out)) == L.FT_ERR_STATE
    assert push(mono._h, xp, nr, good, R, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_STATE
    assert n_out.value == -7 and np.all(out == 7.0)
    got.append(ms.push(*rest, final=True).copy())
    assert np.array_equal(bits(np.concatenate(got)), bits(y))
    assert push(ms._h, None, 0, None, 0, 0, yp, len(y), C.byref(n_out)) == L.FT_ERR_STATE                         # after `final`
    assert push(ms._h, None, 0, None, 0, 1, yp, len(y), C.byref(n_out)) == L.FT_ERR_STATE
    ym = eng.mix_live(x, case.clip, sample_rate=8000, params=case.params)[0]
    assert np.array_equal(bits(mono.push(x, final=True)), bits(ym))       # the mono stream went on undisturbed
    ms.close()
    mono.close()
    del keep
    with pytest.raises(RuntimeError, match="closed"):
        ms.push(None)
    with pytest.raises(ValueError, match="region"):                       # the Python wrapper judges before any device work
        eng.mix_live_stereo(x, case.clip, [(0, len(x) + 1, 0)], sample_rate=8000, params=case.params)
