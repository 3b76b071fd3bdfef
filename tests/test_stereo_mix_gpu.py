"""GPU: the stereo mix stage through the C ABI (include/fishtts_hip.h: "Stereo mix"; ft_codec_mix_stereo,
CodecHipEngine.mix_stereo) against its restatement tests/stereo_ref.py.  The two sides of the bed at the output rate come
from the existing calls - intake() per channel, then the resampler hook - so the stage is compared from the timeline onward
and every comparison is exact: D_k, N, the counts, every sample's bits in both channels, pk, sg.  The pair level is the one
figure that is not: L against the restatement within 1e-9 LU, and g within one float32 step of the restatement's (2^-23
relative, plus the 1.2e-10 that 1e-9 LU moves a gain) - the sides are then scaled by the g the call reports, and compared
bit for bit.  Fo = 8000 (H = 160); SPAN is what one workgroup of mix_stereo_kernel covers (stage_kernels.h: MX_SPAN)."""
import ctypes as C

import numpy as np
import pytest

from tests import mix_ref as R
from tests import stereo_ref as SR
from tests.test_codec_gpu import encode_shape, make_codec
from tests.test_mix_gpu import bed_at, bed_clip, bits, clip, native, noise, speech

pytestmark = pytest.mark.gpu
FO = 8000
H = 160
SPAN = 256 * 4 * 4
PANS = (-100, -37, 0, 1, 100)


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(encode_shape(), max_frames=1024)
    yield e
    e.close()


_CLIPS, _SIDES = {}, {}


def made(name):
    """The beds of this file, made once: (WAV bytes, WavInfo)."""
    if name not in _CLIPS:
        rng = np.random.default_rng(len(name))
        t = np.arange(5006)
        if name == "stereo":                               # two different sides; 5006 frames at 44.1 kHz are 909 at 8 kHz: odd
            v = np.stack([0.2 * np.sin(2 * np.pi * 330.0 * t / 44100), 0.15 * np.sin(2 * np.pi * 495.0 * t / 44100)], 1)
            _CLIPS[name] = clip((v + 0.03 * rng.standard_normal(v.shape)).astype(np.float32), "f32", 44100)
        elif name == "stereo-s16":
            v = 0.2 * rng.standard_normal((6000, 2))
            _CLIPS[name] = clip(np.clip(np.round(v * 32768), -32767, 32767).astype(np.int64), "s16", 48000)
        elif name == "mono":
            _CLIPS[name] = clip(noise(5006, 78), "f32", 44100)
        elif name == "six":
            _CLIPS[name] = clip((0.2 * rng.standard_normal((5006, 6))).astype(np.float32), "f32", 44100)
        elif name == "long":                               # 1.4 s (61 740 samples at 44.1 kHz: what the resampler hook takes):
            tt = np.arange(22400)                          # 14 whole hops, 11 blocks for the level stage to gate
            v = np.stack([0.3 * np.sin(2 * np.pi * 330.0 * tt / 16000), 0.1 * np.sin(2 * np.pi * 1250.0 * tt / 16000)], 1)
            v[8000:17600] *= 0.0001                        # 0.6 s that the absolute gate drops: three whole blocks
            _CLIPS[name] = clip((v * (1.0 + 0.05 * rng.standard_normal(v.shape))).astype(np.float32), "f32", 16000)
        elif name == "zeros":
            _CLIPS[name] = clip(np.zeros((3000, 2), dtype=np.float32), "f32", 44100)
    return _CLIPS[name]


def sides_at(eng, c, rate, loudness, channel, rep):
    """(side 0, side 1, what info->bed must be) at the output rate by the existing calls; one array twice where the sides are
    one.  Two different sides are scaled by the gain the call reported (`rep`), itself held against the restatement."""
    ch = SR.sides(-1 if channel is None else channel, c[1].channels)
    if ch[0] == ch[1]:
        bed, brep = bed_at(eng, c, rate, loudness, channel)
        return bed, bed, brep
    key = (c[0], rate)
    if key not in _SIDES:
        _SIDES[key] = [eng.intake([c], channel=k) for k in ch]
    (p0, r0), (p1, r1) = _SIDES[key]
    target = 0 if loudness is None else int(round(100 * loudness))
    want = SR.pair_measure(p0[0], p1[0], target)
    lv = rep.bed.level
    print(f"pair level: L {lv.lufs:.12f} (ref {want.L:.12f}), p {lv.peak:.8g}, g {lv.gain:.8g} (ref {float(want.g):.8g}), "
          f"gate margin {want.margin:.3g} LU")
    assert want.margin >= 1e-3                             # no block can change sides through rounding
    assert (lv.lufs == want.L or abs(lv.lufs - want.L) <= 1e-9) and np.float32(lv.peak) == want.p     # (-inf: digital silence)
    assert (lv.blocks, lv.gated, lv.capped) == (want.blocks, want.gated, want.capped)
    assert abs(lv.gain / float(want.g) - 1.0) <= 2.0 ** -23 + 2e-10 and (target != 0 or lv.gain == 1.0)
    assert rep.bed.n44 == r0[0].n44 == r1[0].n44 and rep.bed.cut == r0[0].cut
    assert (rep.bed.clipped, rep.bed.nonfinite) == (r0[0].clipped + r1[0].clipped, r0[0].nonfinite + r1[0].nonfinite)
    g = np.float32(lv.gain)
    out = []
    for piece in (p0[0], p1[0]):
        b44 = (piece * g).astype(np.float32) if target != 0 else piece.copy()
        out.append(b44 if rate == 44100 else eng.test_resample(b44, rate).copy())
    return out[0], out[1], None


def check(eng, x, c, regions, p: R.Params, rate=FO, loudness=None, channel=None):
    """One call against the restatement, everything exact.  Returns (got y, report, reference)."""
    params = native(p, 0 if loudness is None else int(round(100 * loudness)), -1 if channel is None else channel)
    y, rep, D = eng.mix_stereo(x, c, regions, sample_rate=rate, nodes=True, params=params)
    if c is None:
        b0 = b1 = brep = None
    else:
        b0, b1, brep = sides_at(eng, c, rate, loudness, channel, rep)
    want = SR.mix(x, b0, b1, regions, rate, p)
    assert (rep.n, rep.bed_len, rep.hops, rep.active) == (want.N, 0 if c is None else len(b0), want.Nh, int(want.act.sum()))
    assert np.array_equal(D, want.D) and rep.duck_max == want.dmax / 100.0
    assert np.float32(rep.peak) == want.pk and np.float32(rep.gain) == want.sg and rep.capped == want.capped
    if c is None:
        assert rep.bed.n44 == 0 and rep.bed.level.blocks == 0 and rep.bed.level.gain == 0.0        # zeroed
    elif brep is not None:
        assert rep.bed == brep
    same = bits(y) == bits(want.y)
    assert y.shape == (want.N, 2) and same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    return y, rep, want


def spread(n, lead, step=97):
    """Regions over a programme of n samples that exercise the lookup: touching pairs, single frames, holes, all five pans,
    and - where the timeline reaches it - edges one frame before, on and one frame behind the first SPAN boundary."""
    regions, at, k = [], 0, 0
    edges = sorted({a for a in (SPAN - 1 - lead, SPAN - lead, SPAN + 1 - lead) if 0 < a < n})
    while at < n:
        e = min(n, at + (1 if k % 5 == 2 else 2 if k % 5 == 3 else step + k))
        for cut in edges:
            if at < cut < e:
                e = cut
        regions.append((at, e, PANS[k % 5]))
        at = e if k % 3 else e + (k % 7)                   # touching, or a hole of up to six frames
        k += 1
    return regions


@pytest.mark.parametrize("N", [1, H - 1, H, H + 1, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 3])
@pytest.mark.parametrize("lead", [0, 37, 164])
def test_sizes_leads_and_regions(eng, N, lead):
    """Every size at every alignment of the programme, a stereo bed of odd length that wraps inside four-frame groups (the
    offset is no multiple of 4), regions with edges inside groups and around the SPAN boundary."""
    x = speech(N, seed=N + lead, quiet=[(N // 3, N // 2)])
    p = R.Params(depth=1200, attack=3, release=5, lead=lead, tail=lead // 4, fade_in=50, fade_out=120, offset=11)
    y, rep, want = check(eng, x, made("stereo"), spread(N, lead), p)
    assert rep.bed_len == 909


@pytest.mark.parametrize("loop", [1, 0])
def test_a_bed_that_wraps_or_ends_inside_a_group(eng, loop):
    x = speech(2 * 909 + 77, seed=5, amp=0.1, quiet=[(300, 700)])
    for offset in (0, 1, 2, 3, 906, 907, 908, 909, 2 * 909 + 5):
        check(eng, x, made("stereo"), [(10, 500, -37), (500, 1500, 100)], R.Params(depth=900, attack=3, release=4, offset=offset, loop=loop))
    check(eng, x, made("mono"), [(0, len(x), 1)], R.Params(offset=907, loop=loop, lead=2))


REGION_CASES = {
    "none": lambda n: [],
    "one-over-everything": lambda n: [(0, n, -37)],
    "edge-inside-a-group": lambda n: [(0, 6, 100), (6, 7, -100), (9, n - 1, 1)],
    "on-the-span-boundary": lambda n: [(0, SPAN, -100), (SPAN, n, 100)],
    "one-before-the-boundary": lambda n: [(5, SPAN - 1, -100), (SPAN - 1, SPAN + 2, 37)],
    "one-behind-the-boundary": lambda n: [(0, SPAN + 1, 100), (SPAN + 1, SPAN + 2, -100)],
    "one-frame": lambda n: [(SPAN + 77, SPAN + 78, 100)],
    "last-frame": lambda n: [(n - 1, n, -100)],
    "4096-of-one-frame": lambda n: [(i, i + 1, PANS[i % 5]) for i in range(4096)],
    "4096-apart": lambda n: [(2 * i + 1, 2 * i + 2, PANS[(i * 3) % 5]) for i in range(4096)],
    "touching": lambda n: [(100, 200, -37), (200, 300, 37), (300, 301, -37), (301, SPAN + 300, 1)],
}


@pytest.mark.parametrize("name", list(REGION_CASES))
@pytest.mark.parametrize("lead", [0, 37])
def test_regions(eng, name, lead):
    n = 2 * SPAN + 203
    x = speech(n, seed=len(name), amp=0.15, quiet=[(SPAN - 300, SPAN - 100)])
    y, rep, want = check(eng, x, made("stereo"), REGION_CASES[name](n), R.Params(depth=900, attack=3, release=4, lead=lead, tail=3))
    if name == "one-frame":
        i = lead + SPAN + 77
        assert want.s[i, 0] == 0 and want.s[i, 1] == x[SPAN + 77] and np.array_equal(want.s[i + 1], [x[SPAN + 78]] * 2)


@pytest.mark.parametrize("name,channel", [("stereo", None), ("stereo-s16", None), ("mono", None), ("six", None), ("six", 4),
                                          ("stereo", 1), (None, None)],
                         ids=["f32-stereo", "s16-stereo-48k", "mono", "six-first-two", "six-channel-4", "stereo-channel-1", "no-bed"])
def test_bed_sides(eng, name, channel):
    x = speech(9 * H + 13, seed=21, amp=0.15, quiet=[(2 * H, 4 * H)])
    c = None if name is None else made(name)
    p = R.Params(depth=900, attack=3, release=4, lead=8, tail=5, offset=3)
    y, rep, want = check(eng, x, c, [(0, 500, -100), (500, 900, 37)], p, channel=channel)
    if name is None:
        assert rep.bed_len == 0 and not y[:8].any() and not y[8 + len(x):].any()
        l, r = SR.gains_of(37)
        assert np.array_equal(bits(y[8 + 500:8 + 900, 1]), bits(x[500:900] * r)) and not rep.capped
    elif name in ("stereo", "stereo-s16", "six") and channel is None:
        assert not np.array_equal(y[:8, 0], y[:8, 1])      # the lead: the bed alone, two different sides
    else:
        assert np.array_equal(bits(y[:8, 0]), bits(y[:8, 1]))


def test_a_two_sided_bed_at_its_own_rate(eng):
    """Fo = 44100: nothing is resampled, the two sides are copied to the bed buffer by the resampler's copy mode, and with
    5006 samples a side (no multiple of four) side 1 begins on its 16-byte pitch, two samples behind the end of side 0.  The
    bed wraps twice under nine hops and an odd remainder.  (The same bed through a stereo stream at this rate:
    tests/test_stereo_live_gpu.py, limited-44100.)"""
    h = 44100 // 50
    x = speech(9 * h + 17, seed=44, amp=0.15, quiet=[(2 * h, 4 * h)])
    p = R.Params(depth=900, attack=3, release=4, lead=8, tail=5, offset=3)
    y, rep, want = check(eng, x, made("stereo"), [(0, 500, -100), (500, 4 * h + 1, 37), (7 * h, len(x), 100)], p, rate=44100)
    assert rep.bed_len == 5006 and rep.bed_len % 4 != 0
    assert not np.array_equal(y[:8, 0], y[:8, 1])          # the lead: the bed alone, two different sides


@pytest.mark.parametrize("loudness", [None, -30.0])
@pytest.mark.parametrize("name", ["long", "stereo-s16"])
def test_pair_level(eng, name, loudness):
    """bed_loudness 0 and -3000 on a bed with two different sides: L, p, g against the restatement (in sides_at), one g."""
    x = speech(30 * H + 7, seed=8, amp=0.1, quiet=[(10 * H, 18 * H)])
    y, rep, want = check(eng, x, made(name), [(0, 10 * H, -37)], R.Params(), loudness=loudness)
    lv = rep.bed.level
    assert np.isfinite(lv.lufs) and (lv.gain != 1.0) == (loudness is not None)
    if name == "long":
        assert lv.blocks == 11 and 0 < lv.gated < lv.blocks


def test_ceiling_binds_on_the_right_channel_only(eng):
    x = speech(7 * H + 5, seed=12, amp=0.05)
    x[400] = 0.97
    y, rep, want = check(eng, x, made("zeros"), [(390, 410, 100)], R.Params())
    assert rep.capped and np.float32(rep.peak) == np.float32(0.97) and np.abs(want.m[:, 0]).max() < 0.5
    assert np.array_equal(bits(y[:, 0]), bits(want.m[:, 0] * want.sg)) and np.array_equal(bits(y[:, 1]), bits(want.m[:, 1] * want.sg))
    x[400] = 0.5                                           # under the ceiling: mix_scale_kernel does not run
    y, rep, want = check(eng, x, made("zeros"), [(390, 410, 100)], R.Params())
    assert not rep.capped and rep.gain == 1.0 and np.array_equal(bits(y[:390, 0]), bits(x[:390])) and not y[390:410, 0].any()


@pytest.mark.parametrize("loudness", [None, -30.0])
def test_centred_over_a_mono_bed_is_the_mix_stage_twice(eng, loudness):
    x = speech(SPAN + 3 * H + 7, seed=14, quiet=[(5 * H, 9 * H)])
    p = R.Params(depth=1500, attack=5, release=9, lead=37, tail=2, fade_in=40, fade_out=300, offset=5)
    params = native(p, 0 if loudness is None else -3000)
    m, mrep, mD = eng.mix(x, made("mono"), sample_rate=FO, params=params, nodes=True)
    for regions in ([], [(0, len(x), 0)], [(3, 4, 0), (4, SPAN, 0)]):
        y, rep, D = eng.mix_stereo(x, made("mono"), regions, sample_rate=FO, params=params, nodes=True)
        assert np.array_equal(bits(y[:, 0]), bits(m)) and np.array_equal(bits(y[:, 1]), bits(m))
        assert rep == mrep and np.array_equal(D, mD)
    six = made("six")                                      # ... and with one channel of a file on both sides
    m, mrep = eng.mix(x, six, sample_rate=FO, params=native(p, 0 if loudness is None else -3000, 4))
    y, rep = eng.mix_stereo(x, six, [], sample_rate=FO, params=native(p, 0 if loudness is None else -3000, 4))
    assert np.array_equal(bits(y[:, 0]), bits(m)) and np.array_equal(bits(y[:, 1]), bits(m)) and rep == mrep


def test_each_channel_is_the_mono_call_over_its_programme(eng):
    """bed_loudness = 0, uncapped: channel c is ft_codec_mix with channel = c over s_c (the pans keep every hop's activity)."""
    n = SPAN + 5 * H + 3
    x = speech(n, seed=15, amp=0.1, quiet=[(3 * H, 6 * H)])
    regions = [(0, 2 * H + 5, -37), (2 * H + 5, 8 * H, 1), (SPAN - 1, SPAN + 9, -37)]
    p = R.Params(depth=1200, threshold=1e-6, attack=3, release=5, lead=4, tail=9, fade_in=30, fade_out=50, offset=7)
    c = made("stereo")
    y, rep, D = eng.mix_stereo(x, c, regions, sample_rate=FO, params=native(p), nodes=True)
    assert not rep.capped
    left, right = SR.gains_of(SR.region_pans(regions, n))
    for k, gain in enumerate((left, right)):
        m, mrep, mD = eng.mix((x * gain).astype(np.float32), c, sample_rate=FO, params=native(p, 0, k), nodes=True)
        assert not mrep.capped and np.array_equal(mD, D) and np.array_equal(bits(y[:, k]), bits(m))


def test_a_nan_is_never_the_peak_and_stays_in_both_channels(eng):
    x = speech(6 * H, seed=16, amp=0.1)
    x[5 * H + 1] = np.nan
    for pan in (-100, 0, 100):
        y, rep, want = check(eng, x, made("stereo"), [(5 * H, 5 * H + 2, pan)], R.Params(depth=1200, attack=2, release=2))
        assert np.isnan(y[5 * H + 1]).all() and np.isfinite(rep.peak) and np.isfinite(y[5 * H]).all()


def test_buffers_regrow_and_calls_repeat(eng):
    small, big = speech(3 * H, seed=30), speech(5 * SPAN + 1, seed=31, quiet=[(SPAN, 2 * SPAN)])
    p = R.Params(depth=1500, attack=5, release=9, lead=3, tail=2, fade_out=300)
    a1, _, _ = check(eng, small, made("stereo"), [(7, 90, -37)], p, loudness=-30.0)
    b1, _, _ = check(eng, big, made("long"), spread(len(big), 3, step=1500), p, loudness=-30.0)
    a2, _, _ = check(eng, small, made("stereo"), [(7, 90, -37)], p, loudness=-30.0)
    b2, _, _ = check(eng, big, made("long"), spread(len(big), 3, step=1500), p, loudness=-30.0)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))
    m, _ = eng.mix(small, bed_clip(), sample_rate=FO, params=native(p))      # the mix stage between them is as it was
    a3, _, _ = check(eng, small, made("stereo"), [(7, 90, -37)], p, loudness=-30.0)
    m2, _ = eng.mix(small, bed_clip(), sample_rate=FO, params=native(p))
    assert np.array_equal(bits(a1), bits(a3)) and np.array_equal(bits(m), bits(m2))


# ---- refusals, in the header's order: each refused call leaves the next good call's result as it was
def _raw(eng, x, c, regions=((2, 9, -37), (9, 30, 100)), mp_kw=None, rate=FO, item_kw=None, null=None, cap=None, n=None, R=None):
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
    reg = (L.ft_pan_region * max(len(regions), 1))(*[L.ft_pan_region(a, e, pan, 0) for a, e, pan in regions])
    n = len(x) if n is None else n
    N = max(1, len(x) + 5 + 6)
    y = np.full((N, 2), 7.0, dtype=np.float32)
    D = np.full(N // H + 3, -7, dtype=np.int32)
    total, out = C.c_int64(-7), L.ft_mix_info()
    args = dict(x=x.ctypes.data_as(C.c_void_p), regions=reg, bed=C.byref(it), mp=C.byref(m), y=y.ctypes.data_as(C.c_void_p),
                total=C.byref(total), info=C.byref(out))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_mix_stereo(eng._h, args["x"], n, rate, args["regions"], len(regions) if R is None else R, args["bed"],
                                     args["mp"], args["y"], N if cap is None else cap, args["total"], D.ctypes.data_as(C.c_void_p),
                                     args["info"])
    return st, y, D, total.value, buf


REFUSALS = [
    ("x", dict(null="x")), ("mp", dict(null="mp")), ("y", dict(null="y")), ("total", dict(null="total")), ("info", dict(null="info")),
    ("rate", dict(rate=7999)), ("rate-L", dict(rate=44101)),
    ("n", dict(n=0)),
    ("regions-null", dict(null="regions")), ("R-high", dict(R=4097)), ("R-neg", dict(R=-1)),
    ("region-order", dict(regions=((9, 30, 0), (2, 9, 0)))), ("region-overlap", dict(regions=((2, 10, 0), (9, 30, 0)))),
    ("region-empty", dict(regions=((4, 4, 0),))), ("region-neg", dict(regions=((-1, 4, 0),))),
    ("region-past-n", dict(regions=((2, 4 * H + 4, 0),))),
    ("pan-high", dict(regions=((2, 9, 101),))), ("pan-low", dict(regions=((2, 9, -101),))),
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
    ("bed-channel", dict(mp_kw=dict(channel=2))), ("bed-channel-low", dict(mp_kw=dict(channel=-2))),
    ("bed-rate", dict(item_kw=dict(rate=7000))),
    ("bed-length", dict(item_kw=dict(n_frames=1 << 29), too_long=True)),
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(eng, name, kw):
    from fish_tts_amd import _lib as L
    kw = dict(kw)
    want_st = L.FT_ERR_TOO_LONG if kw.pop("too_long", False) else L.FT_ERR_ARG
    x = speech(4 * H + 3, seed=40)
    c = made("stereo")
    st, y0, D0, t0, _ = _raw(eng, x, c)
    assert st == L.FT_OK and t0 == len(x) + 11
    st, y, D, t, _ = _raw(eng, x, c, **kw)
    assert st == want_st, (name, st, eng.lib.ft_last_error(eng._h))
    assert np.all(y == 7.0) and np.all(D == -7) and t == -7          # nothing written
    st, y1, D1, t1, _ = _raw(eng, x, c)
    assert st == L.FT_OK and t1 == t0 and np.array_equal(bits(y1), bits(y0)) and np.array_equal(D1, D0)
    p = R.Params(depth=1200, threshold=0.01, attack=15, release=40, lead=5, tail=6, fade_out=100)
    b0, b1, _ = sides_at(eng, c, FO, None, None, eng.mix_stereo(x, c, [], sample_rate=FO, params=native(p))[1])
    assert np.array_equal(bits(y1), bits(SR.mix(x, b0, b1, [(2, 9, -37), (9, 30, 100)], FO, p).y))      # ... and it is right


def test_a_null_bed_and_an_empty_table_are_no_refusals(eng):
    from fish_tts_amd import _lib as L
    x = speech(4 * H + 3, seed=40)
    st, y, D, t, _ = _raw(eng, x, made("stereo"), null="bed")
    assert st == L.FT_OK and t == len(x) + 11 and not y[:5].any()
    st, y, D, t, _ = _raw(eng, x, made("stereo"), regions=(), null="regions")     # R = 0: the table is not read
    assert st == L.FT_OK and t == len(x) + 11
    st, *_ = _raw(eng, x, made("stereo"), null="bed", mp_kw=dict(depth=-1))        # mp is judged without a bed too
    assert st == L.FT_ERR_ARG


def test_the_earlier_reason_wins(eng):
    """The order of the checks: a call wrong in two ways is refused for the earlier one (the message names it)."""
    from fish_tts_amd import _lib as L
    x = speech(2 * H, seed=41)
    order = [("sample rate", dict(rate=7999)), ("n must", dict(n=0)), ("null region table", dict(null="regions")),
             ("R outside", dict(R=4097)), ("out of order", dict(regions=((5, 5, 0),))), ("pan outside", dict(regions=((5, 6, 101),))),
             ("bed_loudness", dict(mp_kw=dict(bed_loudness=-1))),
             ("depth", dict(mp_kw=dict(depth=-1))), ("threshold", dict(mp_kw=dict(threshold=-1.0))),
             ("attack", dict(mp_kw=dict(attack=0))), ("release", dict(mp_kw=dict(release=0))), ("lead", dict(mp_kw=dict(lead=-1))),
             ("tail", dict(mp_kw=dict(tail=-1))), ("fade_in", dict(mp_kw=dict(fade_in=-1))), ("fade_out", dict(mp_kw=dict(fade_out=-1))),
             ("offset", dict(mp_kw=dict(offset=-1))), ("loop", dict(mp_kw=dict(loop=3))), ("capacity", dict(cap=1)),
             ("fmt", dict(item_kw=dict(fmt=9)))]
    for (w1, k1), (w2, k2) in zip(order, order[1:]):
        if "regions" in k1 and "regions" in k2:
            continue                                       # (one table cannot be wrong in both ways at one region)
        kw = {}
        for k in (k2, k1):
            for key, v in k.items():
                kw[key] = {**kw.get(key, {}), **v} if isinstance(v, dict) else v
        st, *_ = _raw(eng, x, made("stereo"), **kw)
        msg = eng.lib.ft_last_error(eng._h).decode()
        assert st == L.FT_ERR_ARG and w1 in msg and w2 not in msg.replace(w1, ""), (w1, w2, msg)
    st, *_ = _raw(eng, x, made("stereo"), regions=((5, 5, 101),))      # the place of a region before its pan
    assert st == L.FT_ERR_ARG and "out of order" in eng.lib.ft_last_error(eng._h).decode()
