"""GPU: the level stage (level_filter_kernel, level_gain_kernel, level_scale_kernel) through ft_codec_loudness against the
float64 restatement tests/level_ref.py at five rates - hop sums, loudness, peak, gain, block counts, the multiply - then the
decode calls that carry a level against ft_codec_loudness over the rows of the level-less call, bit for bit, and the refusals.

Bounds (from the issue that asked for the stage): each hop sum within 1e-9 of the largest one; L within 1e-6 LU (float64
sums of at most 2^24 terms in any order sit near 1e-10 relative; 1e-6 LU is 2.3e-7 in energy; a wrong coefficient, a dropped
hop or a gate on the wrong side moves L by more than 1e-3); the peak bit for bit; the gain within 4e-7 relative (1.2e-7 from
the L bound plus two float32 roundings).  Every non-degenerate input has a gate margin of at least 1e-3 LU in the
restatement, asserted here, so that no block can change sides through rounding."""
import ctypes as CT

import numpy as np
import pytest

from tests import level_ref as R
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec
from tests.test_timescale_gpu import _codes

pytestmark = pytest.mark.gpu

# A lane of level_filter_kernel owns one hop and a workgroup 64 of them: the long input spans two whole workgroups and a
# third that is partly filled, its last lane over a hop that is cut short.
LANES = 64
LONG_HOPS = 2 * LANES + 5
MAX_FRAMES = 9600          # ft_codec_loudness takes 2 * max_frames * frame_len * 48000 / 44100 samples: the long input at 48 kHz
TARGET = -1600


@pytest.fixture(scope="module")
def tiny():
    eng, _ = make_codec(tiny_codec_shape(), max_frames=MAX_FRAMES)
    yield eng
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inputs(rate):
    """name -> (x float32, degenerate).  Seeds were picked on the CPU for a gate margin >= 1e-3 LU (asserted by the test)."""
    H = R.hop(rate)
    rng = np.random.default_rng(rate)
    xs = {}
    for n in (1, H - 1, 4 * H - 1, 4 * H, 4 * H + 1, 7 * H + 3):
        xs[f"noise {n}"] = (0.1 * rng.standard_normal(n)).astype(np.float32), False
    # 2.5 s: bursts of noise between silences, one passage 15 dB down, everything on a 0.05 DC offset
    n = int(2.5 * rate)
    t = np.arange(n) / rate
    env = np.zeros(n)
    env[(t >= 0.1) & (t < 0.9)] = 0.2
    env[(t >= 1.1) & (t < 1.7)] = 0.2 * 10.0 ** (-15.0 / 20.0)
    env[(t >= 1.9) & (t < 2.4)] = 0.2
    xs["bursts"] = (env * rng.standard_normal(n) + 0.05).astype(np.float32), False
    # a 20 Hz tone plus noise over LONG_HOPS hops and a little more: a wrong hand-over of filter state shows here
    n = LONG_HOPS * H + 7
    xs["long tone"] = (0.4 * np.sin(2.0 * np.pi * 20.0 * np.arange(n) / rate) + 0.02 * rng.standard_normal(n)).astype(np.float32), False
    xs["silence"] = np.zeros(7 * H + 3, dtype=np.float32), True
    # an impulse train over faint noise: the ceiling binds
    x = 1e-3 * rng.standard_normal(9 * H + 5)
    x[::H // 3] = 0.95
    x[5 * H + 11] = -0.97
    xs["impulses"] = x.astype(np.float32), False
    return xs


@pytest.fixture(scope="module")
def refs():
    """The restatement of every input at TARGET, computed once."""
    out = {}
    for rate in R.RATES:
        for name, (x, degenerate) in _inputs(rate).items():
            out[rate, name] = (x, degenerate, R.measure(x, rate, TARGET))
    return out


@pytest.mark.parametrize("rate", R.RATES)
def test_loudness_against_the_restatement(tiny, refs, rate):
    H = R.hop(rate)
    assert (rate == 11025) == (rate % 10 != 0) and (rate != 11025 or H == 1102)
    saw = set()
    for (r, name), (x, degenerate, ref) in refs.items():
        if r != rate:
            continue
        if not degenerate:
            assert ref.margin >= 1e-3, (rate, name, ref.margin)
            assert np.isfinite(ref.L), (rate, name)
        info, y = tiny.loudness(x, rate, TARGET / 100.0)
        e = tiny.test_level_hops()
        print(f"{rate} {name}: L {info.lufs:.6f} (ref {ref.L:.6f}), p {info.peak:.6g}, g {info.gain:.7g} (ref {float(ref.g):.7g}), "
              f"blocks {info.blocks}/{info.gated}, capped {info.capped}, margin {ref.margin:.3g}, "
              f"hop err {np.max(np.abs(e - ref.e)) / max(np.max(ref.e), 1e-300) if len(e) else 0:.2e}")
        assert len(e) == len(ref.e) == (len(x) + H - 1) // H, (rate, name)
        assert np.all(np.abs(e - ref.e) <= 1e-9 * np.max(ref.e)), (rate, name)
        assert (info.blocks, info.gated) == (ref.blocks, ref.gated), (rate, name)
        if np.isfinite(ref.L):
            assert abs(info.lufs - ref.L) <= 1e-6, (rate, name, info.lufs, ref.L)
        else:
            assert info.lufs == -np.inf and info.gain == 1.0, (rate, name)
        assert _bits(np.float32(info.peak)) == _bits(ref.p), (rate, name)
        assert abs(info.gain / float(ref.g) - 1.0) <= 4e-7, (rate, name, info.gain, float(ref.g))
        assert info.capped == ref.capped, (rate, name)
        assert np.array_equal(_bits(y), _bits(np.float32(info.gain) * x)), (rate, name)
        if info.capped:
            assert np.max(np.abs(y)) <= np.float32(R.CEILING * (1 + 2.0 ** -23)), (rate, name)
            saw.add("capped")
        if ref.gated < ref.blocks and ref.gated:
            saw.add("gated")
        # target = 0 measures only and leaves the samples alone; a second call gives the same bits
        m, y0 = tiny.loudness(x, rate)
        assert np.array_equal(_bits(y0), _bits(x)) and m.gain == 1.0 and not m.capped, (rate, name)
        assert (m.lufs, m.peak, m.blocks, m.gated) == (info.lufs, info.peak, info.blocks, info.gated), (rate, name)
        info2, y2 = tiny.loudness(x, rate, TARGET / 100.0)
        assert info2 == info and np.array_equal(_bits(y2), _bits(y)), (rate, name)
        assert np.array_equal(tiny.test_level_hops().view(np.uint64), e.view(np.uint64)), (rate, name)
    assert saw == {"capped", "gated"}, saw            # the ceiling bound somewhere, and a gate cut something somewhere
    ref = refs[rate, "bursts"][2]
    assert 0 < ref.gated < ref.blocks


def test_an_empty_item_and_a_null_output(tiny):
    from fish_tts_amd import _lib as L
    info = L.ft_level_info()
    x = np.zeros(4, dtype=np.float32)
    tiny._check(tiny.lib.ft_codec_loudness(tiny._h, x.ctypes.data_as(CT.c_void_p), 0, 16000, TARGET, CT.byref(info), None),
                "ft_codec_loudness")
    assert info.lufs == -np.inf and info.gain == 1.0 and info.peak == 0.0 and info.blocks == 0 and info.gated == 0
    x = (0.1 * np.random.default_rng(1).standard_normal(8000)).astype(np.float32)
    tiny._check(tiny.lib.ft_codec_loudness(tiny._h, x.ctypes.data_as(CT.c_void_p), len(x), 16000, TARGET, CT.byref(info), None),
                "ft_codec_loudness")
    want, _ = tiny.loudness(x, 16000, TARGET / 100.0)
    assert (info.lufs, info.gain, info.blocks) == (want.lufs, np.float32(want.gain), want.blocks)


LENS = np.array([3, 900, 12], dtype=np.int32)       # 900 frames: at least five whole hops (two blocks) through every chain below
STAGES = [dict(), dict(sample_rate=16000), dict(speed=1.25, pitch=3)]


@pytest.fixture(scope="module")
def block():
    shape = tiny_codec_shape()
    b = np.zeros((len(LENS), shape.n_codebooks + 1, int(LENS.max())), dtype=np.int32)
    for i, T in enumerate(LENS):
        b[i, :, :T] = _codes(shape, int(T), 70 + i)
    return b


@pytest.mark.parametrize("kw", STAGES, ids=["44k", "16k", "speed+pitch"])
def test_decode_with_a_level_is_loudness_over_the_rows(tiny, block, kw):
    from fish_tts_amd.codec_engine import OutputFx
    fx = OutputFx.of(**kw)
    plain = tiny.decode(block, LENS, **kw)
    assert np.array_equal(_bits(tiny.decode(block, LENS, loudness=None, **kw)), _bits(plain))
    levels = []
    got = tiny.decode(block, LENS, loudness=TARGET / 100.0, levels=levels, **kw)
    assert got.shape == plain.shape and len(levels) == len(LENS)
    for b, T in enumerate(LENS):
        n = fx.out_len(int(T) * tiny.frame_len)
        info, y = tiny.loudness(plain[b, :n], fx.wav_rate, TARGET / 100.0)
        assert levels[b] == info, (b, levels[b], info)
        assert np.array_equal(_bits(got[b, :n]), _bits(y)), b
        assert not np.any(_bits(got[b, n:])), b              # zeros past a shorter item's end
        assert not np.array_equal(_bits(y), _bits(plain[b, :n])), b
    assert levels[1].blocks > 1 and np.isfinite(levels[1].lufs)
    if not levels[1].capped:
        after, _ = tiny.loudness(got[1, :fx.out_len(900 * tiny.frame_len)], fx.wav_rate)
        assert abs(after.lufs - TARGET / 100.0) <= 1e-3


@pytest.mark.parametrize("kw", STAGES[:2], ids=["44k", "16k"])
def test_decode_join_with_a_level_is_the_join_of_the_levelled_rows(tiny, block, kw):
    from fish_tts_amd.codec_engine import OutputFx
    fx = OutputFx.of(**kw)
    rows = tiny.decode(block, LENS, loudness=TARGET / 100.0, **kw)
    items = [rows[b, :fx.out_len(int(T) * tiny.frame_len)] for b, T in enumerate(LENS)]
    codes = [block[b, :, :T] for b, T in enumerate(LENS)]
    peak = max(float(np.max(np.abs(x))) for x in items)
    params, gaps = (0.3 * peak, 40, 60, 20), [5, 7, 9]
    levels = []
    audio, cuts = tiny.decode_join(codes, params=params, gaps=gaps, loudness=TARGET / 100.0, levels=levels, **kw)
    y, total, wcuts = tiny.test_join(items, params, gaps)
    assert len(audio) == total > 0 and np.array_equal(_bits(audio), _bits(y[:total]))
    assert cuts.tolist() == wcuts.tolist() and len(levels) == len(LENS)
    for b, x in enumerate(items):
        assert levels[b] == tiny.loudness(tiny.decode(block[b:b + 1, :, :LENS[b]], **kw)[0], fx.wav_rate, TARGET / 100.0)[0], b
    # the items split over two calls, `started` carried
    a, ca = tiny.decode_join(codes[:1], params=params, gaps=gaps[:1], loudness=TARGET / 100.0, **kw)
    b2, cb = tiny.decode_join(codes[1:], params=params, gaps=gaps[1:], started=len(a) > 0, loudness=TARGET / 100.0, **kw)
    assert np.array_equal(_bits(np.concatenate([a, b2])), _bits(audio))
    assert np.concatenate([ca, cb]).tolist() == cuts.tolist()
    # without a level the call is the one it was
    p0, c0 = tiny.decode_join(codes, params=params, gaps=gaps, **kw)
    p1, c1 = tiny.decode_join(codes, params=params, gaps=gaps, loudness=None, **kw)
    assert np.array_equal(_bits(p0), _bits(p1)) and c0.tolist() == c1.tolist()


def test_bad_targets_are_refused_before_any_device_work(tiny, block):
    from fish_tts_amd import _lib as L
    lib, h = tiny.lib, tiny._h
    P = lambda a: a.ctypes.data_as(CT.c_void_p)      # noqa: E731
    x = np.full(4000, 0.25, dtype=np.float32)
    B, _, T = block.shape
    for bad in (-5001, -499, -1, 1, 1600, -(1 << 31)):
        y = np.full(4000, 123.0, dtype=np.float32)
        info = L.ft_level_info(7.0, 7.0, 7.0, 7, 7, 7)
        assert lib.ft_codec_loudness(h, P(x), len(x), 16000, bad, CT.byref(info), P(y)) == L.FT_ERR_ARG, bad
        assert np.all(y == 123.0) and (info.lufs, info.gain, info.blocks) == (7.0, 7.0, 7), bad
        audio = np.full((B, T * tiny.frame_len), 123.0, dtype=np.float32)
        out_lens = np.full(B, -7, dtype=np.int64)
        infos = (L.ft_level_info * B)(*[L.ft_level_info(7.0, 7.0, 7.0, 7, 7, 7) for _ in range(B)])
        assert lib.ft_codec_decode_level(h, P(block), B, T, P(LENS), 44100, 100, 0, bad, P(audio), P(out_lens), infos) == L.FT_ERR_ARG
        assert np.all(audio == 123.0) and np.all(out_lens == -7) and all(i.blocks == 7 for i in infos), bad
        jp = L.ft_join_params(0.0, 220, 0, 0)
        gaps = np.zeros(B, dtype=np.int64)
        total, cuts = CT.c_int64(-7), np.full((B, 2), -7, dtype=np.int64)
        flat = np.full(B * T * tiny.frame_len, 123.0, dtype=np.float32)
        assert lib.ft_codec_decode_join_level(h, P(block), B, T, P(LENS), 44100, 100, 0, bad, CT.byref(jp), P(gaps), 0, P(flat),
                                              len(flat), CT.byref(total), P(cuts), infos) == L.FT_ERR_ARG, bad
        assert np.all(flat == 123.0) and total.value == -7 and np.all(cuts == -7) and all(i.blocks == 7 for i in infos), bad
    info = L.ft_level_info()
    assert lib.ft_codec_loudness(h, P(x), len(x), 12345, TARGET, CT.byref(info), None) == L.FT_ERR_ARG      # a refused rate
    assert lib.ft_codec_loudness(h, P(x), len(x), 16000, TARGET, None, None) == L.FT_ERR_ARG
    assert lib.ft_codec_loudness(h, None, len(x), 16000, TARGET, CT.byref(info), None) == L.FT_ERR_ARG
    too_long = 2 * MAX_FRAMES * tiny.frame_len * 48000 // 44100 + 2
    assert lib.ft_codec_loudness(h, P(x), too_long, 48000, TARGET, CT.byref(info), None) == L.FT_ERR_TOO_LONG
    for bad in (-50.5, -4, 0, 3, float("nan"), True):
        with pytest.raises(ValueError):
            tiny.decode(block, LENS, loudness=bad)
        with pytest.raises(ValueError):
            tiny.decode_join([block[0, :, :3]], loudness=bad)
        with pytest.raises(ValueError):
            tiny.loudness(x, 16000, bad)


def test_streams_refuse_a_level(tiny):
    from fish_tts_amd.codec_engine import CodecStream, OutputFx
    fx = OutputFx.of(sample_rate=16000, loudness=-16)
    before = set(tiny._streams)
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        tiny.stream(fx=fx)
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        CodecStream(tiny, fx=OutputFx.of(loudness=-16))
    assert set(tiny._streams) == before
    st = tiny.stream(sample_rate=16000)
    try:
        object.__setattr__(st, "fx", fx)                # a stream that came by a level all the same
        with pytest.raises(ValueError, match="loudness needs the whole utterance"):
            tiny.decode_streams([st], [np.zeros((tiny.R, 2), dtype=np.int32)])
    finally:
        object.__setattr__(st, "fx", OutputFx.of(sample_rate=16000))
        st.close()
