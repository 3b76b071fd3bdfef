"""GPU: the pitch stage behind pitch= (pitch_kernel) and the time-scale stage at its rational rate - through the test hook
against the restatements of tests/pitch_ref.py (the time-scaled intermediate given the kernel's alignments, every alignment
within the float32 summation bound of the best one, the shifted samples within the float32 bound of their sum); a tone's
spectrum; ft_codec_decode_fxp against the hook over ft_codec_decode's waveform, alone, with a sample rate and with a
speed; pitched streams (ft_codec_stream_decode_many_at) bit for bit against the hook on their own 44.1 kHz output whatever
the chunking, alone and mixed with other streams in one call; the path without pitch unchanged; refusals."""
import ctypes as CT

import numpy as np
import pytest

from oracle import codec as C
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.pitch_ref import frame_scores_q, n_frames_q, n_out_q, pitch_ref, pitch_table, rate_of, timescale_ref_q
from tests.test_codec_gpu import make_codec
from tests.test_timescale_gpu import PLANS, _codes, _native_chunks, _same
from tests.test_timescale_host import D, N, n_out_of

pytestmark = pytest.mark.gpu

FI = 44100
COMBOS = ((100, -1200), (100, -700), (100, -1), (100, 1), (100, 700), (100, 1200), (125, 300), (80, -500), (200, 1200),
          (50, -1200))


@pytest.fixture(scope="module")
def tiny():
    eng, _ = make_codec(tiny_codec_shape(), max_frames=2048)      # the hook takes up to max_frames * 32 samples
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(0)
    xs = {"noise": rng.uniform(-1, 1, 12345).astype(np.float32),
          "tone": (0.5 * np.sin(2 * np.pi * 200 * np.arange(20000) / FI)).astype(np.float32)}
    for n in (1, 31, 1023, 1025):
        xs[f"n{n}"] = rng.uniform(-1, 1, n).astype(np.float32)
    return xs


def _check_hook(x, pct, cents, y, mid, d, what):
    num, den = rate_of(pct, cents)
    assert len(y) == n_out_of(len(x), pct), what
    if num == den:                                       # no time-scale stage: the pitch stage reads x itself
        assert len(d) == 0 and _same(mid, x), what
    else:
        assert len(mid) == n_out_q(len(x), num, den), what
        assert len(d) == n_frames_q(len(x), num, den) and d[0] == 0 and np.all(np.abs(d) <= D), what
        err = np.max(np.abs(mid - timescale_ref_q(x, num, den, deltas=d)))
        print(what, "max |mid - ref| =", err)
        assert err <= 1e-6, (what, err)
        for k, (c, cabs) in enumerate(frame_scores_q(x, num, den, d), start=1):
            slack = 2 * N * 2.0 ** -24 * cabs.max()
            assert c[d[k] + D] >= c.max() - slack, (what, k, c[d[k] + D], c.max(), slack)
    want, bound = pitch_ref(mid, cents, len(y))
    over = np.abs(y - want) - bound
    print(what, "max |y - ref| =", np.max(np.abs(y - want)), "max bound =", bound.max(), "worst margin =", over.max())
    assert np.all(over <= 0), (what, int(np.argmax(over)), over.max())


@pytest.mark.parametrize("pct,cents", COMBOS)
def test_hook_against_restatement(tiny, inputs, pct, cents):
    for name, x in inputs.items():
        y, mid, d = tiny.test_pitch(x, pct, cents)
        _check_hook(x, pct, cents, y, mid, d, (name, pct, cents))


def test_tone_moves_by_the_ratio(tiny):
    S = pitch_table(700)[0]
    x = (0.5 * np.sin(2 * np.pi * 440 * np.arange(40000) / FI)).astype(np.float32)
    y = tiny.test_pitch(x, 100, 700)[0]
    assert len(y) == len(x)
    seg = y[8192:8192 + 16384].astype(np.float64) * np.hanning(16384)
    peak = int(np.argmax(np.abs(np.fft.rfft(seg))))
    want = 440 * S / 2 ** 20 * 16384 / FI
    assert abs(peak - want) <= 2, (peak, want)


@pytest.mark.parametrize("real", [False, True])
def test_one_shot_decode_at_pitch(real):
    """decode(pitch=) rows = the hook over decode()'s rows bit for bit, exact lengths, zeros past the end of a shorter item;
    None, 0 and 0.0 are decode() bit for bit; with a sample rate as well it is the resample hook over the pitch hook, with a
    speed as well the hook at that percentage, bit for bit."""
    shape = C.CodecShape() if real else tiny_codec_shape()
    T = 60 if real else 215
    eng, _ = make_codec(shape, max_frames=256 if real else 512)     # the resample hook takes the slowed waveform
    try:
        codes = np.stack([_codes(shape, T, 1), _codes(shape, T, 2)])
        lens = np.array([T, T // 3], dtype=np.int32)
        fl = eng.frame_len
        n = [int(t) * fl for t in lens]
        base = eng.decode(codes, lens)
        for none in (None, 0, 0.0):
            assert _same(eng.decode(codes, lens, pitch=none), base)
        assert _same(eng.decode(codes, lens, speed=1.25, pitch=0), eng.decode(codes, lens, speed=1.25))
        assert _same(eng.decode(codes, lens, sample_rate=16000, pitch=None), eng.decode(codes, lens, sample_rate=16000))
        for pct, cents in (((100, 700), (80, -500)) if real else ((100, 700), (100, -1200), (125, 300), (80, -500), (200, 1200))):
            kw = {"pitch": cents / 100}
            if pct != 100:
                kw["speed"] = pct / 100
            got = eng.decode(codes, lens, **kw)
            no = [n_out_of(v, pct) for v in n]
            assert got.shape == (2, no[0]), (pct, cents, got.shape)
            hooks = [eng.test_pitch(base[b, :n[b]], pct, cents)[0] for b in range(2)]
            for b in range(2):
                assert _same(got[b, :no[b]], hooks[b]), (pct, cents, b)
            assert not np.any(got[1, no[1]:])
            assert not _same(got[:, :min(no[0], n[0])], base[:, :min(no[0], n[0])])
            for rate in (16000, 48000):
                both = eng.decode(codes, lens, sample_rate=rate, **kw)
                for b in range(2):
                    want = eng.test_resample(hooks[b], rate)
                    assert _same(both[b, :len(want)], want), (pct, cents, rate, b)
                    assert not np.any(both[b, len(want):])
                assert both.shape[1] == len(eng.test_resample(hooks[0], rate))
    finally:
        eng.close()


@pytest.mark.parametrize("pi", range(len(PLANS)))
def test_stream_chunkings_equal_the_hook(pi):
    """A pitched stream's chunks, whatever the chunking (the tail from final=True or from finish()), concatenate bit for
    bit to the hook applied to the same chunks' 44.1 kHz output - and to the resample hook over it when the stream has a
    rate as well.  32 samples per frame: single-frame chunks are shorter than the filter."""
    shape = tiny_codec_shape()
    plan = PLANS[pi]
    eng, _ = make_codec(shape, max_frames=512)
    try:
        codes = _codes(shape, 215, 7)
        x = _native_chunks(eng, codes, plan)
        for pct, cents in ((100, 700), (125, 300), (200, 1200)):
            ps = eng.test_pitch(x, pct, cents)[0]
            assert len(ps) == n_out_of(len(x), pct)
            for rate in (None, 16000, 48000):
                want = ps if rate is None else eng.test_resample(ps, rate)
                st = eng.stream(rate, speed=pct / 100, pitch=cents / 100)
                got, t = [], 0
                for k, T in enumerate(plan):
                    last = k == len(plan) - 1 and pi % 2 == 0
                    got.append(st.decode(codes[:, t:t + T], final=last))
                    t += T
                got.append(st.finish())
                assert st.finished and (pi % 2 or len(got[-1]) == 0)
                st.close()
                assert _same(np.concatenate(got), want), (plan[:4], pct, cents, rate)
    finally:
        eng.close()


def test_mixed_calls_equal_single_stream_calls():
    """One decode_streams call per round over a native stream, a rate-only one, a speed-only one and two pitched ones of
    different cents (one with a speed and a rate), at different positions (staggered starts, different chunk lengths, one
    ending with final=True, one with a tail-only chunk): every stream's samples are, bit for bit, those its own
    single-stream calls give."""
    shape = tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=512)
    try:
        kinds = [(None, None, None), (16000, None, None), (None, 1.25, None), (None, None, 7.0), (48000, 0.8, -5.0)]
        sizes = [1, 7, 20, 3, 33]
        rounds = 6
        plan = [[sizes[(r + j) % 5] for r in range(j % 2, rounds)] for j in range(len(kinds))]
        codes = [_codes(shape, sum(p), 40 + j) for j, p in enumerate(plan)]
        fin_at = {3: len(plan[3]) - 1}                             # final with the last chunk
        streams = [eng.stream(r, speed=v, pitch=p) for r, v, p in kinds]
        got = [[] for _ in kinds]
        pos = [0] * len(kinds)
        for r in range(rounds):
            ids = [j for j in range(len(kinds)) if r >= j % 2]
            chunks, fin = [], []
            for j in ids:
                T = plan[j][r - j % 2]
                chunks.append(codes[j][:, pos[j]:pos[j] + T])
                fin.append(fin_at.get(j) == r - j % 2)
                pos[j] += T
            for j, a in zip(ids, eng.decode_streams([streams[j] for j in ids], chunks, fin)):
                got[j].append(a)
        empty = np.zeros((shape.n_codebooks + 1, 0), np.int32)      # stream 4's tail alone, beside a chunk of stream 0
        tail_call = eng.decode_streams([streams[4], streams[0]], [empty, _codes(shape, 5, 99)], [True, False])
        got[4].append(tail_call[0])
        got[0].append(tail_call[1])
        for j, (rate, v, p) in enumerate(kinds):
            single = eng.stream(rate, speed=v, pitch=p)
            want = [single.decode(codes[j][:, sum(plan[j][:k]):sum(plan[j][:k + 1])], final=fin_at.get(j) == k)
                    for k in range(len(plan[j]))]
            if j == 4:
                want.append(single.finish())
            if j == 0:
                want.append(single.decode(_codes(shape, 5, 99)))
            single.close()
            assert len(got[j]) == len(want), j
            for k, (a, b) in enumerate(zip(got[j], want)):
                assert _same(a, b), (j, k)
            if p is not None:                      # and the whole is the pitch-less length of the stream's input
                total = sum(len(a) for a in got[j])
                n_ts = n_out_of(sum(plan[j]) * eng.frame_len, 100 if v is None else round(v * 100))
                assert total == (n_ts if rate is None else int(eng.lib.ft_resampled_len(rate, n_ts))), j
        for st in streams:
            st.close()
    finally:
        eng.close()


def test_refusals(tiny):
    eng = tiny
    shape = tiny_codec_shape()
    codes = _codes(shape, 40, 5)
    lib = eng.lib
    for bad in (12.01, -12.01, float("nan")):
        with pytest.raises(ValueError):
            eng.stream(pitch=bad)
        with pytest.raises(ValueError):
            eng.decode(codes, pitch=bad)
    for speed, pitch in ((2.0, -1), (0.5, 1)):
        with pytest.raises(ValueError):
            eng.stream(speed=speed, pitch=pitch)
        with pytest.raises(ValueError):
            eng.decode(codes, speed=speed, pitch=pitch)
    # the C ABI itself: bad cents and bad combinations are FT_ERR_ARG
    c = np.ascontiguousarray(codes[:, :10])
    buf = np.zeros(4 * 10 * eng.frame_len, np.float32)
    out = np.zeros(1, np.int64)
    lens = np.array([10], np.int32)
    h = CT.c_void_p()
    res = np.zeros(256, np.float32)
    n = CT.c_int64(0)
    P = CT.c_void_p
    for pct, cents in ((100, 1201), (100, -1201), (200, -100), (50, 100), (49, 100), (201, 1200)):
        assert lib.ft_codec_stream_begin_fxp(eng._h, FI, pct, cents, CT.byref(h)) == 1 and not h
        assert lib.ft_codec_decode_fxp(eng._h, c.ctypes.data_as(P), 1, 10, lens.ctypes.data_as(P), FI, pct, cents,
                                       buf.ctypes.data_as(P), out.ctypes.data_as(P)) == 1
        assert lib.ft_test_pitch(eng._h, buf.ctypes.data_as(P), 64, pct, cents, res.ctypes.data_as(P), CT.byref(n),
                                 None, None, None, None) == 1
    assert lib.ft_codec_stream_begin_fxp(eng._h, 7999, 100, 700, CT.byref(h)) == 1
    # the native-rate entry points refuse a pitched stream, and leave it unchanged
    st = eng.stream(pitch=7)
    assert lib.ft_codec_stream_decode(eng._h, st._h, c.ctypes.data_as(P), 10, buf.ctypes.data_as(P)) == 3
    hs = (CT.c_void_p * 1)(st._h.value)
    assert lib.ft_codec_stream_decode_many(eng._h, 1, hs, c.ctypes.data_as(P), lens.ctypes.data_as(P), buf.ctypes.data_as(P)) == 3
    ref = eng.stream(pitch=7)
    assert _same(st.decode(codes[:, :10], final=True), ref.decode(codes[:, :10], final=True))
    with pytest.raises(Exception):
        st.decode(codes[:, 10:12])                 # a stream whose tail went out takes no further chunk
    assert "final chunk" in lib.ft_last_error(eng._h).decode()
    assert len(st.finish()) == 0
    st.close()
    ref.close()
