"""GPU: the time-scale stage behind speed= (timescale_kernel) - through the test hook against the float64 restatement of
tests/test_timescale_host.py (samples given the kernel's alignments; every alignment within the float32 summation bound
of the best one; exact ties); ft_codec_decode_fx against the restatement of ft_codec_decode's waveform, alone and with a
sample rate; time-scaled streams (ft_codec_stream_decode_many_at) bit for bit against the hook on their own 44.1 kHz
output whatever the chunking, alone and mixed with other streams in one call; the path without speed unchanged;
refusals."""
import ctypes as CT

import numpy as np
import pytest
import torch

from oracle import codec as C
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec
from tests.test_timescale_host import D, HS, N, PCTS, frame_scores, impulse_train, n_frames_of, n_out_of, timescale_ref

pytestmark = pytest.mark.gpu

FI = 44100


def _codes(shape, T, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.zeros(shape.n_codebooks + 1, T, dtype=torch.long)
    codes[0] = torch.randint(0, shape.semantic_codebook_size, (T,), generator=g)
    codes[1:] = torch.randint(0, shape.codebook_size, (shape.n_codebooks, T), generator=g)
    return codes.numpy().astype(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


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


def _check_hook(x, pct, y, d, what):
    assert len(y) == n_out_of(len(x), pct), what                                   # (d)
    assert len(d) == n_frames_of(len(x), pct) and d[0] == 0 and np.all(np.abs(d) <= D), what
    err = np.max(np.abs(y - timescale_ref(x, pct, deltas=d)))
    print(what, "max |y - ref| =", err)
    assert err <= 1e-6, (what, err)                                                # (a)
    for k, (c, cabs) in enumerate(frame_scores(x, pct, d), start=1):               # (b)
        slack = 2 * N * 2.0 ** -24 * cabs.max()
        assert c[d[k] + D] >= c.max() - slack, (what, k, c[d[k] + D], c.max(), slack)


@pytest.mark.parametrize("pct", PCTS)
def test_hook_against_restatement(tiny, inputs, pct):
    for name, x in inputs.items():
        y, d = tiny.test_timescale(x, pct)
        _check_hook(x, pct, y, d, (name, pct))
    x = impulse_train(6880)                                                        # (c)
    y, d = tiny.test_timescale(x, pct)
    want, dref = timescale_ref(x, pct, return_deltas=True)
    assert np.array_equal(d, dref), pct
    assert len(y) == len(want) and np.max(np.abs(y - want)) <= 1e-6


@pytest.mark.parametrize("real", [False, True])
def test_one_shot_decode_at_speed(real):
    """decode(speed=) = the restatement applied to decode()'s rows with the alignments the hook reports for that row
    (1e-6), exact lengths, zeros past the end of a shorter item; None and 1.0 are decode() bit for bit; with a sample rate
    as well it is the resample hook over the time-scale hook, bit for bit."""
    shape = C.CodecShape() if real else tiny_codec_shape()
    T = 60 if real else 215
    eng, _ = make_codec(shape, max_frames=256 if real else 512)     # the resample hook takes the half-speed waveform
    try:
        codes = np.stack([_codes(shape, T, 1), _codes(shape, T, 2)])
        lens = np.array([T, T // 3], dtype=np.int32)
        fl = eng.frame_len
        base = eng.decode(codes, lens)
        assert _same(eng.decode(codes, lens, speed=None), base)
        assert _same(eng.decode(codes, lens, speed=1.0), base)
        assert _same(eng.decode(codes, lens, speed=1), base)
        for pct in ((50, 125, 200) if real else PCTS):
            got = eng.decode(codes, lens, speed=pct / 100)
            n = [int(t) * fl for t in lens]
            no = [n_out_of(v, pct) for v in n]
            assert got.shape == (2, no[0]), (pct, got.shape)
            hooks = []
            for b in range(2):
                y, d = eng.test_timescale(base[b, :n[b]], pct)
                hooks.append(y)
                err = np.max(np.abs(got[b, :no[b]] - timescale_ref(base[b, :n[b]], pct, deltas=d)))
                print("decode", real, pct, b, "max |y - ref| =", err)
                assert err <= 1e-6, (pct, b, err)
                assert _same(got[b, :no[b]], y), (pct, b)
            assert not np.any(got[1, no[1]:])
            for rate in (16000, 48000):
                both = eng.decode(codes, lens, sample_rate=rate, speed=pct / 100)
                for b in range(2):
                    want = eng.test_resample(hooks[b], rate)
                    assert _same(both[b, :len(want)], want), (pct, rate, b)
                    assert not np.any(both[b, len(want):])
                assert both.shape[1] == len(eng.test_resample(hooks[0], rate))
    finally:
        eng.close()


PLANS = ([215], [20] * 10 + [15], [1, 3, 7, 20] * 6 + [29], [1] * 15 + [200])


def _native_chunks(eng, codes, plan):
    nat = eng.stream()
    pieces, t = [], 0
    for T in plan:
        pieces.append(nat.decode(codes[:, t:t + T]))
        t += T
    nat.close()
    return np.concatenate(pieces)


@pytest.mark.parametrize("pi", range(len(PLANS)))
def test_stream_chunkings_equal_the_hook(pi):
    """A time-scaled stream's chunks, whatever the chunking (the tail from final=True or from finish()), concatenate
    bit for bit to the hook applied to the same chunks' 44.1 kHz output - and to the resample hook over it when the
    stream has a rate as well.  32 samples per frame: single-frame chunks are far shorter than a hop."""
    shape = tiny_codec_shape()
    plan = PLANS[pi]
    eng, _ = make_codec(shape, max_frames=512)                      # the resample hook takes the half-speed waveform
    try:
        codes = _codes(shape, 215, 7)
        x = _native_chunks(eng, codes, plan)
        for pct in (50, 125, 200):
            ts = eng.test_timescale(x, pct)[0]
            for rate in (None, 16000, 48000):
                want = ts if rate is None else eng.test_resample(ts, rate)
                st = eng.stream(rate, speed=pct / 100)
                got, t = [], 0
                for k, T in enumerate(plan):
                    last = k == len(plan) - 1 and pi % 2 == 0
                    got.append(st.decode(codes[:, t:t + T], final=last))
                    t += T
                got.append(st.finish())
                assert st.finished and (pi % 2 or len(got[-1]) == 0)
                st.close()
                assert _same(np.concatenate(got), want), (plan[:4], pct, rate)
    finally:
        eng.close()


def test_stream_real_shape_equals_the_hook():
    shape = C.CodecShape()
    eng, _ = make_codec(shape, max_frames=256)
    try:
        codes = _codes(shape, 60, 7)
        plan = [1, 20, 7, 32]
        x = _native_chunks(eng, codes, plan)
        for pct, rate in ((50, None), (125, 16000), (200, 48000)):
            ts = eng.test_timescale(x, pct)[0]
            want = ts if rate is None else eng.test_resample(ts, rate)
            st = eng.stream(rate, speed=pct / 100)
            got, t = [], 0
            for T in plan:
                got.append(st.decode(codes[:, t:t + T]))
                t += T
            got.append(st.finish())
            st.close()
            assert _same(np.concatenate(got), want), (pct, rate)
    finally:
        eng.close()


def test_mixed_calls_equal_single_stream_calls():
    """One decode_streams call per round over streams of different speeds and rates, some plain, at different positions
    (staggered starts, different chunk lengths, some ending with final=True, one with a tail-only chunk): every stream's
    samples are, bit for bit, those its own single-stream calls give."""
    shape = tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=512)
    try:
        kinds = [(None, None), (None, 0.5), (16000, 1.25), (48000, 2.0), (16000, None), (None, 1.25), (None, None)]
        sizes = [1, 7, 20, 3, 33]
        rounds = 6
        plan = [[sizes[(r + j) % 5] for r in range(j % 2, rounds)] for j in range(len(kinds))]
        codes = [_codes(shape, sum(p), 30 + j) for j, p in enumerate(plan)]
        fin_at = {1: len(plan[1]) - 1, 3: len(plan[3]) - 1}        # final with the last chunk
        streams = [eng.stream(r, speed=v) for r, v in kinds]
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
        # stream 2's and 5's tails alone, in a call with a chunk of stream 4
        empty = np.zeros((shape.n_codebooks + 1, 0), np.int32)
        tail_call = eng.decode_streams([streams[2], streams[4], streams[5]], [empty, _codes(shape, 5, 99), empty],
                                       [True, False, True])
        got[2].append(tail_call[0])
        got[4].append(tail_call[1])
        got[5].append(tail_call[2])
        for j, (rate, v) in enumerate(kinds):
            single = eng.stream(rate, speed=v)
            want = [single.decode(codes[j][:, sum(plan[j][:k]):sum(plan[j][:k + 1])], final=fin_at.get(j) == k)
                    for k in range(len(plan[j]))]
            if j in (2, 5):
                want.append(single.finish())
            if j == 4:
                want.append(single.decode(_codes(shape, 5, 99)))
            single.close()
            assert len(got[j]) == len(want), j
            for k, (a, b) in enumerate(zip(got[j], want)):
                assert _same(a, b), (j, k)
            if v is not None:                      # and the whole is the time-scaled length of the stream's input
                total = sum(len(a) for a in got[j])
                n_ts = n_out_of(sum(plan[j]) * eng.frame_len, round(v * 100))
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
    for bad in (0.49, 2.01):
        with pytest.raises(ValueError):
            eng.stream(speed=bad)
        with pytest.raises(ValueError):
            eng.decode(codes, speed=bad)
    # the C ABI itself: 49 and 201 percent are FT_ERR_ARG
    c = np.ascontiguousarray(codes[:, :10])
    buf = np.zeros(4 * 10 * eng.frame_len, np.float32)
    out = np.zeros(1, np.int64)
    lens = np.array([10], np.int32)
    h = CT.c_void_p()
    res = np.zeros(256, np.float32)
    n, k = CT.c_int64(0), CT.c_int32(0)
    for pct in (49, 201):
        assert lib.ft_codec_stream_begin_fx(eng._h, FI, pct, CT.byref(h)) == 1
        assert lib.ft_codec_decode_fx(eng._h, c.ctypes.data_as(CT.c_void_p), 1, 10, lens.ctypes.data_as(CT.c_void_p), FI, pct,
                                      buf.ctypes.data_as(CT.c_void_p), out.ctypes.data_as(CT.c_void_p)) == 1
        assert lib.ft_test_timescale(eng._h, buf.ctypes.data_as(CT.c_void_p), 64, pct, res.ctypes.data_as(CT.c_void_p),
                                     CT.byref(n), None, CT.byref(k)) == 1
    assert lib.ft_codec_stream_begin_fx(eng._h, 7999, 125, CT.byref(h)) == 1
    # the native-rate entry points refuse a time-scaled stream, and leave it unchanged
    st = eng.stream(speed=1.25)
    assert lib.ft_codec_stream_decode(eng._h, st._h, c.ctypes.data_as(CT.c_void_p), 10, buf.ctypes.data_as(CT.c_void_p)) == 3
    hs = (CT.c_void_p * 1)(st._h.value)
    assert lib.ft_codec_stream_decode_many(eng._h, 1, hs, c.ctypes.data_as(CT.c_void_p), lens.ctypes.data_as(CT.c_void_p),
                                           buf.ctypes.data_as(CT.c_void_p)) == 3
    ref = eng.stream(speed=1.25)
    assert _same(st.decode(codes[:, :10], final=True), ref.decode(codes[:, :10], final=True))
    with pytest.raises(Exception):
        st.decode(codes[:, 10:12])                 # a stream whose tail went out takes no further chunk
    assert len(st.finish()) == 0
    st.close()
    ref.close()
