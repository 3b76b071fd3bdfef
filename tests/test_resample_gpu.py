"""GPU: the resampler behind sample_rate= (resample_kernel) - through the test hook against tones and the float64
restatement of tests/test_resample_host.py; ft_codec_decode_at against the restatement of ft_codec_decode's waveform;
resampled streams (ft_codec_stream_decode_many_at) bit for bit against the hook on their own 44.1 kHz output, alone and
mixed with streams of other rates in one call; the codec's own rate unchanged; refusals."""
import ctypes as CT

import numpy as np
import pytest
import torch

from oracle import codec as C
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec
from tests.test_resample_host import RATES, filter_table, resample_ref

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


def test_hook_tones_and_restatement(tiny):
    eng = tiny
    n = 40000
    x = np.sin(2 * np.pi * 1000 * np.arange(n) / FI).astype(np.float32)
    noise = np.random.default_rng(0).uniform(-1, 1, 12345).astype(np.float32)
    for rate in RATES:
        L, M, K, w = tab = filter_table(rate)
        y = eng.test_resample(x, rate)
        assert len(y) == -(-n * L // M)
        edge = (K * L) // M + 4
        want = np.sin(2 * np.pi * 1000 * np.arange(len(y)) / rate)
        err = np.max(np.abs(y[edge:-edge] - want[edge:-edge]))
        assert err <= 1e-3, (rate, err)
        assert np.max(np.abs(y - resample_ref(x, rate, tab))) <= 2e-5, rate
        z = eng.test_resample(noise, rate)
        assert np.max(np.abs(z - resample_ref(noise, rate, tab))) <= 2e-5, rate
        if rate < FI:               # a tone at 0.6 Fo (in the stop band) is gone
            t = np.sin(2 * np.pi * 0.6 * rate * np.arange(n) / FI).astype(np.float32)
            s = eng.test_resample(t, rate)[edge:-edge]
            att = -20 * np.log10(np.sqrt(np.mean(s.astype(np.float64) ** 2)) / np.sqrt(0.5))
            assert att >= 70, (rate, att)
    assert _same(eng.test_resample(noise, FI), noise)


@pytest.mark.parametrize("real", [False, True])
def test_one_shot_decode_at(real):
    """ft_codec_decode_at = the restatement applied to ft_codec_decode's waveform (2e-5), exact lengths, zeros past the
    end of a shorter utterance; None and 44100 are ft_codec_decode byte for byte."""
    shape = C.CodecShape() if real else tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=256)
    try:
        codes = np.stack([_codes(shape, 215, 1), _codes(shape, 215, 2)])
        lens = np.array([215, 90], dtype=np.int32)
        fl = eng.frame_len
        base = eng.decode(codes, lens)
        assert _same(eng.decode(codes, lens, sample_rate=None), base)
        assert _same(eng.decode(codes, lens, sample_rate=FI), base)
        for rate in ((8000, 16000, 24000, 48000) if real else RATES):
            L, M, K, w = tab = filter_table(rate)
            got = eng.decode(codes, lens, sample_rate=rate)
            n0, n1 = (-(-int(T) * fl * L // M) for T in lens)
            assert got.shape == (2, n0), (rate, got.shape)
            if rate == 16000 and real:
                assert n0 == 159754
            assert np.max(np.abs(got[0] - resample_ref(base[0], rate, tab))) <= 2e-5, rate
            assert np.max(np.abs(got[1, :n1] - resample_ref(base[1, :90 * fl], rate, tab))) <= 2e-5, rate
            assert not np.any(got[1, n1:])
    finally:
        eng.close()


@pytest.mark.parametrize("real", [False, True])
def test_stream_chunkings_equal_the_hook(real):
    """A resampled stream's chunks, whatever the chunking (the tail from final=True or from finish()), concatenate bit
    for bit to the hook applied to the same chunks' 44.1 kHz output."""
    shape = C.CodecShape() if real else tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=256)
    try:
        codes = _codes(shape, 215, 7)
        plans = [[215], [20] * 10 + [15], [1, 3, 7, 20] * 6 + [29], [1] * 15 + [200]]
        for pi, plan in enumerate(plans):
            nat = eng.stream()
            pieces, t = [], 0
            for T in plan:
                pieces.append(nat.decode(codes[:, t:t + T]))
                t += T
            nat.close()
            x = np.concatenate(pieces)
            for rate in (16000, 48000, 11025):
                want = eng.test_resample(x, rate)
                st = eng.stream(rate)
                got, t = [], 0
                for k, T in enumerate(plan):
                    last = k == len(plan) - 1 and pi % 2 == 0
                    got.append(st.decode(codes[:, t:t + T], final=last))
                    t += T
                got.append(st.finish())
                assert st.finished and (pi % 2 or len(got[-1]) == 0)
                st.close()
                assert _same(np.concatenate(got), want), (plan[:4], rate)
    finally:
        eng.close()


@pytest.mark.parametrize("real", [False, True])
def test_mixed_rate_calls_equal_single_stream_calls(real):
    """One decode_streams call per round over 44.1, 16, 24 and 48 kHz streams at different positions (staggered starts,
    different chunk lengths, some ending with final=True, one with a tail-only chunk): every stream's samples are, bit
    for bit, those its own single-stream calls give."""
    shape = C.CodecShape() if real else tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=512)
    try:
        rates = [None, 16000, 24000, 48000, 16000, None]
        sizes = [1, 7, 20, 3, 33]
        rounds = 5
        plan = [[sizes[(r + j) % 5] for r in range(j % 2, rounds)] for j in range(len(rates))]
        codes = [_codes(shape, sum(p), 30 + j) for j, p in enumerate(plan)]
        fin_at = {1: len(plan[1]) - 1, 3: len(plan[3]) - 1}        # final with the last chunk
        streams = [eng.stream(r) for r in rates]
        got = [[] for _ in rates]
        pos = [0] * len(rates)
        for r in range(rounds):
            ids = [j for j in range(len(rates)) if r >= j % 2]
            chunks, fin = [], []
            for j in ids:
                T = plan[j][r - j % 2]
                chunks.append(codes[j][:, pos[j]:pos[j] + T])
                fin.append(fin_at.get(j) == r - j % 2)
                pos[j] += T
            for j, a in zip(ids, eng.decode_streams([streams[j] for j in ids], chunks, fin)):
                got[j].append(a)
        # stream 2's tail alone, in a call with a chunk of stream 4
        tail_call = eng.decode_streams([streams[2], streams[4]], [np.zeros((shape.n_codebooks + 1, 0), np.int32),
                                                                  _codes(shape, 5, 99)], [True, False])
        got[2].append(tail_call[0])
        got[4].append(tail_call[1])
        for j, rate in enumerate(rates):
            single = eng.stream(rate)
            want = [single.decode(codes[j][:, sum(plan[j][:k]):sum(plan[j][:k + 1])], final=fin_at.get(j) == k)
                    for k in range(len(plan[j]))]
            if j == 2:
                want.append(single.finish())
            if j == 4:
                want.append(single.decode(_codes(shape, 5, 99)))
            single.close()
            assert len(got[j]) == len(want), j
            for k, (a, b) in enumerate(zip(got[j], want)):
                assert _same(a, b), (j, k)
        for st in streams:
            st.close()
    finally:
        eng.close()


def test_native_rate_unchanged_and_refusals(tiny):
    eng = tiny
    shape = tiny_codec_shape()
    codes = _codes(shape, 40, 5)
    a, b = eng.stream(), eng.stream(FI)
    assert b.rate is None
    x = [a.decode(codes[:, :13]), a.decode(codes[:, 13:])]
    y = eng.decode_streams([b], [codes[:, :13]], [True]) + [b.decode(codes[:, 13:], final=True)]
    assert all(_same(p, q) for p, q in zip(x, y)) and len(b.finish()) == 0
    a.close()
    b.close()
    with pytest.raises(ValueError):
        eng.stream(7999)
    with pytest.raises(ValueError):
        eng.decode(codes, sample_rate=44099)
    lib = eng.lib
    st = eng.stream(16000)
    c = np.ascontiguousarray(codes[:, :10])
    buf = np.zeros(10 * eng.frame_len, np.float32)
    # the native-rate entry points refuse a resampled stream, and leave it unchanged
    assert lib.ft_codec_stream_decode(eng._h, st._h, c.ctypes.data_as(CT.c_void_p), 10, buf.ctypes.data_as(CT.c_void_p)) == 3
    h = (CT.c_void_p * 1)(st._h.value)
    lens = np.array([10], np.int32)
    assert lib.ft_codec_stream_decode_many(eng._h, 1, h, c.ctypes.data_as(CT.c_void_p), lens.ctypes.data_as(CT.c_void_p),
                                           buf.ctypes.data_as(CT.c_void_p)) == 3
    out = np.zeros(1, np.int64)
    zero = np.array([0], np.int32)
    # a chunk of 0 frames without final
    assert lib.ft_codec_stream_decode_many_at(eng._h, 1, h, c.ctypes.data_as(CT.c_void_p), zero.ctypes.data_as(CT.c_void_p),
                                              None, buf.ctypes.data_as(CT.c_void_p), out.ctypes.data_as(CT.c_void_p)) == 1
    res = np.zeros(64, np.float32)
    n = CT.c_int64(0)
    assert lib.ft_test_resample(eng._h, buf.ctypes.data_as(CT.c_void_p), 64, 48001, res.ctypes.data_as(CT.c_void_p),
                                CT.byref(n)) == 1
    ref = eng.stream(16000)
    assert _same(st.decode(codes[:, :10], final=True), ref.decode(codes[:, :10], final=True))
    with pytest.raises(Exception):
        st.decode(codes[:, 10:12])                 # a stream whose tail went out takes no further chunk
    st.close()
    ref.close()
