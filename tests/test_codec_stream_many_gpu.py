"""GPU: ft_codec_stream_decode_many / CodecHipEngine.decode_streams - one chunk of each of several streams in one pass
through the codec - against the single-stream decode (ft_codec_stream_decode), bit for bit."""
import ctypes as CT

import numpy as np
import pytest
import torch

from oracle import codec as C
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec

pytestmark = pytest.mark.gpu


def _codes(shape, T, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.zeros(shape.n_codebooks + 1, T, dtype=torch.long)
    codes[0] = torch.randint(0, shape.semantic_codebook_size, (T,), generator=g)
    codes[1:] = torch.randint(0, shape.codebook_size, (shape.n_codebooks, T), generator=g)
    return codes.numpy().astype(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_batched_streams_equal_their_single_stream_decodes():
    """Real widths, 8 streams with staggered starts (fresh, fewer than window - 1 carried rows, a full carry - in one
    call), every call mixing chunks of 1, 7, 20, 64 and 130 frames (shorter than a convolution's halo, longer than the
    window) until t0 passes 127: every stream equals its own single-stream decode of the same chunks and the one-chunk
    decode of all its codes, bit for bit; one stream alone (n = 1) equals ft_codec_stream_decode."""
    shape = C.CodecShape()
    eng, _ = make_codec(shape, max_frames=512)
    sizes = [1, 7, 20, 64, 130]
    n, rounds = 8, 6
    plan = [[sizes[(r + j) % 5] for r in range(rounds) if r >= j % 3] for j in range(n)]   # stream j starts at round j % 3
    codes = [_codes(shape, sum(p), 100 + j) for j, p in enumerate(plan)]
    streams = [eng.stream() for _ in range(n)]
    got = [[] for _ in range(n)]
    pos = [0] * n
    for r in range(rounds):
        ids = [j for j in range(n) if r >= j % 3]
        chunks = []
        for j in ids:
            T = plan[j][r - j % 3]
            chunks.append(codes[j][:, pos[j]:pos[j] + T])
            pos[j] += T
        for j, a in zip(ids, eng.decode_streams([streams[j] for j in ids], chunks)):
            got[j].append(a)
    assert all(st.frames == sum(p) for st, p in zip(streams, plan)) and max(pos) > 127
    for j in range(n):
        single, t = eng.stream(), 0
        want = []
        for T in plan[j]:
            want.append(single.decode(codes[j][:, t:t + T]))
            t += T
        single.close()
        whole = eng.stream()
        one = whole.decode(codes[j])
        whole.close()
        g = np.concatenate(got[j])
        assert _same(g, np.concatenate(want)), (j, int(np.argmax(g != np.concatenate(want))) // eng.frame_len)
        assert _same(g, one), j
    # n = 1
    a, b = eng.stream(), eng.stream()
    c = _codes(shape, 30, 7)
    for lo, hi in ((0, 13), (13, 30)):
        assert _same(eng.decode_streams([a], [c[:, lo:hi]])[0], b.decode(c[:, lo:hi]))
    assert eng.decode_streams([], []) == []
    for st in streams + [a, b]:
        st.close()
    eng.close()


def test_batched_streams_tiny_32_streams():
    """Tiny widths (other kernel variants, two decoder blocks): 32 streams x 3 rounds of 20 frames."""
    shape = tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=704)
    n = 32
    codes = [_codes(shape, 60, j) for j in range(n)]
    streams = [eng.stream() for _ in range(n)]
    got = [[] for _ in range(n)]
    for r in range(3):
        for j, a in enumerate(eng.decode_streams(streams, [c[:, 20 * r:20 * r + 20] for c in codes])):
            got[j].append(a)
    for j in range(n):
        single = eng.stream()
        want = np.concatenate([single.decode(codes[j][:, 20 * r:20 * r + 20]) for r in range(3)])
        single.close()
        assert _same(np.concatenate(got[j]), want), j
    for st in streams:
        st.close()
    eng.close()


def test_batched_stream_refusals_change_nothing():
    """Every refused call returns its code before any device work: the good calls after it give what they give without
    it, and no stream has moved."""
    from fish_tts_amd import _lib as L
    shape = tiny_codec_shape()
    eng, _ = make_codec(shape, max_frames=64)
    other, _ = make_codec(shape, seed=1)
    R = shape.n_codebooks + 1
    codes = _codes(shape, 40, 11)
    lib = eng.lib

    def run(refusals):
        sa, sb = eng.stream(), eng.stream()
        out = eng.decode_streams([sa, sb], [codes[:, :5], codes[:, 5:9]])
        for streams, lens, want in refusals(sa, sb):
            h = (CT.c_void_p * max(len(streams), 1))(*[s.value if isinstance(s, CT.c_void_p) else s._h.value for s in streams])
            flat = np.zeros(R * max(sum(max(x, 0) for x in lens), 1), dtype=np.int32)
            la = np.array(lens if lens else [1], dtype=np.int32)
            audio = np.empty(flat.size * eng.frame_len, dtype=np.float32)
            rc = lib.ft_codec_stream_decode_many(eng._h, len(streams), h, flat.ctypes.data_as(CT.c_void_p),
                                                 la.ctypes.data_as(CT.c_void_p), audio.ctypes.data_as(CT.c_void_p))
            assert rc == want, (lens, rc, lib.ft_last_error(eng._h))
            assert (sa.frames, sb.frames) == (5, 4)
        out += eng.decode_streams([sb, sa], [codes[:, 9:16], codes[:, 16:17]])
        sa.close()
        sb.close()
        return out

    # a stream of a destroyed context
    dead = other.stream()
    handle = dead._h
    other._streams.discard(dead)
    other.close()
    dead._h = CT.c_void_p()
    foreign_eng, _ = make_codec(shape, seed=2)
    foreign = foreign_eng.stream()

    def refusals(sa, sb):
        yield [], [], L.FT_ERR_ARG                                         # n = 0
        yield [sa, sb], [3, 0], L.FT_ERR_ARG                               # a chunk of no frames
        yield [sa, sa], [2, 2], L.FT_ERR_ARG                               # a stream named twice
        yield [sa, foreign], [2, 2], L.FT_ERR_STATE                        # another context's stream
        yield [sb, handle], [2, 2], L.FT_ERR_STATE                         # a destroyed context's stream
        yield [sa, sb], [2, 61], L.FT_ERR_TOO_LONG                         # t0 + lens > max_frames
        yield [sa] + [eng.stream() for _ in range(64)], [1] * 65, L.FT_ERR_TOO_LONG   # n > 64
    plain = run(lambda sa, sb: iter(()))
    refused = run(refusals)
    assert len(plain) == len(refused) == 4 and all(_same(x, y) for x, y in zip(plain, refused))
    # sum(lens) > max_frames, each stream within its own limit
    ss = [eng.stream() for _ in range(3)]
    with pytest.raises(Exception, match="max_frames together"):
        lib_ok = eng.lib.ft_codec_stream_decode_many
        flat = np.zeros(R * 66, dtype=np.int32)
        la = np.array([22, 22, 22], dtype=np.int32)
        audio = np.empty(66 * eng.frame_len, dtype=np.float32)
        h = (CT.c_void_p * 3)(*[s._h.value for s in ss])
        eng._check(lib_ok(eng._h, 3, h, flat.ctypes.data_as(CT.c_void_p), la.ctypes.data_as(CT.c_void_p),
                          audio.ctypes.data_as(CT.c_void_p)), "ft_codec_stream_decode_many")
    # ... which decode_streams splits over two calls instead
    outs = eng.decode_streams(ss, [codes[:, :22]] * 3)
    assert [s.frames for s in ss] == [22, 22, 22]
    single = eng.stream()
    assert all(_same(o, single.decode(codes[:, :22])) if k == 0 else _same(o, outs[0]) for k, o in enumerate(outs))
    # decode_streams refuses another engine's stream with the native message
    with pytest.raises(Exception, match="another"):
        eng.decode_streams([single, foreign], [codes[:, :2], codes[:, :2]])
    assert single.frames == 22
    L.load().ft_codec_stream_end(None, handle)
    foreign_eng.close()
    eng.close()
