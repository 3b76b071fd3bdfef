"""GPU, public API: pitch= on every output path, tiny synthetic models - identity at 0, WAV / PCM of exactly the pitch-less
length that differ from the pitch-less output and equal the engine layer (CodecHipEngine.decode / CodecStream at the pitch)
on the same codes, batch and server streams carrying the stage's tail, seamless=False chunks shifted one by one, header
rate and length with a sample rate and a speed as well, ValueError for a bad pitch or combination before any work."""
import io
import wave

import numpy as np
import pytest

from tests.test_api_serve_gpu import _codes, _tiny_tts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth():
    s = _tiny_tts()
    yield s
    if s._server is not None:
        s._server.close(cancel=True)


def _wav(data):
    with wave.open(io.BytesIO(data), "rb") as wf:
        return wf.getframerate(), np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16)


def _stream_fx(synth, codes, pitch, sizes, rate=None, speed=None):
    """One CodecStream(pitch=) fed `codes` in chunks of `sizes` (cycled), its tail from finish()."""
    st = synth._vocoder.stream(rate, speed=speed, pitch=pitch)
    try:
        out, t, k = [], 0, 0
        while t < codes.shape[1]:
            T = min(sizes[k % len(sizes)], codes.shape[1] - t)
            out.append(st.decode(codes[:, t:t + T]))
            t, k = t + T, k + 1
        out.append(st.finish())
        return (np.concatenate(out) * 32767).astype(np.int16).tobytes()
    finally:
        st.close()


def test_identity_at_zero(synth):
    text, mt = "Hello pitched world", 24
    base = synth.synthesize(text, max_tokens=mt)
    for none in (0, 0.0, None, 0.004):
        assert synth.synthesize_at(text, max_tokens=mt, pitch=none) == base
    texts, seeds = ["One", "the second text"], [3, 4]
    assert synth.synthesize_batch(texts, seeds=seeds, max_tokens=20, pitch=0) == synth.synthesize_batch(texts, seeds=seeds, max_tokens=20)
    a = list(synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=20, chunk_tokens=6, min_first_chunk=3, pitch=0))
    b = list(synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=20, chunk_tokens=6, min_first_chunk=3))
    assert sorted(a) == sorted(b)
    for seamless in (False, True):
        kw = dict(chunk_tokens=5, min_first_chunk=3, max_tokens=mt, seamless=seamless)
        assert list(synth.synthesize_stream(text, pitch=0, **kw)) == list(synth.synthesize_stream(text, **kw))
    with synth.serve(burst=4) as srv:
        assert srv.synthesize(text, seed=2, max_tokens=mt, pitch=0) == srv.synthesize(text, seed=2, max_tokens=mt)
        kw = dict(seamless=True, seed=2, max_tokens=mt, chunk_tokens=5, min_first_chunk=2)
        assert list(srv.synthesize_stream(text, pitch=0, **kw)) == list(srv.synthesize_stream(text, **kw))


def test_other_pitches_and_batch(synth):
    from fish_tts_amd.codec_engine import resampled_len
    text, mt = "Hello pitched world", 24
    rate0, base = _wav(synth.synthesize(text, max_tokens=mt))
    n = len(base)
    codes = _codes(synth, text, 0, mt, None)
    assert rate0 == 44100 and n == codes.shape[1] * synth._vocoder.frame_len
    for pitch in (4, -4):
        rate, pcm = _wav(synth.synthesize_at(text, max_tokens=mt, pitch=pitch))
        assert rate == 44100 and len(pcm) == n and not np.array_equal(pcm, base), pitch
        want = (np.clip(synth._vocoder.decode(codes, pitch=pitch)[0], -1, 1) * 32767).astype(np.int16)
        assert np.array_equal(pcm, want), pitch
        rate, pcm = _wav(synth.synthesize_at(text, max_tokens=mt, pitch=pitch, speed=1.25, sample_rate=16000))
        assert rate == 16000 and len(pcm) == resampled_len(16000, -(-100 * n // 125)), (pitch, len(pcm))
        want = (np.clip(synth._vocoder.decode(codes, sample_rate=16000, speed=1.25, pitch=pitch)[0], -1, 1) * 32767).astype(np.int16)
        assert np.array_equal(pcm, want), pitch
    texts, seeds = ["One", "the second text", "three"], [3, 4, 5]
    plain = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20)
    for pitch in (4, -4):
        shifted = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20, pitch=pitch)
        for i, (a, b) in enumerate(zip(plain, shifted)):
            assert _wav(b)[0] == 44100 and len(_wav(b)[1]) == len(_wav(a)[1]) and a != b
            c = _codes(synth, texts[i], seeds[i], 20, None)
            want = (np.clip(synth._vocoder.decode(c, pitch=pitch)[0], -1, 1) * 32767).astype(np.int16)
            assert np.array_equal(_wav(b)[1], want), (pitch, i)


def test_streams_at_a_pitch(synth):
    texts, seeds, mt = ["batch one", "and batch two is longer"], [7, 8], 40
    for pitch in (4, -4):
        got = {0: [], 1: []}
        for i, pcm in synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=mt, chunk_tokens=6, min_first_chunk=3, pitch=pitch):
            got[i].append(pcm)
        plain = {0: [], 1: []}
        for i, pcm in synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=mt, chunk_tokens=6, min_first_chunk=3):
            plain[i].append(pcm)
        want = {}
        for i, (t, s) in enumerate(zip(texts, seeds)):
            codes = _codes(synth, t, s, mt, None)
            want[i] = _stream_fx(synth, codes, pitch, [1, 9, 4])
            assert got[i][-1] == b"" and got[i].count(b"") == 1
            assert b"".join(got[i]) == want[i], (pitch, i)
            assert len(want[i]) == len(b"".join(plain[i])) and want[i] != b"".join(plain[i])
            assert len(want[i]) // 2 == codes.shape[1] * synth._vocoder.frame_len
        with synth.serve(burst=4) as srv:
            for i, (t, s) in enumerate(zip(texts, seeds)):
                pcm = b"".join(srv.synthesize_stream(t, seamless=True, seed=s, max_tokens=mt, chunk_tokens=5, min_first_chunk=2,
                                                     pitch=pitch))
                assert pcm == want[i], (pitch, i)
            wav = srv.synthesize(texts[0], seed=seeds[0], max_tokens=mt, pitch=pitch)
            both = srv.synthesize(texts[0], seed=seeds[0], max_tokens=mt, pitch=pitch, speed=1.25, sample_rate=16000)
        assert wav == synth.synthesize_batch([texts[0]], seeds=[seeds[0]], max_tokens=mt, pitch=pitch)[0]
        assert both == synth.synthesize_batch([texts[0]], seeds=[seeds[0]], max_tokens=mt, pitch=pitch, speed=1.25, sample_rate=16000)[0]
        assert _wav(both)[0] == 16000


class _Recorder:
    """A CodecStream that notes the codes it is fed."""

    def __init__(self, st, fed):
        self._st, self._fed = st, fed

    def decode(self, codes, *a, **k):
        self._fed.append(np.array(codes))
        return self._st.decode(codes, *a, **k)

    def __getattr__(self, name):
        return getattr(self._st, name)


def test_instance_seamless_stream_carries_one_stage(synth, monkeypatch):
    """The instance's own seamless stream: one carried stage, its tail in a last chunk - the pitched CodecStream of the
    codes it was fed, bit for bit, and as long as the pitch-less stream."""
    text = "A streamed sentence here"
    kw = dict(chunk_tokens=5, min_first_chunk=3, max_tokens=30, seamless=True)
    nat = b"".join(synth.synthesize_stream(text, **kw))
    real = synth._vocoder.stream
    for pitch in (4, -4):
        fed = []
        monkeypatch.setattr(synth._vocoder, "stream", lambda *a, **k: _Recorder(real(*a, **k), fed))
        seam = b"".join(synth.synthesize_stream(text, pitch=pitch, **kw))
        monkeypatch.undo()
        assert len(seam) == len(nat) and seam != nat
        assert seam == _stream_fx(synth, np.concatenate(fed, axis=1), pitch, [3, 5])


def test_zero_state_chunks_are_shifted_one_by_one(synth, monkeypatch):
    text, mt = "A streamed sentence here", 30
    native = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt))
    real = synth._decode_to_pcm
    for pitch in (4, -4):
        seen = []
        monkeypatch.setattr(synth, "_decode_to_pcm", lambda codes, *a, **k: (seen.append(np.array(codes)), real(codes, *a, **k))[1])
        plain = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt, pitch=pitch))
        monkeypatch.undo()
        assert len(plain) == len(native) == len(seen) > 1
        for a, b, codes in zip(plain, native, seen):
            assert len(a) == len(b) and a != b
            assert a == (synth._vocoder.decode(codes, pitch=pitch)[0] * 32767).astype(np.int16).tobytes()


def test_bad_pitches_raise_before_any_work(synth):
    bads = [dict(pitch=p) for p in (12.01, -12.01, "1", True, float("nan"))] + [dict(pitch=-1, speed=2.0), dict(pitch=1, speed=0.5)]
    for bad in bads:
        with pytest.raises(ValueError):
            synth.synthesize_at("x", **bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch(["x"], **bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch_stream(["x"], **bad)
        for seamless in (False, True):
            with pytest.raises(ValueError):
                list(synth.synthesize_stream("x", seamless=seamless, **bad))
    with synth.serve(burst=4) as srv:
        for bad in bads:
            with pytest.raises(ValueError):
                srv.synthesize("x", **bad)
            with pytest.raises(ValueError):
                srv.synthesize_stream("x", seamless=True, **bad)
            with pytest.raises(ValueError):
                srv.submit(None, **bad)
            with pytest.raises(ValueError):
                synth.synthesize_at("x", **bad)          # through the open server
