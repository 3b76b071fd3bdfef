"""GPU, public API: speed= on every output path, tiny synthetic models - identity at 1.0, WAV lengths (alone and with a
sample rate), PCM equal to the engine layer (CodecHipEngine.decode / CodecStream at the speed) on the same codes, batch
and server streams carrying the stage's tail, seamless=False chunks time-scaled one by one, ValueError for a bad speed
before any work."""
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


def _ts_len(n, pct):
    return -(-100 * n // pct)


def _stream_fx(synth, codes, speed, sizes, rate=None):
    """One CodecStream(speed=) fed `codes` in chunks of `sizes` (cycled), its tail from finish()."""
    st = synth._vocoder.stream(rate, speed=speed)
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


def test_identity_at_one(synth):
    text, mt = "Hello paced world", 24
    base = synth.synthesize(text, max_tokens=mt)
    assert synth.synthesize_at(text, max_tokens=mt, speed=1.0) == base
    assert synth.synthesize_at(text, max_tokens=mt, speed=None) == base
    assert synth.synthesize_at(text, max_tokens=mt, speed=1) == base


def test_other_speeds_and_batch(synth):
    from fish_tts_amd.codec_engine import resampled_len
    text, mt = "Hello paced world", 24
    rate0, base = _wav(synth.synthesize(text, max_tokens=mt))
    n = len(base)
    codes = _codes(synth, text, 0, mt, None)
    assert rate0 == 44100 and n == codes.shape[1] * synth._vocoder.frame_len
    for speed, pct in ((0.8, 80), (1.5, 150)):
        rate, pcm = _wav(synth.synthesize_at(text, max_tokens=mt, speed=speed))
        assert rate == 44100 and len(pcm) == _ts_len(n, pct), (speed, len(pcm))
        want = (np.clip(synth._vocoder.decode(codes, speed=speed)[0], -1, 1) * 32767).astype(np.int16)
        assert np.array_equal(pcm, want), speed
        rate, pcm = _wav(synth.synthesize_at(text, max_tokens=mt, speed=speed, sample_rate=16000))
        assert rate == 16000 and len(pcm) == resampled_len(16000, _ts_len(n, pct)), (speed, len(pcm))
    texts, seeds = ["One", "the second text", "three"], [3, 4, 5]
    plain = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20)
    fast = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20, speed=1.25)
    for a, b in zip(plain, fast):
        assert _wav(b)[0] == 44100 and len(_wav(b)[1]) == _ts_len(len(_wav(a)[1]), 125)


def test_streams_at_a_speed(synth):
    texts, seeds, mt = ["batch one", "and batch two is longer"], [7, 8], 40
    got = {0: [], 1: []}
    for i, pcm in synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=mt, chunk_tokens=6, min_first_chunk=3, speed=1.25):
        got[i].append(pcm)
    want = {}
    for i, (t, s) in enumerate(zip(texts, seeds)):
        codes = _codes(synth, t, s, mt, None)
        want[i] = _stream_fx(synth, codes, 1.25, [1, 9, 4])
        assert got[i][-1] == b"" and got[i].count(b"") == 1
        assert b"".join(got[i]) == want[i], i
        assert len(want[i]) // 2 == _ts_len(codes.shape[1] * synth._vocoder.frame_len, 125)
    with synth.serve(burst=4) as srv:
        for i, (t, s) in enumerate(zip(texts, seeds)):
            pcm = b"".join(srv.synthesize_stream(t, seamless=True, seed=s, max_tokens=mt, chunk_tokens=5, min_first_chunk=2,
                                                 speed=1.25))
            assert pcm == want[i], i
        wav = srv.synthesize(texts[0], seed=seeds[0], max_tokens=mt, speed=1.25, sample_rate=16000)
    assert wav == synth.synthesize_batch([texts[0]], seeds=[seeds[0]], max_tokens=mt, speed=1.25, sample_rate=16000)[0]
    # the instance's own seamless stream: one carried stage, its tail in a last chunk
    text = "A streamed sentence here"
    seam = b"".join(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=30, seamless=True, speed=0.8))
    nat = b"".join(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=30, seamless=True))
    assert len(seam) // 2 == _ts_len(len(nat) // 2, 80)


def test_zero_state_chunks_are_scaled_one_by_one(synth):
    text, mt = "A streamed sentence here", 30
    native = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt))
    for speed, pct in ((1.25, 125), (0.8, 80)):
        plain = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt, speed=speed))
        assert len(plain) == len(native) > 1
        for a, b in zip(plain, native):
            assert len(a) // 2 == _ts_len(len(b) // 2, pct)


def test_bad_speeds_raise_before_any_work(synth):
    for bad in (0.49, 2.01, 0, -1, "1", True, float("nan")):
        with pytest.raises(ValueError):
            synth.synthesize_at("x", speed=bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch(["x"], speed=bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch_stream(["x"], speed=bad)
        with pytest.raises(ValueError):
            list(synth.synthesize_stream("x", speed=bad))
    with synth.serve(burst=4) as srv:
        for bad in (0.49, 2.01, 0, -1, "1", True, float("nan")):
            with pytest.raises(ValueError):
                srv.synthesize("x", speed=bad)
            with pytest.raises(ValueError):
                srv.synthesize_stream("x", seamless=True, speed=bad)
            with pytest.raises(ValueError):
                srv.submit(None, speed=bad)
            with pytest.raises(ValueError):
                synth.synthesize_at("x", speed=bad)          # through the open server
