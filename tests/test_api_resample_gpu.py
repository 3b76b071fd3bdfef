"""GPU, public API: sample_rate= on every output path, tiny synthetic models - WAV headers and lengths, PCM equal to the
engine layer (CodecHipEngine.decode / CodecStream at the rate) on the same codes, seamless streams carrying the
resampler's tail, a server with concurrent callers at mixed rates, ValueError for an unsupported rate."""
import io
import threading
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


def _stream_at(synth, codes, rate):
    st = synth._vocoder.stream(rate)
    try:
        return ((st.decode(codes, final=True)) * 32767).astype(np.int16).tobytes()
    finally:
        st.close()


def test_synthesize_at_and_batch(synth):
    from fish_tts_amd.codec_engine import resampled_len
    fl = synth._vocoder.frame_len
    text, mt = "Hello resampled world", 24
    assert synth.synthesize_at(text, max_tokens=mt) == synth.synthesize(text, max_tokens=mt)
    assert synth.synthesize_at(text, max_tokens=mt, sample_rate=44100) == synth.synthesize(text, max_tokens=mt)
    codes = _codes(synth, text, 0, mt, None)
    for rate in (16000, 8000, 48000):
        rate_got, pcm = _wav(synth.synthesize_at(text, max_tokens=mt, sample_rate=rate))
        assert rate_got == rate
        assert len(pcm) == resampled_len(rate, codes.shape[1] * fl)
        want = (np.clip(synth._vocoder.decode(codes, sample_rate=rate)[0], -1, 1) * 32767).astype(np.int16)
        assert np.array_equal(pcm, want), rate
    texts, seeds = ["One", "the second text", "three"], [3, 4, 5]
    wavs = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20, sample_rate=24000)
    for t, s, w in zip(texts, seeds, wavs):
        c = _codes(synth, t, s, 20, None)
        rate_got, pcm = _wav(w)
        assert rate_got == 24000
        assert np.array_equal(pcm, (np.clip(synth._vocoder.decode(c, sample_rate=24000)[0], -1, 1) * 32767).astype(np.int16))


def test_streams_at_a_rate(synth, monkeypatch):
    from fish_tts_amd import codec_engine
    from fish_tts_amd.codec_engine import resampled_len
    text, mt = "A streamed sentence here", 30
    native = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt))
    plain = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt, sample_rate=24000))
    assert len(plain) == len(native) > 1
    for a, b in zip(plain, native):          # every chunk resampled on its own, with its tail
        assert len(a) // 2 == resampled_len(24000, len(b) // 2)
    seen = []
    orig = codec_engine.CodecStream.decode

    def spy(self, codes, final=False):
        seen.append(np.array(codes))
        return orig(self, codes, final)
    monkeypatch.setattr(codec_engine.CodecStream, "decode", spy)
    seam = list(synth.synthesize_stream(text, chunk_tokens=5, min_first_chunk=3, max_tokens=mt, seamless=True,
                                        sample_rate=16000))
    monkeypatch.undo()
    assert len(seam) == len(seen) + 1         # the last chunk: the resampler's tail
    assert b"".join(seam) == _stream_at(synth, np.concatenate(seen, axis=1), 16000)
    # synthesize_batch_stream: each utterance's PCM is one resampled stream of its codes, the tail before (i, b"")
    texts, seeds = ["batch one", "and batch two is longer"], [7, 8]
    got = {0: [], 1: []}
    for i, pcm in synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=24, chunk_tokens=6, min_first_chunk=3,
                                                sample_rate=22050):
        got[i].append(pcm)
    for i, (t, s) in enumerate(zip(texts, seeds)):
        assert got[i][-1] == b"" and got[i].count(b"") == 1
        assert b"".join(got[i]) == _stream_at(synth, _codes(synth, t, s, 24, None), 22050), i


def test_server_mixed_rates_and_bad_rates(synth):
    plan = [("wav", "first caller", 1, 20, 16000), ("seam", "second caller", 2, 26, 24000), ("wav", "third", 3, 18, None),
            ("seam", "fourth one here", 4, 22, None), ("seam", "fifth", 5, 30, 16000), ("wav", "sixth", 6, 16, 48000)]
    want = {}
    for i, (kind, text, seed, mt, rate) in enumerate(plan):
        c = _codes(synth, text, seed, mt, None)
        if kind == "wav":
            want[i] = synth.synthesize_batch([text], seeds=[seed], max_tokens=mt, sample_rate=rate)[0]
        elif rate is None:
            st = synth._vocoder.stream()
            want[i] = (st.decode(c) * 32767).astype(np.int16).tobytes()
            st.close()
        else:
            want[i] = _stream_at(synth, c, rate)
    for bad in (7999, 44099, 0, 48001):
        with pytest.raises(ValueError):
            synth.synthesize_at("x", sample_rate=bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch(["x"], sample_rate=bad)
        with pytest.raises(ValueError):
            list(synth.synthesize_stream("x", sample_rate=bad))
    got, errors = {}, []
    with synth.serve(burst=4) as srv:
        with pytest.raises(ValueError):
            srv.synthesize("x", sample_rate=12345)
        with pytest.raises(ValueError):
            srv.synthesize_stream("x", seamless=True, sample_rate=1)

        def call(i, kind, text, seed, mt, rate):
            try:
                if kind == "wav":
                    got[i] = srv.synthesize(text, seed=seed, max_tokens=mt, sample_rate=rate)
                else:
                    got[i] = b"".join(srv.synthesize_stream(text, seamless=True, seed=seed, max_tokens=mt,
                                                            chunk_tokens=5, min_first_chunk=3, sample_rate=rate))
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=call, args=(i,) + p) for i, p in enumerate(plan)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
    assert not errors, errors
    for i, (kind, _, _, _, rate) in enumerate(plan):
        assert got[i] == want[i], (i, kind, rate)
        if kind == "wav":
            assert _wav(got[i])[0] == (rate or 44100)
