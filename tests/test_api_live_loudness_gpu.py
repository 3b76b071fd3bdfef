"""GPU, public API: live_loudness= on the three streaming calls, tiny synthetic models.  The instance's own seamless stream
gives the same bytes at two chunk_tokens values, and they are the ride stage (CodecHipEngine.ride) over the un-levelled
stream of the codes it was fed; synthesize_batch_stream and BatchServer.synthesize_stream give, for one seed, the same bytes
as each other: the ride over the un-levelled stream of that seed's codes (those two decode Utterance.codes(), the
instance's own stream every generated column - which is why each is held against the ride of its own codes, as the other
stages' tests do).  The result differs from the un-levelled stream, its sample peak is at most -1 dBFS within one int16
step, and loudness= is still refused on all three.

The synthetic codec emits full-scale noise and decodes 96 frames of 32 samples at most - less than one hop at any rate - so
no measure completes and what acts here is the stage's peak guard and its emission at the end of a stream; the measure
itself is tests/test_ride_gpu.py's."""
import numpy as np
import pytest

from tests.test_api_pitch_gpu import _Recorder
from tests.test_api_serve_gpu import _codes, _tiny_tts

pytestmark = pytest.mark.gpu

TARGET = -20.0
TEXT = "A streamed sentence here"
CEILING = 10.0 ** (-1.0 / 20.0)


@pytest.fixture(scope="module")
def synth():
    s = _tiny_tts()
    yield s
    if s._server is not None:
        s._server.close(cancel=True)


def _pcm(audio):
    return (audio * 32767).astype(np.int16).tobytes()


def _plain(synth, codes, **kw):
    """The un-levelled streamed decode of `codes`, float32."""
    st = synth._vocoder.stream(**kw)
    try:
        return np.concatenate([st.decode(codes), st.finish()])
    finally:
        st.close()


def _peak_ok(pcm):
    return np.max(np.abs(np.frombuffer(pcm, dtype=np.int16).astype(np.int64))) <= int(CEILING * 32767) + 1


def test_instance_stream_rides_whatever_the_chunking(synth, monkeypatch):
    real = synth._vocoder.stream
    for kw in (dict(), dict(sample_rate=16000, speed=1.25, pitch=3)):
        got = []
        for chunk_tokens in (5, 8):
            fed = []
            monkeypatch.setattr(synth._vocoder, "stream", lambda *a, **k: _Recorder(real(*a, **k), fed))
            got.append(b"".join(synth.synthesize_stream(TEXT, chunk_tokens=chunk_tokens, min_first_chunk=3, max_tokens=30,
                                                        seamless=True, live_loudness=TARGET, **kw)))
            monkeypatch.undo()
        assert got[0] == got[1] and got[0]
        codes = np.concatenate(fed, axis=1)
        bare = _plain(synth, codes, **kw)
        print(kw, "peak of the un-levelled stream", float(np.max(np.abs(bare))), "samples", len(bare))
        assert got[0] == _pcm(synth._vocoder.ride(bare, kw.get("sample_rate"), TARGET)), kw
        assert got[0] != _pcm(bare) and len(got[0]) == 2 * len(bare), kw
        assert _peak_ok(got[0]) and not _peak_ok(_pcm(bare)), kw
        plain = b"".join(synth.synthesize_stream(TEXT, chunk_tokens=5, min_first_chunk=3, max_tokens=30, seamless=True, **kw))
        assert plain == _pcm(bare), kw


def test_batch_stream_and_server_give_the_same_bytes(synth):
    texts, seeds, mt = ["batch one", "and batch two is longer"], [7, 8], 40
    kw = dict(sample_rate=16000)
    got = {0: [], 1: []}
    for i, pcm in synth.synthesize_batch_stream(texts, seeds=seeds, max_tokens=mt, chunk_tokens=6, min_first_chunk=3,
                                                live_loudness=TARGET, **kw):
        got[i].append(pcm)
    want = {}
    for i, (t, s) in enumerate(zip(texts, seeds)):
        bare = _plain(synth, _codes(synth, t, s, mt, None), **kw)
        print(i, "peak of the un-levelled stream", float(np.max(np.abs(bare))), "samples", len(bare))
        want[i] = _pcm(synth._vocoder.ride(bare, 16000, TARGET))
        assert got[i][-1] == b"" and got[i].count(b"") == 1
        assert b"".join(got[i]) == want[i] != _pcm(bare), i
        assert _peak_ok(want[i]) and len(want[i]) == 2 * len(bare), i
    with synth.serve(burst=4) as srv:
        for i, (t, s) in enumerate(zip(texts, seeds)):
            for chunk_tokens in (5, 9):
                pcm = b"".join(srv.synthesize_stream(t, seamless=True, seed=s, max_tokens=mt, chunk_tokens=chunk_tokens,
                                                     min_first_chunk=2, live_loudness=TARGET, **kw))
                assert pcm == want[i], (i, chunk_tokens)
        # through the open server, the instance's call joins the batch and gives the server's bytes
        assert b"".join(synth.synthesize_stream(texts[0], seamless=True, seed=seeds[0], max_tokens=mt, live_loudness=TARGET, **kw)) == want[0]
        with pytest.raises(ValueError, match="loudness needs the whole utterance"):
            srv.synthesize_stream(texts[0], seamless=True, loudness=TARGET)
        with pytest.raises(ValueError, match="seamless=True"):
            srv.synthesize_stream(texts[0], live_loudness=TARGET)
        with pytest.raises(ValueError, match="not both"):
            srv.synthesize_stream(texts[0], seamless=True, loudness=TARGET, live_loudness=TARGET)


def test_loudness_is_still_refused_and_bad_targets_raise(synth, monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth, "_get_prompt_data", no_work)
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        synth.synthesize_batch_stream(["x", "y"], loudness=TARGET)
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        next(synth.synthesize_stream("x", seamless=True, loudness=TARGET))
    with pytest.raises(ValueError, match="seamless=True"):
        next(synth.synthesize_stream("x", live_loudness=TARGET))
    for bad in (-51, -4.9, 0, "loud", True, float("nan")):
        with pytest.raises(ValueError):
            synth.synthesize_batch_stream(["x"], live_loudness=bad)
        with pytest.raises(ValueError):
            next(synth.synthesize_stream("x", seamless=True, live_loudness=bad))
    with pytest.raises(TypeError):
        synth.synthesize_at("x", live_loudness=TARGET)          # the one-shot calls have loudness=
    with pytest.raises(ValueError, match="rides a stream"):
        from fish_tts_amd.codec_engine import OutputFx
        synth._vocoder.decode(np.zeros((10, 4), dtype=np.int32), fx=OutputFx.of(live_loudness=TARGET))
