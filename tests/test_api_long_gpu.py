"""GPU, public API: FishTTS.synthesize_long / synthesize_long_stream on tiny synthetic models - the WAV equals the numpy
restatement of the join (tests/join_ref.py) over CodecHipEngine.decode of every segment's codes, without trimming, with a
silence threshold that trims, and at another rate and speed; one voice throughout without references, the user's prefix
cache untouched; a single sentence equals synthesize_batch; the stream's chunks concatenate to the WAV's samples; both
calls through an open BatchServer give the same bytes; every bad argument raises ValueError on every entry point.

Cuts that move.  The synthetic codec emits full-scale noise (peaks 0.997 to 0.99996, more than half of the samples at or
above 0.501), and a segment of max_tokens=20 is 19 frames x 32 = 608 samples, shorter than the 30 ms = 1323 samples kept
around the loud part: at silence_db=-6 and max_tokens=20 no seed can move a cut (seeds 0 to 15 were tried: every cut is
(0, 608)), so that case compares the faded and joined PCM only.  The case that asserts a moved cut therefore uses
segments longer than twice the kept margin (max_tokens=90: 2848 samples, four native calls of the join) and thresholds just
under the noise's peaks (silence_db=-0.01 and -0.002: 0.99885 and 0.99977), with the seed picked so that cuts move at the
front, at the back, and one segment is dropped whole."""
import io
import wave

import numpy as np
import pytest

from tests import join_ref as J
from tests.test_api_serve_gpu import _codes, _tiny_tts

pytestmark = pytest.mark.gpu

TEXT = ("The first sentence is right here. And the second one follows it.\r\n\r\n"
        "A new paragraph begins with this.  It ends\nwith one more sentence.")
SEGMENTS = [("The first sentence is right here.", False), ("And the second one follows it.", False),
            ("A new paragraph begins with this.", True), ("It ends with one more sentence.", False)]
SEED, MT = 11, 20
TRIM_DB = -6.0            # far above the default: the synthetic codec's noise is trimmed


@pytest.fixture(scope="module")
def synth():
    s = _tiny_tts()
    yield s
    if s._server is not None:
        s._server.close(cancel=True)


@pytest.fixture(scope="module")
def voice():
    import fish_tts_amd as ft
    rng = np.random.default_rng(0)
    ref = np.concatenate([rng.integers(0, 2048, (1, 40)), rng.integers(0, 1024, (9, 40))]).astype(np.int32)
    return [ft.VoiceProfile(codes=ref, text="the reference text", name="v")]


@pytest.fixture(scope="module")
def voiced_codes(synth, voice):
    """The codes of every segment of TEXT with the reference voice: single runs, computed once."""
    return [_codes(synth, seg, SEED + i, MT, voice) for i, (seg, _) in enumerate(SEGMENTS)]


def _wav(data):
    with wave.open(io.BytesIO(data), "rb") as wf:
        assert wf.getnchannels() == 1 and wf.getsampwidth() == 2
        return wf.getframerate(), wf.readframes(wf.getnframes())


def _pcm(audio):
    return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()


def _want(synth, codes, silence_db, rate=None, speed=None, pause=0.2, paragraph_pause=0.5):
    """join_ref over the engine's decode of every segment: (PCM bytes, cuts, the segments' lengths)."""
    from fish_tts_amd.longform import join_params
    jp, gap, pgap = join_params(rate, pause, paragraph_pause, silence_db)
    rows = [synth._vocoder.decode(c, sample_rate=rate, speed=speed)[0] for c in codes]
    gaps = [pgap if par else gap for _, par in SEGMENTS[:len(codes)]]
    audio, cuts, _ = J.join(rows, jp.threshold, jp.hop, jp.keep, jp.fade, gaps, 0)
    return _pcm(audio), cuts, [len(r) for r in rows]


def test_the_text_splits_as_expected():
    from fish_tts_amd.longform import split_text
    assert [tuple(s) for s in split_text(TEXT)] == [(t, bool(p)) for t, p in SEGMENTS]


def test_long_equals_the_join_of_the_segments(synth, voice, voiced_codes):
    kw = dict(references=voice, max_tokens=MT, seed=SEED)
    rate, pcm = _wav(synth.synthesize_long(TEXT, silence_db=None, **kw))
    want, cuts, lens = _want(synth, voiced_codes, None)
    assert rate == 44100 and pcm == want
    assert cuts.tolist() == [[0, n] for n in lens]
    assert len(pcm) // 2 == sum(lens) + 8820 + 22050 + 8820          # 0.2 s, 0.5 s at the paragraph break, 0.2 s
    # a threshold that trims
    rate, pcm = _wav(synth.synthesize_long(TEXT, silence_db=TRIM_DB, **kw))
    want, cuts, lens = _want(synth, voiced_codes, TRIM_DB)
    print("cuts at", TRIM_DB, "dB:", cuts.tolist(), "of", lens)
    assert any(e > a for a, e in cuts.tolist()), "everything was trimmed away: pick another seed"
    assert rate == 44100 and pcm == want
    # other pauses
    rate, pcm = _wav(synth.synthesize_long(TEXT, silence_db=TRIM_DB, pause=0, paragraph_pause=0.013, **kw))
    assert pcm == _want(synth, voiced_codes, TRIM_DB, pause=0, paragraph_pause=0.013)[0]


LONG_SEED, LONG_MT = 8, 90


def test_a_threshold_that_moves_cuts(synth, voice):
    """Segments longer than twice the kept margin, thresholds just under the noise peaks (module docstring)."""
    codes = [_codes(synth, seg, LONG_SEED + i, LONG_MT, voice) for i, (seg, _) in enumerate(SEGMENTS)]
    assert sum(c.shape[1] for c in codes) > synth._vocoder.max_frames          # more than one native call
    kw = dict(references=voice, max_tokens=LONG_MT, seed=LONG_SEED)
    seen = set()
    for db in (-0.01, -0.002):
        rate, pcm = _wav(synth.synthesize_long(TEXT, silence_db=db, **kw))
        want, cuts, lens = _want(synth, codes, db)
        print("cuts at", db, "dB:", cuts.tolist(), "of", lens)
        assert any(e > a for a, e in cuts.tolist()), "everything was trimmed away: pick another seed"
        assert any((a > 0 or e < n) for (a, e), n in zip(cuts.tolist(), lens)), "no cut moved: pick another seed"
        assert rate == 44100 and pcm == want, db
        assert b"".join(synth.synthesize_long_stream(TEXT, silence_db=db, **kw)) == pcm, db
        for (a, e), n in zip(cuts.tolist(), lens):
            seen |= {"front"} if a > 0 else set()
            seen |= {"back"} if 0 < e < n else set()
            seen |= {"dropped"} if e == a else set()
    assert seen == {"front", "back", "dropped"}, seen


def test_long_at_a_rate_and_speed(synth, voice, voiced_codes):
    kw = dict(references=voice, max_tokens=MT, seed=SEED, sample_rate=16000, speed=1.25)
    for db in (None, TRIM_DB):
        rate, pcm = _wav(synth.synthesize_long(TEXT, silence_db=db, **kw))
        want, cuts, lens = _want(synth, voiced_codes, db, 16000, 1.25)
        assert rate == 16000 and pcm == want, db
    assert len(_wav(synth.synthesize_long(TEXT, silence_db=None, pitch=3, **kw))[1]) == len(_want(synth, voiced_codes, None, 16000, 1.25)[0])


def test_one_voice_without_references(synth):
    import fish_tts_amd as ft
    assert synth.num_references == 0
    first = _codes(synth, SEGMENTS[0][0], SEED, MT, None)
    assert first.shape[1] > 0
    made = [ft.VoiceProfile(codes=first, text=SEGMENTS[0][0])]
    codes = [first] + [_codes(synth, seg, SEED + i, MT, made) for i, (seg, _) in enumerate(SEGMENTS) if i]
    before = len(synth._prefix_cache)
    keys = list(synth._prefix_cache._entries)
    wav = synth.synthesize_long(TEXT, max_tokens=MT, seed=SEED, silence_db=None)
    assert len(synth._prefix_cache) == before and list(synth._prefix_cache._entries) == keys
    assert _wav(wav)[1] == _want(synth, codes, None)[0]
    assert b"".join(synth.synthesize_long_stream(TEXT, max_tokens=MT, seed=SEED, silence_db=None)) == _wav(wav)[1]
    assert len(synth._prefix_cache) == before
    with synth.serve(burst=4):
        assert synth.synthesize_long(TEXT, max_tokens=MT, seed=SEED, silence_db=None) == wav
        assert b"".join(synth.synthesize_long_stream(TEXT, max_tokens=MT, seed=SEED, silence_db=None)) == _wav(wav)[1]
        assert len(synth._prefix_cache) == before
    assert len(synth._prefix_cache) == before


def test_single_sentence_equals_synthesize_batch(synth, voice):
    text = "Just one short sentence."
    for refs in (None, voice):
        assert synth.synthesize_long(text, references=refs, max_tokens=24, seed=5, silence_db=None) == \
            synth.synthesize_batch([text], references=refs, seeds=[5], max_tokens=24)[0]
    assert synth.synthesize_long(text, max_tokens=24, seed=5, silence_db=None, sample_rate=16000, speed=0.8, pitch=-2) == \
        synth.synthesize_batch([text], seeds=[5], max_tokens=24, sample_rate=16000, speed=0.8, pitch=-2)[0]


def test_stream_equals_the_wav(synth, voice):
    for kw in (dict(silence_db=None), dict(silence_db=TRIM_DB), dict(silence_db=TRIM_DB, sample_rate=16000, speed=1.25)):
        kw.update(references=voice, max_tokens=MT, seed=SEED)
        chunks = list(synth.synthesize_long_stream(TEXT, **kw))
        assert chunks and all(len(c) > 0 for c in chunks)
        assert b"".join(chunks) == _wav(synth.synthesize_long(TEXT, **kw))[1], kw
    gen = synth.synthesize_long_stream(TEXT, references=voice, max_tokens=MT, seed=SEED)
    assert next(gen)
    gen.close()                                    # abandoned: generation stops and lets go of the engine
    assert synth._gen_lock.acquire(timeout=60)
    synth._gen_lock.release()


def test_through_an_open_server(synth, voice, voiced_codes):
    kws = [dict(silence_db=None), dict(silence_db=TRIM_DB, sample_rate=16000, speed=1.25)]
    for kw in kws:
        kw.update(references=voice, max_tokens=MT, seed=SEED)
    want = [synth.synthesize_long(TEXT, **kw) for kw in kws]
    with synth.serve(burst=4) as srv:
        for kw, w in zip(kws, want):
            assert synth.synthesize_long(TEXT, **kw) == w
            chunks = list(synth.synthesize_long_stream(TEXT, **kw))
            assert all(len(c) > 0 for c in chunks) and b"".join(chunks) == _wav(w)[1]
        assert srv.stats()["completed"] >= 4 * len(SEGMENTS)
        req = srv.submit_codes(SEGMENTS[0][0], voice, max_tokens=MT, seed=SEED)
        assert np.array_equal(srv.take_codes(req), voiced_codes[0])
    assert synth.synthesize_long(TEXT, **kws[0]) == want[0]          # the instance serves itself again


BAD = [dict(pause=-0.1), dict(pause=5.1), dict(pause=float("nan")), dict(pause="1"), dict(paragraph_pause=-1),
       dict(paragraph_pause=5.5), dict(paragraph_pause=None), dict(silence_db=0.5), dict(silence_db=-91), dict(silence_db="x"),
       dict(max_chars=15), dict(max_chars=1001), dict(min_chars=-1), dict(min_chars=201), dict(sample_rate=12345),
       dict(speed=2.5), dict(pitch=12.5), dict(pitch=-1, speed=2.0)]


def test_bad_arguments_raise_before_any_work(synth):
    def both():
        for bad in BAD:
            with pytest.raises(ValueError):
                synth.synthesize_long("Some text.", **bad)
            with pytest.raises(ValueError):
                list(synth.synthesize_long_stream("Some text.", **bad))
        for empty in ("", " \n\r\n "):
            with pytest.raises(ValueError, match="No text to synthesize"):
                synth.synthesize_long(empty)
            with pytest.raises(ValueError, match="No text to synthesize"):
                list(synth.synthesize_long_stream(empty))
    both()
    with synth.serve(burst=4):
        both()


def test_new_symbols_resolve(synth):
    lib = synth._vocoder.lib
    for name in ("ft_codec_decode_join", "ft_test_join"):
        assert getattr(lib, name) is not None
