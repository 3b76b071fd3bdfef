"""GPU, public API: FishTTS.synthesize_script / synthesize_script_stream on tiny synthetic models (a codec frame of 32
samples, max_tokens=20).  A script of one plain Line is synthesize_long; a four-line script in two voices and the default -
one slow line, one pitched, one at its own loudness, one behind an explicit pause - equals the numpy restatement of the join
(tests/join_ref.py) over CodecHipEngine.decode of every segment's codes through that segment's own chain, the codes being
those of single runs in the line's voice with seed + i; the stream's chunks concatenate to the WAV's samples with the same
marks; without trimming the marks are the cumulative sums of lengths and gaps; the SSML form of the script gives the same
bytes; so does an open BatchServer; every bad argument raises ValueError before any work.  All comparisons are equalities."""
import io
import wave

import numpy as np
import pytest

from tests import join_ref as J
from tests.test_api_serve_gpu import _codes, _tiny_tts

pytestmark = pytest.mark.gpu

TEXT = ("The first sentence is right here. And the second one follows it.\r\n\r\n"
        "A new paragraph begins with this.  It ends\nwith one more sentence.")
SEED, MT = 11, 20
TRIM_DB = -6.0            # far above the default: the synthetic codec's full-scale noise is trimmed, and a line levelled
                          # to -20 LUFS (peaks near 0.1) is dropped whole - its mark is then an empty span
LEVELLED_DB = -30.0       # with every line levelled to -23 LUFS: a threshold below the levelled peaks


def _voice(seed, name):
    import fish_tts_amd as ft
    rng = np.random.default_rng(seed)
    ref = np.concatenate([rng.integers(0, 2048, (1, 40)), rng.integers(0, 1024, (9, 40))]).astype(np.int32)
    return [ft.VoiceProfile(codes=ref, text=f"the reference text of {name}", name=name)]


@pytest.fixture(scope="module")
def synth():
    s = _tiny_tts()
    yield s
    if s._server is not None:
        s._server.close(cancel=True)


@pytest.fixture(scope="module")
def voices():
    return {"anna": _voice(1, "anna"), "ben": _voice(2, "ben")}


@pytest.fixture(scope="module")
def default():
    return _voice(0, "v")


def _script():
    from fish_tts_amd import Line
    return [Line("This line is spoken slowly by Anna.", voice="anna", speed=0.8),
            Line("Ben answers at a higher pitch. He takes two sentences for it.", voice="ben", pitch=2),
            Line("The narrator stands at a level of his own.", loudness=-20.0),
            Line("And Anna closes after a pause.", voice="anna", pause=1.0)]


SSML = ('<speak><voice name="anna"><prosody rate="80%">This line is spoken slowly by Anna.</prosody></voice>'
        '<voice name="ben"><prosody pitch="+2st">Ben answers at a higher pitch. He takes two sentences for it.</prosody></voice>'
        'The narrator stands at a level of his own.'
        '<break time="1s"/><voice name="anna">And Anna closes after a pause.</voice></speak>')


def _wav(data):
    with wave.open(io.BytesIO(data), "rb") as wf:
        assert wf.getnchannels() == 1 and wf.getsampwidth() == 2
        return wf.getframerate(), wf.readframes(wf.getnframes())


def _pcm(audio):
    return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()


@pytest.fixture(scope="module")
def expected(synth, voices, default):
    """The script's plan and every segment's codes - single runs in the line's voice, seed + i - computed once."""
    from fish_tts_amd.script import plan_script

    def plan(**kw):
        return plan_script(_script(), voices, **kw)
    p = plan()
    assert p.line_of == [0, 1, 1, 2, 3] and p.voices == ["anna", "ben", "ben", None, "anna"]
    codes = [_codes(synth, t, SEED + i, MT, default if v is None else voices[v]) for i, (t, v) in enumerate(zip(p.texts, p.voices))]
    assert all(c.shape[1] > 0 for c in codes)
    return plan, codes


def _want(synth, plan, codes):
    """join_ref over the engine's decode of every segment through its own chain: (PCM, cuts, lengths)."""
    rows = [synth._vocoder.decode(c, fx=f)[0] for c, f in zip(codes, plan.fx)]
    audio, cuts, _ = J.join(rows, plan.jp.threshold, plan.jp.hop, plan.jp.keep, plan.jp.fade, plan.gaps, 0)
    return _pcm(audio), cuts, [len(r) for r in rows]


def test_one_plain_line_is_synthesize_long(synth, default):
    from fish_tts_amd import Line
    for kw in (dict(), dict(loudness=-18.0, sample_rate=16000), dict(silence_db=TRIM_DB, pause=0.1, paragraph_pause=0.3, speed=1.25)):
        kw.update(references=default, max_tokens=MT, seed=SEED)
        assert synth.synthesize_script([Line(TEXT)], **kw) == synth.synthesize_long(TEXT, **kw), kw
    # without any reference voice the rule of synthesize_long holds: the first segment is the voice of the others
    assert synth.num_references == 0
    kw = dict(max_tokens=MT, seed=SEED, silence_db=None)
    keys = list(synth._prefix_cache._entries)
    assert synth.synthesize_script([Line(TEXT)], **kw) == synth.synthesize_long(TEXT, **kw)
    assert list(synth._prefix_cache._entries) == keys


def test_the_script_equals_the_join_of_its_segments(synth, voices, default, expected):
    plan, codes = expected
    for kw in (dict(silence_db=None), dict(silence_db=TRIM_DB), dict(silence_db=LEVELLED_DB, sample_rate=16000, loudness=-23.0, speed=1.25)):
        p = plan(**kw)
        want, cuts, lens = _want(synth, p, codes)
        marks = []
        rate, pcm = _wav(synth.synthesize_script(_script(), voices, default, max_tokens=MT, seed=SEED, marks=marks, **kw))
        assert rate == p.rate and pcm == want, kw
        assert len(marks) == 4 and marks[-1][1] == len(pcm) // 2 and marks[0][0] == 0
        assert all(a <= e for a, e in marks) and all(marks[j][1] <= marks[j + 1][0] for j in range(3))
    # the chains differ from line to line: the slow line is longer than its codes at the model's pace, the levelled one moved
    p = plan(silence_db=None)
    assert [(f.pct, f.cents, f.level) for f in p.fx] == [(80, None, None), (None, 200, None), (None, 200, None), (None, None, -2000),
                                                         (None, None, None)]
    lens = _want(synth, p, codes)[2]
    assert lens[0] == -(-100 * codes[0].shape[1] * 32 // 80) and lens[1] == codes[1].shape[1] * 32


def test_marks_without_trimming_are_sums_of_lengths_and_gaps(synth, voices, default, expected):
    plan, codes = expected
    p = plan(silence_db=None, line_pause=0.3)
    lens = _want(synth, p, codes)[2]
    marks = []
    synth.synthesize_script(_script(), voices, default, max_tokens=MT, seed=SEED, silence_db=None, line_pause=0.3, marks=marks)
    g = p.gaps
    assert g[1:] == [13230, 8820, 13230, 44100]
    ends = np.cumsum([n + (gap if i else 0) for i, (n, gap) in enumerate(zip(lens, g))]).tolist()
    assert marks == [(0, ends[0]), (ends[0] + g[1], ends[2]), (ends[2] + g[3], ends[3]), (ends[3] + g[4], ends[4])]


def test_the_stream_equals_the_wav_and_its_marks(synth, voices, default):
    for kw in (dict(silence_db=None), dict(silence_db=TRIM_DB), dict(silence_db=LEVELLED_DB, sample_rate=16000, loudness=-23.0)):
        kw.update(voices=voices, references=default, max_tokens=MT, seed=SEED)
        m_wav, m_stream = [], []
        pcm = _wav(synth.synthesize_script(_script(), marks=m_wav, **kw))[1]
        chunks = list(synth.synthesize_script_stream(_script(), marks=m_stream, **kw))
        assert chunks and all(len(c) > 0 for c in chunks)
        assert b"".join(chunks) == pcm, kw
        assert m_stream == m_wav and len(m_wav) == 4
    gen = synth.synthesize_script_stream(_script(), voices, default, max_tokens=MT, seed=SEED)
    assert next(gen)
    gen.close()                                    # abandoned: generation stops and lets go of the engine
    assert synth._gen_lock.acquire(timeout=60)
    synth._gen_lock.release()


def test_the_ssml_form_gives_the_same_bytes(synth, voices, default):
    from fish_tts_amd import parse_ssml
    assert parse_ssml(SSML) == [ln._replace(loudness=None) for ln in _script()]
    kw = dict(voices=voices, references=default, max_tokens=MT, seed=SEED, silence_db=TRIM_DB)
    lines = [ln._replace(loudness=None) for ln in _script()]
    assert synth.synthesize_script(SSML, **kw) == synth.synthesize_script(lines, **kw)
    assert b"".join(synth.synthesize_script_stream(SSML, **kw)) == _wav(synth.synthesize_script(lines, **kw))[1]


def test_lines_without_a_voice_and_without_references(synth, voices):
    """The lines in the call's voice follow synthesize_long's rule among themselves; the named voice is untouched by it."""
    import fish_tts_amd as ft
    from fish_tts_amd import Line
    from fish_tts_amd.script import plan_script
    lines = [Line("Anna opens the piece with this.", voice="anna"), Line("Nobody in particular goes on."),
             Line("And the same nobody ends it.", pitch=-1)]
    p = plan_script(lines, voices, silence_db=None)
    assert p.voices == ["anna", None, None] and synth.num_references == 0
    first = _codes(synth, p.texts[1], SEED + 1, MT, None)
    made = [ft.VoiceProfile(codes=first, text=p.texts[1])]
    codes = [_codes(synth, p.texts[0], SEED, MT, voices["anna"]), first, _codes(synth, p.texts[2], SEED + 2, MT, made)]
    keys = set(synth._prefix_cache._entries)            # (anna's prefix is in the cache by now; a hit renews its place)
    wav = synth.synthesize_script(lines, voices, max_tokens=MT, seed=SEED, silence_db=None)
    assert _wav(wav)[1] == _want(synth, p, codes)[0]
    assert b"".join(synth.synthesize_script_stream(lines, voices, max_tokens=MT, seed=SEED, silence_db=None)) == _wav(wav)[1]
    assert set(synth._prefix_cache._entries) == keys
    with synth.serve(burst=4):
        assert synth.synthesize_script(lines, voices, max_tokens=MT, seed=SEED, silence_db=None) == wav
    assert set(synth._prefix_cache._entries) == keys


def test_through_an_open_server(synth, voices, default):
    kws = [dict(silence_db=None), dict(silence_db=LEVELLED_DB, sample_rate=16000, loudness=-23.0)]
    for kw in kws:
        kw.update(voices=voices, references=default, max_tokens=MT, seed=SEED)
    want, want_marks = [], []
    for kw in kws:
        want_marks.append([])
        want.append(synth.synthesize_script(_script(), marks=want_marks[-1], **kw))
    with synth.serve(burst=4) as srv:
        for kw, w, wm in zip(kws, want, want_marks):
            m1, m2 = [], []
            assert synth.synthesize_script(_script(), marks=m1, **kw) == w
            chunks = list(synth.synthesize_script_stream(_script(), marks=m2, **kw))
            assert all(len(c) > 0 for c in chunks) and b"".join(chunks) == _wav(w)[1]
            assert m1 == wm and m2 == wm
        assert srv.stats()["completed"] >= 4 * 5
    assert synth.synthesize_script(_script(), **kws[0]) == want[0]          # the instance serves itself again


def test_bad_arguments_raise_before_any_work(synth, voices, default, monkeypatch):
    from fish_tts_amd import Line
    t = "Some text is here."

    def no_work(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    bad_calls = [dict(line_pause=-0.1), dict(line_pause=5.5), dict(line_pause="1"), dict(pause=-0.1), dict(paragraph_pause=None),
                 dict(silence_db=0.5), dict(max_chars=15), dict(min_chars=-1), dict(sample_rate=12345), dict(speed=2.5),
                 dict(pitch=12.5), dict(pitch=-1, speed=2.0), dict(loudness=-4), dict(marks=()), dict(voices=["anna"])]
    bad_scripts = [[], "<speak> </speak>", "<speak><emphasis>x</emphasis></speak>", [Line(t, voice="carl")], [Line(t), Line(t, speed=3)],
                   [Line(t, pitch=-13)], [Line(t, speed=2.0, pitch=-1)], [Line(t, loudness=-3)], [Line(t, volume=2)],
                   [Line(t, loudness=-6, volume=2)], [Line(t, pause=6)], [Line(" ")], [t], None]
    nine = {f"v{i}": _voice(10 + i, f"v{i}") for i in range(9)}
    crowd = [Line(t, voice=f"v{i}") for i in range(9)]

    def every():
        for bad in bad_calls:
            kw = dict(voices=voices)
            kw.update(bad)
            with pytest.raises(ValueError):
                synth.synthesize_script([Line(t)], **kw)
            with pytest.raises(ValueError):
                synth.synthesize_script_stream([Line(t)], **kw)          # checked at the call, not at the first next()
        for bad in bad_scripts:
            with pytest.raises(ValueError):
                synth.synthesize_script(bad, voices)
            with pytest.raises(ValueError):
                synth.synthesize_script_stream(bad, voices)
        # nine voices: one more than the reference cache holds (eight named ones and the call's own are nine too)
        with pytest.raises(ValueError, match="9 voices"):
            synth.synthesize_script(crowd, nine)
        with pytest.raises(ValueError, match="9 voices"):
            synth.synthesize_script_stream(crowd[:8] + [Line(t)], nine, default)

    keys = list(synth._prefix_cache._entries)
    handles = [synth._prefix_cache._entries[k].handle for k in keys]
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth._vocoder, "decode_join", no_work)
    every()
    with synth.serve(burst=4) as srv:
        monkeypatch.setattr(srv, "submit_codes", no_work)
        every()
    assert list(synth._prefix_cache._entries) == keys
    assert [synth._prefix_cache._entries[k].handle for k in keys] == handles
    assert synth._gen_lock.acquire(timeout=5)
    synth._gen_lock.release()
    monkeypatch.undo()
    # eight voices are taken - the limit is the cache's capacity - and nine without a cache would be too
    assert synth._prefix_cache.capacity == 8
    synth._script_plan(crowd[:8], nine, None, 0.2, 0.5, 0.4, -45.0, 200, 24, None, None, None, None, None)
    cache, synth._prefix_cache = synth._prefix_cache, None
    try:
        synth._script_plan(crowd, nine, None, 0.2, 0.5, 0.4, -45.0, 200, 24, None, None, None, None, None)
    finally:
        synth._prefix_cache = cache
