"""GPU, public API: loudness= on every output path that has the whole utterance, tiny synthetic models - the WAV equals the
engine layer's levelled decode of the same codes and measures at the target, None is byte for byte the call without it,
synthesize_long levels every segment before the join and its stream's chunks concatenate to it, a BatchServer gives the
direct call's bytes, and every streaming call refuses a loudness before any work.

The target.  The synthetic codec emits full-scale noise (about -4 LUFS, peaks near 1.0), so at -20 LUFS the gain is well
below 1 and the -1 dBFS ceiling cannot bind: the target of the issue is used as it stands, and the tests assert that no
item's info reports the ceiling."""
import io
import math
import wave

import numpy as np
import pytest

from tests.test_api_serve_gpu import _codes, _tiny_tts

pytestmark = pytest.mark.gpu

TARGET = -20.0
TEXT = ("The first sentence is right here. And the second one follows it.\r\n\r\n"
        "A new paragraph begins with this.  It ends\nwith one more sentence.")
SEGMENTS = [("The first sentence is right here.", False), ("And the second one follows it.", False),
            ("A new paragraph begins with this.", True), ("It ends with one more sentence.", False)]
SEED, MT = 11, 20


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


def _wav(data):
    with wave.open(io.BytesIO(data), "rb") as wf:
        assert wf.getnchannels() == 1 and wf.getsampwidth() == 2
        return wf.getframerate(), wf.readframes(wf.getnframes())


def _pcm(audio):
    return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()


def _levelled(synth, codes, **kw):
    """(PCM of the engine's levelled decode of `codes`, its LevelInfo)."""
    levels = []
    audio = synth._vocoder.decode(codes, loudness=TARGET, levels=levels, **kw)[0]
    return _pcm(audio), levels[0]


def test_synthesize_at_a_loudness(synth):
    text, mt = "Hello levelled world", 24
    base = synth.synthesize(text, max_tokens=mt)
    assert synth.synthesize_at(text, max_tokens=mt, loudness=None) == base
    before = synth.measure_loudness(base)
    codes = _codes(synth, text, 0, mt, None)
    for kw in (dict(), dict(sample_rate=16000, speed=1.25, pitch=3)):
        wav = synth.synthesize_at(text, max_tokens=mt, loudness=TARGET, **kw)
        want, info = _levelled(synth, codes, **kw)
        rate, pcm = _wav(wav)
        assert rate == kw.get("sample_rate", 44100) and pcm == want, kw
        assert pcm != _wav(synth.synthesize_at(text, max_tokens=mt, **kw))[1]
        got = synth.measure_loudness(wav)
        print(f"{kw}: {before:.3f} LUFS before, {info.lufs:.3f} in the stage, gain {info.gain:.4f}, {got:.3f} LUFS after")
        assert not info.capped and math.isfinite(info.lufs), info
        assert abs(got - TARGET) <= 0.1, (kw, got)
    assert abs(before - TARGET) > 1.0          # the stage had something to do


def test_batch_at_a_loudness(synth):
    texts, seeds = ["One", "the second text", "three"], [3, 4, 5]
    plain = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20)
    assert synth.synthesize_batch(texts, seeds=seeds, max_tokens=20, loudness=None) == plain
    levelled = synth.synthesize_batch(texts, seeds=seeds, max_tokens=20, loudness=TARGET)
    for i, (a, b) in enumerate(zip(plain, levelled)):
        want, info = _levelled(synth, _codes(synth, texts[i], seeds[i], 20, None))
        assert _wav(b)[1] == want and a != b and len(a) == len(b), i
        assert not info.capped and abs(synth.measure_loudness(b) - TARGET) <= 0.1, i


def test_long_levels_every_segment_before_the_join(synth, voice):
    from fish_tts_amd.longform import join_params
    kw = dict(references=voice, max_tokens=MT, seed=SEED)
    codes = [_codes(synth, seg, SEED + i, MT, voice) for i, (seg, _) in enumerate(SEGMENTS)]
    for db, extra in ((None, dict()), (-24.0, dict()), (-24.0, dict(sample_rate=16000, speed=1.25))):
        plain = synth.synthesize_long(TEXT, silence_db=db, **kw, **extra)
        assert synth.synthesize_long(TEXT, silence_db=db, loudness=None, **kw, **extra) == plain
        rate, pcm = _wav(synth.synthesize_long(TEXT, silence_db=db, loudness=TARGET, **kw, **extra))
        jp, gap, pgap = join_params(extra.get("sample_rate"), 0.2, 0.5, db)
        levels = []
        rows = [synth._vocoder.decode(c, loudness=TARGET, levels=levels, **extra)[0] for c in codes]
        gaps = [pgap if par else gap for _, par in SEGMENTS]
        y, total, cuts = synth._vocoder.test_join(rows, tuple(jp), gaps)
        assert rate == extra.get("sample_rate", 44100) and pcm == _pcm(y[:total]), (db, extra)
        assert pcm != _wav(plain)[1] and not any(i.capped for i in levels)
        if db is not None:
            # the levelled noise peaks near -16 dBFS: a threshold of -24 dBFS, judged on the levelled samples, finds it loud
            assert any(e > a for a, e in cuts.tolist())
        chunks = list(synth.synthesize_long_stream(TEXT, silence_db=db, loudness=TARGET, **kw, **extra))
        assert b"".join(chunks) == pcm and all(chunks), (db, extra)
        assert b"".join(synth.synthesize_long_stream(TEXT, silence_db=db, loudness=None, **kw, **extra)) == _wav(plain)[1]


def test_server_gives_the_direct_bytes(synth, voice):
    text, mt = "batch one", 24
    direct = synth.synthesize_batch([text], seeds=[7], max_tokens=mt, loudness=TARGET)[0]
    long_direct = synth.synthesize_long(TEXT, references=voice, max_tokens=MT, seed=SEED, silence_db=-24.0, loudness=TARGET)
    with synth.serve(burst=4) as srv:
        assert srv.synthesize(text, seed=7, max_tokens=mt, loudness=TARGET) == direct
        assert srv.synthesize(text, seed=7, max_tokens=mt, loudness=None) == srv.synthesize(text, seed=7, max_tokens=mt)
        assert synth.synthesize_long(TEXT, references=voice, max_tokens=MT, seed=SEED, silence_db=-24.0, loudness=TARGET) == long_direct
        assert abs(synth.measure_loudness(direct) - TARGET) <= 0.1           # (under the server's codec lock)
        with pytest.raises(ValueError, match="loudness needs the whole utterance"):
            srv.synthesize_stream(text, seamless=True, loudness=TARGET)
        with pytest.raises(ValueError, match="loudness needs the whole utterance"):
            srv.synthesize_stream(text, loudness=TARGET)
        with pytest.raises(ValueError, match="loudness needs the whole utterance"):
            next(synth.synthesize_stream(text, loudness=TARGET))                 # through the open server
        for bad in (-51, -4.9, 0, True, float("nan")):
            with pytest.raises(ValueError):
                srv.synthesize(text, loudness=bad)
    assert direct != synth.synthesize_batch([text], seeds=[7], max_tokens=mt)[0]


def test_streaming_calls_refuse_a_loudness(synth, monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work was started")
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth, "_get_prompt_data", no_work)
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        synth.synthesize_batch_stream(["x", "y"], loudness=TARGET)                # at the call
    for seamless in (False, True):
        gen = synth.synthesize_stream("x", seamless=seamless, loudness=TARGET)
        with pytest.raises(ValueError, match="loudness needs the whole utterance"):
            next(gen)                                                             # at the first next(), as its other checks
    for bad in (-51, -4.9, 0, "loud", True, float("nan")):
        with pytest.raises(ValueError):
            synth.synthesize_at("x", loudness=bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch(["x"], loudness=bad)
        with pytest.raises(ValueError):
            synth.synthesize_long("A sentence.", loudness=bad)
        with pytest.raises(ValueError):
            synth.synthesize_long_stream("A sentence.", loudness=bad)
        with pytest.raises(ValueError):
            synth.synthesize_batch_stream(["x"], loudness=bad)
        with pytest.raises(ValueError):
            next(synth.synthesize_stream("x", loudness=bad))


def test_measure_loudness(synth):
    # the tiny codec decodes 96 frames of 32 samples at most, and the stage takes what a decode can give: 0.8 s at 8 kHz,
    # eight hops and five blocks, fits (the restatement reads -2.997 there)
    rate, n = 8000, 6400
    most = synth._vocoder.max_level_samples
    assert n <= most == -(-2 * synth._vocoder.max_frames * synth._vocoder.frame_len * 48000 // 44100)

    def clip(n):
        x = np.sin(2.0 * np.pi * 997.0 * np.arange(n) / rate)
        buf = io.BytesIO()
        with wave.open(buf, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(rate)
            wf.writeframes((x * 32767).astype(np.int16).tobytes())
        return buf.getvalue()

    assert abs(synth.measure_loudness(clip(n)) - -3.01) <= 0.1                    # EBU Tech 3341's tolerance
    assert abs(synth.measure_loudness(clip(most)) - -3.01) <= 0.1                 # the longest clip the stage takes
    with pytest.raises(ValueError, match="samples"):
        synth.measure_loudness(clip(most + 1))
    for rate, width, ch in ((12345, 2, 1), (16000, 1, 1), (16000, 2, 2)):
        buf = io.BytesIO()
        with wave.open(buf, "wb") as wf:
            wf.setnchannels(ch)
            wf.setsampwidth(width)
            wf.setframerate(rate)
            wf.writeframes(b"\0" * 64)
        with pytest.raises(ValueError):
            synth.measure_loudness(buf.getvalue())
    import inspect
    assert list(inspect.signature(synth.synthesize).parameters) == ["text", "references", "temperature", "top_p",
                                                                    "repetition_penalty", "max_tokens"]
