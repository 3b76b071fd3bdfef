"""GPU, public API: `live_bed=` of FishTTS.synthesize_long_stream / synthesize_script_stream on the tiny synthetic models of
tests/test_api_script_gpu.py.  The chunks of a stream with a live bed concatenate to the int16 packing of
CodecHipEngine.mix_live over the programme the plain stream joins (a spy on decode_join collects it), at the codec's rate, at
16 kHz with `loudness`, through an open BatchServer, and for a script with its marks moved by `lead`; with a `lead` longer than
the stage holds back the first chunk is out before anything was decoded; a bed of digital silence returns lead zeros, the piece,
tail zeros; `bed=` is still refused; a bad Bed raises at the call, before any device work.  All comparisons are equalities
(the stage's own arithmetic is tests/test_mix_live_gpu.py's)."""
import inspect

import numpy as np
import pytest

from tests import intake_ref as IR
from tests.test_api_mix_gpu import _bed, _music
from tests.test_api_script_gpu import MT, SEED, TEXT, _pcm, _script, _voice
from tests.test_api_serve_gpu import _tiny_tts

pytestmark = pytest.mark.gpu


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


@pytest.fixture
def spy(synth, monkeypatch):
    """The joined audio of every decode_join call of a test, in order."""
    calls = []
    real = synth._vocoder.decode_join

    def decode_join(*a, **k):
        out = real(*a, **k)
        calls.append(np.array(out[0], dtype=np.float32))
        return out
    monkeypatch.setattr(synth._vocoder, "decode_join", decode_join)
    return calls


def _both(synth, spy, call, bed, kw):
    """(plain PCM, live PCM, the stage's own answer for the plain stream's programme)."""
    del spy[:]
    plain = b"".join(call(**kw))
    prog = np.concatenate(spy)
    assert _pcm(prog) == plain
    del spy[:]
    got = b"".join(call(live_bed=bed, **kw))
    assert _pcm(np.concatenate(spy)) == plain                       # the same programme went into the stage
    rate = kw.get("sample_rate") or 44100
    clip, mp = synth._bed_args(bed, rate, kw.get("silence_db", -45.0))
    y, rep = synth._vocoder.mix_live(prog, clip, sample_rate=rate, params=mp)
    assert len(y) == mp.lead + len(prog) + mp.tail and rep.active > 0
    return plain, got, _pcm(y)


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=16000, loudness=-23.0, silence_db=-30.0)], ids=["native", "16k-levelled"])
def test_the_long_stream_is_mix_live_over_its_programme(synth, default, spy, kw):
    kw = dict(kw, references=default, max_tokens=MT, seed=SEED)
    bed = _bed(lead=0.013, tail=0.021, duck_db=9.0, attack=0.04, release=0.06)
    plain, got, want = _both(synth, spy, lambda **k: synth.synthesize_long_stream(TEXT, **k), bed, kw)
    assert got == want and got != plain
    assert b"".join(synth.synthesize_long_stream(TEXT, live_bed=None, **kw)) == plain


def test_the_script_stream_and_its_marks(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, silence_db=-30.0)
    bed = _bed(lead=0.013, tail=0.021, threshold_db=-20.0, loop=False, offset=0.002)
    lead = int(round(0.013 * 44100))
    m0, m1 = [], []
    plain, got, want = _both(synth, spy, lambda **k: synth.synthesize_script_stream(_script(), voices, marks=m1 if "live_bed" in k else m0, **k),
                             bed, kw)
    assert got == want
    assert m0 and m1 == [(a + lead, b + lead) for a, b in m0]


def test_through_an_open_server(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, silence_db=-30.0)
    bed = _bed(lead=0.6, tail=0.01, duck_db=6.0)
    _, want, stage = _both(synth, spy, lambda **k: synth.synthesize_long_stream(TEXT, **k), bed, kw)
    assert want == stage
    m0, m1 = [], []
    want_script = b"".join(synth.synthesize_script_stream(_script(), voices, marks=m0, live_bed=bed, **kw))
    with synth.serve(burst=4):
        assert b"".join(synth.synthesize_long_stream(TEXT, live_bed=bed, **kw)) == want
        assert b"".join(synth.synthesize_script_stream(_script(), voices, marks=m1, live_bed=bed, **kw)) == want_script
    assert m1 == m0


def test_a_long_lead_plays_before_anything_is_decoded(synth, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED)
    bed = _bed(lead=1.0, attack=0.1, fade_out=0.05)
    clip, mp = synth._bed_args(bed, 44100, -45.0)
    head = synth._vocoder.mix_live_plan(44100, mp, 0, False)[0]
    assert head == (50 - 5 - 5) * 882                                # 50 hops of lead, the attack's 5 and the limiter's 5 held back
    gen = synth.synthesize_long_stream(TEXT, live_bed=bed, **kw)
    assert not spy
    first = next(gen)
    assert not spy and len(first) == 2 * head                        # the bed alone, before any group was decoded
    rest = b"".join(gen)
    y, _ = synth._vocoder.mix_live(np.concatenate(spy), clip, sample_rate=44100, params=mp)
    assert first + rest == _pcm(y)
    # abandoned after the first chunk: the generator closes its stream and stops the batch
    gen = synth.synthesize_long_stream(TEXT, live_bed=bed, **kw)
    assert next(gen) == first
    gen.close()
    assert b"".join(synth.synthesize_long_stream(TEXT, live_bed=bed, **kw)) == first + rest


def test_a_silent_bed_returns_the_piece(synth, voices, default):
    # (levelled: the piece then peaks far below the -1 dBFS ceiling, so the limiter has nothing to do)
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)
    silence = IR.wav_bytes(np.zeros((3000, 2), dtype=np.int64), "s16", 48000)
    plain = b"".join(synth.synthesize_script_stream(_script(), voices, **kw))
    got = b"".join(synth.synthesize_script_stream(_script(), voices, live_bed=_bed(wav=silence, lead=0.01, tail=0.02, level=None), **kw))
    assert got == b"\0\0" * 160 + plain + b"\0\0" * 320


def test_bed_is_still_refused_and_both_raise(synth, voices, default):
    with pytest.raises(ValueError, match="whole piece") as e:
        synth.synthesize_long_stream(TEXT, references=default, bed=_bed())
    assert "use live_bed=" in str(e.value)
    with pytest.raises(ValueError, match="whole piece"):
        synth.synthesize_script_stream(_script(), voices, references=default, bed=_bed())
    with pytest.raises(ValueError, match="live_bed"):
        synth.synthesize_long_stream(TEXT, references=default, bed=_bed(), live_bed=_bed())
    with pytest.raises(ValueError, match="live_bed"):
        synth.synthesize_script_stream(_script(), voices, references=default, bed=_bed(), live_bed=_bed())
    for name in ("synthesize_long", "synthesize_script", "synthesize_stream", "synthesize", "mix"):
        assert "live_bed" not in inspect.signature(getattr(synth, name)).parameters, name


def test_bad_beds_raise_at_the_call_before_any_work(synth, voices, default, monkeypatch):
    from fish_tts_amd import Bed, Line

    def no_work(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    ok = _music()
    bad = [dict(level=-4.0), dict(duck_db=60.5), dict(threshold_db=0.5), dict(attack=0.0), dict(release=11), dict(lead=-0.1),
           dict(tail="1"), dict(fade_in=float("nan")), dict(fade_out=None), dict(offset=1e9), dict(loop=1), dict(channel=1),
           dict(wav=b"not a wav"), dict(wav=None), dict(wav=IR.wav_bytes(np.zeros(100, dtype=np.float32), "f32", 7000))]
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth._vocoder, "decode_join", no_work)
    monkeypatch.setattr(synth._vocoder, "mix_stream", no_work)
    monkeypatch.setattr(synth._vocoder.lib, "ft_codec_mix_stream_begin", no_work, raising=False)
    monkeypatch.setattr(synth._vocoder.lib, "ft_codec_intake", no_work, raising=False)
    for kw in bad:
        kw.setdefault("wav", ok)
        b = Bed(**kw)
        with pytest.raises(ValueError):                              # at the call, not at the first next()
            synth.synthesize_long_stream(TEXT, references=default, live_bed=b)
        with pytest.raises(ValueError):
            synth.synthesize_script_stream([Line("Some text is here.")], voices, references=default, live_bed=b)
    for notbed in (ok, (ok,), {"wav": ok}, "bed.wav"):
        with pytest.raises(ValueError, match="Bed"):
            synth.synthesize_long_stream(TEXT, references=default, live_bed=notbed)
