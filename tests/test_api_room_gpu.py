"""GPU, public API: `room=` of FishTTS.synthesize_long / synthesize_script and FishTTS.reverb on the tiny synthetic models of
tests/test_api_script_gpu.py.  room=None is the call as it was; with a Room the room stage is given the joined piece itself
(a spy on CodecHipEngine.room: its programme, packed, is the un-roomed call's PCM) behind the join and before either mix
stage, and the WAV is the packing of what the last stage returns, the room's tail longer; a line whose send is muted, with no
earlier tail reaching it, is the dry call's PCM; the marks do not move; an open BatchServer gives the same bytes; the streams
refuse a room; every bad Room raises ValueError before any device work.  All comparisons are equalities (the stage's own
arithmetic is tests/test_room_gpu.py's)."""
import math

import numpy as np
import pytest

from tests import intake_ref as IR
from tests.test_api_mix_gpu import _bed
from tests.test_api_script_gpu import MT, SEED, TEXT, _pcm, _script, _voice, _wav
from tests.test_api_serve_gpu import _tiny_tts
from tests.test_api_stereo_gpu import _pack, _wav2

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


def _response(n=300, rate=44100, seed=5):
    v = 0.5 * np.random.default_rng(seed).standard_normal(n) * np.exp(-np.arange(n) / (0.25 * n))
    return IR.wav_bytes(v.astype(np.float32), "f32", rate)


def _room(**kw):
    from fish_tts_amd import Room
    kw.setdefault("wav", _response())
    kw.setdefault("fade", 0.001)
    return Room(**kw)


@pytest.fixture
def spy(synth, monkeypatch):
    """Every call of the three stages behind the join in a test, in order: (stage, programme, regions, rate, params, extra,
    (y, report))."""
    calls = []
    voc = synth._vocoder
    real_room, real_mix, real_stereo = voc.room, voc.mix, voc.mix_stereo

    def room(audio, clip, regions=(), sample_rate=None, params=None, ceiling=True):
        out = real_room(audio, clip, regions, sample_rate=sample_rate, params=params, ceiling=ceiling)
        calls.append(("room", np.array(audio, dtype=np.float32), list(regions), sample_rate, params, (clip, ceiling), out))
        return out

    def mix(x, bed, sample_rate=None, params=None, nodes=False):
        out = real_mix(x, bed, sample_rate=sample_rate, params=params, nodes=nodes)
        calls.append(("mix", np.array(x, dtype=np.float32), None, sample_rate, params, bed, out))
        return out

    def mix_stereo(x, bed, regions=(), sample_rate=None, params=None, nodes=False):
        out = real_stereo(x, bed, regions, sample_rate=sample_rate, params=params, nodes=nodes)
        calls.append(("mix_stereo", np.array(x, dtype=np.float32), list(regions), sample_rate, params, bed, out))
        return out
    monkeypatch.setattr(voc, "room", room)
    monkeypatch.setattr(voc, "mix", mix)
    monkeypatch.setattr(voc, "mix_stereo", mix_stereo)
    return calls


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_room_none_is_the_call_as_it_was(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED)
    assert synth.synthesize_long(TEXT, room=None, **kw) == synth.synthesize_long(TEXT, **kw)
    m1, m2 = [], []
    assert synth.synthesize_script(_script(), voices, room=None, marks=m1, **kw) == synth.synthesize_script(_script(), voices, marks=m2, **kw)
    assert m1 == m2 and not spy


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=16000, loudness=-23.0, silence_db=-30.0)], ids=["native", "16k-levelled"])
def test_a_long_text_is_the_join_then_the_room(synth, default, spy, kw):
    from fish_tts_amd.room import room_params
    kw = dict(kw, references=default, max_tokens=MT, seed=SEED)
    rate = kw.get("sample_rate", 44100)
    room = _room(wet_db=-9.0, predelay=0.002)
    plain = synth.synthesize_long(TEXT, **kw)
    got = synth.synthesize_long(TEXT, room=room, **kw)
    (call,) = spy
    stage, x, regions, r, rp, (clip, ceiling), (y, rep) = call
    assert stage == "room" and r == rate and rp == room_params(room, rate) and ceiling is True and regions == []
    assert _pcm(x) == _wav(plain)[1]                                            # the programme is the joined piece itself
    assert rep.n == len(y) == len(x) + rp.predelay + rep.taps - 1 and rep.taps == rep.ir_len
    assert _wav(got) == (rate, _pcm(y))
    del spy[:]
    again, _ = synth._vocoder.room(x, clip, (), sample_rate=rate, params=rp, ceiling=True)     # ... and the engine's own call
    assert np.array_equal(bits(again), bits(y))


def test_with_a_bed_and_in_stereo_the_mix_stages_see_the_lengthened_piece(synth, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)
    room, bed = _room(tail=0.004), _bed(lead=0.01, tail=0.02)
    plain = synth.synthesize_long(TEXT, **kw)
    got = synth.synthesize_long(TEXT, room=room, bed=bed, **kw)
    (s0, x0, _, _, rp, (_, ceiling), (y0, rep0)), (s1, x1, _, r1, mp, _, (y1, rep1)) = spy
    assert (s0, s1) == ("room", "mix") and ceiling is False and not rep0.capped and rep0.gain == 1.0
    assert _pcm(x0) == _wav(plain)[1] and len(y0) == len(x0) + 64 and rp.tail == 64
    assert np.array_equal(bits(x1), bits(y0)) and rep1.n == len(y0) + mp.lead + mp.tail      # the mix stage sees the tail
    assert _wav(got) == (16000, _pcm(y1))
    del spy[:]
    got = synth.synthesize_long(TEXT, room=room, bed=bed, stereo=True, pan=-0.5, **kw)
    (s0, x0, _, _, _, (_, ceiling), (y0, _)), (s1, x1, regions, _, _, clip, (y1, _)) = spy
    assert (s0, s1) == ("room", "mix_stereo") and ceiling is False and clip is not None
    assert np.array_equal(bits(x1), bits(y0)) and regions == [(0, len(y0), -50)]            # the tail rings where the voice is
    r, ch, frames = _wav2(got)
    assert (r, ch) == (16000, 2) and np.array_equal(frames, _pack(y1))
    del spy[:]
    synth.synthesize_long(TEXT, room=room, stereo=True, **kw)                                # stereo without a bed, in the centre
    assert [c[0] for c in spy] == ["room", "mix_stereo"] and spy[0][5][1] is False and spy[1][2] == [] and spy[1][5] is None


def test_a_script_with_sends_and_muted_lines(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)
    room = _room(wet_db=-6.0)                                       # 109 taps at 16 kHz: far shorter than any pause
    plain_marks, marks = [], []
    plain = synth.synthesize_script(_script(), voices, marks=plain_marks, **kw)
    got = synth.synthesize_script(_script(), voices, marks=marks, room=room, sends={"anna": -math.inf, 2: -6.0}, **kw)
    (call,) = spy
    stage, x, regions, r, rp, (clip, ceiling), (y, rep) = call
    (a0, e0), (a1, e1), (a2, e2), (a3, e3) = plain_marks            # anna, ben, the narrator, anna
    assert stage == "room" and ceiling is True and _pcm(x) == _wav(plain)[1]
    assert regions == [(a0, e0, -1), (a2, e2, 600), (a3, e3, -1)]
    assert marks == plain_marks                                     # the marks do not move
    rate, pcm = _wav(got)
    dry = np.frombuffer(_wav(plain)[1], dtype=np.int16)
    wet = np.frombuffer(pcm, dtype=np.int16)
    assert not rep.capped and len(wet) == len(dry) + rep.taps - 1
    assert np.array_equal(wet[a0:e0], dry[a0:e0])                   # the opening line is muted and nothing rang before it
    assert a3 - e2 > rep.taps and np.array_equal(wet[a3:e3], dry[a3:e3])      # ... the closing one stands behind a long pause
    assert not np.array_equal(wet[a1:e1], dry[a1:e1]) and not np.array_equal(wet[a2:e2], dry[a2:e2])
    assert not wet[e3 + 1:].any()                                   # a muted last line leaves no tail
    # a line index wins over its voice; a line without an entry sends at 0 dB
    del spy[:]
    synth.synthesize_script(_script(), voices, room=room, sends={"anna": -3.0, 3: -math.inf}, **kw)
    assert spy[0][2] == [(a0, e0, 300), (a3, e3, -1)]
    # through an open server: the same bytes
    with synth.serve(burst=4):
        assert synth.synthesize_script(_script(), voices, room=room, sends={"anna": -math.inf, 2: -6.0}, **kw) == got


def test_reverb_on_a_finished_wav(synth, default, spy):
    from fish_tts_amd.room import room_params
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=24000)
    plain = synth.synthesize_long("Some text is here.", **kw)
    room = _room(dry_db=-3.0, tail=0.001)
    report = []
    got = synth.reverb(plain, room, report=report)
    (call,) = spy
    stage, x, regions, r, rp, (clip, ceiling), (y, rep) = call
    audio = np.frombuffer(_wav(plain)[1], dtype=np.int16).astype(np.float32) / 32768.0
    assert stage == "room" and r == 24000 and ceiling is True and regions == [] and rp == room_params(room, 24000)
    assert np.array_equal(x, audio) and report == [rep] and rep.n == len(audio) + 24
    assert _wav(got) == (24000, _pcm(y))
    with synth.serve(burst=4):
        assert synth.reverb(plain, room) == got
    for bad in (lambda: synth.reverb(plain, None), lambda: synth.reverb(plain, "room.wav"),
                lambda: synth.reverb(synth._to_wav_bytes(np.zeros((4, 2), np.float32), 24000), room),
                lambda: synth.reverb(synth._to_wav_bytes(np.zeros(4, np.float32), 7000), room)):
        with pytest.raises(ValueError):
            bad()


def test_bad_rooms_raise_before_any_work(synth, voices, default, monkeypatch, spy):
    from fish_tts_amd import Line, Room

    def no_work(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    t = "Some text is here."
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth._vocoder, "decode_join", no_work)
    monkeypatch.setattr(synth._vocoder.lib, "ft_codec_room", no_work, raising=False)
    script = lambda *a, **k: synth.synthesize_script(*a, references=default, **k)      # noqa: E731
    long_ = lambda **k: synth.synthesize_long(t, references=default, **k)               # noqa: E731
    bad = [lambda: long_(room="room.wav"), lambda: long_(room=_room(wet_db=1.0)), lambda: long_(room=_room(dry_db=-61.0)),
           lambda: long_(room=_room(predelay=1.5)), lambda: long_(room=_room(length=0.0)), lambda: long_(room=_room(tail=-1.0)),
           lambda: long_(room=_room(normalize=1)), lambda: long_(room=_room(channel=1)),                  # a mono file has no channel 1
           lambda: long_(room=Room(b"not a wav")), lambda: long_(room=_room(wav=_response(rate=7000))),
           lambda: script([Line(t)], voices, sends={"anna": -6.0}),                                        # sends without a room
           lambda: script([Line(t)], voices, room=_room(), sends={"carl": -6.0}),
           lambda: script([Line(t)], voices, room=_room(), sends={1: -6.0}),
           lambda: script([Line(t)], voices, room=_room(), sends={"anna": 1.0}),
           lambda: script([Line(t)], voices, room=_room(), sends={"anna": float("nan")}),
           lambda: synth.synthesize_long_stream(t, references=default, room=_room()),
           lambda: synth.synthesize_script_stream([Line(t)], voices, references=default, room=_room()),
           lambda: synth.synthesize_script_stream([Line(t)], voices, references=default, sends={0: -6.0})]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    assert not spy
