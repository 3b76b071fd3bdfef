"""GPU, public API: `live_room=` / `live_sends=` of FishTTS.synthesize_long_stream / synthesize_script_stream on the tiny
synthetic models of tests/test_api_script_gpu.py, on the fixtures of tests/test_api_live_bed_gpu.py.  How the segments fall
into groups is the feeder's timing, so nothing here depends on it: a spy on decode_join collects the programme the stream
joins, spies on CodecHipEngine.room_stream and mix_stream record every push, and each stream is held against the engine's own
whole calls over what went in - CodecHipEngine.room(..., ceiling=False) for the room, then mix_live / mix_live_stereo / a
bare limiter stream in one push for the mixer.  All comparisons are equalities (the stages' own arithmetic is
tests/test_room_live_gpu.py's)."""
import inspect
import math

import numpy as np
import pytest

from tests import intake_ref as IR
from tests.test_api_mix_gpu import _bed
from tests.test_api_room_gpu import _room, bits
from tests.test_api_script_gpu import MT, SEED, TEXT, _pcm, _script, _voice
from tests.test_api_serve_gpu import _tiny_tts
from tests.test_api_stereo_gpu import _pack

pytestmark = pytest.mark.gpu
CEILING = int(10.0 ** (-1.0 / 20.0) * 32767) + 1          # -1 dBFS in int16, one step for the rounding of the factor
LEVELLED = dict(sample_rate=16000, loudness=-23.0, silence_db=-30.0)     # peaks near 0.1: no limiter has anything to do
PANS = {"anna": -0.5, "ben": 0.5}


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
def joined(synth, monkeypatch):
    """The joined audio of every decode_join call of a test, in order (tests/test_api_live_bed_gpu.py's spy)."""
    calls = []
    real = synth._vocoder.decode_join

    def decode_join(*a, **k):
        out = real(*a, **k)
        calls.append(np.array(out[0], dtype=np.float32))
        return out
    monkeypatch.setattr(synth._vocoder, "decode_join", decode_join)
    return calls


@pytest.fixture
def streams(synth, monkeypatch):
    """Every room stream and mix stream a test opens: dict(kind, clip / bed, rate, params, stereo, bedless, stream,
    pushes=[(x, regions, final, y)])."""
    opened = []
    voc = synth._vocoder
    real_room, real_mix = voc.room_stream, voc.mix_stream

    def wrap(rec, st, with_regions):
        push = st.push

        def spied(x=None, *a, **k):
            regions = list(a[0] if a else k.get("regions", ())) if with_regions else []
            y = push(x, *a, **k)
            rec["pushes"].append((np.zeros(0, dtype=np.float32) if x is None else np.array(x, dtype=np.float32), regions,
                                  bool(k.get("final", False)), np.array(y, dtype=np.float32)))
            return y
        st.push = spied
        rec["stream"] = st
        opened.append(rec)
        return st

    def room_stream(clip, sample_rate=None, params=None):
        return wrap(dict(kind="room", clip=clip, rate=sample_rate, params=params, pushes=[]),
                    real_room(clip, sample_rate=sample_rate, params=params), True)

    def mix_stream(bed, sample_rate=None, params=None, stereo=False, bedless=False):
        return wrap(dict(kind="mix", bed=bed, rate=sample_rate, params=params, stereo=stereo, bedless=bedless, pushes=[]),
                    real_mix(bed, sample_rate=sample_rate, params=params, stereo=stereo, bedless=bedless), stereo)
    monkeypatch.setattr(voc, "room_stream", room_stream)
    monkeypatch.setattr(voc, "mix_stream", mix_stream)
    return opened


def _whole(rec):
    """(input, regions over it, output) of a recorded stream: its pushes laid end to end, the regions moved to the timeline."""
    x = np.concatenate([p[0] for p in rec["pushes"]])
    regions, at = [], 0
    for xk, rk, _, _ in rec["pushes"]:
        for a, e, q in rk:
            if regions and regions[-1][1] == a + at and regions[-1][2] == q:
                regions[-1] = (regions[-1][0], e + at, q)
            else:
                regions.append((a + at, e + at, q))
        at += len(xk)
    return x, regions, np.concatenate([p[3] for p in rec["pushes"]])


def _check_room(synth, rec, prog, want_regions):
    """The room stream of a call against the whole call over the programme; returns the roomed piece."""
    x, regions, y = _whole(rec)
    assert np.array_equal(bits(x), bits(prog)) and regions == want_regions
    assert rec["pushes"][-1][2] and len(rec["pushes"][-1][0]) == 0 and rec["stream"]._h is None     # the tail's push; closed
    assert all(len(p[3]) == len(p[0]) for p in rec["pushes"][:-1])                                  # nothing is held back
    whole, rep = synth._vocoder.room(prog, rec["clip"], regions, sample_rate=rec["rate"], params=rec["params"], ceiling=False)
    assert np.array_equal(bits(y), bits(whole))
    return whole, rep


def _bare(synth, x, rate):
    with synth._vocoder.mix_stream(None, sample_rate=rate, bedless=True) as ms:
        return np.array(ms.push(x, final=True))


def test_a_one_sample_response_is_the_plain_stream(synth, default, joined, streams):
    kw = dict(references=default, max_tokens=MT, seed=SEED, loudness=-23.0, silence_db=-30.0)
    from fish_tts_amd import Room
    one = Room(IR.wav_bytes(np.ones(1, dtype=np.float32), "f32", 44100), wet_db=0.0, dry_db=None, fade=0.0)
    plain = b"".join(synth.synthesize_long_stream(TEXT, **kw))
    assert not streams
    chunks = list(synth.synthesize_long_stream(TEXT, live_room=one, **kw))
    assert all(chunks) and b"".join(chunks) == plain
    mixer, room = streams
    assert (mixer["kind"], mixer["bedless"], mixer["stereo"], mixer["bed"], room["kind"]) == ("mix", True, False, None, "room")
    assert b"".join(synth.synthesize_long_stream(TEXT, live_room=None, **kw)) == plain and len(streams) == 2


def test_a_decaying_response_rings_on_and_the_marks_stay(synth, voices, default, joined, streams):
    kw = dict(references=default, max_tokens=MT, seed=SEED, **LEVELLED)
    room = _room(wet_db=-6.0, predelay=0.002)
    m0, m1 = [], []
    plain = b"".join(synth.synthesize_script_stream(_script(), voices, marks=m0, **kw))
    prog = np.concatenate(joined)
    del joined[:]
    got = b"".join(synth.synthesize_script_stream(_script(), voices, marks=m1, live_room=room, **kw))
    assert _pcm(np.concatenate(joined)) == plain                                # the same programme went into the room
    mixer, rec = streams
    whole, rep = _check_room(synth, rec, prog, [])
    tl = rec["params"].predelay + rep.taps - 1
    assert rec["params"].predelay == 32 and rep.taps == rep.ir_len and tl > 100
    assert len(got) == len(plain) + 2 * tl and m1 == m0 and len(m0) == 4        # longer by exactly the tail; the marks stay
    mx, _, my = _whole(mixer)
    assert np.array_equal(bits(mx), bits(whole)) and mixer["bedless"] and len(mixer["pushes"][-1][0]) == tl
    assert got == _pcm(my) == _pcm(_bare(synth, whole, 16000))
    assert got == _pcm(whole)                                                   # a levelled piece: the limiter had nothing to do


def test_a_loud_piece_stays_under_the_ceiling(synth, default, joined, streams):
    kw = dict(references=default, max_tokens=MT, seed=SEED)                     # the synthetic codec's full-scale noise
    got = b"".join(synth.synthesize_long_stream(TEXT, live_room=_room(wet_db=0.0), **kw))
    mixer, rec = streams
    whole, rep = _check_room(synth, rec, np.concatenate(joined), [])
    assert rep.peak > 10.0 ** (-1.0 / 20.0)                                     # the room stage alone would have needed its ceiling
    assert got == _pcm(_bare(synth, whole, 44100)) and got != _pcm(whole)
    assert int(np.abs(np.frombuffer(got, dtype=np.int16).astype(np.int32)).max()) <= CEILING


def test_with_a_live_bed(synth, default, joined, streams):
    kw = dict(references=default, max_tokens=MT, seed=SEED, **LEVELLED)
    room, bed = _room(tail=0.004), _bed(lead=0.013, tail=0.021, duck_db=9.0, attack=0.04, release=0.06)
    got = b"".join(synth.synthesize_long_stream(TEXT, live_room=room, live_bed=bed, **kw))
    mixer, rec = streams
    whole, rep = _check_room(synth, rec, np.concatenate(joined), [])
    assert len(whole) == len(np.concatenate(joined)) + 64 and not mixer["bedless"] and not mixer["stereo"]
    mx, _, my = _whole(mixer)
    assert np.array_equal(bits(mx), bits(whole))                                # the mixer sees the piece with its tail
    y, mrep = synth._vocoder.mix_live(whole, mixer["bed"], sample_rate=16000, params=mixer["params"])
    assert got == _pcm(my) == _pcm(y) and len(y) == mixer["params"].lead + len(whole) + mixer["params"].tail


@pytest.mark.parametrize("with_bed", [False, True], ids=["no-bed", "bed"])
def test_with_live_stereo_the_tail_stays_at_the_last_lines_pan(synth, voices, default, joined, streams, with_bed):
    from tests.test_api_stereo_gpu import _stereo_music
    kw = dict(references=default, max_tokens=MT, seed=SEED, **LEVELLED)
    bed = _bed(wav=_stereo_music(), level=-40.0, lead=0.013, tail=0.021, fade_out=0.01) if with_bed else None
    marks = []
    chunks = list(synth.synthesize_script_stream(_script(), voices, marks=marks, live_room=_room(wet_db=-6.0), live_bed=bed,
                                                 live_stereo=True, live_pans=PANS, **kw))
    mixer, rec = streams
    prog = np.concatenate(joined)
    whole, rep = _check_room(synth, rec, prog, [])
    tl = rep.taps - 1
    mx, regions, my = _whole(mixer)
    assert mixer["stereo"] and not mixer["bedless"] and (mixer["bed"] is None) == (not with_bed)
    assert np.array_equal(bits(mx), bits(whole))
    (a0, e0), (a1, e1), _, (a3, e3) = [(a - (mixer["params"].lead if with_bed else 0), e - (mixer["params"].lead if with_bed else 0))
                                       for a, e in marks]
    assert mixer["pushes"][-1][1] == [(0, tl, -50)] and e3 == len(prog)         # anna spoke last: the tail rings on her side
    assert regions == [(a0, e0, -50), (a1, e1, 50), (a3, e3 + tl, -50)]         # ... as the one-shot call's extended region
    y, _ = synth._vocoder.mix_live_stereo(whole, mixer["bed"], regions, sample_rate=16000, params=mixer["params"])
    assert all(chunks) and b"".join(chunks) == _pack(my).tobytes() == _pack(y).tobytes()


def test_live_sends_with_a_muted_narrator(synth, voices, default, joined, streams):
    kw = dict(references=default, max_tokens=MT, seed=SEED, **LEVELLED)
    room = _room(wet_db=-6.0)                                                   # 109 taps at 16 kHz: far shorter than any pause
    m0, m1 = [], []
    plain = b"".join(synth.synthesize_script_stream(_script(), voices, marks=m0, **kw))
    prog = np.concatenate(joined)
    del joined[:]
    got = b"".join(synth.synthesize_script_stream(_script(), voices, marks=m1, live_room=room,
                                                  live_sends={2: -math.inf, "ben": -6.0}, **kw))
    (a0, e0), (a1, e1), (a2, e2), (a3, e3) = m0                                 # anna, ben, the narrator, anna
    mixer, rec = streams
    whole, rep = _check_room(synth, rec, prog, [(a1, e1, 600), (a2, e2, -1)])
    assert m1 == m0 and got == _pcm(whole)
    dry, wet = np.frombuffer(plain, dtype=np.int16), np.frombuffer(got, dtype=np.int16)
    assert a3 - e2 > rep.taps and not np.array_equal(wet[a3:e3], dry[a3:e3])    # anna stands in the room ...
    assert a2 - e1 > rep.taps and e2 > a2 and np.array_equal(wet[a2:e2], dry[a2:e2])     # ... the narrator, behind ben's ring-out, does not
    # the same through an open server
    del streams[:]
    with synth.serve(burst=4):
        assert b"".join(synth.synthesize_script_stream(_script(), voices, live_room=room, live_sends={2: -math.inf, "ben": -6.0},
                                                      **kw)) == got


def test_an_abandoned_stream_closes_both(synth, default, streams):
    kw = dict(references=default, max_tokens=MT, seed=SEED, **LEVELLED)
    gen = synth.synthesize_long_stream(TEXT, live_room=_room(), live_bed=_bed(lead=1.0), **kw)
    assert next(gen)
    mixer, rec = streams
    assert mixer["stream"]._h is not None and rec["stream"]._h is not None
    gen.close()
    assert mixer["stream"]._h is None and rec["stream"]._h is None


def test_refusals_at_the_call(synth, voices, default, monkeypatch):
    from fish_tts_amd import Line, Room

    def no_work(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth._vocoder, "decode_join", no_work)
    monkeypatch.setattr(synth._vocoder, "room_stream", no_work)
    monkeypatch.setattr(synth._vocoder, "mix_stream", no_work)
    ok = _room().wav
    for kw in (dict(wet_db=0.5), dict(dry_db=-61.0), dict(predelay=1.01), dict(length=0.0), dict(fade=-1.0), dict(tail="1"),
               dict(normalize=1), dict(channel=1), dict(wav=b"not a wav"), dict(wav=None),
               dict(wav=IR.wav_bytes(np.zeros(100, dtype=np.float32), "f32", 7000))):
        kw.setdefault("wav", ok)
        r = Room(**kw)
        with pytest.raises(ValueError):                              # at the call, not at the first next()
            synth.synthesize_long_stream(TEXT, references=default, live_room=r)
        with pytest.raises(ValueError):
            synth.synthesize_script_stream([Line("Some text is here.")], voices, references=default, live_room=r)
    with pytest.raises(ValueError, match="live_sends needs live_room"):
        synth.synthesize_script_stream(_script(), voices, references=default, live_sends={"anna": -3.0})
    with pytest.raises(ValueError, match="whole piece") as e:
        synth.synthesize_long_stream(TEXT, references=default, room=_room())
    assert "live_room=" in str(e.value)
    with pytest.raises(ValueError, match="whole piece"):
        synth.synthesize_script_stream(_script(), voices, references=default, sends={"anna": -3.0}, live_room=_room())
    for name in ("synthesize_long", "synthesize_script", "synthesize_stream", "synthesize", "reverb"):
        assert "live_room" not in inspect.signature(getattr(synth, name)).parameters, name
    assert "live_sends" not in inspect.signature(synth.synthesize_long_stream).parameters
