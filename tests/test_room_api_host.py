"""`room=` without a GPU: room.room_params (a Room's seconds and dB as native integers, the refusals), room.send_regions'
merging, script.plan_script's sends, segments.join_wav putting the room stage behind the join and before either mix stage -
with the ceiling only where no mix stage follows, the lengthened piece handed on, the last pan region extended over the
tail - on the fake codec of tests/test_segments_host.py, and the streams' refusals."""
import math
import threading

import numpy as np
import pytest

import fish_tts_amd.segments as S
from fish_tts_amd import Room
from fish_tts_amd.room import MUTED, RoomParams, native_send, room_bytes, room_params, send_regions
from fish_tts_amd.script import Line, line_marks, plan_script
from tests.test_segments_host import LONG, MIXED, JoinCodec, _codes, _kw, _no_server, _plan

T = "Some text is here."
VOICES = {"anna": [], "ben": []}


def test_room_params_native_values():
    assert room_params(Room(b""), 44100) == RoomParams(-1, 1, 1200, 0, 0, 0, 0, 2205, 0, -1)
    r = Room(b"x", wet_db=-6.004, dry_db=None, predelay=0.02, length=1.5, fade=0.1, offset=0.003, tail=2.0, normalize=False, channel=1)
    assert room_params(r, 16000) == RoomParams(1, 0, 600, MUTED, 0, 48, 24000, 1600, 320, 32000)
    assert room_params(Room(b"", wet_db=0, dry_db=-60, predelay=1.0, tail=0), 8000)[2:5] == (0, 6000, 0)
    assert room_params(Room(b"", predelay=1.0, tail=0), 8000)[-2:] == (8000, 0)
    assert room_params(Room("some/file.wav"), 44100).wet == 1200 and room_bytes(Room(bytearray(b"abc"))) == b"abc"
    assert [native_send("s", v) for v in (0, -0.004, -6, -60.0, -math.inf)] == [0, 0, 600, 6000, MUTED]


def test_room_params_refusals():
    nan = float("nan")
    bad = [dict(wav=123), dict(wav=None), dict(wet_db=0.1), dict(wet_db=-60.1), dict(wet_db=None), dict(wet_db=nan), dict(wet_db=True),
           dict(dry_db=1), dict(dry_db=-61), dict(dry_db="0"), dict(dry_db=nan), dict(predelay=-0.001), dict(predelay=1.001),
           dict(predelay=None), dict(length=0), dict(length=0.00001), dict(length=-1), dict(length=601), dict(fade=-1), dict(fade=nan),
           dict(offset=-0.5), dict(offset="1"), dict(tail=-1), dict(tail=601), dict(normalize=1), dict(normalize=None),
           dict(channel=-1), dict(channel=True), dict(channel=0.0)]
    for kw in bad:
        with pytest.raises(ValueError, match="room"):
            room_params(Room(**{"wav": b"", **kw}), 44100)
            pytest.fail(f"accepted: {kw}")
    for v in ("room.wav", b"", None, 5, ("a", "b")):
        with pytest.raises(ValueError, match="must be a Room"):
            room_params(v, 44100)
    for v in (0.1, -60.5, nan, True, "0", None, math.inf):
        with pytest.raises(ValueError):
            native_send("send", v)


def test_send_regions_merge_as_pan_regions_do():
    marks = [(0, 10), (15, 30), (30, 30), (35, 50), (55, 60), None, (60, 70), (75, 80)]
    assert send_regions([600, 600, 20, 600, 0, 99, MUTED, MUTED], marks) == [(0, 50, 600), (60, 80, MUTED)]
    assert send_regions([10, 0, 10], [(0, 5), (5, 9), (9, 12)]) == [(0, 5, 10), (9, 12, 10)]
    assert send_regions([10, MUTED, 10], [(0, 5), (5, 9), (9, 12)]) == [(0, 5, 10), (5, 9, MUTED), (9, 12, 10)]
    assert send_regions([0, 0], [(0, 5), (5, 9)]) == [] and send_regions([7], [None]) == [] and send_regions([7], [(3, 3)]) == []


def test_plan_script_sends():
    lines = [Line(T, voice="anna"), Line(T, voice="ben"), Line(T), Line(T, voice="anna")]
    p = plan_script(lines, VOICES, room=True, sends={"anna": -6.0, 3: -math.inf, "ben": 0})
    assert p.sends == [600, 0, 0, MUTED] and len(p.sends) == p.n_lines        # a line's own entry wins over its voice's
    assert plan_script(lines, VOICES, room=True).sends == [0, 0, 0, 0]        # no sends: every line at 0 dB
    assert plan_script(lines, VOICES).sends is None                           # no room: the plan as it was
    assert plan_script(lines, VOICES)[:9] == plan_script(lines, VOICES, room=True, sends={2: -3})[:9]
    assert Line._fields[-1] == "pan"                                          # a Line is as it was: sends come by voice or index
    nan = float("nan")
    bad = [dict(sends={"anna": -6.0}), dict(sends={}), dict(room=1), dict(room=None), dict(room=True, sends={"carl": -6.0}),
           dict(room=True, sends=[("anna", -6.0)]), dict(room=True, sends={None: -6.0}), dict(room=True, sends={4: -6.0}),
           dict(room=True, sends={-1: -6.0}), dict(room=True, sends={True: -6.0})]
    for v in (0.1, -60.01, nan, True, "-6", None, math.inf):
        bad += [dict(room=True, sends={"anna": v}), dict(room=True, sends={0: v})]
    for kw in bad:
        with pytest.raises(ValueError):
            plan_script(lines, VOICES, **kw)
            pytest.fail(f"accepted: {kw}")
    with pytest.raises(ValueError, match="no line"):
        plan_script([Line(T)], None, room=True, sends={1: -6.0})
    flip = [Line(T) for _ in range(4097)]
    assert len(plan_script(flip[:4096], room=True, sends={i: -6.0 for i in range(0, 4096, 2)}).sends) == 4096
    with pytest.raises(ValueError, match="send regions"):
        plan_script(flip * 2 + [Line(T)], room=True, sends={i: -6.0 for i in range(0, 8195, 2)})


def _joined(codes, gaps):
    """What RoomCodec.decode_join gives: the fake codec's pieces behind their gaps, none before the first (the join's layout)."""
    rows = [np.asarray(c)[0].astype(np.float32) / 1e6 for c in codes]
    return np.concatenate([np.concatenate([np.zeros(g if b else 0, dtype=np.float32), r]) for b, (g, r) in enumerate(zip(gaps, rows))])


class RoomCodec(JoinCodec):
    """The three stages behind the join, each recording what it was given; the join lays the gaps out as the real one does
    (the lines' marks then lie inside the piece), and the room adds a tail of TAIL samples."""
    TAIL = 7

    def __init__(self, held=None):
        super().__init__(held)
        self.calls = []

    def decode_join(self, group, params=None, gaps=None, started=False, fx=None, item_fx=None):
        _, cuts = super().decode_join(group, params=params, gaps=gaps, started=started, fx=fx, item_fx=item_fx)
        return _joined(group, gaps), cuts

    def _note(self, what, **kw):
        self.calls.append(dict(what=what, locked=self.held.locked() if self.held is not None else None, **kw))

    def room(self, audio, clip, regions=(), sample_rate=None, params=None, ceiling=True):
        self._note("room", x=np.array(audio), clip=clip, regions=list(regions), rate=sample_rate, params=params, ceiling=ceiling)
        return np.concatenate([np.asarray(audio, dtype=np.float32) * 2, np.full(self.TAIL, 0.5, dtype=np.float32)]), "room report"

    def mix(self, x, bed, sample_rate=None, params=None, nodes=False):
        self._note("mix", x=np.array(x), bed=bed, rate=sample_rate, params=params)
        return np.asarray(x) + 1, "report"

    def mix_stereo(self, x, bed, regions=(), sample_rate=None, params=None, nodes=False):
        self._note("mix_stereo", x=np.array(x), bed=bed, regions=list(regions), rate=sample_rate, params=params)
        return np.stack([x, -x], 1), "report"


def _generate(codes):
    def generate(emit, stopped):
        for i in (2, 0, 3, 1):
            emit(i, codes[i])
    return generate


def test_join_wav_puts_the_room_behind_the_join_and_holds_the_ceiling_when_alone():
    codes = [_codes(i, 3 + i) * 1000 for i in range(4)]
    mono = _joined(codes, _plan(LONG).gaps)
    codec = RoomCodec()
    audio, cuts = S.join_wav(_plan(LONG), **_kw(codec, None, _no_server, _generate(codes)), room=("ir", "rp"))
    (call,) = codec.calls
    assert call["what"] == "room" and np.array_equal(call["x"], mono) and (call["clip"], call["params"]) == ("ir", "rp")
    assert call["ceiling"] is True and call["regions"] == [] and call["rate"] == 44100
    assert len(audio) == len(mono) + RoomCodec.TAIL and np.array_equal(audio[:len(mono)], mono * 2)
    plain, plain_cuts = S.join_wav(_plan(LONG), **_kw(RoomCodec(), None, _no_server, _generate(codes)))
    assert np.array_equal(plain, mono) and np.array_equal(cuts, plain_cuts)           # the cuts do not move


def test_join_wav_with_a_bed_leaves_the_ceiling_to_the_mix_stage():
    codes = [_codes(i, 3 + i) * 1000 for i in range(4)]
    codec = RoomCodec()
    audio, _ = S.join_wav(_plan(LONG), **_kw(codec, None, _no_server, _generate(codes)), bed=("clip", "mp"), room=("ir", "rp"))
    assert [c["what"] for c in codec.calls] == ["room", "mix"] and codec.calls[0]["ceiling"] is False
    roomed = np.concatenate([codec.calls[0]["x"] * 2, np.full(7, 0.5, dtype=np.float32)])
    assert np.array_equal(codec.calls[1]["x"], roomed) and codec.calls[1]["bed"] == "clip"      # the mix stage sees the tail
    assert np.array_equal(audio, roomed + 1)


def test_join_wav_sends_and_the_last_pan_region_over_the_tail():
    codes = [_codes(i, 3 + i) * 1000 for i in range(4)]
    plan = _plan(MIXED)._replace(line_of=[0, 0, 1, 2], n_lines=3, pans=[-50, 0, 50], sends=[600, MUTED, 0])
    codec = RoomCodec()
    audio, cuts = S.join_wav(plan, **_kw(codec, None, _no_server, _generate(codes)), room=("ir", "rp"))
    room, stereo = codec.calls
    assert (room["what"], stereo["what"]) == ("room", "mix_stereo") and room["ceiling"] is False and stereo["bed"] is None
    found = [None] * 3
    line_marks(plan.line_of, plan.gaps, cuts, found)
    assert room["regions"] == [(found[0][0], found[0][1], 600), (found[1][0], found[1][1], MUTED)]
    n = len(room["x"])
    assert found[2][1] == n and len(stereo["x"]) == n + 7
    assert stereo["regions"] == [(found[0][0], found[0][1], -50), (found[2][0], n + 7, 50)]       # the tail rings where line 2 is
    assert audio.shape == (n + 7, 2)
    # the last line in the centre: no region, nothing to extend; a long text at a pan: its one region covers the tail
    codec = RoomCodec()
    S.join_wav(plan._replace(pans=[-50, 20, 0]), **_kw(codec, None, _no_server, _generate(codes)), room=("ir", "rp"))
    assert codec.calls[1]["regions"] == [(found[0][0], found[0][1], -50), (found[1][0], found[1][1], 20)]
    codec = RoomCodec()
    S.join_wav(_plan(LONG)._replace(pans=[30]), **_kw(codec, None, _no_server, _generate(codes)), bed=("clip", "mp"), room=("ir", "rp"))
    assert codec.calls[1]["regions"] == [(0, n + 7, 30)] and codec.calls[0]["regions"] == [] and codec.calls[1]["bed"] == "clip"
    # without a room the stereo call is as it was
    codec = RoomCodec()
    S.join_wav(_plan(LONG)._replace(pans=[30]), **_kw(codec, None, _no_server, _generate(codes)))
    assert [c["what"] for c in codec.calls] == ["mix_stereo"] and codec.calls[0]["regions"] == [(0, n, 30)]


def test_the_room_stage_runs_under_the_servers_codec_lock():
    lock = threading.Lock()
    codes = [_codes(i, 4) * 1000 for i in range(4)]

    class Srv:
        codec_lock = lock
    codec = RoomCodec(held=lock)
    serve = lambda srv: ([lambda c=c: c for c in codes], lambda cancel=False: None)      # noqa: E731
    S.join_wav(_plan(LONG), **_kw(codec, Srv(), serve, None), bed=("clip", "mp"), room=("ir", "rp"))
    assert [c["locked"] for c in codec.calls] == [True, True] and codec.joins[0]["locked"] is True


def test_the_streams_refuse_a_room():
    from fish_tts_amd.synthesizer import FishTTS, _no_streamed_room
    tts = FishTTS.__new__(FishTTS)                           # the refusal comes before anything of the instance is used
    room = Room(b"")
    with pytest.raises(ValueError, match="room needs the whole piece"):
        tts.synthesize_long_stream(T, room=room)
    with pytest.raises(ValueError, match="room needs the whole piece"):
        tts.synthesize_script_stream([Line(T)], room=room)
    with pytest.raises(ValueError, match="room needs the whole piece"):
        tts.synthesize_script_stream([Line(T)], sends={0: -6.0})
    _no_streamed_room(None, "synthesize_long_stream")
