"""`live_room=` without a GPU: room.push_send_regions - the regions segments.join_chunks hands to each push of a room stream -
against room.send_regions of the whole piece for every grouping of a small script (a muted line, a line without audio, equal
neighbours across a group border); join_chunks on a fake codec whose streams record their pushes - the call order, the tail
into the mixer's final push at the last pan, the bare limiter chosen only when no other mixer is, both streams closed when
the generator ends or is abandoned; and every ValueError of the two public calls, before any device work."""
import math
import threading

import numpy as np
import pytest

import fish_tts_amd.segments as S
from fish_tts_amd.room import Room, push_send_regions, send_regions
from fish_tts_amd.script import Line, line_marks
from tests.test_segments_host import _kw, _no_server
from tests.test_stereo_live_api_host import GAPS, LINE_OF, PANS, SIZES, FakeStereoStream, GapCodec, NoDevice, _codes, _merged, _pack

TL = 6                                  # the fake room's tail
#          line 0, 1: one send; 2: no audio (separates nothing); 3: muted; 4: the call's send, 0 dB
SENDS = [300, 300, -1, -1, 0]
OTHER = [-1, 0, 500, 500, 500]


class FakeRoomStream:
    """Gives back what it gets, times two; the final push adds TL samples of 0.125."""

    def __init__(self, log):
        self.log, self.closed, self.s = log, False, np.zeros(0, dtype=np.int64)

    def push(self, x=None, regions=(), final=False):
        assert not self.closed
        x = np.zeros(0, dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32)
        regions = [tuple(r) for r in regions]
        self.log.append(("room", len(x), regions, final))
        at, s = 0, np.zeros(len(x), dtype=np.int64)
        for a, e, send in regions:                         # the stage's own rule for one push
            assert at <= a < e <= len(x) and -1 <= send <= 6000 and send != 0, (regions, len(x))
            s[a:e], at = send, e
        self.s = np.concatenate([self.s, s])
        return np.concatenate([2 * x] + ([np.full(TL, 0.125, dtype=np.float32)] if final else []))

    def close(self):
        self.log.append(("room-close",))
        self.closed = True


class FakeMonoStream:
    def __init__(self, log, lead, tail, hold):
        self.log, self.tail, self.hold = log, tail, hold
        self.buf = np.full(lead, 0.25, dtype=np.float32)
        self.out, self.closed = 0, False

    def push(self, x=None, final=False):
        assert not self.closed
        x = np.zeros(0, dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32)
        self.log.append(("push", len(x), None, final))
        self.buf = np.concatenate([self.buf, x] + ([np.full(self.tail, 0.25, dtype=np.float32)] if final else []))
        end = len(self.buf) if final else max(self.out, len(self.buf) - self.hold)
        got, self.out = self.buf[self.out:end], end
        return got

    def close(self):
        self.log.append(("close",))
        self.closed = True


class RoomCodec(GapCodec):
    def mix_stream(self, bed, sample_rate=None, params=None, stereo=False, bedless=False):
        self.log.append(("open", bed, sample_rate, params, stereo, bedless))
        self.stream = (FakeStereoStream if stereo else FakeMonoStream)(self.log, *self.shape)
        return self.stream

    def room_stream(self, clip, sample_rate=None, params=None):
        self.log.append(("room-open", clip, sample_rate, params))
        self.room = FakeRoomStream(self.log)
        return self.room


def _plan(sends=SENDS, pans=None):
    n = len(LINE_OF)
    return S.SegmentPlan([str(i + 1) for i in range(n)], [None] * n, list(GAPS), (0.5, 4, 2, 1), 44100, [f"fx{i}" for i in range(n)],
                         list(LINE_OF), max(LINE_OF) + 1, None if pans is None else list(pans), None if sends is None else list(sends))


def _whole(sends):
    cuts = [(0, k) for k in SIZES]
    found = [None] * (max(LINE_OF) + 1)
    at, _ = line_marks(LINE_OF, GAPS, cuts, found)
    return found, send_regions(sends, found), at


def _stream(plan, order, codec, **kw):
    codes = [_codes(i, k) for i, k in enumerate(SIZES)]

    def generate(emit, stopped):
        for i in order:
            emit(i, codes[i])
    return list(S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_room=("ir", "rp"), **kw))


@pytest.mark.parametrize("sends", [SENDS, OTHER], ids=["sends", "other"])
def test_every_grouping_of_the_segments_gives_the_one_shot_regions(sends):
    """All 128 ways to cut the eight segments into groups: the regions of the pushes, moved to the timeline and joined where
    equal sends touch, are send_regions of the whole piece's marks; each lies inside its push."""
    found, want, total = _whole(sends)
    if sends is SENDS:
        assert want == [(0, found[1][1], 300), (found[3][0], found[3][1], -1)]    # lines 0 + 1 merged; line 2 gave nothing
    for mask in range(128):
        bounds = [0] + [b for b in range(1, 8) if mask >> (b - 1) & 1] + [8]
        back, place = [], (0, False, 0)
        for first, end in zip(bounds, bounds[1:]):
            at = place[0]
            regions, *place = push_send_regions(sends, LINE_OF[first:end], GAPS[first:end], [(0, k) for k in SIZES[first:end]], *place)
            n = place[0] - at
            assert all(0 <= a < e <= n and s != 0 for a, e, s in regions), (bounds, first, regions)
            assert all(e1 <= a2 for (_, e1, _), (a2, _, _) in zip(regions, regions[1:]))
            if first > 0 and LINE_OF[first] == LINE_OF[first - 1] and sends[LINE_OF[first]] != 0 and SIZES[first] > 0 and at > 0:
                assert regions[0][0] == 0 and regions[0][2] == sends[LINE_OF[first]], (bounds, first, regions)   # a line goes on
            back += [(a + at, e + at, s) for a, e, s in regions]
        assert place[0] == total and _merged(back) == want, (bounds, back)


def test_one_group_per_segment():
    regions, at, started, before = [], 0, False, 0
    for b in range(8):
        r, at2, started, before = push_send_regions(SENDS, LINE_OF[b:b + 1], GAPS[b:b + 1], [(0, SIZES[b])], at, started, before)
        n, at = at2 - at, at2
        if b == 0:
            assert r == [(0, 5, 300)] and n == 5                 # the first audio: no gap in front
        if b == 3:
            assert r == [(0, GAPS[3] + 6, 300)]                  # another line, the same send: the gap goes along
        if b == 4:
            assert r == [] and n == 0 and before == 300          # no audio (though muted): no region, and it separates nothing
        if b == 5:
            assert r == [(GAPS[5], GAPS[5] + 3, -1)]             # a muted line: a region of its own, behind the gap
        if b == 6:
            assert r == [(0, GAPS[6] + 8, -1)]                   # the same line goes on, across the border
        if b == 7:
            assert r == [] and before == 0                       # 0 dB: no region


@pytest.mark.parametrize("order", [list(range(8)), [1, 0, 3, 2, 7, 6, 5, 4], [7, 6, 5, 4, 3, 2, 1, 0]],
                         ids=["in-order", "pairs", "last-first"])
def test_join_chunks_call_order_and_the_bare_limiter(order):
    plan, codec = _plan(), RoomCodec()
    chunks = _stream(plan, order, codec)
    found, want, total = _whole(SENDS)
    log = codec.log
    # the bare limiter, then the room, then the mixer's empty push; the room is closed before the mixer
    assert log[0] == ("open", None, plan.rate, None, False, True) and log[1] == ("room-open", "ir", plan.rate, "rp")
    assert log[2] == ("push", 0, None, False) and log[-2:] == [("room-close",), ("close",)]
    body = log[3:-2]
    # every group: the room's push, then the mixer's with as many samples; at the end the room's final push, its tail into the
    # mixer's final push
    assert len(body) % 2 == 0 and body[-2] == ("room", 0, [], True) and body[-1] == ("push", TL, None, True)
    back, at = [], 0
    for r, m in zip(body[:-2:2], body[1:-2:2]):
        assert r[0] == "room" and m[0] == "push" and r[1] == m[1] > 0 and not r[3] and not m[3]
        back += [(a + at, e + at, s) for a, e, s in r[2]]
        at += r[1]
    assert at == total and _merged(back) == want
    s = np.zeros(total, dtype=np.int64)
    for a, e, v in want:
        s[a:e] = v
    assert codec.room.s.tolist() == s.tolist()                                  # every sample went in with the one-shot send
    pcm = b"".join(chunks)
    assert all(chunks) and len(pcm) == 2 * (total + TL)
    assert pcm[-2 * TL:] == _pack(np.full(TL, 0.125, dtype=np.float32))         # the tail went out through the mixer


def test_the_marks_do_not_move():
    plan, codec, seen = _plan(), RoomCodec(), []
    codes = [_codes(i, k) for i, k in enumerate(SIZES)]

    def generate(emit, stopped):
        for i in range(8):
            emit(i, codes[i])
    list(S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_room=("ir", "rp"),
                       on_cuts=lambda first, cuts: seen.append((first, [tuple(int(v) for v in c) for c in cuts]))))
    assert [c for _, cs in seen for c in cs] == [(0, k) for k in SIZES]


def test_with_a_live_bed_or_a_stereo_stream_that_mixer_is_the_limiter():
    plan, codec = _plan(), RoomCodec(lead=9, tail=2, hold=4)
    chunks = _stream(plan, list(range(8)), codec, live_bed=("clip", "params"))
    assert codec.log[0] == ("open", "clip", plan.rate, "params", False, False)
    assert chunks[0] == _pack(np.full(5, 0.25, dtype=np.float32))               # the bed alone goes out first
    total = _whole(SENDS)[2]
    assert len(b"".join(chunks)) == 2 * (9 + total + TL + 2)
    plan, codec = _plan(pans=PANS), RoomCodec()
    _stream(plan, list(range(8)), codec, live_stereo=True)
    assert codec.log[0] == ("open", None, plan.rate, None, True, False)
    plan, codec = _plan(pans=PANS), RoomCodec()
    _stream(plan, list(range(8)), codec, live_stereo=True, live_bed=("clip", "params"))
    assert codec.log[0] == ("open", "clip", plan.rate, "params", True, False)
    assert not any(e[0] == "open" and e[5] for e in codec.log)


@pytest.mark.parametrize("pans,last", [([-50, -50, 30, 30, 0], 0), ([-50, -50, 30, 30, 70], 70), ([0, 0, 0, -20, -20], -20)])
def test_on_a_stereo_stream_the_tail_stays_at_the_last_pan(pans, last):
    plan, codec = _plan(pans=pans), RoomCodec()
    chunks = _stream(plan, [1, 0, 2, 3, 4, 5, 7, 6], codec, live_stereo=True)
    pushes = [e for e in codec.log if e[0] == "push"]
    assert pushes[-1] == ("push", TL, [(0, TL, last)] if last else [], True)
    total = _whole(SENDS)[2]
    assert codec.stream.q[total:].tolist() == [last] * TL and len(b"".join(chunks)) == 4 * (total + TL)
    rooms = [e for e in codec.log if e[0] == "room"]
    assert [r[1] for r in rooms[:-1]] == [p[1] for p in pushes[1:-1]]           # the mixer sees what the room gave, group by group


def test_a_long_text_has_no_sends():
    n = 4
    plan = S.SegmentPlan([str(i + 1) for i in range(n)], [None] * n, [10, 20, 30, 40], (0.5, 4, 2, 1), 44100, "fx")
    codec = RoomCodec()
    codes = [_codes(i, 3 + i) for i in range(n)]

    def generate(emit, stopped):
        for i in (1, 0, 3, 2):
            emit(i, codes[i])
    list(S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_room=("ir", "rp")))
    assert all(e[2] == [] for e in codec.log if e[0] == "room") and codec.log[0][5] is True


def test_without_live_room_nothing_changes():
    plan, codec = _plan(sends=None), RoomCodec()
    codes = [_codes(i, k) for i, k in enumerate(SIZES)]

    def generate(emit, stopped):
        for i in range(8):
            emit(i, codes[i])
    chunks = list(S.join_chunks(plan, **_kw(codec, None, _no_server, generate)))
    assert codec.log == [] and len(b"".join(chunks)) == 2 * _whole(SENDS)[2]


def test_an_abandoned_generator_closes_both_streams():
    plan, codec, go = _plan(), RoomCodec(), threading.Event()

    def generate(emit, stopped):
        emit(0, _codes(0, 9))
        go.wait(10)
    gen = S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_room=("ir", "rp"))
    assert next(gen)
    assert not codec.stream.closed and not codec.room.closed
    go.set()
    gen.close()
    assert codec.stream.closed and codec.room.closed and codec.log[-2:] == [("room-close",), ("close",)]
    assert not any(e[0] in ("push", "room") and e[3] for e in codec.log)        # no final push: the piece did not end


def test_a_room_that_fails_to_open_still_closes_the_mixer():
    class Broken(RoomCodec):
        def room_stream(self, clip, sample_rate=None, params=None):
            raise RuntimeError("no room")
    plan, codec = _plan(), Broken()
    with pytest.raises(RuntimeError, match="no room"):
        next(S.join_chunks(plan, **_kw(codec, None, _no_server, lambda emit, stopped: None), live_room=("ir", "rp")))
    assert codec.stream.closed


def _synth():
    from fish_tts_amd.synthesizer import FishTTS
    s = object.__new__(FishTTS)                            # no engines: every refusal comes before the first use of any
    s._vocoder = NoDevice()
    s._prefix_cache = None
    return s


def test_refusals_before_any_device_work():
    s, t = _synth(), "Some text is here."
    voices = {"anna": []}
    good = Room(b"RIFF")
    with pytest.raises(ValueError, match="live_sends needs live_room"):
        s.synthesize_script_stream([Line(t, voice="anna")], voices, live_sends={"anna": -6.0})
    with pytest.raises(ValueError, match="live_sends needs live_room"):
        s.synthesize_script_stream([Line(t)], live_sends={})
    with pytest.raises(TypeError):                                              # a long text is one line: it has no sends
        s.synthesize_long_stream(t, live_room=good, live_sends={})
    for call, arg in ((s.synthesize_long_stream, t), (s.synthesize_script_stream, [Line(t)])):
        with pytest.raises(ValueError, match="room must be a Room"):
            call(arg, live_room=b"RIFF")
        with pytest.raises(ValueError, match="wet_db"):
            call(arg, live_room=Room(b"RIFF", wet_db=1.0))
        with pytest.raises(ValueError, match="predelay"):
            call(arg, live_room=Room(b"RIFF", predelay=1.5))
        with pytest.raises(ValueError, match="length"):
            call(arg, live_room=Room(b"RIFF", length=0.0))
        with pytest.raises(ValueError, match="wav must be"):
            call(arg, live_room=Room(17))
        with pytest.raises(ValueError):                                         # bytes that are no WAV
            call(arg, live_room=good)
        with pytest.raises(ValueError, match="room needs the whole piece.*live_room="):     # room= stays refused, with the hint
            call(arg, room=good)
        with pytest.raises(ValueError, match="room needs the whole piece"):
            call(arg, room=good, live_room=good)
    with pytest.raises(ValueError, match="room needs the whole piece"):
        s.synthesize_script_stream([Line(t)], sends={})
    with pytest.raises(ValueError, match="sends must be a dict"):
        s.synthesize_script_stream([Line(t)], live_room=good, live_sends=[1])
    with pytest.raises(ValueError, match="neither a voice"):
        s.synthesize_script_stream([Line(t, voice="anna")], voices, live_room=good, live_sends={"carl": -3.0})
    with pytest.raises(ValueError, match="no line of this script"):
        s.synthesize_script_stream([Line(t)], live_room=good, live_sends={1: -3.0})
    with pytest.raises(ValueError, match=r"\[-60, 0\]"):
        s.synthesize_script_stream([Line(t, voice="anna")], voices, live_room=good, live_sends={"anna": 1.0})
    with pytest.raises(ValueError, match=r"\[-60, 0\]"):
        s.synthesize_script_stream([Line(t)], live_room=good, live_sends={0: math.nan})
    with pytest.raises(ValueError, match=r"\[-60, 0\]"):
        s.synthesize_script_stream([Line(t)], live_room=good, live_sends={0: True})


def test_the_script_plan_carries_the_live_sends():
    from fish_tts_amd.script import plan_script
    lines = [Line("One line is here.", voice="anna"), Line("Another line is here."), Line("A third line is here.", voice="anna")]
    plan = plan_script(lines, {"anna": []}, room=True, sends={"anna": -6.0, 2: -math.inf})
    assert plan.sends == [600, 0, -1]
