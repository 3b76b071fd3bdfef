"""`live_stereo=` without a GPU: script.push_regions - the regions segments.join_chunks hands to each push of a stereo mix
stream - on a fake codec whose join lays the pieces out by the join's own rule (gaps behind the first audio, empty pieces) and
a fake stereo stream that records its pushes: lines that cross group boundaries, a line without audio, neighbouring lines of
equal pan; concatenated and shifted back the regions are pan_regions of the final marks.  Then the refusals of the two public
calls, each before any device work, and the stream closed when the generator is abandoned."""
import itertools
import threading

import numpy as np
import pytest

import fish_tts_amd.segments as S
from fish_tts_amd.script import Line, line_marks, pan_regions, push_regions
from tests.test_segments_host import JoinCodec, _kw, _no_server


def _pack(audio):
    return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()


class FakeStereoStream:
    def __init__(self, log, lead, tail, hold):
        self.log, self.tail, self.hold = log, tail, hold
        self.buf = np.full((lead, 2), 0.25, dtype=np.float32)
        self.q = np.zeros(0, dtype=np.int64)               # the pan of every programme sample pushed so far
        self.out, self.closed = 0, False

    def push(self, x=None, regions=(), final=False):
        assert not self.closed
        x = np.zeros(0, dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32)
        regions = [tuple(r) for r in regions]
        self.log.append(("push", len(x), regions, final))
        at, q = 0, np.zeros(len(x), dtype=np.int64)
        for a, e, pan in regions:                          # the stage's own rule for one push
            assert at <= a < e <= len(x) and -100 <= pan <= 100 and pan != 0, (regions, len(x))
            q[a:e], at = pan, e
        self.q = np.concatenate([self.q, q])
        self.buf = np.concatenate([self.buf, np.stack([x, q / 1000.0], 1).astype(np.float32)] +
                                  ([np.full((self.tail, 2), 0.25, dtype=np.float32)] if final else []))
        end = len(self.buf) if final else max(self.out, len(self.buf) - self.hold)
        got, self.out = self.buf[self.out:end], end
        return got

    def close(self):
        self.log.append(("close",))
        self.closed = True


class GapCodec(JoinCodec):
    """decode_join by the join's layout rule: piece b is row 0 of its codes / 1e6 (nothing where the row is empty), behind
    gaps[b] zeros once audio has gone out."""

    def __init__(self, lead=0, tail=0, hold=0):
        super().__init__()
        self.log, self.shape = [], (lead, tail, hold)

    def decode_join(self, group, params=None, gaps=None, started=False, fx=None, item_fx=None):
        self.joins.append(dict(n=len(group), gaps=list(gaps), started=started))
        out, cuts = [], []
        for c, g in zip(group, gaps):
            row = np.asarray(c)[0].astype(np.float32) / 1e6
            cuts.append((0, len(row)))
            if len(row):
                out += ([np.zeros(int(g), dtype=np.float32)] if started else []) + [row]
                started = True
        return (np.concatenate(out) if out else np.zeros(0, dtype=np.float32)), np.array(cuts, dtype=np.int64).reshape(-1, 2)

    def mix_stream(self, bed, sample_rate=None, params=None, stereo=False):
        self.log.append(("open", bed, sample_rate, params, stereo))
        self.stream = FakeStereoStream(self.log, *self.shape)
        return self.stream


def _codes(i, n):
    return np.full((10, n), 1000 * (i + 1), dtype=np.int32)


def _merged(regions):
    out = []
    for a, e, q in regions:
        if out and out[-1][1] == a and out[-1][2] == q:
            out[-1] = (out[-1][0], e, q)
        else:
            out.append((a, e, q))
    return out


def _stream(plan, codes, order, codec, live_bed=None):
    """The chunks of one stereo stream whose segments complete in `order` (how they fall into groups is the feeder's timing:
    what the tests assert holds for every grouping)."""
    def generate(emit, stopped):
        for i in order:
            emit(i, codes[i])
    return list(S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_bed=live_bed, live_stereo=True))


# line:      0        1     2 (no audio)   3        3        4
LINE_OF = [0, 0, 0, 1, 2, 3, 3, 4]
SIZES = [5, 7, 4, 6, 0, 3, 8, 5]
GAPS = [10, 2, 3, 9, 4, 6, 1, 7]
PANS = [-50, -50, 30, 30, 0]           # lines 0 and 1 at one place; line 2 (silent) separates nothing; line 3; the centre


def _script_plan(pans=PANS):
    n = len(LINE_OF)
    return S.SegmentPlan([str(i + 1) for i in range(n)], [None] * n, list(GAPS), (0.5, 4, 2, 1), 44100, [f"fx{i}" for i in range(n)],
                         list(LINE_OF), max(LINE_OF) + 1, list(pans))


def _whole(pans=PANS):
    """(the whole piece's marks, pan_regions of them, its length) by the one-shot rule."""
    cuts = [(0, k) for k in SIZES]
    found = [None] * (max(LINE_OF) + 1)
    at, _ = line_marks(LINE_OF, GAPS, cuts, found)
    return found, pan_regions(pans, found), at


def test_every_grouping_of_the_segments_gives_the_one_shot_regions():
    """All 128 ways to cut the eight segments into groups: the regions of the pushes, shifted back and joined where they
    touch at one pan, are pan_regions of the whole piece's marks; each lies inside its push."""
    found, want, total = _whole()
    assert want == [(0, found[1][1], -50), (found[3][0], found[3][1], 30)]      # lines 0 + 1 merged; line 2 gave nothing
    for mask in range(128):
        bounds = [0] + [b for b in range(1, 8) if mask >> (b - 1) & 1] + [8]
        back, place = [], (0, False, 0)
        for first, end in zip(bounds, bounds[1:]):
            at = place[0]
            regions, *place = push_regions(PANS, LINE_OF[first:end], GAPS[first:end], [(0, k) for k in SIZES[first:end]], *place)
            n = place[0] - at
            assert all(0 <= a < e <= n for a, e, _ in regions), (bounds, first, regions)
            assert all(e1 <= a2 for (_, e1, _), (a2, _, _) in zip(regions, regions[1:]))
            # a line that continues from the group before: its gap is covered by the continued region
            if first > 0 and LINE_OF[first] == LINE_OF[first - 1] and PANS[LINE_OF[first]] != 0 and SIZES[first] > 0 and at > 0:
                assert regions[0][0] == 0 and regions[0][2] == PANS[LINE_OF[first]], (bounds, first, regions)
            back += [(a + at, e + at, q) for a, e, q in regions]
        assert place[0] == total and _merged(back) == want, (bounds, back)


@pytest.mark.parametrize("order", [list(range(8)), [1, 0, 3, 2, 7, 6, 5, 4], [7, 6, 5, 4, 3, 2, 1, 0]],
                         ids=["in-order", "pairs", "last-first"])
def test_join_chunks_pushes_every_group_with_its_regions(order):
    plan, codec = _script_plan(), GapCodec()
    codes = [_codes(i, k) for i, k in enumerate(SIZES)]
    chunks = _stream(plan, codes, order, codec)
    found, want, total = _whole()
    pushes = [e for e in codec.log if e[0] == "push"]
    assert pushes[0][1:] == (0, [], False) and pushes[-1][1:] == (0, [], True)
    assert codec.log[0] == ("open", None, plan.rate, None, True) and codec.log[-1] == ("close",)
    back, at = [], 0
    for _, n, regions, _ in pushes[1:-1]:
        back += [(a + at, e + at, q) for a, e, q in regions]
        at += n
    assert at == total and _merged(back) == want
    q = np.zeros(total, dtype=np.int64)
    for a, e, pan in want:
        q[a:e] = pan
    assert codec.stream.q.tolist() == q.tolist()                                # every sample went in with the one-shot pan
    pcm = b"".join(chunks)
    assert all(chunks) and len(pcm) == 4 * total                                # interleaved int16, no empty chunk
    frames = np.frombuffer(pcm, dtype=np.int16).reshape(-1, 2)
    assert frames[:, 1].tobytes() == _pack((q / 1000.0).astype(np.float32))    # the fake's right channel: the pans it was given


def test_a_line_without_audio_and_neighbours_of_equal_pan():
    # one group per segment: line 1 (pan -50 as line 0) begins a group - its region starts with the push, over its gap;
    # line 2 has no audio: nothing is pushed for it; line 3 (pan 30 as line 2, which was never heard) follows line 1's -50:
    # its region begins behind its gap
    regions, at, started, before = [], 0, False, 0
    for b in range(8):
        r, at2, started, before = push_regions(PANS, LINE_OF[b:b + 1], GAPS[b:b + 1], [(0, SIZES[b])], at, started, before)
        regions.append(r)
        n, at = at2 - at, at2
        if b == 0:
            assert r == [(0, 5, -50)] and n == 5                 # the first audio: no gap in front
        if b == 3:
            assert r == [(0, GAPS[3] + 6, -50)] and n == GAPS[3] + 6      # another line, the same place: the gap goes along
        if b == 4:
            assert r == [] and n == 0 and before == -50          # no audio: no region, and it separates nothing
        if b == 5:
            assert r == [(GAPS[5], GAPS[5] + 3, 30)]             # a new place: behind the gap
        if b == 6:
            assert r == [(0, GAPS[6] + 8, 30)]                   # the same line goes on
        if b == 7:
            assert r == [] and before == 0                       # the centre: no region
    # centred lines between two lines at one place separate them, as in pan_regions
    r1, at, st, bf = push_regions([20, 0, 20], [0], [5], [(0, 4)])
    r2, at, st, bf = push_regions([20, 0, 20], [1], [5], [(0, 4)], at, st, bf)
    r3, at, st, bf = push_regions([20, 0, 20], [2], [5], [(0, 4)], at, st, bf)
    assert (r1, r2, r3) == ([(0, 4, 20)], [], [(5, 9, 20)])


def test_with_a_live_bed_the_head_goes_out_first_and_marks_move_by_lead():
    plan, codec = _script_plan(), GapCodec(lead=9, tail=2, hold=4)
    codes = [_codes(i, k) for i, k in enumerate(SIZES)]
    chunks = _stream(plan, codes, [1, 0, 2, 3, 4, 5, 6, 7], codec, live_bed=("clip", "params"))
    assert codec.log[0] == ("open", "clip", plan.rate, "params", True)
    assert chunks[0] == _pack(np.full((5, 2), 0.25, dtype=np.float32))          # lead 9, 4 held back: the bed alone, in stereo
    total = _whole()[2]
    assert len(b"".join(chunks)) == 4 * (9 + total + 2)
    # the regions are the programme's: they do not move by the lead (the stage places the programme behind it)
    back, at = [], 0
    for _, n, regions, _ in [e for e in codec.log if e[0] == "push"][1:-1]:
        back += [(a + at, e + at, q) for a, e, q in regions]
        at += n
    assert _merged(back) == _whole()[1]


def test_a_long_text_is_one_line_at_its_place():
    n = 4
    plan = S.SegmentPlan([str(i + 1) for i in range(n)], [None] * n, [10, 20, 30, 40], (0.5, 4, 2, 1), 44100, "fx", pans=[-50])
    codec = GapCodec()
    codes = [_codes(i, 3 + i) for i in range(n)]
    _stream(plan, codes, [1, 0, 3, 2], codec)
    pushes = [e for e in codec.log if e[0] == "push"][1:-1]
    assert [p[2] for p in pushes] == [[(0, p[1], -50)] for p in pushes] and len(pushes) >= 1     # every push whole, gaps included
    codec = GapCodec()
    _stream(plan._replace(pans=[0]), codes, [0, 1, 2, 3], codec)
    assert all(p[2] == [] for p in codec.log if p[0] == "push")
    with pytest.raises(ValueError, match="pans"):
        next(S.join_chunks(plan._replace(pans=None), **_kw(GapCodec(), None, _no_server, lambda emit, stopped: None), live_stereo=True))


def test_an_abandoned_generator_closes_the_stream():
    plan, codec, go = _script_plan(), GapCodec(), threading.Event()

    def generate(emit, stopped):
        emit(0, _codes(0, 9))
        go.wait(10)
    gen = S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_stereo=True)
    assert next(gen)
    assert not codec.stream.closed
    go.set()
    gen.close()
    assert codec.stream.closed and codec.log[-1] == ("close",)
    assert not any(e[0] == "push" and e[3] for e in codec.log)                  # no final push: the piece did not end


class NoDevice:
    """A vocoder that fails the test when anything reaches it."""

    def __getattr__(self, name):
        raise AssertionError(f"device work before the refusal: {name}")


def _synth():
    from fish_tts_amd.synthesizer import FishTTS
    s = object.__new__(FishTTS)                            # no engines: every refusal comes before the first use of any
    s._vocoder = NoDevice()
    s._prefix_cache = None
    return s


def test_refusals_before_any_device_work():
    s, t = _synth(), "Some text is here."
    voices = {"anna": []}
    with pytest.raises(ValueError, match="live_pans needs live_stereo"):
        s.synthesize_script_stream([Line(t, voice="anna")], voices, live_pans={"anna": 0.5})
    with pytest.raises(ValueError, match="live_pans needs live_stereo"):
        s.synthesize_script_stream([Line(t)], live_pans={})
    with pytest.raises(ValueError, match="stereo"):                             # a Line.pan on a mono stream: as it was
        s.synthesize_script_stream([Line(t, pan=0.5)])
    with pytest.raises(ValueError, match="live_stereo must be"):
        s.synthesize_script_stream([Line(t)], live_stereo=1)
    with pytest.raises(ValueError, match="no voice"):
        s.synthesize_script_stream([Line(t)], live_stereo=True, live_pans={"carl": 0.5})
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        s.synthesize_script_stream([Line(t, pan=1.5)], live_stereo=True)
    with pytest.raises(ValueError, match="live_pan=0.5 needs live_stereo"):
        s.synthesize_long_stream(t, live_pan=0.5)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        s.synthesize_long_stream(t, live_stereo=True, live_pan=-1.01)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        s.synthesize_long_stream(t, live_pan=float("nan"))
    with pytest.raises(ValueError, match="live_stereo must be"):
        s.synthesize_long_stream(t, live_stereo="yes")
    for call, arg in ((s.synthesize_long_stream, t), (s.synthesize_script_stream, [Line(t)])):
        for kw in (dict(stereo=True), dict(pan=0.5), dict(pans={})):           # the one-shot keywords stay unknown to the streams
            with pytest.raises(TypeError):
                call(arg, **kw)
        with pytest.raises(ValueError, match="live_bed"):                       # bed= on a stream stays refused
            call(arg, bed=object(), live_stereo=True)


def test_the_engine_judges_regions_before_any_device_work():
    from fish_tts_amd.codec_engine import MAX_PAN_REGIONS, pan_region_table
    reg, R = pan_region_table("t", [(0, 3, -100), (3, 4, 100)], 4)
    assert R == 2 and (reg[1].a, reg[1].e, reg[1].pan) == (3, 4, 100)
    assert pan_region_table("t", [], 0)[1] == 0
    for bad, n in (([(0, 5, 0)], 4), ([(2, 2, 0)], 4), ([(0, 2, 0), (1, 3, 0)], 4), ([(0, 1, 101)], 4), ([(0, 1, 0)], 0),
                   ([(0, 1.0, 0)], 4), ([(0, 1, True)], 4), ([(0, 1)], 4)):
        with pytest.raises(ValueError):
            pan_region_table("t", bad, n)
    with pytest.raises(ValueError, match="4097 pan regions"):
        pan_region_table("t", [(i, i + 1, 0) for i in range(MAX_PAN_REGIONS + 1)], 5000)
    assert len(list(itertools.islice(pan_region_table("t", [(i, i + 1, 1) for i in range(MAX_PAN_REGIONS)], 4096)[0], 3))) == 3
