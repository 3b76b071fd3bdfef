"""fish_tts_amd.segments.join_chunks with `live_bed=`, without a GPU: on the fake codec of tests/test_segments_host.py and a
fake mix stream that puts `lead` samples in front, holds back `hold` samples and adds `tail` at the end.  The order of the
pushes, the empty first push whose output goes out before any group, the lock every push runs under, the marks a caller
shifts by `lead`, and close() - after the last chunk, on an abandoned generator, and when the feeding thread fails."""
import threading

import numpy as np
import pytest

import fish_tts_amd.segments as S
from tests.test_segments_host import LONG, MIXED, JoinCodec, _codes, _kw, _no_server, _plan

KINDS = pytest.mark.parametrize("refs", [LONG, MIXED], ids=["long", "script"])
BED_VALUE = np.float32(0.25)


def _pack(audio):
    return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()


class FakeMixStream:
    def __init__(self, log, lead, tail, hold, held):
        self.log, self.lead, self.tail, self.hold, self.held = log, lead, tail, hold, held
        self.buf = np.full(lead, BED_VALUE, dtype=np.float32)
        self.out, self.closed = 0, False

    def push(self, x=None, final=False):
        assert not self.closed
        x = np.zeros(0, dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32)
        self.log.append(("push", len(x), final, self.held.locked() if self.held is not None else None))
        self.buf = np.concatenate([self.buf, x] + ([np.full(self.tail, BED_VALUE, dtype=np.float32)] if final else []))
        end = len(self.buf) if final else max(self.out, len(self.buf) - self.hold)
        got, self.out = self.buf[self.out:end], end
        return got

    def close(self):
        self.log.append(("close", self.held.locked() if self.held is not None else None))
        self.closed = True


class MixCodec(JoinCodec):
    def __init__(self, held=None, lead=7, tail=3, hold=4):
        super().__init__(held)
        self.log, self.shape = [], (lead, tail, hold)

    def mix_stream(self, bed, sample_rate=None, params=None):
        self.log.append(("open", bed, sample_rate, params, self.held.locked() if self.held is not None else None))
        self.stream = FakeMixStream(self.log, *self.shape, self.held)
        return self.stream


def _expected(codes, lead, tail):
    prog = np.concatenate([np.asarray(c)[0].astype(np.float32) / 1e6 for c in codes])
    return _pack(np.concatenate([np.full(lead, BED_VALUE, dtype=np.float32), prog, np.full(tail, BED_VALUE, dtype=np.float32)]))


@KINDS
def test_the_pushes_in_order_and_the_head_before_any_group(refs):
    plan, codec, go = _plan(refs), MixCodec(), threading.Event()
    codes = [_codes(i, 3 + i) * 1000 for i in range(4)]

    def generate(emit, stopped):
        assert go.wait(10)                             # nothing is ready until the head went out
        emit(1, codes[1])
        emit(0, codes[0])
        emit(3, codes[3])
        emit(2, codes[2])
    seen = []
    gen = S.join_chunks(plan, **_kw(codec, None, _no_server, generate), on_cuts=lambda first, cuts: seen.append((first, len(cuts))),
                        live_bed=("clip", "params"))
    assert not codec.log                               # the stream is opened at the first next()
    head = next(gen)
    assert head == _pack(np.full(3, BED_VALUE, dtype=np.float32))      # lead 7, 4 held back
    assert codec.log[0][:4] == ("open", "clip", plan.rate, "params") and codec.log[1][:3] == ("push", 0, False) and not codec.joins
    go.set()
    chunks = [head] + list(gen)
    assert all(chunks) and b"".join(chunks) == _expected(codes, 7, 3)
    pushes = [e for e in codec.log if e[0] == "push"]
    assert [p[1] for p in pushes[1:-1]] == [sum(3 + i for i in range(f, f + j["n"])) for f, j in
                                            zip(np.cumsum([0] + [j["n"] for j in codec.joins]).tolist(), codec.joins)]
    assert pushes[-1][:3] == ("push", 0, True) and [p[2] for p in pushes[:-1]] == [False] * (len(pushes) - 1)
    assert codec.log[-1][0] == "close" and [e[0] for e in codec.log].count("close") == 1
    assert sum(n for _, n in seen) == 4


def test_marks_move_by_lead():
    """What synthesize_script_stream does with on_cuts: line_marks from `lead` on gives the plain marks plus lead."""
    from fish_tts_amd.script import line_marks
    cuts = [(2, 9), (0, 5), (4, 4), (1, 8)]
    line_of, gaps = [0, 0, 1, 2], [10, 20, 30, 40]
    plain, moved = [None] * 3, [None] * 3
    line_marks(line_of, gaps, cuts, plain, 0, False)
    at, started = line_marks(line_of[:2], gaps[:2], cuts[:2], moved, 441, False)      # two groups, as a stream reports them
    line_marks(line_of[2:], gaps[2:], cuts[2:], moved, at, started)
    assert moved == [(a + 441, b + 441) for a, b in plain]


def test_every_push_and_the_close_run_under_the_codec_lock():
    from tests.test_segments_host import _server
    from tests.test_serve_host import MovingEngine
    srv = _server(MovingEngine(max_batch=4))[0]
    try:
        codec = MixCodec(held=srv.codec_lock)
        plan = _plan(LONG)
        codes = [_codes(i, 4) * 1000 for i in range(4)]

        def serve(s):
            return [lambda c=c: c for c in codes], lambda cancel=False: None
        chunks = list(S.join_chunks(plan, **_kw(codec, srv, serve, None), live_bed=("clip", "params")))
        assert b"".join(chunks) == _expected(codes, 7, 3)
        assert all(j["locked"] for j in codec.joins)
        assert all(e[-1] is True for e in codec.log), codec.log
    finally:
        srv.close(cancel=True)


def test_an_abandoned_generator_closes_the_stream():
    plan, codec, go = _plan(LONG), MixCodec(), threading.Event()

    def generate(emit, stopped):
        emit(0, _codes(0, 9) * 1000)
        go.wait(10)
    gen = S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_bed=("clip", "params"))
    assert next(gen) and next(gen)                     # the head, then the first group's samples
    assert not codec.stream.closed
    go.set()
    gen.close()
    assert codec.stream.closed and codec.log[-1][0] == "close"
    assert not any(e[0] == "push" and e[2] for e in codec.log)      # no final push: the piece did not end


def test_a_failing_feeder_still_closes_the_stream():
    plan, codec = _plan(LONG), MixCodec(lead=0)

    def generate(emit, stopped):
        raise RuntimeError("the batch broke")
    gen = S.join_chunks(plan, **_kw(codec, None, _no_server, generate), live_bed=("clip", "params"))
    with pytest.raises(RuntimeError, match="the batch broke"):
        list(gen)
    assert codec.stream.closed


def test_without_a_live_bed_nothing_is_opened():
    plan, codec = _plan(LONG), MixCodec()
    codes = [_codes(i, 3) * 1000 for i in range(4)]

    def generate(emit, stopped):
        for i, c in enumerate(codes):
            emit(i, c)
    chunks = list(S.join_chunks(plan, **_kw(codec, None, _no_server, generate)))
    assert not codec.log and b"".join(chunks) == b"".join(_pack(np.asarray(c)[0].astype(np.float32) / 1e6) for c in codes)
