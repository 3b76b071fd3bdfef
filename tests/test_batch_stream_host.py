"""fish_tts_amd.batch_stream without a GPU: run_batch on the fake engine of the scheduler tests, a fake codec that records
its calls - chunking, the held-back column, end marks, one chunk per utterance per codec call, shutdown and errors."""
import threading
import time

import numpy as np
import pytest

from tests.test_host_logic import FakeEngine, _fake_utt


class FakeStream:
    def __init__(self, codec):
        self.codec, self.frames, self.closed = codec, 0, False
        codec.opened.append(self)

    def close(self):
        self.closed = True


class FakeCodec:
    """decode_streams returns, per chunk, its codes row 0 as float samples / 1e6 (one sample per frame)."""
    max_frames = 10_000

    def __init__(self, delay=0.0, fail_at=None):
        self.calls, self.opened, self.delay, self.fail_at = [], [], delay, fail_at

    def stream(self, fx=None):
        return FakeStream(self)

    def decode_streams(self, streams, chunks, final=None):
        assert len(set(map(id, streams))) == len(streams)
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError("codec failed")
        self.calls.append([(s, c.shape[1]) for s, c in zip(streams, chunks)])
        time.sleep(self.delay)
        out = []
        for s, c in zip(streams, chunks):
            s.frames += c.shape[1]
            out.append(c[0].astype(np.float32) / 1e6)
        return out


def _runner(eng, utts, burst=8):
    from fish_tts_amd.batch import run_batch

    def run(on_frames, on_done):
        run_batch(eng, utts, burst=burst, on_frames=on_frames, on_done=on_done)
    return run


def _pcm(codes_row):
    return (np.asarray(codes_row, dtype=np.float32) / 1e6 * 32767).astype(np.int16).tobytes()


def test_chunks_holdback_and_end_marks():
    from fish_tts_amd.batch_stream import stream_utterances
    eng = FakeEngine()
    budgets = [40, 23, 1, 12, 11]
    utts = [_fake_utt(i + 1, b) for i, b in enumerate(budgets)] + [_fake_utt(9, 30, eos_at=17)]
    codec = FakeCodec()
    items = list(stream_utterances(_runner(eng, utts), len(utts), codec, chunk_tokens=7, min_first_chunk=5))
    by = {i: [p for j, p in items if j == i] for i in range(len(utts))}
    for i, u in enumerate(utts):
        assert by[i][-1] == b"" and by[i].count(b"") == 1                  # one end mark, after the last chunk
        codes = u.codes()                                                  # what synthesize_batch decodes
        n = codes.shape[1]
        want = [5] + [7] * max(0, (n - 5) // 7) if n >= 5 else []
        rest = n - sum(want)
        if rest:
            want.append(rest)
        lens = [len(p) // 2 for p in by[i][:-1]]
        assert lens == want, (i, lens, n)
        assert b"".join(by[i][:-1]) == _pcm(codes[0])                        # the codes, in order, the last column held back
    assert by[2] == [b""]                                                  # one frame generated: no codes, the end mark only
    # at most one chunk per utterance per call; a stream per utterance, all ended
    for call in codec.calls:
        assert len({id(s) for s, _ in call}) == len(call)
    assert all(s.closed for s in codec.opened) and len(codec.opened) == len(utts) - 1


def test_chunks_ready_together_share_one_call():
    """A burst of 8 frames for three utterances cuts several chunks each: every call takes one chunk of every utterance
    that has one ready, so the first call holds all three."""
    from fish_tts_amd.batch_stream import stream_utterances
    eng = FakeEngine()
    utts = [_fake_utt(i + 1, 30) for i in range(3)]
    gate = threading.Event()

    def run(on_frames, on_done):
        from fish_tts_amd.batch import run_batch
        collected = []
        run_batch(eng, utts, burst=30, on_frames=lambda i, b: collected.append((i, b)), on_done=lambda i: collected.append((i, None)))
        for i, b in collected:                                            # everything arrives before the codec first wakes
            on_frames(i, b) if b is not None else on_done(i)
        gate.set()
    codec = FakeCodec()
    items = list(stream_utterances(run, 3, codec, chunk_tokens=4, min_first_chunk=2))
    assert gate.is_set()
    assert [len(c) for c in codec.calls][:1] == [3]
    lens = [[n for s, n in c] for c in codec.calls]
    assert lens[0] == [2, 2, 2] and all(len(c) == 3 for c in codec.calls)  # equal budgets: every round holds all three
    assert sum(1 for _, p in items if p == b"") == 3


def test_early_close_stops_the_producer_and_joins():
    from fish_tts_amd.batch_stream import stream_utterances
    eng = FakeEngine()
    eng.max_new_tokens = 10_000
    utts = [_fake_utt(i + 1, 10_000) for i in range(3)]
    codec = FakeCodec()
    before = threading.active_count()
    gen = stream_utterances(_runner(eng, utts, burst=4), 3, codec, chunk_tokens=4, min_first_chunk=4)
    got = [next(gen) for _ in range(5)]
    assert all(p for _, p in got)
    gen.close()
    assert threading.active_count() == before                              # both threads joined
    steps = sum(eng.widths) if eng.widths else 0
    time.sleep(0.05)
    assert sum(eng.widths) == steps                                         # the producer stopped
    assert len(eng.widths) * 4 < 10_000
    assert all(s.closed for s in codec.opened)


def test_errors_are_raised_from_the_generator():
    from fish_tts_amd.batch_stream import stream_utterances
    eng = FakeEngine()
    utts = [_fake_utt(i + 1, 30) for i in range(3)]
    with pytest.raises(RuntimeError, match="codec failed"):
        list(stream_utterances(_runner(eng, utts), 3, FakeCodec(fail_at=1), chunk_tokens=4, min_first_chunk=4))

    def bad_run(on_frames, on_done):
        on_frames(0, np.zeros((11, 6), dtype=np.int32))
        raise ValueError("generation failed")
    codec = FakeCodec()
    with pytest.raises(ValueError, match="generation failed"):
        list(stream_utterances(bad_run, 2, codec))
    assert all(s.closed for s in codec.opened)
