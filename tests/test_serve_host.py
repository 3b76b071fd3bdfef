"""fish_tts_amd.serve without a GPU: BatchServer on the fake engine of the scheduler tests (given a move_slot) and the fake
codec of the batch-stream tests - admission order, the compaction moves, width and padding, cancellation, errors, an idle
server, close."""
import threading
import time

import numpy as np
import pytest

from tests.test_batch_stream_host import FakeCodec, _pcm
from tests.test_host_logic import FakeEngine, _fake_utt


class MovingEngine(FakeEngine):
    """FakeEngine with move_slot; `gate` (an Event) holds every decode until set; `fail_at`: that decode call raises."""
    max_batch = 4

    def __init__(self, max_batch=4, path="", gate=None, fail_at=None):
        super().__init__()
        self.max_batch, self.path, self.gate, self.fail_at = max_batch, path, gate, fail_at
        self.moves = []

    def frame_path(self):
        return self.path

    def move_slot(self, src, dst):
        assert src != dst and src in self.slot_utt
        self.moves.append((src, dst))
        self.slot_utt[dst], self.count[dst] = self.slot_utt.pop(src), self.count[src]

    def decode(self, k, sps, poll):
        if self.gate is not None:
            assert self.gate.wait(10)
        if self.fail_at is not None and len(self.widths) == self.fail_at:
            raise RuntimeError("device lost")
        return super().decode(k, sps, poll)


EOS = {}     # uid -> frame count at which the fake engine draws <|im_end|>


def _prepare(text, references, temperature, top_p, repetition_penalty, max_tokens, seed):
    uid = int(text)
    return _fake_utt(uid, max_tokens, eos_at=EOS.get(uid, 0)), 0


def _wav(codes, fx=None):
    return np.ascontiguousarray(codes[0], dtype=np.int32).tobytes()


def _plain(codes, fx=None):
    return b"P" + np.ascontiguousarray(codes[0], dtype=np.int32).tobytes()


def _server(eng, burst=4, codec=None, on_close=None):
    from fish_tts_amd.serve import BatchServer
    return BatchServer(eng, codec or FakeCodec(), burst, prepare=_prepare, decode_wav=_wav, decode_pcm=_plain,
                       on_close=on_close)


def _frames(uid, n):
    """Row 0 of the fake engine's first n frames of utterance uid."""
    return np.array([1000 * uid + c for c in range(1, n + 1)], dtype=np.int32)


def _wait(cond, timeout=10.0):
    t = time.time()
    while not cond():
        assert time.time() - t < timeout, "timed out"
        time.sleep(0.002)


def test_compaction_moves_and_width_rule():
    from fish_tts_amd.serve import compaction_moves, lockstep_width
    assert compaction_moves([]) == [] and compaction_moves([0, 1, 2]) == []
    assert compaction_moves([11]) == [(11, 0)]
    assert compaction_moves([0, 7, 19]) == [(19, 1), (7, 2)]
    assert compaction_moves([2, 1]) == [(2, 0)]
    assert compaction_moves([0, 2, 3, 5]) == [(5, 1)]
    # run_batch's rule: 2..4 rows ride up to 5 where the MFMA launches exist (wide_from = 5 <= B); otherwise the width is n
    assert [lockstep_width(n, 32, 5) for n in (1, 2, 3, 4, 5, 9)] == [1, 5, 5, 5, 5, 9]
    assert [lockstep_width(n, 4, 5) for n in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [lockstep_width(n, 8, 9) for n in (1, 3, 8)] == [1, 3, 8]


def test_admission_first_come_first_served_into_the_lowest_slots():
    gate = threading.Event()
    eng = MovingEngine(gate=gate)
    with _server(eng) as srv:
        out = {}
        t0 = threading.Thread(target=lambda: out.__setitem__(1, srv.synthesize("1", max_tokens=20)))
        t0.start()
        _wait(lambda: eng.prefills)                         # 1 is in slot 0, its first burst waits at the gate
        reqs = {}
        for uid in (2, 3, 4, 5, 6):
            reqs[uid] = srv.submit(*_prepare(str(uid), None, 0.7, 0.8, 1.1, 6 + uid, 0))
        gate.set()
        t0.join()
        for uid, r in reqs.items():
            out[uid] = r.out.get(timeout=10)
    assert [p for p in eng.prefills[:4]] == [(1, 0), (2, 1), (3, 2), (4, 3)]
    assert [uid for uid, _ in eng.prefills[4:]] == [5, 6]  # then in arrival order as slots free up
    budgets = {1: 20, 2: 8, 3: 9, 4: 10, 5: 11, 6: 12}
    for uid, n in budgets.items():
        assert out[uid] == _wav(_frames(uid, n - 1)[None]), uid   # Utterance.codes(): the last column dropped
    s = srv.stats()
    assert s["admitted"] == 6 and s["completed"] == 6 and s["cancelled"] == 0


def test_compaction_moves_a_lone_survivor_to_slot_zero():
    gate = threading.Event()
    eng = MovingEngine(gate=gate)
    with _server(eng) as srv:
        long_ = srv.submit(*_prepare("3", None, 0.7, 0.8, 1.1, 30, 0))
        _wait(lambda: eng.prefills)
        a = srv.submit(*_prepare("1", None, 0.7, 0.8, 1.1, 9, 0))
        b = srv.submit(*_prepare("2", None, 0.7, 0.8, 1.1, 9, 0))
        gate.set()
        got = [r.out.get(timeout=10) for r in (long_, a, b)]
    assert got[0] == _wav(_frames(3, 29)[None])
    assert eng.moves == []                                        # the longest request holds slot 0: no hole ever opens
    # the other order: 3 lands in slot 2 behind two shorter requests
    gate = threading.Event()
    eng = MovingEngine(gate=gate)
    with _server(eng) as srv:
        a = srv.submit(*_prepare("1", None, 0.7, 0.8, 1.1, 9, 0))
        _wait(lambda: eng.prefills)
        b = srv.submit(*_prepare("2", None, 0.7, 0.8, 1.1, 9, 0))
        long_ = srv.submit(*_prepare("3", None, 0.7, 0.8, 1.1, 30, 0))
        gate.set()
        got = [r.out.get(timeout=10) for r in (a, b, long_)]
        s = srv.stats()
    assert eng.prefills[:3] == [(1, 0), (2, 1), (3, 2)]
    assert eng.moves == [(2, 0)] and s["slot_moves"] == 1        # 1 ends first: 3 moves from slot 2 into slot 0
    assert got[2] == _wav(_frames(3, 29)[None])                   # its frames go on counting across the move
    assert eng.widths[-1] == 1 and s["steps_by_width"][1] > 0 and 3 in s["steps_by_width"]
    assert sum(k for k in s["steps_by_width"].values()) > 0


def test_mfma_padding_rule_and_parked_rows():
    gate = threading.Event()
    eng = MovingEngine(max_batch=8, path="launch path; lock-step batches of >= 5 rows: MFMA launches", gate=gate)
    with _server(eng, burst=4) as srv:
        reqs = [srv.submit(*_prepare("1", None, 0.7, 0.8, 1.1, 14, 0))]
        _wait(lambda: eng.prefills)
        reqs += [srv.submit(*_prepare(str(u), None, 0.7, 0.8, 1.1, 14, 0)) for u in (2, 3)]
        gate.set()
        for r in reqs:
            r.out.get(timeout=10)
        s = srv.stats()
    assert eng.widths[0] == 1 and set(eng.widths[1:]) == {5}   # three rows run five wide (two parked rows ride along)
    assert set(s["steps_by_width"]) == {1, 5}
    assert {3, 4} <= set(eng.parked)


def test_streams_seamless_and_plain_chunks():
    eng = MovingEngine()
    codec = FakeCodec()
    with _server(eng, codec=codec) as srv:
        seam = list(srv.synthesize_stream("1", chunk_tokens=4, min_first_chunk=3, seamless=True, max_tokens=14))
        plain = list(srv.synthesize_stream("2", chunk_tokens=4, min_first_chunk=3, max_tokens=14))
    codes = _frames(1, 13)                                        # held back: the last generated column
    assert [len(p) // 2 for p in seam] == [3, 4, 4, 2] and b"".join(seam) == _pcm(codes)
    cols = _frames(2, 14)                                         # every column, each chunk decoded on its own
    assert plain == [_plain(cols[None, a:b]) for a, b in ((0, 3), (3, 7), (7, 11), (11, 14))]
    assert all(s.closed for s in codec.opened) and len(codec.opened) == 1


def test_a_dropped_stream_frees_its_slot_at_the_next_boundary():
    eng = MovingEngine()
    eng.max_new_tokens = 100_000
    codec = FakeCodec()
    with _server(eng, codec=codec) as srv:
        gen = srv.synthesize_stream("1", chunk_tokens=4, min_first_chunk=4, seamless=True, max_tokens=100_000)
        assert next(gen)
        gen.close()
        _wait(lambda: srv.stats()["active"] == 0)
        n = len(eng.widths)
        assert srv.stats()["cancelled"] == 1 and 0 in eng.parked
        assert srv.synthesize("2", max_tokens=5) == _wav(_frames(2, 4)[None])   # the slot serves the next request
        assert eng.prefills[-1] == (2, 0)
    assert len(eng.widths) < n + 5 and all(s.closed for s in codec.opened)


def test_an_idle_server_makes_no_decode_calls():
    eng = MovingEngine()
    with _server(eng) as srv:
        time.sleep(0.1)
        assert eng.widths == [] and eng.prefills == [] and sorted(eng.parked) == [0, 1, 2, 3]
        srv.synthesize("1", max_tokens=6)
        n = len(eng.widths)
        time.sleep(0.1)
        assert len(eng.widths) == n


def test_an_error_reaches_every_waiter_and_closes_the_server():
    gate = threading.Event()
    eng = MovingEngine(gate=gate, fail_at=1)
    closed = []
    srv = _server(eng, on_close=closed.append)
    errors = []

    def call(uid, stream):
        try:
            if stream:
                list(srv.synthesize_stream(str(uid), chunk_tokens=2, min_first_chunk=2, max_tokens=30))
            else:
                srv.synthesize(str(uid), max_tokens=30)
        except RuntimeError as e:
            errors.append(str(e))
    threads = [threading.Thread(target=call, args=(u, u % 2 == 0)) for u in range(1, 8)]   # 7 requests, 4 slots: some queue
    for t in threads:
        t.start()
    _wait(lambda: srv.stats()["queued"] + srv.stats()["active"] == 7)
    gate.set()
    for t in threads:
        t.join(10)
        assert not t.is_alive()
    assert errors == ["device lost"] * 7
    _wait(lambda: closed == [srv])
    from fish_tts_amd.serve import ServerClosed
    with pytest.raises(ServerClosed):
        srv.synthesize("9")
    srv.close()
    assert closed == [srv]


def test_close_finishes_or_cancels():
    gate = threading.Event()
    eng = MovingEngine(gate=gate)
    closed = []
    srv = _server(eng, on_close=closed.append)
    before = threading.active_count()
    reqs = [srv.submit(*_prepare(str(u), None, 0.7, 0.8, 1.1, 12, 0)) for u in range(1, 7)]   # six: two wait in the queue
    t = threading.Thread(target=srv.close)
    t.start()
    time.sleep(0.05)
    from fish_tts_amd.serve import ServerClosed
    with pytest.raises(ServerClosed):
        srv.submit(*_prepare("9", None, 0.7, 0.8, 1.1, 12, 0))    # no admission once closing
    gate.set()
    t.join(10)
    assert [r.out.get(timeout=1) for r in reqs] == [_wav(_frames(u, 11)[None]) for u in range(1, 7)]
    assert closed == [srv] and threading.active_count() <= before - 2
    srv.close()
    assert closed == [srv]
    # cancel=True: the callers get an error at once, nothing hangs
    gate = threading.Event()
    eng = MovingEngine(gate=gate)
    srv = _server(eng)
    reqs = [srv.submit(*_prepare(str(u), None, 0.7, 0.8, 1.1, 12, 0)) for u in range(1, 7)]
    _wait(lambda: eng.prefills)
    threading.Timer(0.05, gate.set).start()
    srv.close(cancel=True)
    outs = [r.out.get(timeout=1) for r in reqs]
    assert all(type(o).__name__ == "_Failed" and "cancelled" in str(o.error) for o in outs)
    s = srv.stats()
    assert s["cancelled"] == 6 and s["completed"] == 0


def _run_threads(fns, timeout=10.0):
    threads = [threading.Thread(target=f, daemon=True) for f in fns]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
        assert not t.is_alive(), "a caller hangs"


@pytest.mark.parametrize("where", ["wav", "streams"])
def test_a_codec_error_reaches_every_waiter(where):
    """The codec worker fails (a WAV decode, or the batched stream decode): every caller gets the error, none hangs."""
    from fish_tts_amd.serve import BatchServer

    def bad_wav(codes, fx=None):
        raise RuntimeError("codec failed")
    gate = threading.Event()
    eng = MovingEngine(gate=gate)
    closed = []
    codec = FakeCodec(fail_at=0 if where == "streams" else None)
    srv = BatchServer(eng, codec, 4, prepare=_prepare, decode_wav=bad_wav if where == "wav" else _wav,
                      decode_pcm=_plain, on_close=closed.append)
    errors = []

    def wav(uid):
        def f():
            try:
                srv.synthesize(str(uid), max_tokens=6)
            except RuntimeError as e:
                errors.append(str(e))
        return f

    def stream(uid, seamless):
        def f():
            try:
                list(srv.synthesize_stream(str(uid), chunk_tokens=2, min_first_chunk=2, seamless=seamless, max_tokens=40))
            except RuntimeError as e:
                errors.append(str(e))
        return f
    fns = [wav(1), wav(2), stream(3, True), stream(4, False), wav(5)]
    threading.Timer(0.1, gate.set).start()
    _run_threads(fns)
    assert errors == ["codec failed"] * 5
    _wait(lambda: closed == [srv])


class _Prefix:
    def __init__(self, n_pos):
        self.handle, self.n_pos = True, n_pos

    def free(self):
        self.handle = None


class VoiceEngine(MovingEngine):
    """build_prefix / restore semantics: a prompt pass that restores a freed prefix fails, as ARHipEngine.kv_restore does."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.built, self.groups = [], []

    def build_prefix(self, cols, slot=0):
        self.built.append((int(cols[2, 0]), slot))
        return _Prefix(cols.shape[1])

    def prefill_many(self, prompts, sps, slots, prefixes):
        for pf in prefixes:
            if pf is not None and not pf.handle:
                raise ValueError("KV prefix belongs to another engine or was freed")
        self.groups.append(list(slots))
        return super().prefill_many(prompts, sps, slots, prefixes)


def test_more_voices_in_one_admission_than_the_prefix_cache_holds():
    from fish_tts_amd.generation import PrefixCache
    from fish_tts_amd.serve import BatchServer

    def prepare(text, references, temperature, top_p, repetition_penalty, max_tokens, seed):
        uid, voice = (int(v) for v in text.split(":"))
        utt = _fake_utt(uid, max_tokens)
        utt.prompt[2, :2] = voice                       # the first two columns: the voice's prefix
        return utt, 2 if voice else 0
    gate = threading.Event()
    eng = VoiceEngine(max_batch=8, gate=gate)
    srv = BatchServer(eng, FakeCodec(), 4, prepare=prepare, decode_wav=_wav, decode_pcm=_plain,
                      prefix_cache=PrefixCache(capacity=2, min_positions=2))
    with srv:
        first = srv.submit(*prepare("1:0", None, 0.7, 0.8, 1.1, 12, 0))
        _wait(lambda: eng.prefills)                     # slot 0 busy, its burst waits: the rest arrive together
        plan = [(2, 1), (3, 2), (4, 3), (5, 1), (6, 4)]
        reqs = [srv.submit(*prepare(f"{u}:{v}", None, 0.7, 0.8, 1.1, 9, 0)) for u, v in plan]
        gate.set()
        outs = [r.out.get(timeout=10) for r in [first] + reqs]
    assert outs[0] == _wav(_frames(1, 11)[None])
    assert outs[1:] == [_wav(_frames(u, 8)[None]) for u, _ in plan]
    assert eng.groups[1:] == [[1, 2], [3, 4], [5]]     # at most two distinct voices per prompt pass
    # voice 3 evicted voice 1 (capacity 2): voice 1 is built again, after the first group restored it
    assert [v for v, _ in eng.built] == [1, 2, 3, 1, 4] and [s for _, s in eng.built] == [1, 2, 3, 4, 5]


def test_a_stream_dropped_before_its_first_read_never_runs():
    eng = MovingEngine()
    with _server(eng) as srv:
        gen = srv.synthesize_stream("1", max_tokens=40)
        del gen
        time.sleep(0.1)
        assert srv.stats()["admitted"] == 0 and eng.prefills == [] and eng.widths == []


def test_overlapping_closes_return_after_the_instance_is_handed_back():
    handed = []

    def on_close(srv):
        time.sleep(0.2)
        handed.append(srv)
    srv = _server(MovingEngine(), on_close=on_close)
    seen = []

    def close():
        srv.close()
        seen.append(len(handed))
    _run_threads([close, close, close])
    assert len(handed) == 1 and seen == [1, 1, 1]
