"""fish_tts_amd.segments without a GPU: the pipeline under synthesize_long / synthesize_script and their streams.  generate
on a fake batch callable that records what it is asked to run; serve, join_wav and join_chunks on a BatchServer over the fake
engine and codec of the server tests - for a long text (every segment in the call's voice, one chain of output stages) and
for a script (two segments with voices of their own, one chain per segment).  Which segment runs first, which references
and seed each gets, what is freed when, what a closing server leaves behind, and how a stream ends."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import fish_tts_amd.segments as S
from fish_tts_amd import VoiceProfile
from tests import test_serve_host as H
from tests.test_serve_host import FakeCodec, MovingEngine, _frames, _prepare, _wait

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 40
CALL = [VoiceProfile(codes=np.zeros((10, 3), dtype=np.int64), text="the call's voice")]
ANNA = [VoiceProfile(codes=np.ones((10, 3), dtype=np.int64), text="anna")]
BEN = [VoiceProfile(codes=np.full((10, 3), 2, dtype=np.int64), text="ben")]
LONG = [None, None, None, None]
MIXED = [ANNA, None, BEN, None]
KINDS = pytest.mark.parametrize("refs", [LONG, MIXED], ids=["long", "script"])


def _plan(refs, n=None):
    """Segment i has the text str(i + 1) - the fake engine's utterance id.  A long text: one chain for all; a script: one
    per segment."""
    n = len(refs) if n is None else n
    refs = list(refs) + [None] * (n - len(refs))
    fx = "fx" if all(r is None for r in refs) else [f"fx{i}" for i in range(n)]
    return S.SegmentPlan([str(i + 1) for i in range(n)], refs, [10 * (i + 1) for i in range(n)], (0.5, 4, 2, 1), 44100, fx)


def _codes(i, n=5):
    return np.full((10, n), i + 1, dtype=np.int32)


class Prefix:
    def __init__(self):
        self.freed = 0

    def free(self):
        self.freed += 1


class Run:
    """The batch callable of generate: records (indices, segment references, call references, seeds, made given) and emits
    five frames of codes per segment - none for the segments in `empty`; call number `fail_on` raises after it has built
    its prefix; with `spin` it goes on handing frames to on_frames after its segments are complete."""

    def __init__(self, empty=(), fail_on=None, spin=False):
        self.calls, self.prefixes, self.empty, self.fail_on, self.spin = [], [], empty, fail_on, spin

    def __call__(self, idx, seg_refs, references, seeds, made, on_frames, on_done):
        self.calls.append((list(idx), list(seg_refs), references, list(seeds), made is not None))
        if made is not None and "engine" not in made:
            made["engine"] = Prefix()
            self.prefixes.append(made["engine"])
        if len(self.calls) == self.fail_on:
            raise RuntimeError("device lost")
        for j, i in enumerate(idx):
            on_frames(j, None)
            on_done(j, _codes(i, 0 if i in self.empty else 5))
        t = time.time()
        while self.spin and time.time() - t < 10:
            on_frames(0, None)
            time.sleep(0.001)


def _generate(plan, run, references=None, stopped=lambda: False):
    got, lock = {}, threading.Lock()
    try:
        S.generate(plan, references, lambda: references is not None, SEED, run, lock, got.__setitem__, stopped)
    finally:
        assert not lock.locked()
    return got


def test_the_voice_rule_on_a_table():
    v = ANNA
    table = [([], None), ([None], None), ([v], None), ([v, v, v], None), ([None, None], 0), ([None, v, None], 0),
             ([v, None, v, None, None], 1), ([v, v, None], None), ([v, None, None], 1)]
    for seg_refs, want in table:
        assert S.first_alone(seg_refs, False) == want, seg_refs
        assert S.first_alone(seg_refs, True) is None, seg_refs


@KINDS
def test_with_a_call_voice_everything_is_one_batch(refs):
    run = Run()
    got = _generate(_plan(refs), run, CALL)
    assert run.calls == [([0, 1, 2, 3], refs, CALL, [SEED, SEED + 1, SEED + 2, SEED + 3], False)]
    assert sorted(got) == [0, 1, 2, 3] and all(np.array_equal(got[i], _codes(i)) for i in got)
    assert run.prefixes == []


@KINDS
def test_without_a_voice_the_first_own_segment_runs_alone_and_becomes_the_voice(refs):
    plan, run = _plan(refs), Run()
    k = S.first_alone(refs, False)
    assert k == (0 if refs is LONG else 1)
    got = _generate(plan, run)
    rest = [i for i in range(4) if i != k]
    assert len(run.calls) == 2
    assert run.calls[0] == ([k], [None], None, [SEED + k], False)
    idx, seg_refs, voice, seeds, made = run.calls[1]
    assert (idx, seeds, made) == (rest, [SEED + i for i in rest], True)
    assert len(voice) == 1 and isinstance(voice[0], VoiceProfile)
    assert np.array_equal(voice[0].codes, _codes(k)) and voice[0].text == plan.texts[k]
    # a segment with a voice of its own keeps it: the made-up voice is the CALL's voice, for the entries that are None
    assert all(s is r for s, r in zip(seg_refs, [refs[i] for i in rest]))
    assert sorted(got) == [0, 1, 2, 3] and all(np.array_equal(got[i], _codes(i)) for i in got)
    assert [p.freed for p in run.prefixes] == [1]


@KINDS
def test_an_empty_first_result_leaves_the_others_without_a_voice(refs):
    k = S.first_alone(refs, False)
    run = Run(empty=(k,))
    got = _generate(_plan(refs), run)
    assert run.calls[0][0] == [k] and got[k].shape == (10, 0)
    assert run.calls[1][2] is None and run.calls[1][4] is False and run.prefixes == []
    assert sorted(got) == [0, 1, 2, 3]


@KINDS
def test_the_made_prefix_is_freed_once_when_the_batch_raises(refs):
    run = Run(fail_on=2)
    with pytest.raises(RuntimeError, match="device lost"):
        _generate(_plan(refs), run)
    assert [p.freed for p in run.prefixes] == [1]
    run = Run(fail_on=1)                        # the first segment itself fails: nothing was made
    with pytest.raises(RuntimeError, match="device lost"):
        _generate(_plan(refs), run)
    assert run.prefixes == [] and len(run.calls) == 1


def test_one_segment_and_voiced_segments_only_wait_for_nobody():
    for refs in ([None], [ANNA, BEN], [ANNA, None]):
        run = Run()
        _generate(_plan(refs), run)
        assert [c[0] for c in run.calls] == [list(range(len(refs)))] and run.calls[0][4] is False


def test_a_stopped_consumer_ends_generation_at_the_next_frames():
    run = Run()
    with pytest.raises(S.Stopped):
        _generate(_plan(LONG), run, CALL, stopped=lambda: True)
    assert len(run.calls) == 1


# ---- through a BatchServer on the fake engine
SAMPLING = (0.7, 0.8, 1.1, 8)              # max_tokens 8: seven columns of codes per segment


def _server(eng, cache=None):
    """(server, log of (text, references, seed) per prepared request, list of retired caches)."""
    from fish_tts_amd.serve import BatchServer
    log, retired = [], []

    def prepare(text, references, temperature, top_p, repetition_penalty, max_tokens, seed):
        log.append((text, references, seed))
        return _prepare(text, references, temperature, top_p, repetition_penalty, max_tokens, seed)
    srv = BatchServer(eng, JoinCodec(), 4, prepare=prepare, decode_wav=H._wav, decode_pcm=H._plain, prefix_cache=cache)
    retire = srv.retire_cache
    srv.retire_cache = lambda c: (retired.append(c), retire(c))[1]
    return srv, log, retired


def _cache():
    from fish_tts_amd.generation import PrefixCache
    return PrefixCache(capacity=8, min_positions=2)


def _served_codes(i, n=7):
    return np.tile(_frames(i + 1, n), (10, 1))


@KINDS
def test_served_with_a_call_voice(refs):
    srv, log, retired = _server(MovingEngine(), _cache())
    with srv:
        takes, release = S.serve(srv, _plan(refs), CALL, lambda: True, SAMPLING, SEED, _cache())
        codes = [t() for t in takes]
        release()
    voiced = [i for i in range(4) if refs[i] is not None]
    order = voiced + [i for i in range(4) if refs[i] is None]          # the voiced segments are queued first
    assert [(int(t) - 1, s) for t, _, s in log] == [(i, SEED + i) for i in order]
    assert all(r is (CALL if refs[i] is None else refs[i]) for (_, r, _), i in zip(log, order))
    assert all(np.array_equal(c, _served_codes(i)) for i, c in enumerate(codes))     # takes: in segment order
    assert retired == [] and srv.stats()["completed"] == 4


@KINDS
def test_served_without_a_voice(refs):
    from fish_tts_amd.generation import PrefixCache
    k = S.first_alone(refs, False)
    srv, log, retired = _server(MovingEngine(), _cache())
    with srv:
        takes, release = S.serve(srv, _plan(refs), None, lambda: False, SAMPLING, SEED, _cache())
        done_at_return = srv.stats()["completed"]
        codes = [t() for t in takes]
        release()
        assert len(retired) == 1 and isinstance(retired[0], PrefixCache) and retired[0].capacity == 1
        assert retired[0].min_positions == 2
    voiced = [i for i in range(4) if refs[i] is not None]
    order = voiced + [k] + [i for i in range(4) if refs[i] is None and i != k]
    assert [(int(t) - 1, s) for t, _, s in log] == [(i, SEED + i) for i in order]   # voiced ones before the awaited first
    assert done_at_return >= 1
    for (_, r, _), i in zip(log, order):
        if refs[i] is not None:
            assert r is refs[i]
        elif i == k:
            assert r is None
        else:
            assert np.array_equal(r[0].codes, _served_codes(k)) and r[0].text == str(k + 1) and len(r) == 1
    assert all(np.array_equal(c, _served_codes(i)) for i, c in enumerate(codes))
    # without a prefix cache on the instance there is none for the call either
    srv, log, retired = _server(MovingEngine())
    with srv:
        takes, release = S.serve(srv, _plan(refs), None, lambda: False, SAMPLING, SEED, None)
        release()
    assert retired == []


@KINDS
def test_release_cancels_the_open_requests_and_retires_the_cache(refs, monkeypatch):
    k = S.first_alone(refs, False)
    monkeypatch.setitem(H.EOS, k + 1, 3)           # the awaited first segment ends at once, the others run on and on
    eng = MovingEngine()
    eng.max_new_tokens = 100_000
    srv, log, retired = _server(eng, _cache())
    with srv:
        takes, release = S.serve(srv, _plan(refs), None, lambda: False, (0.7, 0.8, 1.1, 100_000), SEED, _cache())
        assert takes[k]().shape == (10, 2)
        release(cancel=True)
        _wait(lambda: srv.stats()["cancelled"] == 3 and srv.stats()["active"] == 0)
        for i in range(4):
            if i != k:
                with pytest.raises(RuntimeError, match="cancelled"):
                    takes[i]()
        assert len(retired) == 1 and srv.stats()["queued"] == 0


def test_a_server_closed_before_the_call():
    from fish_tts_amd.serve import ServerClosed
    for refs, voice in ((LONG, None), (MIXED, None), (LONG, CALL), (MIXED, CALL)):
        srv, log, retired = _server(MovingEngine(), _cache())
        srv.close()
        with pytest.raises(ServerClosed):
            S.serve(srv, _plan(refs), voice, lambda: voice is not None, SAMPLING, SEED, _cache())
        assert S.codes_served(srv, lambda s: S.serve(s, _plan(refs), voice, lambda: voice is not None, SAMPLING, SEED,
                                                     None)) is None
        s = srv.stats()
        assert s["queued"] == 0 and s["admitted"] == 0 and retired == []      # (no cache was made yet)


@KINDS
def test_a_server_closed_in_the_middle_of_the_submissions(refs, monkeypatch):
    """The awaited first segment short and the others endless, as many slots as leave two segments waiting in the queue,
    and the server starts closing (it finishes what it took) as the last segment is prepared.  ServerClosed comes out, the
    call's requests are cancelled - a closing server would otherwise run them to the end for nobody - and its cache is
    retired."""
    from fish_tts_amd.serve import ServerClosed
    n, slots = (6, 2) if refs is LONG else (8, 4)
    plan = _plan(refs, n)
    k = S.first_alone(plan.refs, False)
    monkeypatch.setitem(H.EOS, k + 1, 3)
    eng = MovingEngine(max_batch=slots)
    eng.max_new_tokens = 100_000
    srv, log, retired = _server(eng, _cache())
    closer = threading.Thread(target=srv.close, daemon=True)
    prepare = srv._prepare

    def closing_prepare(*a):
        if len(log) == n - 1:
            closer.start()
            _wait(lambda: srv._closing)
        return prepare(*a)
    srv._prepare = closing_prepare
    with pytest.raises(ServerClosed):
        S.serve(srv, plan, None, lambda: False, (0.7, 0.8, 1.1, 100_000), SEED, _cache())
    assert len(log) == n and srv.stats()["queued"] == 0
    closer.join(10)
    assert not closer.is_alive()
    s = srv.stats()
    assert (s["queued"], s["active"]) == (0, 0), s
    assert (s["completed"], s["cancelled"]) == (1, n - 2), s
    assert s["admitted"] <= 1 + slots and len(retired) == 1         # (two at least were still in the queue)


# ---- the join
class JoinCodec(FakeCodec):
    """decode_join: row 0 of every item's codes as samples / 1e6, concatenated; records its keywords and whether the lock
    `held` was held."""

    def __init__(self, held=None):
        super().__init__()
        self.joins, self.held = [], held

    def decode_join(self, group, params=None, gaps=None, started=False, fx=None, item_fx=None):
        self.joins.append(dict(n=len(group), params=params, gaps=list(gaps), started=started, fx=fx, item_fx=item_fx,
                               locked=self.held.locked() if self.held is not None else None))
        rows = [np.asarray(c)[0].astype(np.float32) / 1e6 for c in group]
        cuts = np.array([(0, len(r)) for r in rows], dtype=np.int64).reshape(-1, 2)
        return (np.concatenate(rows) if rows else np.zeros(0, dtype=np.float32)), cuts


def _pcm(rows):
    return b"".join(H._pcm(np.asarray(r)[0]) for r in rows)


def _no_server(srv):
    raise AssertionError("there is no server")


def _kw(codec, srv, serve, generate):
    return dict(vocoder=codec, server=lambda: srv, serve_=serve, generate_=generate)


@KINDS
def test_chunks_come_in_order_from_out_of_order_completions(refs):
    plan, codec, go = _plan(refs), JoinCodec(), threading.Event()
    codes = [_codes(i, 3 + i) * 1000 for i in range(4)]

    def generate(emit, stopped):
        emit(2, codes[2])
        emit(0, codes[0])
        assert go.wait(10)
        emit(1, codes[1])
        emit(3, codes[3])
    seen = []
    gen = S.join_chunks(plan, **_kw(codec, None, _no_server, generate), on_cuts=lambda first, cuts: seen.append((first, len(cuts))))
    chunks = [next(gen)]
    go.set()
    chunks += list(gen)
    assert chunks[0] == _pcm(codes[:1]) and b"".join(chunks) == _pcm(codes) and all(chunks)
    assert [j["n"] for j in codec.joins][0] == 1 and sum(j["n"] for j in codec.joins) == 4
    assert [j["started"] for j in codec.joins] == [False] + [True] * (len(codec.joins) - 1)
    assert all(j["params"] == plan.jp for j in codec.joins)
    firsts = np.cumsum([0] + [j["n"] for j in codec.joins]).tolist()
    assert seen == [(f, j["n"]) for f, j in zip(firsts, codec.joins)]
    for f, j in zip(firsts, codec.joins):
        assert j["gaps"] == plan.gaps[f:f + j["n"]]
        if refs is LONG:                           # one chain for all, and no item chains: the long-text entry points
            assert j["fx"] == "fx" and j["item_fx"] is None
        else:
            assert j["fx"] is None and j["item_fx"] == plan.fx[f:f + j["n"]]


def test_an_abandoned_stream_stops_generation():
    run, lock = Run(spin=True), threading.Lock()
    before = threading.active_count()

    def generate(emit, stopped):
        S.generate(_plan(LONG), CALL, lambda: True, SEED, run, lock, emit, stopped)
    gen = S.join_chunks(_plan(LONG), **_kw(JoinCodec(), None, _no_server, generate))
    assert next(gen)
    assert lock.locked()                           # generation goes on behind the first chunk
    t = time.time()
    gen.close()
    assert time.time() - t < 5 and not lock.locked() and threading.active_count() <= before


def test_an_error_on_the_feeding_thread_reaches_the_consumer():
    def generate(emit, stopped):
        emit(0, _codes(0))
        raise RuntimeError("device lost")
    with pytest.raises(RuntimeError, match="device lost"):
        list(S.join_chunks(_plan(LONG), **_kw(JoinCodec(), None, _no_server, generate)))
    # and through a server: a cancelled request's error comes out of its take
    srv, log, retired = _server(MovingEngine())
    with srv:
        def serve(s):
            takes, release = S.serve(s, _plan(LONG), CALL, lambda: True, SAMPLING, SEED, None)

            def lost():
                raise RuntimeError("request lost")
            return takes[:2] + [lost] + takes[3:], release
        gen = S.join_chunks(_plan(LONG), **_kw(srv._codec, srv, serve, None))
        with pytest.raises(RuntimeError, match="request lost"):
            list(gen)


def test_a_stream_made_before_the_server_opens_is_served_by_it():
    """The server is looked up at the first next(), not when the generator is made: generating here would wait for the
    engine, which the open server holds."""
    plan, open_ = _plan(LONG), []

    def generate(emit, stopped):
        raise AssertionError("the open server serves the stream")
    srv, log, retired = _server(MovingEngine())
    gen = S.join_chunks(plan, vocoder=srv._codec, server=lambda: open_[0] if open_ else None, generate_=generate,
                        serve_=lambda s: S.serve(s, plan, CALL, lambda: True, SAMPLING, SEED, None))
    with srv:
        open_.append(srv)
        assert b"".join(gen) == _pcm([_served_codes(i) for i in range(4)])
        assert srv.stats()["completed"] == 4 and len(log) == 4


def test_the_call_voice_is_only_asked_for_where_the_rule_depends_on_it():
    def never():
        raise AssertionError("fewer than two segments in the call's voice: nothing depends on it")
    for refs in ([None], [ANNA, BEN], [ANNA, None]):
        assert S._first_alone(_plan(refs), never) is None
    asked = []
    assert S._first_alone(_plan(MIXED), lambda: asked.append(1) or False) == 1 and asked == [1]
    assert S._first_alone(_plan(MIXED), lambda: True) is None


def test_nothing_ready_at_all_is_no_audio():
    def generate(emit, stopped):
        for i in range(4):
            emit(i, _codes(i, 0))
    codec = JoinCodec()
    with pytest.raises(RuntimeError, match="No audio generated"):
        list(S.join_chunks(_plan(LONG), **_kw(codec, None, _no_server, generate)))
    assert sum(j["n"] for j in codec.joins) == 4
    with pytest.raises(RuntimeError, match="No audio generated"):
        S.join_wav(_plan(LONG), **_kw(codec, None, _no_server, generate))


@KINDS
def test_wav_and_chunks_through_a_server_and_without_one(refs):
    plan = _plan(refs)
    want = [_served_codes(i) for i in range(4)]
    kw = dict(fx="fx", item_fx=None) if refs is LONG else dict(fx=None, item_fx=plan.fx)
    srv, log, retired = _server(MovingEngine())
    srv._codec.held = srv.codec_lock

    def serve(s):
        return S.serve(s, plan, CALL, lambda: True, SAMPLING, SEED, None)
    with srv:
        audio, cuts = S.join_wav(plan, **_kw(srv._codec, srv, serve, None))
        assert np.array_equal(audio, np.concatenate([w[0] for w in want]).astype(np.float32) / 1e6) and len(cuts) == 4
        j = srv._codec.joins[-1]
        assert j["locked"] and j["gaps"] == plan.gaps and not j["started"] and (j["fx"], j["item_fx"]) == (kw["fx"], kw["item_fx"])
        assert b"".join(S.join_chunks(plan, **_kw(srv._codec, srv, serve, None))) == _pcm(want)
        assert all(j["locked"] for j in srv._codec.joins)
    assert srv.stats()["completed"] == 8
    # the server has closed: the call generates for itself, and takes no lock of the server's
    codec = JoinCodec(held=srv.codec_lock)

    def generate(emit, stopped):
        for i in (3, 1, 0, 2):
            emit(i, want[i])
    audio, _ = S.join_wav(plan, **_kw(codec, srv, serve, generate))
    assert np.array_equal(audio, np.concatenate([w[0] for w in want]).astype(np.float32) / 1e6)
    assert b"".join(S.join_chunks(plan, **_kw(codec, srv, serve, generate))) == _pcm(want)
    assert not any(j["locked"] for j in codec.joins) and codec.joins[0]["n"] == 4


def test_module_loads_without_torch_or_the_native_library():
    code = ("import sys, importlib.util as u\n"
            "spec = u.spec_from_file_location('segments', sys.argv[1])\n"
            "m = u.module_from_spec(spec); sys.modules['segments'] = m; spec.loader.exec_module(m)\n"
            "assert m.first_alone([None, None], False) == 0 and m.SegmentPlan([], [], [], (), 44100, None).line_of is None\n"
            "assert 'torch' not in sys.modules and 'ctypes' not in sys.modules and 'numpy' not in sys.modules\n")
    path = os.path.join(ROOT, "fish-tts_amd", "segments.py")
    subprocess.run([sys.executable, "-S", "-c", code, path], check=True)
