"""`live_format=` without a GPU: which values the five streaming calls take and refuse; then each path on fakes whose FLAC
stream hands back the quantised int16 samples of every completed "frame" as bytes (so the stream behind its 42-byte head is the
PCM itself) and records its pushes: the head once and first, no empty chunk, one final push, the dtype and channels per path
(the PCM chunks' own int16 on the pcm16 paths; the float32 of the join or the mixer in segments.join_chunks, 2 channels with
live_stereo), every use of the stream under an open BatchServer's codec lock, the stream closed when the generator ends or is
abandoned, `flac_report` filled."""
import types

import numpy as np
import pytest

import fish_tts_amd.segments as S
from fish_tts_amd.batch_stream import checked_live_format
from fish_tts_amd.flacfile import LiveFlac, flac_chunks, flac_tagged_chunks
from fish_tts_amd.script import Line
from tests.test_batch_stream_host import FakeCodec, _runner
from tests.test_host_logic import FakeEngine, _fake_utt
from tests.test_segments_host import CALL, LONG, SAMPLING, SEED, JoinCodec, _kw, _no_server
from tests.test_segments_host import _plan as _long_plan
from tests.test_segments_host import _server as _join_server
from tests.test_serve_host import MovingEngine, _prepare
from tests.test_stereo_live_api_host import SIZES, GapCodec, _codes, _script_plan

T = "Some text is here."
UNKNOWN, KNOWN = b"U" * 42, b"K" * 42


class FakeFlacStream:
    """The samples as the stage quantises them, handed back as int16 bytes once a "frame" of B is complete."""

    def __init__(self, log, rate, channels, B, dtype, held=None):
        self.log, self.channels, self.B, self.dtype, self.held = log, channels, B, np.dtype(dtype), held
        self.buf = np.zeros((0, channels), dtype=np.int16)
        self.n, self.ended, self.closed = 0, False, False
        self.pushes = []
        log.append(("flac-open", rate, channels, B, self.dtype.name, self._locked()))

    def _locked(self):
        return None if self.held is None else self.held.locked()

    def head(self) -> bytes:
        assert not self.closed
        return KNOWN if self.ended else UNKNOWN

    def push(self, x=None, final=False) -> bytes:
        assert not self.closed and not self.ended
        x = np.zeros(0, dtype=self.dtype) if x is None else np.asarray(x)
        if x.size:
            assert x.dtype == self.dtype and x.ndim == self.channels, (x.dtype, x.shape)
        q = x if x.dtype == np.int16 else (np.clip(x, -1.0, 1.0) * 32767).astype(np.int16)
        self.pushes.append((x.dtype.name, x.shape, final, self._locked()))
        self.buf = np.concatenate([self.buf, q.reshape(-1, self.channels)])
        self.n += len(q.reshape(-1, self.channels))
        k = len(self.buf) if final else len(self.buf) // self.B * self.B
        out, self.buf, self.ended = self.buf[:k].tobytes(), self.buf[k:], final
        return out

    def report(self):
        return ("report", self.n)

    def close(self):
        self.log.append(("flac-close", self._locked()))
        self.closed = True


def _with_flac(codec, held=None):
    """`codec` with a flac_stream that makes FakeFlacStreams (kept in codec.flacs) and writes to codec.flog."""
    codec.flacs, codec.flog = [], []

    def flac_stream(sample_rate=None, channels=1, blocksize=4096, dtype=np.float32):
        codec.flacs.append(FakeFlacStream(codec.flog, sample_rate, channels, blocksize, dtype, held))
        return codec.flacs[-1]
    codec.flac_stream = flac_stream
    return codec


def _tts(vocoder=None, server=None):
    from fish_tts_amd.synthesizer import FishTTS
    tts = FishTTS.__new__(FishTTS)                           # the checks come before anything else of the instance is used
    tts._vocoder, tts._server = vocoder, server
    return tts


def _checks(chunks, pcm: bytes, fs: FakeFlacStream, report, tag=()):
    """What every path owes: head once and first, the PCM behind it, no empty chunk, one final push - the last -, closed."""
    assert all(chunks) and chunks[0].startswith(UNKNOWN)
    data = b"".join(chunks)
    assert data[42:] == pcm and data.count(UNKNOWN) == 1
    assert [p[2] for p in fs.pushes].count(True) == 1 and fs.pushes[-1][2]
    assert fs.closed and fs.ended
    assert report == [(*tag, ("report", len(pcm) // 2 // fs.channels), KNOWN)]


def test_values_accepted_and_refused():
    from fish_tts_amd.serve import BatchServer
    assert checked_live_format(None) is None and checked_live_format("flac") == LiveFlac(4096)
    assert checked_live_format(LiveFlac(256)).blocksize == 256 and LiveFlac().blocksize == 4096
    for bad in (300, 0, True, 4096.0, "4096", None):
        with pytest.raises(ValueError, match="blocksize must be one of"):
            LiveFlac(bad)
    tts = _tts()
    for bad in ("wav", "FLAC", "ogg", "", 4096, True, b"flac", ("flac",)):
        with pytest.raises(ValueError, match="live_format must be"):
            checked_live_format(bad)
        for call in (lambda: tts.synthesize_batch_stream([T], live_format=bad), lambda: tts.synthesize_long_stream(T, live_format=bad),
                     lambda: tts.synthesize_script_stream([Line(T)], live_format=bad),
                     lambda: next(tts.synthesize_stream(T, live_format=bad)),          # a generator: at the first next()
                     lambda: next(tts.synthesize_stream(T, seamless=True, live_format=bad)),
                     lambda: BatchServer.__new__(BatchServer).synthesize_stream(T, live_format=bad)):
            with pytest.raises(ValueError, match="live_format must be"):
                call()
    # format= stays refused, with or without a live_format beside it
    with pytest.raises(ValueError, match="format needs the whole piece: synthesize_long_stream"):
        tts.synthesize_long_stream(T, format="flac", live_format="flac")
    with pytest.raises(ValueError, match="format needs the whole piece: synthesize_stream"):
        next(tts.synthesize_stream(T, format="flac", live_format="flac"))


def _generate(codes, order):
    def generate(emit, stopped):
        for i in order:
            emit(i, codes[i])
    return generate


def test_join_chunks_pushes_the_joins_float32_where_pcm_was():
    codes = [_codes(i, 3 + 2 * i) for i in range(4)]                        # 3 + 5 + 7 + 9 samples
    plain = list(S.join_chunks(_long_plan(LONG), **_kw(JoinCodec(), None, _no_server, _generate(codes, (0, 1, 2, 3)))))
    for B in (4, 5, 24, 100):                                               # frames inside groups, across them, the whole, none until the end
        codec, report = _with_flac(JoinCodec()), []
        chunks = list(S.join_chunks(_long_plan(LONG), **_kw(codec, None, _no_server, _generate(codes, (0, 1, 2, 3))),
                                    live_format=types.SimpleNamespace(blocksize=B), flac_report=report))
        fs, = codec.flacs
        _checks(chunks, b"".join(plain), fs, report)
        assert codec.flog[0] == ("flac-open", 44100, 1, B, "float32", None) and codec.flog[-1] == ("flac-close", None)
        assert all(p[0] == "float32" for p in fs.pushes) and sum(p[1][0] for p in fs.pushes) == 24
        if B == 100:
            assert len(chunks) == 1                                          # nothing went out before the final push
    # without live_format nothing of the stage is touched
    codec = _with_flac(JoinCodec())
    assert list(S.join_chunks(_long_plan(LONG), **_kw(codec, None, _no_server, _generate(codes, (0, 1, 2, 3))))) == plain
    assert not codec.flacs


def test_join_chunks_in_stereo_pushes_frames_of_two():
    codes = [_codes(i, k) for i, k in enumerate(SIZES)]
    order = (0, 1, 3, 2, 4, 5, 7, 6)
    plain = list(S.join_chunks(_script_plan(), **_kw(GapCodec(2, 3, 4), None, _no_server, _generate(codes, order)), live_stereo=True))
    codec, report = _with_flac(GapCodec(2, 3, 4)), []
    chunks = list(S.join_chunks(_script_plan(), **_kw(codec, None, _no_server, _generate(codes, order)), live_stereo=True,
                                live_format=types.SimpleNamespace(blocksize=8), flac_report=report))
    fs, = codec.flacs
    _checks(chunks, b"".join(plain), fs, report)
    assert codec.flog[0][:5] == ("flac-open", 44100, 2, 8, "float32")
    assert all(p[0] == "float32" and (len(p[1]) == 2 and p[1][1] == 2 or p[1] == (0,)) for p in fs.pushes)
    assert ("close",) in codec.log and codec.flog[-1][0] == "flac-close"     # closed with the mixer


def test_join_chunks_through_a_server_holds_its_codec_lock():
    from fish_tts_amd.serve import BatchServer  # noqa: F401
    plan = _long_plan(LONG)
    srv, _, _ = _join_server(MovingEngine())
    _with_flac(srv._codec, held=srv.codec_lock)

    def serve(s):
        return S.serve(s, plan, CALL, lambda: True, SAMPLING, SEED, None)
    with srv:
        plain = b"".join(S.join_chunks(plan, **_kw(srv._codec, srv, serve, None)))
        report = []
        chunks = list(S.join_chunks(plan, **_kw(srv._codec, srv, serve, None), live_format=types.SimpleNamespace(blocksize=4),
                                    flac_report=report))
    fs, = srv._codec.flacs
    _checks(chunks, plain, fs, report)
    assert all(p[3] for p in fs.pushes) and srv._codec.flog[0][5] and srv._codec.flog[-1] == ("flac-close", True)


def test_join_chunks_abandoned_closes_the_stream():
    codes = [_codes(i, 6) for i in range(4)]
    codec = _with_flac(JoinCodec())
    gen = S.join_chunks(_long_plan(LONG), **_kw(codec, None, _no_server, _generate(codes, (0, 1, 2, 3))),
                        live_format=types.SimpleNamespace(blocksize=4), flac_report=(report := []))
    assert not codec.flacs                                                  # opened at the first next(), not before
    assert next(gen).startswith(UNKNOWN)
    gen.close()
    fs, = codec.flacs
    assert fs.closed and not fs.ended and report == []
    # nothing generated at all: no chunk, the error as without live_format, the stream closed
    codec = _with_flac(JoinCodec())
    with pytest.raises(RuntimeError, match="No audio generated"):
        list(S.join_chunks(_long_plan(LONG), **_kw(codec, None, _no_server, _generate([_codes(i, 0) for i in range(4)], range(4))),
                           live_format=types.SimpleNamespace(blocksize=4)))
    assert codec.flacs[0].closed


def test_flac_chunks_pushes_the_pcm_chunks_own_int16():
    rng = np.random.default_rng(0)
    pcm = [rng.integers(-32768, 32768, k).astype(np.int16).tobytes() for k in (3, 9, 1, 20, 2)]
    log, report, made, closed = [], [], [], []

    def chunks():
        try:
            yield from pcm
        finally:
            closed.append(True)

    def open_():
        made.append(FakeFlacStream(log, 24000, 1, 8, np.int16))
        return made[-1]
    gen = flac_chunks(chunks(), open_, _Null, report)
    assert not made
    out = list(gen)
    _checks(out, b"".join(pcm), made[0], report)
    assert [p[:3] for p in made[0].pushes] == [("int16", (k,), False) for k in (3, 9, 1, 20, 2)] + [("int16", (0,), True)]
    assert len(out) == 3 and closed == [True]                               # 3: nothing; 12: 8; 5: nothing; 25: 24; 3: nothing; the final 3
    # abandoned: the chunks' generator is closed first, then the stream
    closed.clear()
    gen = flac_chunks(chunks(), open_, _Null, None)
    assert next(gen).startswith(UNKNOWN)
    gen.close()
    assert made[1].closed and not made[1].ended and closed == [True]


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_batch_stream_gives_one_stream_per_utterance():
    from fish_tts_amd.batch_stream import stream_utterances
    budgets = [40, 23, 1, 12]
    utts = [_fake_utt(i + 1, b) for i, b in enumerate(budgets)]
    plain = list(stream_utterances(_runner(FakeEngine(), utts), len(utts), FakeCodec(), chunk_tokens=7, min_first_chunk=5))
    utts = [_fake_utt(i + 1, b) for i, b in enumerate(budgets)]
    log, report, made = [], [], {}

    def open_():
        fs = FakeFlacStream(log, 44100, 1, 6, np.int16)
        made[len(made)] = fs
        return fs
    items = list(flac_tagged_chunks(stream_utterances(_runner(FakeEngine(), utts), len(utts), FakeCodec(), chunk_tokens=7, min_first_chunk=5),
                                    open_, _Null, report))
    by_stream = {id(fs): fs for fs in made.values()}
    assert len(by_stream) == 3                                              # utterance 2 has no audio: no stream, its end mark alone
    for i in range(len(utts)):
        want = b"".join(p for j, p in plain if j == i)
        got = [p for j, p in items if j == i]
        assert got[-1] == b"" and got.count(b"") == 1                       # the end mark stays, once, behind the last frames
        if not want:
            assert got == [b""]
            continue
        assert all(got[:-1]) and got[0].startswith(UNKNOWN) and b"".join(got)[42:] == want
        assert (i, ("report", len(want) // 2), KNOWN) in report
    assert len(report) == 3 and all(fs.closed and fs.ended for fs in made.values())
    # through the public call: checked, then the same wrapper over int16 streams at the call's rate
    tts = _tts()
    with pytest.raises(ValueError, match="live_format must be"):
        tts.synthesize_batch_stream([T], live_format="mp3")


def test_server_stream_pushes_under_the_codec_lock():
    from fish_tts_amd.serve import BatchServer
    codec = FakeCodec()
    srv = BatchServer(MovingEngine(), codec, 4, prepare=_prepare, decode_wav=None, decode_pcm=None)
    _with_flac(codec, held=srv.codec_lock)
    try:
        kw = dict(chunk_tokens=4, min_first_chunk=3, seamless=True, max_tokens=14)
        plain = b"".join(srv.synthesize_stream("1", **kw))
        report = []
        gen = srv.synthesize_stream("1", **kw, live_format=LiveFlac(256), flac_report=report)
        assert not codec.flacs                                              # opened at the first next()
        chunks = list(gen)
        fs, = codec.flacs
        _checks(chunks, plain, fs, report)
        assert codec.flog[0] == ("flac-open", 44100, 1, 256, "int16", True) and codec.flog[-1] == ("flac-close", True)
        assert all(p[0] == "int16" and p[3] for p in fs.pushes) and len(chunks) == 1      # 13 samples: the final push alone
        # the same request through FishTTS.synthesize_stream while the server is open: its lock again, the rate of the call
        tts = _tts(codec, srv)
        report = []
        chunks = list(tts.synthesize_stream("1", **kw, live_format="flac", flac_report=report))
        fs = codec.flacs[-1]
        assert codec.flog[-2] == ("flac-open", 44100, 1, 4096, "int16", True) and codec.flog[-1] == ("flac-close", True)
        _checks(chunks, b"".join(tts.synthesize_stream("1", **kw)), fs, report)
        assert all(p[0] == "int16" and p[3] for p in fs.pushes)
        # abandoned behind its first chunk: the stream is closed, unended, and nothing is reported
        report, small = [], LiveFlac(256)
        object.__setattr__(small, "blocksize", 2)                           # (the fake's frames: two samples, so the first chunk is early)
        gen = srv.synthesize_stream("1", chunk_tokens=4, min_first_chunk=4, seamless=True, max_tokens=100_000,
                                    live_format=small, flac_report=report)
        assert next(gen).startswith(UNKNOWN)
        gen.close()
        fs = codec.flacs[-1]
        assert fs.closed and not fs.ended and report == []
    finally:
        srv.close()
