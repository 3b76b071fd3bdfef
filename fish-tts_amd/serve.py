"""Concurrent synthesize calls served from one continuous lock-step batch (FishTTS.serve -> BatchServer).

The reference serves one request at a time: a server calls synthesize / synthesize_stream of the get_instance() singleton
from many threads and the calls serialize on one model (synthesizer.py:431-584; here FishTTS._gen_lock).  A BatchServer
owns the instance's first AR engine while it is open and runs ONE scheduler thread; requests that arrive at any time join
the running lock-step batch (batch.py) at the next burst boundary and stream their audio back.  At every boundary:

1. retire: finished requests (<|im_end|> or budget spent) and cancelled ones (a consumer that dropped its stream counts)
   leave their slots; freed slots that nothing takes are parked;
2. admit: queued requests, first come first served, into the lowest free slots - their prompt passes in one prefill_many
   call (one per PrefixCache.capacity distinct voices), each with its voice prefix, sampling values and seed, budgets
   clamped as run_batch clamps them;
3. compact: while the active slots are not [0, n), the highest active slot moves into the lowest free one
   (ARHipEngine.move_slot, one launch): a lock-step step decodes slots [0, width), so a batch with holes would not narrow,
   and a lone survivor reaches slot 0, where the batch-1 frame engine serves it;
4. decode: min(burst, budgets) frames at width n (2..4 padded to 5 where the engine has the MFMA launches, run_batch's
   rule), each request handed its columns.

With no work the thread blocks on the request queue: no GPU work, no spinning.  One codec worker thread turns columns into
audio; the AR loop never waits for it.  seamless=True streams are cut as batch_stream cuts them (exactly `min_first_chunk`
frames, then `chunk_tokens`, the last generated column held back) and every ready chunk goes through one decode_streams
call, one CodecStream per request; seamless=False chunks are FishTTS.synthesize_stream's (every generated column, each
chunk decoded from zero state); a non-streaming request's WAV is decoded when it ends; a "codes" request (the segments of FishTTS.synthesize_long) is handed its codes
and no audio - its caller decodes and joins them under codec_lock.  Per request the codes are those of
a single run with the same seed - the draws depend on (seed, frame, codebook, index), not on the slot or the schedule: bit
for bit on an engine of up to 4 slots, within the evaluation-order margin of the MFMA launches beyond (bf16 and fp16, batch.py).

Requests may ask for another output rate (sample_rate=): their WAVs and zero-state chunks are resampled on the device one
by one; their seamless streams resample through their CodecStream, in the same decode_streams call as every other ready
chunk whatever its rate, the last chunk (or a finish() after it) giving the resampler's tail before the end mark.
A speaking rate (speed=) travels the same way: WAVs and zero-state chunks are time-scaled on the device one by one, a
seamless request runs one carried time-scale stage in its CodecStream, its tail out before the end mark.  A pitch shift
(pitch=, semitones) does too, through the carried pitch stage of the request's CodecStream.

A native error in either thread fails every in-flight and queued request with that exception and closes the server."""
from __future__ import annotations

import queue
import threading
import time
from collections import deque
from typing import TYPE_CHECKING, Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .batch_stream import ChunkCutter, checked_format, checked_fx, checked_live_format, pcm16

if TYPE_CHECKING:
    from .batch import Utterance


class ServerClosed(RuntimeError):
    """The server takes no more requests (closed, or failed)."""


class _Failed:
    def __init__(self, error: BaseException):
        self.error = error


_END = object()


def compaction_moves(active: Sequence[int]) -> List[Tuple[int, int]]:
    """(from, to) slot moves that make the active slots [0, n): the highest active slot into the lowest free one while a
    hole is left below it.  [0, 7, 19] -> [(19, 1), (7, 2)]."""
    act = sorted(set(int(s) for s in active))
    moves = []
    while act and act[-1] != len(act) - 1:
        hole = next(s for s in range(len(act)) if s not in act)
        moves.append((act.pop(), hole))
        act = sorted(act + [hole])
    return moves


def lockstep_width(n: int, max_batch: int, wide_from: int) -> int:
    """Width of a step over the active slots [0, n): run_batch's rule - 2..4 rows ride up to `wide_from` (5) where the engine
    has the MFMA launches (the wider launch form is the cheaper one; the idle rows are parked); one row stays alone on
    slot 0 (the frame engine)."""
    return wide_from if 2 <= n < wide_from <= max_batch else n


class _Request:
    """One synthesize / synthesize_stream call: its utterance, chunking and output queue."""

    def __init__(self, utt: Utterance, n_prefix: int, mode: str, chunk_tokens: int, min_first_chunk: int,
                 fx=None):
        self.utt, self.n_prefix, self.mode = utt, n_prefix, mode          # mode: "wav" | "seamless" | "chunks" | "codes"
        self.cache = None             # a PrefixCache of the caller's own for this request's voice (None: the server's)
        self.fx = checked_fx(fx)      # the checked output stages (codec_engine.OutputFx; falsy: none, no tail held back)
        self.cut = None if mode in ("wav", "codes") else ChunkCutter(chunk_tokens, min_first_chunk, hold_back=mode == "seamless")
        self.out: "queue.Queue" = queue.Queue()
        self.cancelled = False        # the caller went away (or close(cancel=True))
        self.finished = False         # generation over: no more columns will come
        self.taken = False            # the codec worker is handing out its last item
        self.ended = False            # the codec side is done with it (end mark, WAV or failure handed out)
        self.stream = None            # CodecStream of a seamless request
        self.t_submit = time.perf_counter()


class BatchServer:
    """Continuous batching of concurrent synthesize / synthesize_stream calls on one AR engine (module docstring); a
    context manager, obtained from FishTTS.serve().  `prepare(text, references, temperature, top_p, repetition_penalty,
    max_tokens, seed) -> (Utterance, n_prefix)` builds and checks a request on the caller's thread; `decode_wav(codes)` /
    `decode_pcm(codes)` give WAV bytes / zero-state PCM of codes (with output stages: `fx=` as well); `prefix_cache` holds the voices' K/V prefixes;
    `on_close(server)` runs once, after both threads have stopped."""

    def __init__(self, engine, codec, burst: int = 8, *, prepare: Optional[Callable] = None,
                 decode_wav: Optional[Callable] = None, decode_pcm: Optional[Callable] = None, prefix_cache=None,
                 on_close: Optional[Callable] = None):
        if burst < 1:
            raise ValueError("burst must be >= 1")
        self._engine, self._codec, self._burst = engine, codec, int(burst)
        self._prepare, self._decode_wav, self._decode_pcm = prepare, decode_wav, decode_pcm
        self._prefix_cache, self._on_close = prefix_cache, on_close
        self.codec_lock = threading.Lock()       # held around the worker's codec calls (FishTTS.encode_reference takes it)
        self._lock = threading.Lock()
        self._work = threading.Condition(self._lock)      # scheduler: arrivals, cancellations, close
        self._codec_cv = threading.Condition(self._lock)  # codec worker: ready chunks, finished requests
        self._queue: deque = deque()
        self._retired: list = []                 # callers' own PrefixCaches (submit(voice_cache=)) to clear: scheduler thread
        self._live: List[_Request] = []          # submitted, not yet ended on the codec side
        self._closing = False
        self._sched_done = False
        self._closed = False
        self._handed_back = threading.Event()   # set once on_close has run
        self._error: Optional[BaseException] = None
        B = engine.max_batch
        self._owner: List[Optional[_Request]] = [None] * B
        self._budget = [0] * B
        self._idle_sp = engine._sampling(0.7, 0.8, 1.0)
        self._sps = [self._idle_sp] * B
        self._parked = [False] * B
        path = engine.frame_path() if hasattr(engine, "frame_path") else ""
        self._wide_from = 5 if "MFMA launches" in path else B + 1
        self._stats = {"admitted": 0, "completed": 0, "cancelled": 0, "slot_moves": 0, "steps_by_width": {}}
        self._threads = [threading.Thread(target=self._schedule, name="fish-tts-serve", daemon=True),
                         threading.Thread(target=self._codec_worker, name="fish-tts-serve-codec", daemon=True)]
        for t in self._threads:
            t.start()

    # ------------------------------------------------------------------ public interface
    def __enter__(self) -> "BatchServer":
        return self

    def __exit__(self, exc_type, exc, tb) -> None:
        self.close(cancel=exc_type is not None)

    def synthesize(self, text: str, references=None, temperature: float = 0.7, top_p: float = 0.8,
                   repetition_penalty: float = 1.1, max_tokens: int = 2048, seed: int = 0,
                   sample_rate: Optional[int] = None, speed: Optional[float] = None,
                   pitch: Optional[float] = None, fx=None, loudness: Optional[float] = None, format: str = "wav") -> bytes:
        """Text -> WAV bytes: FishTTS.synthesize's result for seed 0 (draws with `seed`).  Safe from any number of threads;
        `references=None` means the instance's set_references voices; `sample_rate`, `speed`, `pitch` and `loudness` as
        FishTTS.synthesize_at (an unsupported one raises ValueError here, before anything is queued; requests of different
        voices then come out at one level), or `fx`: these already checked (codec_engine.OutputFx).  `format`: "wav", or
        "flac" for a FLAC file of the same samples (as FishTTS.synthesize_at; any other value raises ValueError here)."""
        fx = checked_fx(fx, sample_rate, speed, pitch, loudness)
        checked_format(format)
        utt, n_prefix = self._prepare(text, references, temperature, top_p, repetition_penalty, max_tokens, seed)
        item = self.submit(utt, n_prefix, fx=fx, format=format).out.get()
        if isinstance(item, _Failed):
            raise item.error
        return item

    def synthesize_stream(self, text: str, references=None, chunk_tokens: int = 20, min_first_chunk: int = 10,
                          seamless: bool = False, sample_rate: Optional[int] = None, speed: Optional[float] = None,
                          pitch: Optional[float] = None, fx=None, loudness: Optional[float] = None,
                          live_loudness: Optional[float] = None, format: Optional[str] = None, live_format=None,
                          flac_report: Optional[list] = None, **sampling) -> Iterator[bytes]:
        """Yields int16 PCM chunks as FishTTS.synthesize_stream does: seamless=False (the reference's default) every chunk
        decoded from zero state; seamless=True one stateful CodecStream per request, the chunks cut as
        synthesize_batch_stream cuts them.  `sampling`: temperature, top_p, repetition_penalty, max_tokens, seed.  The
        prompt is built and checked here (a too-long one raises ValueError now); the request is queued at the first
        next(), so a generator dropped before it never runs, and abandoning it later cancels the request (its slot is
        freed at the next burst boundary).  `sample_rate`, `speed` and `pitch` as FishTTS.synthesize_stream (checked here), or
        `fx`: the three already checked.  `loudness` (or an `fx` with a level) raises ValueError here: the level needs the whole
        utterance.  `live_loudness` (or an `fx` with a ride stage; as FishTTS.synthesize_stream) is what a stream takes
        instead, with seamless=True only (ValueError here otherwise): the request's CodecStream carries the ride stage, in the
        same decode_streams call as every other ready chunk.  `format` is refused (ValueError here): a stream hands out raw
        PCM, and the FLAC stage packs a finished waveform.  `live_format` ("flac" or a flacfile.LiveFlac; as
        FishTTS.synthesize_stream, checked here) is what a stream takes instead: the chunks are the bytes of one FLAC stream - a
        stream of the live FLAC stage, opened at the first next() and pushed the PCM chunks' very int16 samples under
        codec_lock, closed when the generator ends or is abandoned; `flac_report` receives (FlacReport, final head)."""
        if chunk_tokens < 1 or min_first_chunk < 1:
            raise ValueError("chunk_tokens and min_first_chunk must be >= 1")
        if format is not None:
            raise ValueError("format needs the whole piece: BatchServer.synthesize_stream hands out int16 PCM chunks before the "
                             "piece's end, and the FLAC stage packs a finished waveform; use synthesize(format=)")
        fx = checked_fx(fx, sample_rate, speed, pitch, loudness, live_loudness).no_level("BatchServer.synthesize_stream")
        if fx.live is not None and not seamless:
            raise ValueError("live_loudness needs seamless=True: seamless=False chunks are independent waveforms, and "
                             "levelling each on its own would jump")
        live = checked_live_format(live_format)
        utt, n_prefix = self._prepare(text, references, sampling.get("temperature", 0.7), sampling.get("top_p", 0.8),
                                      sampling.get("repetition_penalty", 1.1), sampling.get("max_tokens", 2048),
                                      sampling.get("seed", 0))
        chunks = self._stream(utt, n_prefix, seamless, chunk_tokens, min_first_chunk, fx)
        if live is None:
            return chunks
        from .flacfile import flac_chunks
        if self._codec is None:
            raise RuntimeError("Vocoder not loaded")
        return flac_chunks(chunks, lambda: self._codec.flac_stream(fx.wav_rate, 1, live.blocksize, np.int16),
                           lambda: self.codec_lock, flac_report)

    def _stream(self, utt: Utterance, n_prefix: int, seamless: bool, chunk_tokens: int,
                min_first_chunk: int, fx=None) -> Iterator[bytes]:
        yield from self._chunks(self.submit(utt, n_prefix, stream=True, seamless=seamless, chunk_tokens=chunk_tokens,
                                            min_first_chunk=min_first_chunk, fx=fx))

    def submit(self, utt: Utterance, n_prefix: int = 0, stream: bool = False, seamless: bool = False,
               chunk_tokens: int = 20, min_first_chunk: int = 10, sample_rate: Optional[int] = None,
               speed: Optional[float] = None, pitch: Optional[float] = None, codes: bool = False,
               voice_cache=None, fx=None, format: str = "wav") -> _Request:
        """Queues one prepared utterance (the layer under synthesize / synthesize_stream); its output arrives on
        `.out`.  `codes`: the output is the utterance's codes (Utterance.codes()), no audio; `voice_cache`: the PrefixCache
        its voice prefix lives in instead of the server's.  Raises ServerClosed once the server is closing or has failed."""
        if self._codec is None:
            raise RuntimeError("Vocoder not loaded")
        checked_format(format)                   # (here, on the caller's thread: a bad value must not reach the worker)
        mode = "codes" if codes else ("seamless" if seamless else "chunks") if stream else "wav"
        req = _Request(utt, n_prefix, mode, chunk_tokens, min_first_chunk, checked_fx(fx, sample_rate, speed, pitch))
        req.cache = voice_cache
        req.format = format           # of a "wav" request's file: "wav", or "flac" (decode_wav is then called with format=)
        with self._lock:
            if self._error is not None:
                raise ServerClosed(f"BatchServer failed: {self._error!r}") from self._error
            if self._closing:
                raise ServerClosed("BatchServer is closed")
            self._queue.append(req)
            self._live.append(req)
            self._work.notify_all()
        return req

    def submit_codes(self, text: str, references=None, temperature: float = 0.7, top_p: float = 0.8,
                     repetition_penalty: float = 1.1, max_tokens: int = 2048, seed: int = 0, voice_cache=None) -> _Request:
        """One segment of a long text or of a script (segments.serve, under FishTTS.synthesize_long / synthesize_script and
        their streams; `references`: the segment's own, or the call's): a request whose output is its codes; take_codes
        waits for them.  `voice_cache`: a PrefixCache of the caller's own for the request's voice, so that a voice made up
        for one call stays out of the cache of the user's voices (the caller cancels what is still open and hands the
        cache to retire_cache when it is done, or when the server closes under its submissions)."""
        utt, n_prefix = self._prepare(text, references, temperature, top_p, repetition_penalty, max_tokens, seed)
        return self.submit(utt, n_prefix, codes=True, voice_cache=voice_cache)

    def take_codes(self, req: _Request) -> np.ndarray:
        item = req.out.get()
        if isinstance(item, _Failed):
            raise item.error
        return item

    def cancel(self, req: _Request) -> None:
        """Gives up a submitted request: its slot is freed at the next burst boundary, its caller gets a RuntimeError."""
        with self._lock:
            self._cancel_locked(req, RuntimeError("BatchServer: request cancelled"))
            self._work.notify_all()
            self._codec_cv.notify_all()

    def retire_cache(self, cache) -> None:
        """The caller is done with a PrefixCache it passed as `voice_cache`: the scheduler thread - the only user of the
        engine, and the only one that looks a prefix up - clears it at its next boundary at which no queued request still
        names it (cancel those first); after the scheduler has stopped it is cleared here."""
        with self._lock:
            if not self._sched_done:
                self._retired.append(cache)
                self._work.notify_all()
                return
        cache.clear()

    def _clear_retired_locked(self) -> None:
        """Scheduler thread, at a boundary: every admitted request is past its prompt pass, so a retired cache that no
        queued request names is out of use."""
        keep = [c for c in self._retired if any(r.cache is c for r in self._queue)]
        for c in self._retired:
            if not any(c is k for k in keep):
                c.clear()
        self._retired = keep

    def stats(self) -> dict:
        """Counters: requests admitted / completed / cancelled, slot moves, lock-step frame steps by width
        ({width: steps}), and the queued and active requests now."""
        with self._lock:
            s = dict(self._stats, steps_by_width=dict(self._stats["steps_by_width"]))
            s["queued"] = len(self._queue)
            s["active"] = sum(1 for r in self._owner if r is not None)
            return s

    def close(self, cancel: bool = False) -> None:
        """Takes no new request, then finishes every request already submitted (cancel=False) or cancels them (their
        callers get a RuntimeError), and stops both threads.  Afterwards the FishTTS instance serves its calls itself again.
        Idempotent."""
        with self._lock:
            self._closing = True
            if cancel:
                for r in list(self._live):
                    self._cancel_locked(r, RuntimeError("BatchServer closed: request cancelled"))
            self._work.notify_all()
            self._codec_cv.notify_all()
        for t in self._threads:
            if t is not threading.current_thread():
                t.join()
        with self._lock:
            first, self._closed = not self._closed, True
        if not first:
            self._handed_back.wait()           # a concurrent close() is handing the instance back: return after it
            return
        try:
            if self._on_close is not None:
                self._on_close(self)
        finally:
            self._handed_back.set()

    # ------------------------------------------------------------------ caller side
    def _chunks(self, req: _Request) -> Iterator[bytes]:
        over = False
        try:
            while True:
                item = req.out.get()
                if item is _END:
                    over = True
                    return
                if isinstance(item, _Failed):
                    over = True
                    raise item.error
                yield item
        finally:
            if not over:                        # the consumer dropped the stream
                with self._lock:
                    self._cancel_locked(req, None)
                    self._work.notify_all()
                    self._codec_cv.notify_all()

    def _cancel_locked(self, req: _Request, error: Optional[BaseException]) -> None:
        if req.cancelled or req.ended:
            return
        req.cancelled = True
        if req in self._queue:                  # never admitted: gone at once
            self._queue.remove(req)
            self._stats["cancelled"] += 1
        if error is not None:
            req.out.put(_Failed(error))

    def _fail(self, error: BaseException) -> None:
        """A native error: every in-flight and queued request fails with it and the server closes."""
        with self._lock:
            first = self._error is None
            if first:
                self._error = error
            self._closing = True
            for r in self._live:
                if not r.ended:
                    r.ended = True
                    r.out.put(_Failed(error))
            self._queue.clear()
            self._work.notify_all()
            self._codec_cv.notify_all()
        if first:
            threading.Thread(target=self.close, name="fish-tts-serve-close", daemon=True).start()

    # ------------------------------------------------------------------ scheduler thread
    def _schedule(self) -> None:
        eng = self._engine
        B = eng.max_batch
        try:
            for s in range(B):                  # whatever ran before: every slot idle
                eng.park(s)
                self._parked[s] = True
            while True:
                with self._lock:
                    freed = self._retire_locked()
                    self._clear_retired_locked()
                    while not self._queue and not any(self._owner) and not self._closing:
                        self._work.wait()
                        self._clear_retired_locked()
                    if self._error is not None or (self._closing and not self._queue and not any(self._owner)):
                        return
                    free = [s for s in range(B) if self._owner[s] is None]
                    admits = [self._queue.popleft() for _ in range(min(len(free), len(self._queue)))]
                self._admit(admits, free)
                for s in sorted(set(freed) | set(free)):       # free slots nothing took: idle rows of the coming steps
                    if self._owner[s] is None and not self._parked[s]:
                        eng.park(s)
                        self._parked[s] = True
                for src, dst in compaction_moves([s for s in range(B) if self._owner[s] is not None]):
                    eng.move_slot(src, dst)
                    self._owner[dst], self._owner[src] = self._owner[src], None
                    self._budget[dst], self._budget[src] = self._budget[src], 0
                    self._sps[dst], self._sps[src] = self._sps[src], self._idle_sp
                    self._parked[dst], self._parked[src] = False, True
                    with self._lock:
                        self._stats["slot_moves"] += 1
                active = [s for s in range(B) if self._owner[s] is not None]
                if active:
                    self._decode(active)
        except BaseException as e:  # noqa: BLE001
            self._fail(e)
        finally:
            with self._lock:
                self._sched_done = True
                for c in self._retired:          # (no request is prefilled any more)
                    c.clear()
                self._retired = []
                self._codec_cv.notify_all()

    def _retire_locked(self) -> List[int]:
        """Frees the slots of finished and cancelled requests."""
        freed = []
        for s, r in enumerate(self._owner):
            if r is None or not (r.finished or r.cancelled):
                continue
            if not r.finished:
                self._stats["cancelled"] += 1
            self._owner[s], self._budget[s], self._sps[s] = None, 0, self._idle_sp
            freed.append(s)
        return freed

    def _admit(self, reqs: List[_Request], free: List[int]) -> None:
        """The admitted requests, into the lowest free slots: one prefill_many call per group of at most
        PrefixCache.capacity distinct voices (a group's K/V prefixes are fetched before its prompt passes restore them, and
        a later voice of the same group must not evict one of them).  A request whose generation is over at its first frame
        leaves its slot free."""
        if not reqs:
            return
        cache = self._prefix_cache
        groups: List[list] = [[]]
        voices: set = set()
        for r, s in zip(reqs, free):
            voice = None
            if r.cache is not None:                   # a cache of the caller's own: nothing of the server's can be evicted
                groups[-1].append((r, s, r.n_prefix >= r.cache.min_positions))
                continue
            if cache is not None and r.n_prefix >= cache.min_positions:
                voice = np.ascontiguousarray(r.utt.prompt[:, :r.n_prefix], dtype=np.int32).tobytes()
                if voice not in voices and len(voices) >= max(1, cache.capacity):
                    groups.append([])
                    voices = set()
                voices.add(voice)
            groups[-1].append((r, s, voice is not None))
        for group in groups:
            self._prefill_group(group)

    def _prefill_group(self, group: list) -> None:
        eng = self._engine
        reqs, slots = [r for r, _, _ in group], [s for _, s, _ in group]
        for r, s, voiced in group:
            # built once per voice, in the slot the request is about to take: no active slot is touched
            cache = r.cache if r.cache is not None else self._prefix_cache
            r.utt.prefix = cache.get(eng, r.utt.prompt[:, :r.n_prefix], slot=s) if voiced else None
        sps = [eng._sampling(r.utt.temperature, r.utt.top_p, r.utt.repetition_penalty, r.utt.seed, r.utt.ban_eos)
               for r in reqs]
        firsts = eng.prefill_many([np.ascontiguousarray(r.utt.prompt, dtype=np.int32) for r in reqs], sps, slots,
                                  [r.utt.prefix for r in reqs])
        with self._lock:
            self._stats["admitted"] += len(reqs)
        for s, r, sp, first in zip(slots, reqs, sps, firsts):
            self._parked[s] = False
            n_new = eng._clamp_new(r.utt.prompt.shape[1], r.utt.max_new_tokens)
            over = n_new <= 1 or first[0] == eng.im_end_id
            self._emit(r, first[:, None], over)
            if not over:
                self._owner[s], self._budget[s], self._sps[s] = r, n_new - 1, sp

    def _decode(self, active: List[int]) -> None:
        eng = self._engine
        width = lockstep_width(active[-1] + 1, eng.max_batch, self._wide_from)
        k = min([self._burst] + [self._budget[s] for s in active])
        frames, n = eng.decode(k, self._sps[:width], poll=k)
        with self._lock:
            sw = self._stats["steps_by_width"]
            sw[width] = sw.get(width, 0) + k
        for s in active:
            got = int(n[s])
            self._budget[s] -= got
            over = got < k or (got > 0 and frames[s, got - 1, 0] == eng.im_end_id) or self._budget[s] <= 0
            self._emit(self._owner[s], frames[s, :got].T, over)

    def _emit(self, r: _Request, block: np.ndarray, over: bool) -> None:
        """Hands generated columns to the request and the codec worker; `over`: its generation has ended."""
        with self._lock:
            if r.cancelled or r.ended:
                r.finished = r.finished or over
                return
            if block.shape[1]:
                r.utt.frames.extend(block.T)
                if r.mode == "chunks":
                    r.cut.add(np.maximum(block, 0))      # synthesize_stream's codes (generation.generate_long: < 0 -> 0)
                elif r.mode == "seamless":
                    r.cut.add(block)
            if over:
                r.finished = True
                self._stats["completed"] += 1
                if r.cut is not None:
                    r.cut.finish()
            self._codec_cv.notify_all()

    # ------------------------------------------------------------------ codec worker
    def _last_out(self, r: _Request, item) -> None:
        """The request's last hand-out (WAV, end mark, or nothing for a cancelled one): only now does it leave the live
        list, so that until then a failure still reaches it (_fail)."""
        with self._lock:
            if r.ended:
                return
            if item is not None:
                r.out.put(item)
            r.ended = True
            self._live.remove(r)

    def _codec_worker(self) -> None:
        try:
            while True:
                with self._lock:
                    while True:
                        if self._error is not None:
                            return
                        live = [r for r in self._live if not r.taken]
                        gone = [r for r in live if r.cancelled]
                        seam = [r for r in live if not r.cancelled and r.mode == "seamless" and r.cut.ready]
                        plain = [r for r in live if not r.cancelled and r.mode == "chunks" and r.cut.ready]
                        wavs = [r for r in live if not r.cancelled and r.mode == "wav" and r.finished]
                        coded = [r for r in live if not r.cancelled and r.mode == "codes" and r.finished]
                        ends = [r for r in live if not r.cancelled and r.cut is not None and r.cut.done and not r.cut.ready]
                        if gone or seam or plain or wavs or coded or ends:
                            break
                        if self._sched_done and not self._live:
                            return
                        self._codec_cv.wait()
                    seam_chunks = [r.cut.ready.popleft() for r in seam]
                    seam_final = [r.cut.done and not r.cut.ready for r in seam]
                    plain_chunks = [r.cut.ready.popleft() for r in plain]
                    for r in gone + wavs + coded + ends:
                        r.taken = True                   # its last hand-out is under way: not picked again
                for r in gone + ends:
                    if r in ends and r.fx and r.stream is not None and not r.stream.finished:
                        with self.codec_lock:           # the output stages' tail, before the end mark
                            r.out.put(pcm16(r.stream.finish()))
                    if r.stream is not None:
                        r.stream.close()
                        r.stream = None
                    self._last_out(r, _END if r in ends else None)
                for r in coded:
                    self._last_out(r, r.utt.codes())     # no audio here: the caller decodes and joins under codec_lock
                with self.codec_lock:
                    if seam:
                        for r, c in zip(seam, seam_chunks):
                            if r.stream is None or r.stream.frames + c.shape[1] > self._codec.max_frames:
                                if r.stream is not None:   # the rotation table ends there (as in synthesize_stream)
                                    if r.fx:
                                        r.out.put(pcm16(r.stream.finish()))
                                    r.stream.close()
                                r.stream = self._codec.stream(**r.fx.kw)
                        streams = [r.stream for r in seam]
                        # (final flags only where a stream has a stage: the others have no tail and stay on the plain call)
                        final = [[bool(f and r.fx) for r, f in zip(seam, seam_final)]] if any(r.fx for r in seam) else []
                        audio = self._codec.decode_streams(streams, seam_chunks, *final)
                        for r, a in zip(seam, audio):
                            if len(a) or r.fx.emits_empty:     # (nothing completed in the time-scale, pitch or ride stage: nothing to hand out)
                                r.out.put(pcm16(a))
                    for r, c in zip(plain, plain_chunks):
                        r.out.put(self._decode_pcm(c, **r.fx.kw))
                    for r in wavs:
                        codes = r.utt.codes()
                        if not codes.shape[1]:
                            self._last_out(r, _Failed(RuntimeError("No audio generated")))
                        else:
                            self._last_out(r, self._decode_wav(codes, **r.fx.kw, **({} if r.format == "wav" else {"format": r.format})))
        except BaseException as e:  # noqa: BLE001
            self._fail(e)
        finally:
            with self._lock:
                streams = [r.stream for r in self._live if r.stream is not None]
                for r in self._live:
                    r.stream = None
            for s in streams:
                s.close()
