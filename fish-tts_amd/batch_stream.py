"""Many utterances streamed at once: lock-step generation on one thread, ONE batched stateful codec decode per round of
ready chunks on another (FishTTS.synthesize_batch_stream).

The generation side is any `run(on_frames, on_done)` (batch.run_batch / run_batch_streams with their callbacks bound):
`on_frames(i, (R, k) block)` hands over generated columns of utterance i as they arrive, `on_done(i)` says it has its last
one.  The codes of utterance i are those of Utterance.codes(): rows 1.. of the columns, the last generated column dropped
- so one column is held back until the next one arrives or the utterance ends.  They are cut into chunks of exactly
`min_first_chunk` frames, then `chunk_tokens` frames each, then the remainder.

The codec side needs `stream()` (a CodecStream: `frames`, `close()`), `decode_streams(streams, chunks)` (one chunk of each
of several distinct streams in one pass, codec_engine.CodecHipEngine) and `max_frames`.  Each time the worker wakes it
decodes every ready chunk in one decode_streams call, at most one chunk per utterance; each utterance's chunks go through
its own stream, so its PCM concatenates to one streamed decode of its codes whatever else is in flight.  A stream that
would pass `max_frames` starts afresh (as synthesize_stream does).

With `sample_rate` the streams are `stream(sample_rate)` (their output resampled on the device) and decode_streams takes
one final flag per chunk: an utterance's last chunk is decoded with final=True, or, when its end is known only after its
last chunk went out, the stream's `finish()` gives the held-back tail; either way the tail is out before (i, b"").
`speed` (a speaking rate) and `pitch` (a shift in semitones) are passed through to the streams in the same way:
`stream(sample_rate, speed=speed, pitch=pitch)`, each keyword only when set.  A loudness target is refused (ValueError):
the level stage needs the whole utterance.  `live_loudness` is what a stream takes instead: its streams are
`stream(fx=...)` with the ride stage last, which holds back up to 1.1 s of output like any other tail; a stream that starts
afresh at `max_frames` starts a fresh ride state with it."""
from __future__ import annotations

import queue
import threading
from collections import deque
from typing import Callable, Iterator, List, Optional, Tuple

import numpy as np


class _Stopped(Exception):
    """Raised from on_frames once the consumer has gone: ends the generation within one burst."""


def pcm16(audio: np.ndarray) -> bytes:
    """int16 mono PCM as synthesize_stream(seamless=True) yields it (no clip on the PCM path)."""
    return (audio * 32767).astype(np.int16).tobytes()


class ChunkCutter:
    """One utterance's codes cut into chunks as its generated columns arrive: exactly `min_first_chunk` frames, then
    `chunk_tokens` frames each, then the remainder (`ready`).  `add` takes (R, k) generated columns, rows 1.. being the
    codes.  hold_back=True: the codes of Utterance.codes() - the last column stays back until the next one arrives, and
    `finish` drops it (inference.py:839); hold_back=False: every column (FishTTS.synthesize_stream's chunks)."""

    def __init__(self, chunk_tokens: int, min_first_chunk: int, hold_back: bool = True):
        self.chunk_tokens, self.min_first_chunk, self.hold = chunk_tokens, min_first_chunk, 1 if hold_back else 0
        self.pend: list = []              # columns not yet in a chunk (the held-back one last)
        self.first = True
        self.ready: deque = deque()       # cut chunks waiting for the codec
        self.done = False                 # no more columns will come

    def add(self, block: np.ndarray) -> None:
        if self.done:
            return
        self.pend.extend(np.asarray(block)[1:].T)
        while True:
            thr = self.min_first_chunk if self.first else self.chunk_tokens
            if len(self.pend) - self.hold < thr:
                return
            self.ready.append(np.stack(self.pend[:thr], axis=1))
            del self.pend[:thr]
            self.first = False

    def finish(self) -> None:
        rest = self.pend[:len(self.pend) - self.hold]
        if rest:
            self.ready.append(np.stack(rest, axis=1))
        self.pend = []
        self.done = True


def checked_fx(fx=None, sample_rate=None, speed=None, pitch=None, loudness=None, live_loudness=None):
    """The checked output stages of a call (codec_engine.OutputFx, imported when first needed, as the engines are): `fx`
    itself where the caller checked already, else the keywords checked now (ValueError for a bad one)."""
    if fx is not None:
        return fx
    from .codec_engine import OutputFx
    return OutputFx.of(sample_rate, speed, pitch, loudness, live_loudness)


FORMATS = ("wav", "flac")       # what `format=` of a call that returns a whole file may be


def checked_format(format) -> str:
    """`format` itself when it names a file format the whole calls write (ValueError otherwise, before any work)."""
    if not isinstance(format, str) or format not in FORMATS:
        raise ValueError(f"format must be one of {FORMATS}, got {format!r}")
    return format


def checked_live_format(live_format):
    """`live_format=` of a streaming call, checked before any work: None without one, else the flacfile.LiveFlac - the value
    itself, or LiveFlac() for the shorthand "flac".  Anything else raises ValueError."""
    from .flacfile import LiveFlac
    if live_format is None or isinstance(live_format, LiveFlac):
        return live_format
    if isinstance(live_format, str) and live_format == "flac":
        return LiveFlac()
    raise ValueError(f"live_format must be None, 'flac' or a flacfile.LiveFlac, got {live_format!r}")


def stream_utterances(run: Callable, n: int, codec, chunk_tokens: int = 20,
                      min_first_chunk: int = 10, sample_rate: Optional[int] = None,
                      speed: Optional[float] = None, pitch: Optional[float] = None, fx=None,
                      live_loudness: Optional[float] = None) -> Iterator[Tuple[int, bytes]]:
    """Yields (i, pcm) chunks of the n utterances `run` generates, in the order they become ready, and (i, b"") once
    after utterance i's last chunk.  `run` is called on a producer thread, the codec on a worker thread; abandoning the
    generator stops the producer at its next block of frames and joins both threads.  An exception of either thread is
    raised from the generator."""
    if chunk_tokens < 1 or min_first_chunk < 1:
        raise ValueError("chunk_tokens and min_first_chunk must be >= 1")
    fx = checked_fx(fx, sample_rate, speed, pitch, live_loudness=live_loudness).no_level("stream_utterances")   # truthy: an output stage holds back a tail
    cv = threading.Condition()
    cuts = [ChunkCutter(chunk_tokens, min_first_chunk) for _ in range(n)]
    ended = [False] * n                                 # end mark handed out (worker only)
    streams: List[Optional[object]] = [None] * n
    errors: List[BaseException] = []
    state = {"stop": False, "produced": False}
    out: "queue.Queue" = queue.Queue()

    def on_frames(i: int, block: np.ndarray) -> None:
        with cv:
            if state["stop"]:
                raise _Stopped()
            cuts[i].add(block)
            cv.notify_all()

    def on_done(i: int) -> None:
        with cv:
            if not cuts[i].done:
                cuts[i].finish()
            cv.notify_all()

    def producer() -> None:
        try:
            run(on_frames, on_done)
        except _Stopped:
            pass
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            with cv:
                state["stop"] = True
        finally:
            with cv:
                state["produced"] = True
                cv.notify_all()

    def worker() -> None:
        try:
            while True:
                with cv:
                    while True:
                        if state["stop"]:
                            return
                        batch = [i for i in range(n) if cuts[i].ready]
                        ends = [i for i in range(n) if cuts[i].done and not cuts[i].ready and not ended[i]]
                        if batch or ends:
                            break
                        if state["produced"]:
                            if all(ended):
                                return
                            for c in cuts:              # (a generation that ended without on_done for some)
                                if not c.done:
                                    c.finish()
                            continue
                        cv.wait()
                    chunks = [cuts[i].ready.popleft() for i in batch]
                    final = [cuts[i].done and not cuts[i].ready for i in batch]
                for i in ends:                          # after the utterance's last chunk went out
                    if fx and streams[i] is not None and not streams[i].finished:
                        tail = streams[i].finish()                     # the output stages' tail
                        if len(tail) or fx.emits_empty:
                            out.put((i, pcm16(tail)))
                    if streams[i] is not None:
                        streams[i].close()
                        streams[i] = None
                    ended[i] = True
                    out.put((i, b""))
                if not batch:
                    continue
                for i, c in zip(batch, chunks):
                    s = streams[i]
                    if s is None or s.frames + c.shape[1] > codec.max_frames:   # the rotation table ends there
                        if s is not None:
                            if fx:
                                out.put((i, pcm16(s.finish())))
                            s.close()
                        streams[i] = codec.stream(**fx.kw)
                # (final flags only where the streams have a stage: without one there is no tail, and the plain call stays)
                audio = codec.decode_streams([streams[i] for i in batch], chunks, *([final] if fx else []))
                for i, a in zip(batch, audio):
                    if len(a) or fx.emits_empty:             # (a chunk that completes nothing in the time-scale or pitch stage gives
                        out.put((i, pcm16(a)))          # no samples yet: (i, b"") is the end mark alone)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            with cv:
                state["stop"] = True
                cv.notify_all()
        finally:
            for i, s in enumerate(streams):
                if s is not None:
                    s.close()
                    streams[i] = None
            out.put(None)

    threads = [threading.Thread(target=producer, daemon=True), threading.Thread(target=worker, daemon=True)]
    for t in threads:
        t.start()
    try:
        while True:
            try:
                item = out.get(timeout=0.05)
            except queue.Empty:
                if threads[1].is_alive():
                    continue
                break
            if item is None:
                break
            yield item
    finally:
        with cv:
            state["stop"] = True
            cv.notify_all()
        for t in threads:
            t.join()
    if errors:
        raise errors[0]
