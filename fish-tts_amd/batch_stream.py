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
would pass `max_frames` starts afresh (as synthesize_stream does)."""
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


def stream_utterances(run: Callable, n: int, codec, chunk_tokens: int = 20,
                      min_first_chunk: int = 10) -> Iterator[Tuple[int, bytes]]:
    """Yields (i, pcm) chunks of the n utterances `run` generates, in the order they become ready, and (i, b"") once
    after utterance i's last chunk.  `run` is called on a producer thread, the codec on a worker thread; abandoning the
    generator stops the producer at its next block of frames and joins both threads.  An exception of either thread is
    raised from the generator."""
    if chunk_tokens < 1 or min_first_chunk < 1:
        raise ValueError("chunk_tokens and min_first_chunk must be >= 1")
    cv = threading.Condition()
    pend: List[list] = [[] for _ in range(n)]          # columns not yet in a chunk (the held-back one last)
    first = [True] * n
    ready: List[deque] = [deque() for _ in range(n)]    # cut chunks waiting for the codec
    done = [False] * n                                  # no more columns will come
    ended = [False] * n                                 # end mark handed out (worker only)
    streams: List[Optional[object]] = [None] * n
    errors: List[BaseException] = []
    state = {"stop": False, "produced": False}
    out: "queue.Queue" = queue.Queue()

    def cut(i: int) -> None:
        while True:
            thr = min_first_chunk if first[i] else chunk_tokens
            if len(pend[i]) - 1 < thr:                  # the last column stays back
                return
            ready[i].append(np.stack(pend[i][:thr], axis=1))
            del pend[i][:thr]
            first[i] = False

    def finish(i: int) -> None:
        if pend[i][:-1]:
            ready[i].append(np.stack(pend[i][:-1], axis=1))
        pend[i] = []
        done[i] = True

    def on_frames(i: int, block: np.ndarray) -> None:
        with cv:
            if state["stop"]:
                raise _Stopped()
            if done[i]:
                return
            pend[i].extend(np.asarray(block)[1:].T)
            cut(i)
            cv.notify_all()

    def on_done(i: int) -> None:
        with cv:
            if not done[i]:
                finish(i)
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
                        batch = [i for i in range(n) if ready[i]]
                        ends = [i for i in range(n) if done[i] and not ready[i] and not ended[i]]
                        if batch or ends:
                            break
                        if state["produced"]:
                            if all(ended):
                                return
                            for i in range(n):          # (a generation that ended without on_done for some)
                                if not done[i]:
                                    finish(i)
                            continue
                        cv.wait()
                    chunks = [ready[i].popleft() for i in batch]
                for i in ends:                          # after the utterance's last chunk went out
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
                            s.close()
                        streams[i] = codec.stream()
                audio = codec.decode_streams([streams[i] for i in batch], chunks)
                for i, a in zip(batch, audio):
                    out.put((i, pcm16(a)))
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
