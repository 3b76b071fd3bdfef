"""A FLAC reader's first step, the counterpart of wavfile.parse_wav for the files `format="flac"` returns: what STREAMINFO says
of a stream.  It decodes nothing (the project reads no FLAC references); plain Python without a dependency.

And what `live_format=` of the streaming calls takes and runs on: LiveFlac, the value; LiveFlacFeed, one FLAC stream of the
live FLAC stage (CodecHipEngine.flac_stream) fed push by push; flac_chunks / flac_tagged_chunks, a call's int16 PCM chunks
turned into the chunks of one FLAC stream (of one per utterance)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Iterator, NamedTuple, Optional, Tuple

LIVE_BLOCKSIZES = (256, 512, 1024, 2048, 4096)


@dataclass(frozen=True)
class LiveFlac:
    """`live_format=` of a streaming call: its chunks are the bytes of one FLAC stream, packed on the GPU as the samples
    arrive (the live FLAC stage).  `blocksize`: samples per frame - the stage holds back fewer than that many samples (93 ms
    at 4096 and 44.1 kHz, 5.8 ms at 256), and smaller frames pack a little less tightly.  "flac" is shorthand for LiveFlac()."""
    blocksize: int = 4096

    def __post_init__(self):
        b = self.blocksize
        if isinstance(b, bool) or not isinstance(b, int) or b not in LIVE_BLOCKSIZES:
            raise ValueError(f"LiveFlac: blocksize must be one of {LIVE_BLOCKSIZES}, got {b!r}")


class LiveFlacFeed:
    """One FLAC stream over a call's audio: `stream` is an open CodecHipEngine.flac_stream.  push(x) returns the bytes that
    go out for these samples - the frames they complete, behind the unknown-values head where they are the first bytes of
    the stream, b"" where they complete no frame; push(x, final=True) flushes the short last frame, and `report` (a list)
    then receives (*tag, FlacReport, the final 42-byte head).  close() closes the stream."""

    def __init__(self, stream, report: Optional[list] = None, tag: tuple = ()):
        self._s, self._report, self._tag = stream, report, tag
        self._head = stream.head()               # taken before any push: smallest frame, largest frame and n "unknown"
        self.done = False

    def push(self, x=None, final: bool = False) -> bytes:
        out = self._s.push(x, final=final)
        if final:
            self.done = True
            if self._report is not None:
                self._report.append((*self._tag, self._s.report(), self._s.head()))
        if out and self._head is not None:
            out, self._head = self._head + out, None
        return out

    def close(self) -> None:
        self._s.close()


def flac_chunks(chunks: Iterator[bytes], open_stream: Callable, lock: Callable, report: Optional[list] = None) -> Iterator[bytes]:
    """The int16 PCM `chunks` of a streaming call as the chunks of one FLAC stream: open_stream() (at the first next()) is a
    CodecHipEngine.flac_stream for int16 samples, which is pushed those very samples, so the FLAC decodes to exactly the PCM;
    every use of it runs inside `with lock():`.  A push that completes no frame yields nothing; a final push behind the last
    chunk flushes the short last frame.  The stream is closed when the generator ends or is abandoned, `chunks` first."""
    import numpy as np
    feed = None
    try:
        with lock():
            feed = LiveFlacFeed(open_stream(), report)
        for pcm in chunks:
            with lock():
                out = feed.push(np.frombuffer(pcm, dtype=np.int16))
            if out:
                yield out
        with lock():
            out = feed.push(None, final=True)
        if out:
            yield out
    finally:
        close = getattr(chunks, "close", None)
        if close is not None:
            close()
        if feed is not None:
            with lock():
                feed.close()


def flac_tagged_chunks(items: Iterator[Tuple[int, bytes]], open_stream: Callable, lock: Callable,
                       report: Optional[list] = None) -> Iterator[Tuple[int, bytes]]:
    """flac_chunks for (i, pcm) items that end each utterance with (i, b""): one FLAC stream per i, opened at its first
    chunk, each with its own head; its final push goes out as (i, bytes) before its (i, b""), and `report` receives
    (i, FlacReport, head).  Every stream still open is closed when the generator ends or is abandoned."""
    import numpy as np
    feeds: dict = {}
    try:
        for i, pcm in items:
            if pcm:
                if i not in feeds:
                    with lock():
                        feeds[i] = LiveFlacFeed(open_stream(), report, (i,))
                with lock():
                    out = feeds[i].push(np.frombuffer(pcm, dtype=np.int16))
                if out:
                    yield i, out
                continue
            feed = feeds.get(i)
            if feed is not None and not feed.done:
                with lock():
                    out = feed.push(None, final=True)
                    feed.close()
                if out:
                    yield i, out
            yield i, b""
    finally:
        close = getattr(items, "close", None)
        if close is not None:
            close()
        with lock():
            for feed in feeds.values():
                feed.close()


class FlacInfo(NamedTuple):
    rate: int
    channels: int
    bits: int            # per sample
    samples: int         # per channel; 0: unknown
    min_blocksize: int
    max_blocksize: int   # equal to min_blocksize in a fixed-blocksize stream (what the FLAC stage writes)
    min_frame: int       # bytes; 0: unknown
    max_frame: int
    md5: bytes           # of the little-endian PCM; all zero: not computed (what the FLAC stage writes)
    data_offset: int     # the first frame's byte in the file


def stream_info(data: bytes) -> FlacInfo:
    """FlacInfo of FLAC bytes: the `fLaC` marker, STREAMINFO as the first metadata block, every later block skipped up to the
    one flagged last.  Anything else raises ValueError naming the cause."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data
    n = len(data)
    if n < 4 or bytes(data[0:4]) != b"fLaC":
        raise ValueError("not a FLAC stream (no fLaC marker)")
    at, info = 4, None
    while True:
        if at + 4 > n:
            raise ValueError("FLAC: the metadata runs past the end of the bytes")
        last, kind, size = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        body = at + 4
        if body + size > n:
            raise ValueError("FLAC: a metadata block runs past the end of the bytes")
        if info is None:
            if kind != 0 or size != 34:
                raise ValueError("FLAC: the first metadata block is not a 34-byte STREAMINFO")
            b = bytes(data[body:body + 34])
            v = int.from_bytes(b[10:18], "big")
            info = (v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1), int.from_bytes(b[0:2], "big"),
                    int.from_bytes(b[2:4], "big"), int.from_bytes(b[4:7], "big"), int.from_bytes(b[7:10], "big"), b[18:34])
        elif kind == 0:
            raise ValueError("FLAC: a second STREAMINFO block")
        elif kind == 127:
            raise ValueError("FLAC: metadata block type 127 is not allowed")
        at = body + size
        if last:
            break
    if info[0] == 0:
        raise ValueError("FLAC: STREAMINFO states a sample rate of 0")
    if info[4] < 16 or info[5] < info[4]:
        raise ValueError(f"FLAC: STREAMINFO's blocksizes {info[4]}..{info[5]} are not a range of at least 16")
    return FlacInfo(*info, at)
