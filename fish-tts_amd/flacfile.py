"""A FLAC reader's first step, the counterpart of wavfile.parse_wav for the files `format="flac"` returns: what STREAMINFO says
of a stream.  It decodes nothing (the project reads no FLAC references); plain Python without a dependency."""
from __future__ import annotations

from typing import NamedTuple


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
