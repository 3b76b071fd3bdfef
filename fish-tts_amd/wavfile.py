"""A RIFF/WAVE reader for the reference intake (FishTTS.encode_reference_at): where the frames lie in a file's bytes and
what they are made of.  It decodes nothing - the device reads the frames as they lie (include/fishtts_hip.h: "Reference
intake").  Plain Python without a dependency; Python's own `wave` refuses WAVE_FORMAT_EXTENSIBLE and IEEE-float files,
which is what most tools write for 24-bit, multichannel or float audio."""
from __future__ import annotations

import struct
from typing import NamedTuple

FORMATS = ("u8", "s16", "s24", "s32", "f32")           # all little-endian; the index is ft_intake_item.fmt
WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4}
MAX_CHANNELS = 8

_PCM, _FLOAT, _ALAW, _MULAW, _EXTENSIBLE = 1, 3, 6, 7, 0xFFFE
# a sub-format GUID is the 16-bit format tag followed by these fourteen bytes (KSDATAFORMAT_SUBTYPE_*)
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


class WavInfo(NamedTuple):
    fmt: str             # one of FORMATS
    channels: int
    rate: int
    data_offset: int     # the first frame's byte in the file
    n_frames: int


def parse_wav(data: bytes) -> WavInfo:
    """(fmt, channels, rate, data_offset, n_frames) of WAV bytes.  Accepted: format tags 1 (PCM: 8, 16, 24 or 32 bits) and 3
    (IEEE float: 32 bits), and tag 0xFFFE with a PCM or IEEE-float sub-format, the sample's size taken from the container
    (wBitsPerSample); 1 to 8 channels.  Unknown chunks are skipped, the pad byte of an odd-sized chunk honoured; a `data`
    chunk whose stated size runs past the end of the bytes is clipped to the whole frames that are there.  Anything else
    raises ValueError naming the cause."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data
    n = len(data)
    if n < 12 or bytes(data[0:4]) != b"RIFF" or bytes(data[8:12]) != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    fmt = None
    at = 12
    while at + 8 <= n:
        cid = bytes(data[at:at + 4])
        size = struct.unpack_from("<I", data, at + 4)[0]
        body = at + 8
        if cid == b"fmt ":
            if size < 16 or body + 16 > n:
                raise ValueError("WAV: a `fmt ` chunk shorter than 16 bytes")
            tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", data, body)
            if tag == _EXTENSIBLE:
                if size < 40 or body + 40 > n:
                    raise ValueError("WAV: an extensible `fmt ` chunk shorter than 40 bytes")
                sub = bytes(data[body + 24:body + 40])
                if sub[2:] != _GUID_TAIL:
                    raise ValueError(f"WAV: unsupported sub-format {sub.hex()}")
                tag = struct.unpack_from("<H", sub, 0)[0]
            fmt = (tag, channels, rate, align, bits)
        elif cid == b"data":
            if fmt is None:
                raise ValueError("WAV: no `fmt ` chunk before the `data` chunk")
            return _info(fmt, body, min(size, n - body))
        at = body + size + (size & 1)
    raise ValueError("WAV: no `fmt ` chunk" if fmt is None else "WAV: no `data` chunk")


def _info(fmt, offset: int, size: int) -> WavInfo:
    tag, channels, rate, align, bits = fmt
    if tag in (_ALAW, _MULAW):
        raise ValueError("WAV: A-law / mu-law audio is not supported")
    if tag == _PCM:
        name = {8: "u8", 16: "s16", 24: "s24", 32: "s32"}.get(bits)
        if name is None:
            raise ValueError(f"WAV: {bits}-bit PCM is not supported (8, 16, 24 or 32)")
    elif tag == _FLOAT:
        if bits == 64:
            raise ValueError("WAV: float64 audio is not supported")
        if bits != 32:
            raise ValueError(f"WAV: {bits}-bit float is not supported (32)")
        name = "f32"
    else:
        raise ValueError(f"WAV: unsupported format tag {tag:#x}")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"WAV: {channels} channels (1 to {MAX_CHANNELS} are supported)")
    if align != channels * WIDTH[name]:
        raise ValueError(f"WAV: block_align {align} is not channels * width = {channels * WIDTH[name]}")
    frames = size // align
    if frames < 1:
        raise ValueError("WAV: 0 frames of audio")
    return WavInfo(name, channels, rate, offset, frames)
