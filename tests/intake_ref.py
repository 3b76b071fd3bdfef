"""The reference intake (include/fishtts_hip.h: "Reference intake") restated in float64 on the host: the conversion of the
five sample formats, the downmix, the two counters and the polyphase sum, then the level stage (tests/level_ref.py) and the
trim (tests/join_ref.py) over the result.  Also the WAV writers the tests build their files with."""
import ctypes as C
import math
import struct

import numpy as np

from tests import join_ref, level_ref

FO = 44100
FORMATS = ("u8", "s16", "s24", "s32", "f32")
WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4}
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 48000, 64000, 88200, 96000, 176400, 192000)
_SCALE = {"s16": 32768.0, "s24": 8388608.0, "s32": 2147483648.0}
_EXTREME = {"u8": (0, 255), "s16": (-32768, 32767), "s24": (-8388608, 8388607), "s32": (-2147483648, 2147483647)}


# ---------------------------------------------------------------------------------------------- files
def frames_bytes(v, fmt) -> bytes:
    """v: (n, C) integer codes (u8: 0..255, else signed), or float32 values for f32 -> the interleaved little-endian frames."""
    v = np.asarray(v)
    if v.ndim == 1:
        v = v[:, None]
    if fmt == "u8":
        return v.astype(np.uint8).tobytes()
    if fmt == "s16":
        return v.astype("<i2").tobytes()
    if fmt == "s32":
        return v.astype("<i4").tobytes()
    if fmt == "f32":
        return v.astype("<f4").tobytes()
    b = v.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3]       # s24: the low three bytes
    return np.ascontiguousarray(b).tobytes()


def wav_bytes(v, fmt, rate, extensible=False, extra=b"", data_size=None) -> bytes:
    """A WAV file of frames v (frames_bytes): a plain header (tags 1 and 3) or a WAVE_FORMAT_EXTENSIBLE one; `extra`: raw
    chunks placed between `fmt ` and `data`; `data_size`: the size the `data` chunk states (default: the true one)."""
    v = np.asarray(v)
    ch = 1 if v.ndim == 1 else v.shape[1]
    body = frames_bytes(v, fmt)
    w = WIDTH[fmt]
    tag = 3 if fmt == "f32" else 1
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, ch, rate, rate * ch * w, ch * w, 8 * w)
    if extensible:
        head += struct.pack("<HHI", 22, 8 * w, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    chunks = b"fmt " + struct.pack("<I", len(head)) + head + extra
    chunks += b"data" + struct.pack("<I", len(body) if data_size is None else data_size) + body + (b"\0" if len(body) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


# ---------------------------------------------------------------------------------------------- conversion and downmix
def decode(raw: bytes, fmt: str, channels: int):
    """(d, clipped, bad): d (n, C) float64, the samples as real numbers (a float sample that is not finite: 0); clipped and
    bad (n, C) bool: the sample sits at an extreme code of its format (f32: finite and |v| >= 1), is not finite."""
    if fmt == "s24":
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
    elif fmt == "f32":
        v = np.frombuffer(raw, dtype="<f4")
    else:
        v = np.frombuffer(raw, dtype={"u8": np.uint8, "s16": "<i2", "s32": "<i4"}[fmt]).astype(np.int64)
    v = v.reshape(-1, channels)
    if fmt == "f32":
        bad = ~np.isfinite(v)
        d = np.where(bad, 0.0, v.astype(np.float64))
        return d, (~bad) & (np.abs(d) >= 1.0), bad
    lo, hi = _EXTREME[fmt]
    clipped = (v == lo) | (v == hi)
    d = (v - 128) / 128.0 if fmt == "u8" else v / _SCALE[fmt]
    return d.astype(np.float64), clipped, np.zeros_like(clipped)


def mono(raw: bytes, fmt: str, channels: int, channel=None):
    """(m float32, clipped, nonfinite): the mean over the channels - summed in channel order in float64, one division,
    rounded once - or channel `channel` alone; the counters run over the channels that are used."""
    d, cl, bad = decode(raw, fmt, channels)
    if channel is not None:
        return d[:, channel].astype(np.float32), int(cl[:, channel].sum()), int(bad[:, channel].sum())
    s = np.zeros(len(d), dtype=np.float64)
    for c in range(channels):
        s = s + d[:, c]
    return (s / float(channels)).astype(np.float32), int(cl.sum()), int(bad.sum())


# ---------------------------------------------------------------------------------------------- the filter and the sum
def _lib():
    from fish_tts_amd import _lib as L
    return L.load()


def design(rate_in: int):
    """(L, M, K) as the header derives them."""
    g = math.gcd(rate_in, FO)
    L, M, fmin = FO // g, rate_in // g, min(rate_in, FO)
    if rate_in == FO:
        return L, M, 0
    K = int(math.ceil((75.0 - 7.95) / (2.285 * 2.0 * math.pi * 0.07) * rate_in / fmin))
    return L, M, K + (K & 1)


def filter_table(rate_in: int):
    """(L, M, K, w[L][K] float32) of ft_intake_filter; K = 0 (no table) at 44100."""
    lib = _lib()
    L, M, K = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.ft_intake_filter(rate_in, C.byref(L), C.byref(M), C.byref(K), None) == 0, rate_in
    w = np.zeros((L.value, max(K.value, 1)), dtype=np.float32)
    assert lib.ft_intake_filter(rate_in, None, None, None, w.ctypes.data_as(C.c_void_p)) == 0
    return L.value, M.value, K.value, w[:, :K.value]


def resample(m, rate_in: int, table=None, with_bound=False):
    """What the kernel computes, in float64: output n (u = n M, i0 = u // L, p = u % L) is sum_t w[p][t] m[i0 - K/2 + 1 + t],
    m zero outside the clip; ceil(len(m) L / M) outputs.  with_bound: also sum_t |w[p][t] m[...]| per output."""
    L, M, K, w = table or filter_table(rate_in)
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    if K == 0:
        return (m.copy(), np.abs(m)) if with_bound else m.copy()
    n_out = -(-len(m) * L // M)
    xp = np.concatenate([np.zeros(K), m, np.zeros(K)])
    w = w.astype(np.float64)
    out, mag = np.empty(n_out), np.empty(n_out)
    taps = np.arange(K)
    for a in range(0, n_out, 8192):
        n = np.arange(a, min(n_out, a + 8192), dtype=np.int64)
        u = n * M
        i0, p = u // L, u % L
        prod = w[p] * xp[(i0 - K // 2 + 1 + K)[:, None] + taps[None, :]]
        out[a:a + len(n)] = prod.sum(1)
        mag[a:a + len(n)] = np.abs(prod).sum(1)
    return (out, mag) if with_bound else out


# ---------------------------------------------------------------------------------------------- the chain behind the sum
def chain(y, target: int = 0, params=(0.0, 1, 0, 0)):
    """The level stage and the trim over one clip's float32 samples y at 44.1 kHz: (piece float32, (a, e), level_ref.Ref).
    target: hundredths of a LUFS, 0: measured only; params: (threshold, hop, keep, fade)."""
    y = np.asarray(y, dtype=np.float32)
    ref = level_ref.measure(y, FO, target)
    x = (y * ref.g).astype(np.float32) if target != 0 else y
    threshold, hop, keep, fade = params
    a, e = join_ref.edges(x, np.float32(threshold), hop, keep)
    return join_ref.piece(x, a, e, fade), (a, e), ref
