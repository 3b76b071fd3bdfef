"""Reference for the FLAC stage (include/fishtts_hip.h, "FLAC"): the stated encoder in integer numpy, and an independent general
decoder of the format's CONSTANT / VERBATIM / FIXED subset.  The encoder follows the header's statement rule by rule; the decoder
follows the public format (RFC 9639) and knows nothing of the encoder's choices: wasted bits, both Rice methods, the escape, all
four stereo assignments, every blocksize and rate code.  It checks sync, both CRCs, consecutive frame numbers and STREAMINFO
against what it decoded."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

BLOCKSIZES = (256, 512, 1024, 2048, 4096)
RATE_CODES = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}
KINDS = ("CONSTANT", "VERBATIM", "FIXED0", "FIXED1", "FIXED2", "FIXED3", "FIXED4")
ASSIGNMENTS = (0, 1, 8, 9, 10)      # the channel-assignment codes the encoder writes; the census counts in this order
MAX_K = 14


# ---------------------------------------------------------------------------------------------------------------- CRCs
def _table(poly: int, width: int):
    top, mask = 1 << (width - 1), (1 << width) - 1
    out = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


# ------------------------------------------------------------------------------------------------------------ quantise
def quantise(x) -> np.ndarray:
    """fmt 0: p = (int) trunc(min(1, max(-1, x)) * 32767.0f), one float32 product; a NaN gives 0.  int16 goes through as it is."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int32)
    x = x.astype(np.float32)
    nan = np.isnan(x)
    c = np.minimum(np.float32(1), np.maximum(np.float32(-1), np.where(nan, np.float32(0), x))).astype(np.float32)
    return np.trunc(c * np.float32(32767.0)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------- encoder
class Sub(NamedTuple):
    bits: int          # the subframe's bits
    kind: int          # index into KINDS
    order: int         # the fixed order (0 otherwise)
    P: int             # partition order (FIXED)
    ks: tuple          # Rice parameters, one per partition (FIXED)


class Census(NamedTuple):
    frames: int
    bytes: int
    min_frame: int
    max_frame: int
    kinds: tuple       # a count per KINDS entry
    assignments: tuple # a count per ASSIGNMENTS entry
    subs: list         # per frame: (assignment, [Sub per coded channel], blocksize)


def _residual(s: np.ndarray, o: int) -> np.ndarray:
    e = s.astype(np.int64)
    for _ in range(o):
        e = e[1:] - e[:-1]
    return e                                      # e_o[i] for i = o .. bs - 1


def _fixed_cost(s: np.ndarray, o: int):
    """(residual bits, P, ks) of order o: exhaustive over P and k."""
    bs = len(s)
    e = _residual(s, o)
    u = np.where(e >= 0, 2 * e, -2 * e - 1)
    best = None
    for P in range(9):
        if bs % (1 << P) or (bs >> P) <= o:
            continue
        ln = bs >> P
        full = np.concatenate([np.zeros(o, dtype=np.int64), u]).reshape(1 << P, ln)   # warm-up slots: (0 >> k) adds nothing
        m = np.full(1 << P, ln, dtype=np.int64)
        m[0] -= o
        ks = np.arange(MAX_K + 1, dtype=np.int64)
        cost = 4 + (full[:, :, None] >> ks[None, None, :]).sum(axis=1) + m[:, None] * (ks[None, :] + 1)
        kbest = cost.argmin(axis=1)                # the first minimum: ties to the smaller k
        total = int(cost[np.arange(1 << P), kbest].sum())
        if best is None or total < best[0]:        # ties to the smaller P
            best = (total, P, tuple(int(k) for k in kbest))
    return best


def choose_sub(s: np.ndarray, w: int) -> Sub:
    bs = len(s)
    cands = []
    if np.all(s == s[0]):
        cands.append(Sub(8 + w, 0, 0, 0, ()))
    for o in range(5):
        if o < bs:
            r, P, ks = _fixed_cost(s, o)
            cands.append(Sub(8 + w * o + 6 + r, 2 + o, o, P, ks))
    cands.append(Sub(8 + w * bs, 1, 0, 0, ()))
    best = cands[0]
    for c in cands[1:]:                            # candidates stand in tie order
        if c.bits < best.bits:
            best = c
    return best


def _field(v: int, n: int) -> np.ndarray:
    return np.array([(v >> (n - 1 - b)) & 1 for b in range(n)], dtype=np.uint8)


def _fields(v: np.ndarray, n: int) -> np.ndarray:
    v = v.astype(np.int64) & ((1 << n) - 1)
    return ((v[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8).ravel()


def _sub_bits(s: np.ndarray, w: int, sub: Sub) -> np.ndarray:
    bs = len(s)
    if sub.kind == 0:
        return np.concatenate([_field(0, 8), _fields(s[:1], w)])
    if sub.kind == 1:
        return np.concatenate([_field(1 << 1, 8), _fields(s, w)])
    o = sub.order
    head = np.concatenate([_field((8 | o) << 1, 8), _fields(s[:o], w), _field(0, 2), _field(sub.P, 4)])
    e = _residual(s, o)
    u = np.where(e >= 0, 2 * e, -2 * e - 1)
    ln = bs >> sub.P
    idx = np.arange(o, bs)
    part = idx // ln
    k = np.array(sub.ks, dtype=np.int64)[part]
    first = np.zeros(len(u), dtype=bool)
    first[0] = True
    first[1:] = part[1:] != part[:-1]
    q = u >> k
    length = q + 1 + k + 4 * first
    pos = np.concatenate([[0], np.cumsum(length)[:-1]])
    out = np.zeros(int(length.sum()), dtype=np.uint8)
    for b in range(4):
        out[pos[first] + b] = (k[first] >> (3 - b)) & 1
    start = pos + 4 * first
    out[start + q] = 1
    for b in range(MAX_K):
        sel = k > b
        out[(start + q + 1 + b)[sel]] = (u[sel] >> (k[sel] - 1 - b)) & 1
    return np.concatenate([head, out])


def utf8_number(v: int) -> bytes:
    """The format's UTF-8-style coding of a frame number."""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >> (5 * n + 1):                       # n bytes hold 5 n + 1 bits: 11, 16, 21, 26, 31
        n += 1
    lead = (0xFF << (8 - n)) & 0xFF
    out = [lead | (v >> (6 * (n - 1)))]
    for i in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def frame_header(bs: int, B: int, rate: int, assignment: int, number: int) -> bytes:
    if bs == B:
        bcode, bextra = 8 + BLOCKSIZES.index(B), b""
    elif bs <= 256:
        bcode, bextra = 6, bytes([bs - 1])
    else:
        bcode, bextra = 7, (bs - 1).to_bytes(2, "big")
    rcode, rextra = (RATE_CODES[rate], b"") if rate in RATE_CODES else (13, rate.to_bytes(2, "big"))
    h = bytes([0xFF, 0xF8, (bcode << 4) | rcode, (assignment << 4) | (4 << 1)]) + utf8_number(number) + bextra + rextra
    return h + bytes([crc8(h)])


def streaminfo(B: int, fmin: int, fmax: int, rate: int, channels: int, n: int) -> bytes:
    v = (rate << 44) | ((channels - 1) << 41) | (15 << 36) | n
    return (b"fLaC" + bytes([0x80, 0, 0, 34]) + B.to_bytes(2, "big") * 2 + fmin.to_bytes(3, "big") + fmax.to_bytes(3, "big") +
            v.to_bytes(8, "big") + bytes(16))


def encode_subframes(p: np.ndarray):
    """p: (bs,) or (bs, 2) int32.  (assignment, [Sub], the subframes' bits padded to the byte)."""
    if p.ndim == 1:
        sigs, assignment = [(p, 16)], 0
        subs = [choose_sub(p, 16)]
    else:
        L, R = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
        M, S = (L + R) >> 1, L - R
        dec = {"L": choose_sub(L, 16), "R": choose_sub(R, 16), "M": choose_sub(M, 16), "S": choose_sub(S, 17)}
        sig = {"L": (L, 16), "R": (R, 16), "M": (M, 16), "S": (S, 17)}
        options = [(1, "LR"), (8, "LS"), (9, "SR"), (10, "MS")]
        assignment, names = min(options, key=lambda o: dec[o[1][0]].bits + dec[o[1][1]].bits)   # min keeps the first of equals
        sigs, subs = [sig[c] for c in names], [dec[c] for c in names]
    bits = np.concatenate([_sub_bits(s, w, d) for (s, w), d in zip(sigs, subs)])
    assert len(bits) == sum(d.bits for d in subs), (len(bits), [d.bits for d in subs])
    return assignment, subs, np.packbits(bits).tobytes()       # the frame header is whole bytes: the padding is the frame's


def encode(pcm, rate: int, B: int = 4096, census: bool = False):
    """The stream of `pcm` ((n,) or (n, 2), int: already quantised).  With census=True: (bytes, Census)."""
    p = np.asarray(pcm)
    assert p.dtype.kind == "i" and B in BLOCKSIZES and p.shape[0] >= 1 and (p.ndim == 1 or (p.ndim == 2 and p.shape[1] == 2))
    p = p.astype(np.int32)
    n = p.shape[0]
    frames, rows = [], []
    kinds, assigns = [0] * len(KINDS), [0] * len(ASSIGNMENTS)
    memo = {}                                      # a block's subframes do not depend on its frame number: silence recurs
    for f in range((n + B - 1) // B):
        blk = p[f * B:(f + 1) * B]
        key = (blk.shape, blk.tobytes())
        if key not in memo:
            memo[key] = encode_subframes(blk)
        a, subs, packed = memo[key]
        body = frame_header(blk.shape[0], B, rate, a, f) + packed
        fb = body + crc16(body).to_bytes(2, "big")
        frames.append(fb)
        rows.append((a, subs, blk.shape[0]))
        assigns[ASSIGNMENTS.index(a)] += 1
        for d in subs:
            kinds[d.kind] += 1
    sizes = [len(f) for f in frames]
    out = streaminfo(B, min(sizes), max(sizes), rate, 1 if p.ndim == 1 else 2, n) + b"".join(frames)
    if not census:
        return out
    return out, Census(len(frames), len(out), min(sizes), max(sizes), tuple(kinds), tuple(assigns), rows)


# ------------------------------------------------------------------------------------------------------------- decoder
class Decoded(NamedTuple):
    pcm: np.ndarray          # (n,) or (n, channels) int32
    rate: int
    channels: int
    bits: int
    n: int
    min_block: int
    max_block: int
    min_frame: int
    max_frame: int
    md5: bytes
    frames: list             # per frame: dict(number, blocksize, assignment, size, subs=[dict(kind, order, wasted, method, P, ks, escaped)])


class _Bits:
    def __init__(self, data: bytes, at: int):
        self.data, self.pos = data, at * 8

    def read(self, n: int) -> int:
        if n == 0:
            return 0
        a, e = self.pos >> 3, (self.pos + n + 7) >> 3
        if e > len(self.data):
            raise ValueError("FLAC: the stream ends inside a frame")
        v = int.from_bytes(self.data[a:e], "big")
        v = (v >> (e * 8 - self.pos - n)) & ((1 << n) - 1)
        self.pos += n
        return v

    def signed(self, n: int) -> int:
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self) -> int:
        """Zeros before the next 1 bit; the 1 is consumed."""
        q = 0
        while True:
            a = self.pos >> 3
            if a >= len(self.data):
                raise ValueError("FLAC: the stream ends inside a unary run")
            rest = self.data[a] & (0xFF >> (self.pos & 7))
            if rest:
                lead = 8 - rest.bit_length() - (self.pos & 7)
                self.pos += lead + 1
                return q + lead
            q += 8 - (self.pos & 7)
            self.pos = (a + 1) * 8


_BS_CODE = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_RATE_CODE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_SIZE_CODE = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


def _read_subframe(br: _Bits, bs: int, bps: int) -> tuple:
    if br.read(1):
        raise ValueError("FLAC: a subframe's padding bit is set")
    typ = br.read(6)
    wasted = 0
    if br.read(1):
        wasted = br.unary() + 1
    w = bps - wasted
    info = dict(kind=None, order=0, wasted=wasted, method=None, P=None, ks=(), escaped=0)
    if typ == 0:
        info["kind"] = "CONSTANT"
        s = np.full(bs, br.signed(w), dtype=np.int64)
    elif typ == 1:
        info["kind"] = "VERBATIM"
        s = np.array([br.signed(w) for _ in range(bs)], dtype=np.int64)
    elif 8 <= typ <= 12:
        o = typ - 8
        info.update(kind=f"FIXED{o}", order=o)
        if o > bs:
            raise ValueError("FLAC: a fixed order above the blocksize")
        warm = [br.signed(w) for _ in range(o)]
        method = br.read(2)
        if method > 1:
            raise ValueError("FLAC: reserved residual coding method")
        pbits, esc = (4, 15) if method == 0 else (5, 31)
        P = br.read(4)
        if bs % (1 << P) or ((bs >> P) < o if P else False):
            raise ValueError("FLAC: a partition order the blocksize does not allow")
        res, ks = [], []
        for j in range(1 << P):
            m = (bs >> P) - (o if j == 0 else 0)
            k = br.read(pbits)
            if k == esc:
                raw = br.read(5)
                info["escaped"] += 1
                ks.append(("esc", raw))
                res.extend(br.signed(raw) for _ in range(m))
                continue
            ks.append(k)
            for _ in range(m):
                u = (br.unary() << k) | br.read(k)
                res.append((u >> 1) ^ -(u & 1))
        info.update(method=method, P=P, ks=tuple(ks))
        out = warm + [0] * (bs - o)
        for i in range(o, bs):                     # the format's predictors, written out per order
            e = res[i - o]
            if o == 0:
                out[i] = e
            elif o == 1:
                out[i] = e + out[i - 1]
            elif o == 2:
                out[i] = e + 2 * out[i - 1] - out[i - 2]
            elif o == 3:
                out[i] = e + 3 * out[i - 1] - 3 * out[i - 2] + out[i - 3]
            else:
                out[i] = e + 4 * out[i - 1] - 6 * out[i - 2] + 4 * out[i - 3] - out[i - 4]
        s = np.array(out, dtype=np.int64)
    else:
        raise ValueError(f"FLAC: subframe type {typ:#x} is outside this decoder (LPC or reserved)")
    return s << wasted, info


def decode(data: bytes) -> Decoded:
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise ValueError("FLAC: no fLaC marker")
    at, si = 4, None
    while True:
        if at + 4 > len(data):
            raise ValueError("FLAC: the metadata runs past the end")
        last, typ, size = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        body = data[at + 4:at + 4 + size]
        if typ == 0:
            if size != 34 or si is not None or at != 4:
                raise ValueError("FLAC: STREAMINFO must be the first block, once, of 34 bytes")
            si = body
        at += 4 + size
        if last:
            break
    if si is None:
        raise ValueError("FLAC: no STREAMINFO")
    min_block, max_block = int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big")
    min_frame, max_frame = int.from_bytes(si[4:7], "big"), int.from_bytes(si[7:10], "big")
    v = int.from_bytes(si[10:18], "big")
    rate, channels, bits, n = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    chans, frames, expect = [], [], 0
    while at < len(data):
        start = at
        br = _Bits(data, at)
        if br.read(14) != 0x3FFE or br.read(1):
            raise ValueError(f"FLAC: no frame sync at byte {at}")
        variable = br.read(1)
        bcode, rcode, assignment, scode = br.read(4), br.read(4), br.read(4), br.read(3)
        if br.read(1) or bcode == 0 or rcode == 15 or scode in (3,) or assignment > 10:
            raise ValueError("FLAC: a reserved value in a frame header")
        lead = br.read(8)
        if lead < 0x80:
            number = lead
        else:
            nb = 8 - (lead ^ 0xFF).bit_length()
            if nb < 2 or nb > 7:
                raise ValueError("FLAC: a bad coded number")
            number = lead & (0x7F >> nb)
            for _ in range(nb - 1):
                c = br.read(8)
                if c >> 6 != 2:
                    raise ValueError("FLAC: a bad continuation byte in a coded number")
                number = (number << 6) | (c & 0x3F)
        bs = br.read(8) + 1 if bcode == 6 else br.read(16) + 1 if bcode == 7 else _BS_CODE[bcode]
        frate = rate if rcode == 0 else br.read(8) * 1000 if rcode == 12 else br.read(16) if rcode == 13 else \
            br.read(16) * 10 if rcode == 14 else _RATE_CODE[rcode]
        fbits = bits if scode == 0 else _SIZE_CODE[scode]
        hdr_end = br.pos >> 3
        if br.read(8) != crc8(data[start:hdr_end]):
            raise ValueError(f"FLAC: CRC-8 of frame {len(frames)}")
        if variable:
            raise ValueError("FLAC: a variable-blocksize frame in this decoder's fixed-blocksize check")
        if number != expect:
            raise ValueError(f"FLAC: frame number {number} where {expect} was due")
        if frate != rate or fbits != bits:
            raise ValueError("FLAC: a frame disagrees with STREAMINFO on rate or sample size")
        nch = assignment + 1 if assignment < 8 else 2
        if nch != channels:
            raise ValueError("FLAC: a frame disagrees with STREAMINFO on channels")
        sigs, infos = [], []
        for c in range(nch):
            side = (assignment == 8 and c == 1) or (assignment == 9 and c == 0) or (assignment == 10 and c == 1)
            s, info = _read_subframe(br, bs, fbits + (1 if side else 0))
            sigs.append(s)
            infos.append(info)
        if assignment == 8:
            sigs = [sigs[0], sigs[0] - sigs[1]]
        elif assignment == 9:
            sigs = [sigs[0] + sigs[1], sigs[1]]
        elif assignment == 10:
            mid = (sigs[0] << 1) | (sigs[1] & 1)
            sigs = [(mid + sigs[1]) >> 1, (mid - sigs[1]) >> 1]
        pad = (-br.pos) % 8
        if br.read(pad):
            raise ValueError("FLAC: non-zero padding at a frame's end")
        end = br.pos >> 3
        if br.read(16) != crc16(data[start:end]):
            raise ValueError(f"FLAC: CRC-16 of frame {len(frames)}")
        at = end + 2
        for s in sigs:
            if s.min() < -(1 << (fbits - 1)) or s.max() >= 1 << (fbits - 1):
                raise ValueError("FLAC: a decoded sample outside the sample size")
        chans.append(np.stack(sigs, axis=1))
        frames.append(dict(number=number, blocksize=bs, assignment=assignment, size=at - start, subs=infos))
        expect += 1
    pcm = np.concatenate(chans).astype(np.int32) if chans else np.zeros((0, channels), dtype=np.int32)
    sizes = [f["size"] for f in frames]
    blocks = [f["blocksize"] for f in frames]
    if n and pcm.shape[0] != n:
        raise ValueError(f"FLAC: STREAMINFO states {n} samples, the frames hold {pcm.shape[0]}")
    if frames:
        if any(b > max_block for b in blocks) or any(b < min_block for b in blocks[:-1]):
            raise ValueError("FLAC: a blocksize outside STREAMINFO's bounds")
        if min_block == max_block and any(b != min_block for b in blocks[:-1]):
            raise ValueError("FLAC: a frame before the last is not of the fixed blocksize")
        if (min_frame and min(sizes) != min_frame) or (max_frame and max(sizes) != max_frame):
            raise ValueError("FLAC: STREAMINFO's frame sizes are not those of the frames")
    return Decoded(pcm[:, 0] if channels == 1 else pcm, rate, channels, bits, n, min_block, max_block, min_frame, max_frame,
                   bytes(si[18:34]), frames)
