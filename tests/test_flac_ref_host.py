"""CPU: the FLAC stage's reference (tests/flac_ref.py) against things outside it - the one-frame example of RFC 9639, the CRC
check values, a frame assembled by hand, a brute-force search at blocksize 16 - and its decoder against its encoder over the
whole list of GPU cases (tests/flac_cases.py), with a census that shows the list reaches every path of the stage."""
import functools
import hashlib
import itertools

import numpy as np
import pytest

from tests import flac_cases as FC
from tests import flac_ref as R

# RFC 9639's example of a one-frame stereo stream.  Its CRC-8 (0xBF), CRC-16 (0xAA9A) and MD5 field agree with values computed here.
ANCHOR = bytes.fromhex("664c6143 80000022 10001000 00000f00000f 0ac442f000000001 3e84b41807dc690307586a3dad1a2e0f"
                       "fff869180000bf 0358fd 03128b aa9a".replace(" ", ""))


def test_decoder_reads_the_rfc_example():
    d = R.decode(ANCHOR)
    assert (d.rate, d.channels, d.bits, d.n, d.min_block, d.max_block, d.min_frame, d.max_frame) == (44100, 2, 16, 1, 4096, 4096, 15, 15)
    assert d.pcm.tolist() == [[25588, 10416]]
    assert len(d.frames) == 1 and d.frames[0]["blocksize"] == 1 and d.frames[0]["assignment"] == 1
    assert [(s["kind"], s["wasted"]) for s in d.frames[0]["subs"]] == [("VERBATIM", 2), ("VERBATIM", 4)]
    assert hashlib.md5(d.pcm.astype("<i2").tobytes()).digest() == d.md5
    assert R.crc8(ANCHOR[42:48]) == 0xBF and R.crc16(ANCHOR[42:55]) == 0xAA9A


def test_decoder_refuses_a_damaged_stream():
    for at in (44, 48, 50, 55):                       # header, CRC-8 itself, a subframe, the CRC-16
        bad = bytearray(ANCHOR)
        bad[at] ^= 0x10
        with pytest.raises(ValueError):
            R.decode(bytes(bad))
    with pytest.raises(ValueError):
        R.decode(ANCHOR[:-1])
    good = R.encode(np.arange(600, dtype=np.int32), 44100, 256)
    second = good.index(b"\xff\xf8", 50)
    with pytest.raises(ValueError, match="frame number|CRC"):
        R.decode(good[:42] + good[second:])                            # the first frame is gone: numbers start at 1


def test_crc_check_values():
    assert R.crc8(b"123456789") == 0xF4
    assert R.crc16(b"123456789") == 0xFEE8


def test_decoder_handles_what_the_encoder_never_writes():
    """Rice method 01 with its escape, method 00's escape, wasted bits under a FIXED subframe, assignment by hand."""
    def bits(*fields):
        s = "".join(format(v & ((1 << n) - 1), f"0{n}b") for v, n in fields)
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big")

    def stream(sub, bs, assignment=0, channels=1):
        h = bytes([0xFF, 0xF8, 0x69, (assignment << 4) | 8, 0, bs - 1])
        body = h + bytes([R.crc8(h)]) + sub
        frame = body + R.crc16(body).to_bytes(2, "big")
        return R.streaminfo(4096, len(frame), len(frame), 44100, channels, bs) + frame

    # FIXED 1, wasted bits 1 (15-bit samples): warm-up 5, method 01, P = 1: k = 3 for the one residual behind the warm-up,
    # then the escape with 4 raw bits for two residuals
    sub = bits((0, 1), (9, 6), (1, 1), (1, 1), (5, 15), (1, 2), (1, 4), (3, 5), (1, 1), (5, 3), (31, 5), (4, 5), (-3, 4), (7, 4))
    d = R.decode(stream(sub, 4))
    s = d.frames[0]["subs"][0]
    assert (s["kind"], s["wasted"], s["method"], s["P"], s["escaped"]) == ("FIXED1", 1, 1, 1, 1)
    # residuals: u = (0 << 3) | 5 = 5 -> e = -3; then -3, 7: 5, 2, -1, 6, times 2 for the wasted bit
    assert d.pcm.tolist() == [10, 4, -2, 12]
    # method 00's escape over a whole FIXED 0 subframe
    sub = bits((0, 1), (8, 6), (0, 1), (0, 2), (0, 4), (15, 4), (6, 5), (-32, 6), (31, 6), (0, 6))
    d = R.decode(stream(sub, 3))
    assert d.pcm.tolist() == [-32, 31, 0] and d.frames[0]["subs"][0]["escaped"] == 1
    # mid-side by hand: L = 7, R = 4 -> M = 5, S = 3; side-right: S = 3, R = 4; left-side: L = 7, S = 3
    for a, first, second in ((10, (5, 16), (3, 17)), (9, (3, 17), (4, 16)), (8, (7, 16), (3, 17))):
        sub = bits((0, 8), first, (0, 8), second)
        assert R.decode(stream(sub, 1, a, 2)).pcm.tolist() == [[7, 4]], a


def test_a_silent_frame_by_hand():
    """256 zeros, mono, 44100 Hz, B = 256: the stream head, FF F8, 1000 | 1001, 0000 | 100 | 0, frame 0, CRC-8; a CONSTANT
    subframe (00) of the 16-bit value 0; CRC-16.  The frame is 11 bytes, so are STREAMINFO's two frame sizes."""
    head = "664c6143" "80000022" "0100" "0100" "00000b" "00000b" "0ac440f000000100" + "00" * 16
    want = bytes.fromhex(head + "fff8" "89" "08" "00" "13" + "00" "0000" + "1d81")
    got = R.encode(np.zeros(256, dtype=np.int32), 44100, 256)
    assert got == want
    assert R.crc8(bytes.fromhex("fff8890800")) == 0x13 and R.crc16(bytes.fromhex("fff8890800130000" "00")) == 0x1D81
    assert not R.decode(got).pcm.any()


def test_number_coding():
    assert [R.utf8_number(v).hex() for v in (0, 127, 128, 2047, 2048, 65535, 65536)] == \
        ["00", "7f", "c280", "dfbf", "e0a080", "efbfbf", "f0908080"]


def test_quantise_is_the_wav_rule():
    """For finite input quantise is FishTTS._to_wav_bytes's arithmetic; a NaN gives 0; int16 goes through."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-1.2, 1.2, 5000), [1.0, -1.0, 0.0, -0.0, 1 - 2.0 ** -24, np.inf, -np.inf]]).astype(np.float32)
    assert np.array_equal(R.quantise(x), (np.clip(x, -1.0, 1.0) * 32767).astype(np.int16).astype(np.int32))
    assert R.quantise(np.array([np.nan, 1.5, -7.0], dtype=np.float32)).tolist() == [0, 32767, -32767]
    assert R.quantise(np.array([-32768, 5], dtype=np.int16)).tolist() == [-32768, 5]


# ---- the search at blocksize 16, brute force
def _brute(s, w):
    """The cheapest candidate of a 16-sample signal in tie order, every cost counted on codes written out one by one.  The
    k-vectors of a partition order are enumerated whole where there are at most 15^4 of them (P <= 2).  For P = 3 and 4
    (15^8 and 15^16 vectors) this is a REDUCED check: the candidate is each partition's cheapest k taken by itself - the
    additivity the encoder itself rests on - and what is enumerated whole is a grid of 4^8 and 2^16 vectors around it (every
    partition's k among the values nearest its own best), none of which may be cheaper, nor equal and earlier in the order."""
    bs = len(s)
    best = None

    def offer(bits, what):
        nonlocal best
        if best is None or bits < best[0]:
            best = (bits, what)

    if len(set(s)) == 1:
        offer(8 + w, ("CONSTANT",))
    for o in range(5):
        e = list(s)
        for _ in range(o):
            e = [None] + [e[i] - e[i - 1] if e[i - 1] is not None else None for i in range(1, bs)]
        u = [None if v is None else (2 * v if v >= 0 else -2 * v - 1) for v in e]
        for P in range(5):
            ln = bs >> P
            if ln <= o:
                continue
            table = [[4 + sum((v >> k) + 1 + k for v in u[j * ln:(j + 1) * ln] if v is not None) for k in range(15)]
                     for j in range(1 << P)]
            if P <= 2:
                for ks in itertools.product(range(15), repeat=1 << P):      # lexicographic: the smaller k first
                    offer(8 + w * o + 6 + sum(table[j][k] for j, k in enumerate(ks)), ("FIXED", o, P, ks))
            else:
                ks = tuple(min(range(15), key=lambda k: table[j][k]) for j in range(1 << P))
                mine = sum(table[j][k] for j, k in enumerate(ks))
                width = 4 if P == 3 else 2
                grid = [list(range(max(0, min(k - 1, 15 - width)), max(0, min(k - 1, 15 - width)) + width)) for k in ks]
                assert all(k in g for k, g in zip(ks, grid))
                total = functools.reduce(np.add.outer, [np.array([table[j][k] for k in g]) for j, g in enumerate(grid)])
                first = np.unravel_index(int(total.argmin()), total.shape)          # C order: the smaller k first
                assert int(total.min()) == mine and tuple(g[i] for g, i in zip(grid, first)) == ks
                offer(8 + w * o + 6 + mine, ("FIXED", o, P, ks))
    offer(8 + w * bs, ("VERBATIM",))
    return best


@pytest.mark.parametrize("seed", range(12))
def test_search_is_the_brute_force_minimum_at_16(seed):
    rng = np.random.default_rng(100 + seed)
    w = 17 if seed % 3 == 2 else 16
    amp = [0, 1, 1, 2, 3, 8, 40, 300, 5000, 30000, 65535 if w == 17 else 32767, 2][seed]
    s = rng.integers(-amp, amp + 1, 16)
    if seed == 1:
        s[:] = 0
        s[5] = 1                                      # nearly silent: many candidates tie
    if seed == 11:
        s = np.arange(16) * 3 - 20                    # a ramp: orders 2, 3 and 4 all leave zeros
    sub = R.choose_sub(s.astype(np.int64), w)
    bits, what = _brute([int(v) for v in s], w)
    assert sub.bits == bits
    got = ("CONSTANT",) if sub.kind == 0 else ("VERBATIM",) if sub.kind == 1 else ("FIXED", sub.order, sub.P, sub.ks)
    assert got == what
    assert len(R._sub_bits(s.astype(np.int64), w, sub)) == bits


def test_stereo_ties_go_in_the_stated_order():
    # L = R constant: (L, R) 48 bits, (L, S) 49, (S, R) 49, (M, S) 49 -> 0001; zeros too
    for v in (0, 77):
        _, c = R.encode(np.full((256, 2), v, dtype=np.int32), 44100, 256, census=True)
        assert c.subs[0][0] == 1


# ---- the case list: round trip and census
@pytest.mark.parametrize("name", [c[0] for c in FC.CASES])
def test_decode_of_encode_is_the_input(name):
    data, census, pcm = FC.reference(name)
    d = R.decode(data)
    _, x, rate, B = FC.BY_NAME[name]
    assert np.array_equal(d.pcm, pcm)
    assert (d.rate, d.channels, d.bits, d.n) == (rate, 1 if pcm.ndim == 1 else 2, 16, len(pcm))
    assert (d.min_block, d.max_block, d.min_frame, d.max_frame) == (B, B, census.min_frame, census.max_frame)
    assert d.md5 == bytes(16)
    assert len(d.frames) == census.frames == -(-len(pcm) // B) and len(data) == census.bytes
    # the decoder's account of each frame is the encoder's
    for f, (a, subs, bs) in zip(d.frames, census.subs):
        assert (f["assignment"], f["blocksize"]) == (a, bs)
        for got, want in zip(f["subs"], subs):
            assert got["kind"] == R.KINDS[want.kind] and got["wasted"] == 0
            if want.kind >= 2:
                assert (got["method"], got["P"], got["ks"], got["escaped"]) == (0, want.P, want.ks, 0)
    # nothing exceeds the all-VERBATIM bound
    assert len(data) <= 42 + census.frames * (17 + d.channels) + 2 * d.channels * len(pcm)


def test_the_case_list_reaches_every_path():
    kinds, assigns = np.zeros(len(R.KINDS), dtype=int), np.zeros(len(R.ASSIGNMENTS), dtype=int)
    Ps, ks, extras, numbers, rate_extra = set(), set(), set(), set(), False
    for name, _, rate, B in FC.CASES:
        _, census, _ = FC.reference(name)
        kinds += census.kinds
        assigns += census.assignments
        rate_extra = rate_extra or rate not in R.RATE_CODES
        for f, (_, subs, bs) in enumerate(census.subs):
            numbers.add(len(R.utf8_number(f)))
            if bs != B:
                extras.add(8 if bs <= 256 else 16)
            for s in subs:
                if s.kind >= 2:
                    Ps.add(s.P)
                    ks.update(s.ks)
    assert kinds.all(), dict(zip(R.KINDS, kinds))
    assert assigns.all(), dict(zip(R.ASSIGNMENTS, assigns))
    assert 0 in Ps and max(Ps) >= 3, Ps
    assert 0 in ks and 14 in ks, ks
    assert extras == {8, 16}
    assert {1, 2, 3} <= numbers
    assert rate_extra
