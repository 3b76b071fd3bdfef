"""Host checks of the reference intake (include/fishtts_hip.h: "Reference intake"): the RIFF/WAVE reader against Python's
`wave`, scipy and hand-built headers, with every refusal; the filter design for input rates (ft_intake_filter /
ft_intake_len) and that generalising the design left ft_resample_filter's tables as they were; the float64 restatement
(tests/intake_ref.py, used by the GPU tests) against scipy.signal.resample_poly.  No GPU."""
import ctypes as C
import io
import math
import struct
import wave

import numpy as np
import pytest

from tests import intake_ref as R

FO = 44100


def _lib():
    from fish_tts_amd import _lib as L
    return L.load()


def _parse(b):
    from fish_tts_amd.wavfile import parse_wav
    return parse_wav(b)


def _codes(fmt, n, ch, seed=0):
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        return rng.integers(0, 256, (n, ch))
    if fmt == "f32":
        return rng.uniform(-1, 1, (n, ch)).astype(np.float32)
    bits = 8 * R.WIDTH[fmt]
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, ch))


# ---------------------------------------------------------------------------------------------- the reader
@pytest.mark.parametrize("ch", [1, 2, 8])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32"])
def test_parser_against_wave(fmt, ch):
    n = 37
    body = R.frames_bytes(_codes(fmt, n, ch), fmt)
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(ch); wf.setsampwidth(R.WIDTH[fmt]); wf.setframerate(22050)
        wf.writeframes(body)
    b = buf.getvalue()
    info = _parse(b)
    with wave.open(io.BytesIO(b), "rb") as wf:
        assert (info.channels, info.rate, info.n_frames) == (wf.getnchannels(), wf.getframerate(), wf.getnframes())
        want = wf.readframes(wf.getnframes())
    assert info.fmt == fmt
    assert b[info.data_offset:info.data_offset + n * ch * R.WIDTH[fmt]] == want == body


@pytest.mark.parametrize("ch", [1, 2])
def test_parser_against_scipy_float(ch):
    from scipy.io import wavfile
    v = _codes("f32", 29, ch)
    buf = io.BytesIO()
    wavfile.write(buf, 48000, v if ch > 1 else v[:, 0])
    b = buf.getvalue()
    info = _parse(b)
    assert tuple(info)[:3] == ("f32", ch, 48000) and info.n_frames == 29
    got = np.frombuffer(b, dtype="<f4", count=29 * ch, offset=info.data_offset).reshape(29, ch)
    assert np.array_equal(got, v)
    rate, back = wavfile.read(io.BytesIO(b))
    assert rate == 48000 and np.array_equal(back.reshape(29, ch), got)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_extensible_headers_use_the_container_size(fmt):
    v = _codes(fmt, 11, 3)
    b = R.wav_bytes(v, fmt, 96000, extensible=True)
    info = _parse(b)
    assert tuple(info)[:3] == (fmt, 3, 96000) and info.n_frames == 11
    assert b[info.data_offset:info.data_offset + 11 * 3 * R.WIDTH[fmt]] == R.frames_bytes(v, fmt)
    # 20 valid bits in a 24-bit container: the container decides
    if fmt == "s24":
        at = b.index(b"fmt ") + 8 + 18
        b2 = b[:at] + struct.pack("<H", 20) + b[at + 2:]
        assert _parse(b2).fmt == "s24"


def test_chunks_before_data_pad_bytes_and_a_clipped_data_size():
    v = _codes("s16", 10, 1)
    lst = b"LIST" + struct.pack("<I", 4) + b"INFO"
    odd = b"junk" + struct.pack("<I", 3) + b"abc" + b"\0"            # an odd-sized chunk and its pad byte
    b = R.wav_bytes(v, "s16", 16000, extra=lst + odd)
    info = _parse(b)
    assert info.n_frames == 10 and b[info.data_offset:info.data_offset + 20] == R.frames_bytes(v, "s16")
    # without the pad byte honoured the reader would look for `data` one byte early
    assert b[info.data_offset - 8:info.data_offset - 4] == b"data"
    # a data chunk that claims more than is there (a streamed writer's 0xFFFFFFFF, or a cut file): whole frames only
    v3 = _codes("s24", 7, 2)
    b3 = R.wav_bytes(v3, "s24", 44100, data_size=0xFFFFFFFF)
    assert _parse(b3).n_frames == 7
    assert _parse(b3[:-5]).n_frames == 6                             # 42 bytes of frames less 5: six whole 6-byte frames
    # an odd-sized data chunk followed by nothing
    assert _parse(R.wav_bytes(_codes("u8", 5, 1), "u8", 8000)).n_frames == 5


def _with_fmt(tag, ch, rate, align, bits, body=b"\0" * 16, fmt_chunk=True, data_chunk=True):
    chunks = b""
    if fmt_chunk:
        chunks += b"fmt " + struct.pack("<I", 16) + struct.pack("<HHIIHH", tag, ch, rate, rate * align, align, bits)
    if data_chunk:
        chunks += b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.mark.parametrize("name,data,match", [
    ("not riff", b"RIFX" + b"\0" * 40, "RIFF/WAVE"),
    ("not wave", b"RIFF" + struct.pack("<I", 4) + b"AVI " + b"\0" * 40, "RIFF/WAVE"),
    ("short", b"RIFF", "RIFF/WAVE"),
    ("no fmt", _with_fmt(1, 1, 8000, 2, 16, fmt_chunk=False), "fmt"),
    ("no fmt at all", _with_fmt(1, 1, 8000, 2, 16, fmt_chunk=False, data_chunk=False), "fmt"),
    ("no data", _with_fmt(1, 1, 8000, 2, 16, data_chunk=False), "data"),
    ("float64", _with_fmt(3, 1, 8000, 8, 64), "float64"),
    ("a-law", _with_fmt(6, 1, 8000, 1, 8), "A-law"),
    ("mu-law", _with_fmt(7, 1, 8000, 1, 8), "mu-law"),
    ("0 channels", _with_fmt(1, 0, 8000, 0, 16), "channels"),
    ("9 channels", _with_fmt(1, 9, 8000, 18, 16, body=b"\0" * 36), "channels"),
    ("0 frames", _with_fmt(1, 1, 8000, 2, 16, body=b""), "0 frames"),
    ("less than a frame", _with_fmt(1, 2, 8000, 4, 16, body=b"\0" * 3), "0 frames"),
    ("block align", _with_fmt(1, 2, 8000, 2, 16), "block_align"),
    ("12 bit", _with_fmt(1, 1, 8000, 2, 12), "12-bit"),
    ("adpcm", _with_fmt(2, 1, 8000, 2, 16), "format tag"),
])
def test_refusals_name_the_cause(name, data, match):
    with pytest.raises(ValueError, match=match):
        _parse(data)


def test_extensible_refusals():
    b = bytearray(R.wav_bytes(_codes("s16", 4, 1), "s16", 8000, extensible=True))
    at = bytes(b).index(b"fmt ") + 8 + 24
    for tag, match in ((6, "A-law"), (2, "format tag")):
        c = bytearray(b)
        c[at:at + 2] = struct.pack("<H", tag)
        with pytest.raises(ValueError, match=match):
            _parse(bytes(c))
    c = bytearray(b)
    c[at + 4] ^= 0xFF                                                # not a KSDATAFORMAT GUID
    with pytest.raises(ValueError, match="sub-format"):
        _parse(bytes(c))


# ---------------------------------------------------------------------------------------------- the design
@pytest.mark.parametrize("rate", R.RATES + (FO,))
def test_intake_design_as_derived(rate):
    lib = _lib()
    L, M, K, w = R.filter_table(rate)
    assert (L, M, K) == R.design(rate)
    assert L <= 640 and (K == 0) == (rate == FO) and K % 2 == 0
    if K:
        assert 68 <= K <= 292 and (255 * M + L - 1) // L + K + 1 <= 1404 and L * K * 4 < 169 * 1024
    for n in (0, 1, 255, 4097, 30 * rate):
        assert lib.ft_intake_len(rate, n) == -(-n * L // M)
    assert lib.ft_intake_len(rate, -1) == -1


@pytest.mark.parametrize("rate", [7999, 192001, 44099, 47999, 0, -48000])
def test_refused_input_rates_leave_the_outputs_alone(rate):
    lib = _lib()
    L, M, K = C.c_int32(-5), C.c_int32(-6), C.c_int32(-7)
    t = np.full(4, 9.0, dtype=np.float32)
    assert lib.ft_intake_filter(rate, C.byref(L), C.byref(M), C.byref(K), t.ctypes.data_as(C.c_void_p)) == 1      # FT_ERR_ARG
    assert (L.value, M.value, K.value) == (-5, -6, -7) and np.all(t == 9.0)
    assert lib.ft_intake_len(rate, 2048) == -1


@pytest.mark.parametrize("rate", R.RATES)
def test_intake_filter_quality(rate):
    """The prototype rebuilt from the table (tap t of phase p sits at p + (K/2 - 1 - t) L), at the up-sampled rate L rate:
    >= 70 dB stop band from 0.5 Fmin, <= 0.01 dB pass band ripple up to 0.43 Fmin, on a dense grid."""
    L, M, K, w = R.filter_table(rate)
    proto = np.zeros(L * K)
    for t in range(K):
        proto[np.arange(L) + (K // 2 - 1 - t) * L + (K // 2) * L] = w[:, t]
    proto /= L
    nf = 1 << int(math.ceil(math.log2(len(proto) * 64)))
    H = np.abs(np.fft.rfft(proto, nf))
    f = np.arange(len(H)) * (L * rate) / nf
    fmin = min(rate, FO)
    pb, sb = H[f <= 0.43 * fmin], H[f >= 0.5 * fmin]
    print(rate, K, np.max(np.abs(20 * np.log10(pb))), -20 * np.log10(sb.max()))
    assert np.max(np.abs(20 * np.log10(pb))) <= 0.01, (rate, 20 * np.log10(pb.min()), 20 * np.log10(pb.max()))
    assert -20 * np.log10(sb.max()) >= 70.0, (rate, -20 * np.log10(sb.max()))


def _i0(x):
    s = term = 1.0
    q = x * x / 4.0
    k = 1
    while k < 500 and term > 1e-17 * s:
        term *= q / (float(k) * k)
        s += term
        k += 1
    return s


def _stated_table(fi, fo):
    """The resampler's table from Fi to Fo as include/fishtts_hip.h states it, in Python floats (IEEE float64, the
    operations in the order of the design)."""
    g = math.gcd(fi, fo)
    L, M, fmin = fo // g, fi // g, float(min(fi, fo))
    A = 75.0
    beta = 0.1102 * (A - 8.7)
    K = int(math.ceil((A - 7.95) / (2.285 * 2.0 * math.pi * 0.07) * fi / fmin))
    K += K & 1
    fc, half, ib = 0.465 * fmin / (float(L) * fi), 0.5 * K * L, _i0(beta)
    w = np.zeros((L, K), dtype=np.float32)
    for p in range(L):
        for t in range(K):
            j = p + float(K // 2 - 1 - t) * L
            r, x = j / half, math.pi * 2.0 * fc * j
            sinc = 1.0 if j == 0 else math.sin(x) / x
            w[p, t] = np.float32(2.0 * fc * L * sinc * _i0(beta * math.sqrt(max(0.0, 1.0 - r * r))) / ib)
    return L, M, K, w


@pytest.mark.parametrize("rate", [8000, 11025, 12000, 16000, 22050, 24000, 32000, 48000])
def test_output_tables_are_those_of_the_stated_formula(rate):
    """ft_resample_filter went from a design for (44100, rate) to a wrapper of the design for any pair: its tables are,
    bit for bit, the stated formula's."""
    from tests.test_resample_host import filter_table
    L, M, K, w = filter_table(rate)
    sL, sM, sK, sw = _stated_table(FO, rate)
    assert (L, M, K) == (sL, sM, sK)
    assert np.array_equal(w.view(np.uint32), sw.view(np.uint32)), int(np.sum(w.view(np.uint32) != sw.view(np.uint32)))


@pytest.mark.parametrize("rate", [16000, 48000, 192000])
def test_intake_tables_are_those_of_the_stated_formula(rate):
    L, M, K, w = R.filter_table(rate)
    sL, sM, sK, sw = _stated_table(rate, FO)
    assert (L, M, K) == (sL, sM, sK)
    assert np.array_equal(w.view(np.uint32), sw.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_matches_resample_poly(rate):
    """Alignment (zero phase) and gain against an independent polyphase resampler given the same prototype."""
    from scipy.signal import resample_poly
    L, M, K, w = tab = R.filter_table(rate)
    n = 8192 if rate <= 48000 else 24576
    t = np.arange(n) / rate
    fmin = min(rate, FO)
    x = sum(0.3 * np.sin(2 * np.pi * f * t + ph) for f, ph in ((0.25 * fmin, 0.1), (0.11 * fmin, 1.3), (517.0, 2.0)))
    got = R.resample(x, rate, tab)
    c = (K // 2) * L                            # the tap at j = 0; taps run from j = -c to c - 1
    proto = np.zeros(2 * c + 1)
    for tt in range(K):
        proto[np.arange(L) + (K // 2 - 1 - tt) * L + c] = w[:, tt]
    want = resample_poly(x, L, M, window=proto / L)          # (resample_poly multiplies its filter by L)
    assert len(got) == len(want) == -(-n * L // M)
    edge = K
    err = np.max(np.abs(got[edge:-edge] - want[edge:-edge]))
    assert err <= 1e-9, (rate, err)


def test_conversion_and_downmix():
    # every format's scale and extremes
    d, cl, bad = R.decode(R.frames_bytes([[0], [128], [255]], "u8"), "u8", 1)
    assert d[:, 0].tolist() == [-1.0, 0.0, 127 / 128] and cl[:, 0].tolist() == [True, False, True]
    d, cl, _ = R.decode(R.frames_bytes([[-8388608], [-1], [8388607], [4660]], "s24"), "s24", 1)
    assert d[:, 0].tolist() == [-1.0, -1 / 8388608, 8388607 / 8388608, 4660 / 8388608] and cl.sum() == 2
    d, cl, _ = R.decode(R.frames_bytes([[-2147483648], [2147483647], [65536]], "s32"), "s32", 1)
    assert d[:, 0].tolist() == [-1.0, 2147483647 / 2147483648, 65536 / 2147483648] and cl.sum() == 2
    v = np.array([[0.5], [1.0], [-1.5], [np.inf], [np.nan]], dtype=np.float32)
    m, c, b = R.mono(R.frames_bytes(v, "f32"), "f32", 1)
    assert m.tolist() == [0.5, 1.0, -1.5, 0.0, 0.0] and (c, b) == (2, 2)
    # a 16-bit mono file gives v / 32768, as the reference's reader does
    pcm = np.array([-32768, -3, 0, 12345, 32767], dtype=np.int16)
    m, c, _ = R.mono(pcm.tobytes(), "s16", 1)
    assert np.array_equal(m, pcm.astype(np.float32) / 32768.0) and c == 2
    # the mean is rounded once; one channel alone is that channel
    st = np.array([[3, 4], [32767, -32768], [7, -7]])
    m, c, _ = R.mono(R.frames_bytes(st, "s16"), "s16", 2)
    assert m.tolist() == [np.float32(3.5 / 32768), np.float32(-0.5 / 32768), 0.0] and c == 2
    m, c, _ = R.mono(R.frames_bytes(st, "s16"), "s16", 2, channel=1)
    assert m.tolist() == [4 / 32768, -1.0, -7 / 32768] and c == 1
