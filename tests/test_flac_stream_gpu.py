"""GPU: the live FLAC stage through the C ABI (include/fishtts_hip.h: "Live FLAC"; ft_codec_flac_stream_*,
CodecHipEngine.flac_stream) against tests/flac_ref.py and against ft_codec_flac on the same context, over inputs of
tests/flac_cases.py in several cuttings each.  Every comparison is exact.  The properties are the header's "it follows":
(1) the pushes' bytes concatenate to the one-shot stream behind its 42 leading bytes, (2) the head after the final push is the
one-shot call's and the head before it is the format's "unknown" one, (3) every push emits ft_flac_stream_plan's frames within
its byte bound and the final report is the one-shot call's, (4) streams and one-shot calls interleaved on one context leave
one another's bytes alone.  Every refusal is a host check: no test provokes a device fault."""
import ctypes as C

import numpy as np
import pytest

from tests import flac_cases as FC
from tests import flac_ref as R
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec

pytestmark = pytest.mark.gpu

NAMES = ["n1_mono", "n1_stereo", "n255", "n256", "n257", "n767", "last4", "last5_sine", "constant", "B1024_last257",
         "B1024_last700", "spike_long_run", "frames130", "frames2050", "speech_B256", "speech_B4096", "st_quiet_right",
         "st_speech_pair", "st_white_full", "float_edges", "float_edges_stereo"]


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(tiny_codec_shape())
    yield e
    e.close()


def _taken(sizes, n):
    """The sizes cut to the n samples there are: each at most what is left, the rest in a last push of its own."""
    out, left = [], n
    for k in sizes:
        out.append(min(k, left))
        left -= out[-1]
    return out + [left]


def _until(make, n):
    """Sizes from make(i), i = 0, 1, ..., until n samples are covered (the last one cut to fit)."""
    out, left, i = [], n, 0
    while left > 0:
        out.append(min(make(i), left))
        left -= out[-1]
        i += 1
    return out or [0]


def cuttings(n: int, B: int) -> dict:
    """name -> the push sizes; the last push of each is the final one."""
    rng = np.random.default_rng(1234 + n + B)
    draws = rng.integers(0, 3 * B + 1, 4 + 2 * (n // B + 1))
    draws[::5] = 0                                                       # empty pushes among them
    odd = B + 1 if B % 2 == 0 else B                                     # 3, 5, ..., 2 B + 1, then 3 again
    out = {
        "one final push": [n],
        "every multiple of B, then an empty final push": [B] * (n // B) + ([n % B] if n % B else []) + [0],
        "B - 1, 1, 1, B + 1, the rest": _taken([B - 1, 1, 1, B + 1], n),
        "random sizes in 0 .. 3 B": _until(lambda i: int(draws[i]) if i < len(draws) else B, n) + [0],
        "odd sizes only": _until(lambda i: 3 + 2 * (i % odd), n),
    }
    if n <= 767:
        out["one sample per push"] = [1] * n
    for sizes in out.values():
        assert sum(sizes) == n and min(sizes) >= 0
    return out


def _first_difference(got: bytes, want: bytes) -> str:
    if got == want:
        return ""
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}; first difference at byte {at}: {got[at:at + 8].hex()} against {want[at:at + 8].hex()}"


def _plan(eng, B, ch, before, n, final):
    frames, nbytes = C.c_int64(-1), C.c_int64(-1)
    assert eng.lib.ft_flac_stream_plan(B, ch, before, n, 1 if final else 0, C.byref(frames), C.byref(nbytes)) == 0
    return frames.value, nbytes.value


def _stream(eng, x, rate, B, sizes, check_plan=True):
    """(head before, [bytes per push], head after, final report) of x pushed in `sizes`; each push against the plan."""
    ch = x.ndim
    with eng.flac_stream(rate, ch, B, np.int16 if x.dtype == np.int16 else np.float32) as fs:
        before, outs, at, frames = fs.head(), [], 0, 0
        for i, k in enumerate(sizes):
            final = i + 1 == len(sizes)
            want_frames, bound = _plan(eng, B, ch, at, k, final)
            outs.append(fs.push(x[at:at + k], final=final))
            if check_plan:
                now = fs.report().frames
                assert now - frames == want_frames and len(outs[-1]) <= bound, (i, k, now - frames, want_frames, len(outs[-1]), bound)
                assert (len(outs[-1]) == 0) == (want_frames == 0)
                frames = now
            at += k
        return before, outs, fs.head(), fs.report()


ONE_SHOT = {}


def _one_shot(eng, name):
    if name not in ONE_SHOT:
        _, x, rate, B = FC.BY_NAME[name]
        ONE_SHOT[name] = eng.flac(x, rate, B)
    return ONE_SHOT[name]


@pytest.mark.parametrize("name", NAMES)
def test_any_cutting_gives_the_one_shot_stream(eng, name):
    _, x, rate, B = FC.BY_NAME[name]
    want, census, pcm = FC.reference(name)
    shot, shot_rep = _one_shot(eng, name)
    assert shot == want
    unknown = R.streaminfo(B, 0, 0, rate, x.ndim, 0)                     # (the eight marker bytes in front included)
    assert len(unknown) == 42 and unknown[:8] == b"fLaC" + bytes([0x80, 0, 0, 34])
    decoded = False
    for what, sizes in cuttings(len(x), B).items():
        before, outs, after, rep = _stream(eng, x, rate, B, sizes)
        got = b"".join(outs)
        assert got == want[42:], f"{what}: {_first_difference(got, want[42:])}"                     # property 1
        assert got == shot[42:] and after == shot[:42] == want[:42], what                           # properties 1, 2
        assert before == unknown, what
        assert rep == shot_rep, (what, rep, shot_rep)                                                # property 3
        assert (rep.frames, rep.bytes, rep.min_frame, rep.max_frame) == (census.frames, census.bytes, census.min_frame, census.max_frame)
        assert rep.kinds == census.kinds and rep.assignments == census.assignments
        if not decoded:                          # (the bytes of every cutting are these: one decode of each form serves all)
            for head in (before, after):
                d = R.decode(head + got)
                assert np.array_equal(d.pcm.reshape(pcm.shape), pcm) and d.rate == rate and d.channels == x.ndim, what
            decoded = True


def test_int16_pushes_of_a_float_case_give_its_stream(eng):
    """fmt 1 takes the samples as they are, and the carry is the same whatever fmt is."""
    _, x, rate, B = FC.BY_NAME["speech_B1024"]
    pcm = R.quantise(x).astype(np.int16)
    _, outs, after, _ = _stream(eng, pcm, rate, B, cuttings(len(pcm), B)["odd sizes only"])
    want = FC.reference("speech_B1024")[0]
    assert after + b"".join(outs) == want


def test_interleaved_streams_and_one_shot_calls_leave_each_other_alone(eng):
    """Property 4: a mono and a stereo stream pushed alternately, a one-shot call between their pushes."""
    _, xm, rm, Bm = FC.BY_NAME["speech_B256"]
    _, xs, rs, Bs = FC.BY_NAME["st_speech_pair"]
    _, xo, ro, Bo = FC.BY_NAME["st_quiet_right"]
    cm, cs = cuttings(len(xm), Bm)["random sizes in 0 .. 3 B"], cuttings(len(xs), Bs)["odd sizes only"]
    want_o = FC.reference("st_quiet_right")[0]
    with eng.flac_stream(rm, 1, Bm, np.float32) as fm, eng.flac_stream(rs, 2, Bs, np.float32) as fs:
        got_m, got_s, am, as_ = [], [], 0, 0
        for i in range(max(len(cm), len(cs))):
            if i < len(cm):
                got_m.append(fm.push(xm[am:am + cm[i]], final=i + 1 == len(cm)))
                am += cm[i]
            if i % 7 == 0:
                assert eng.flac(xo, ro, Bo)[0] == want_o
            if i < len(cs):
                got_s.append(fs.push(xs[as_:as_ + cs[i]], final=i + 1 == len(cs)))
                as_ += cs[i]
        assert fm.head() + b"".join(got_m) == FC.reference("speech_B256")[0]
        assert fs.head() + b"".join(got_s) == FC.reference("st_speech_pair")[0]
        assert fm.report().frames == FC.reference("speech_B256")[1].frames


def _push(eng, h, x, n, final, cap, null=None):
    out = np.full(min(max(cap, 1), 1 << 16) + 16, 0xA5, dtype=np.uint8)       # (a refused push's capacity need not be there)
    got = C.c_int64(-7)
    args = dict(fs=h, x=x.ctypes.data_as(C.c_void_p), out=out.ctypes.data_as(C.c_void_p), got=C.byref(got))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_flac_stream_push(args["fs"], args["x"], n, 1 if final else 0, args["out"], cap, args["got"])
    return st, bool((out == 0xA5).all()) and got.value == -7, out[:max(got.value, 0)].tobytes()


def test_refused_pushes_leave_the_stream_as_it_was(eng):
    from fish_tts_amd import _lib as L
    _, x, rate, B = FC.BY_NAME["n767"]
    want = FC.reference("n767")[0]
    fp = L.ft_flac_params(B, 0)
    h = C.c_void_p()
    assert eng.lib.ft_codec_flac_stream_begin(eng._h, 1, 1, rate, C.byref(fp), C.byref(h)) == L.FT_OK
    try:
        st, _, a = _push(eng, h, x[:300], 300, False, 1 << 16)
        assert st == L.FT_OK
        info = L.ft_flac_info()
        assert eng.lib.ft_codec_flac_stream_info(h, C.byref(info)) == L.FT_OK and info.frames == 1
        _, bound = _plan(eng, B, 1, 300, 300, False)
        for change, status, word in ((dict(cap=bound - 1), L.FT_ERR_ARG, b"capacity"), (dict(cap=0), L.FT_ERR_ARG, b"capacity"),
                                     (dict(n=(1 << 28) + 1, cap=1 << 40), L.FT_ERR_TOO_LONG, b"2^28"),
                                     (dict(n=-1), L.FT_ERR_ARG, b"n < 0"), (dict(null="x"), L.FT_ERR_ARG, b"x is null"),
                                     (dict(null="out"), L.FT_ERR_ARG, b"null pointer"), (dict(null="got"), L.FT_ERR_ARG, b"null pointer"),
                                     (dict(n=-1, null="out", cap=0), L.FT_ERR_ARG, b"null pointer"),
                                     (dict(n=(1 << 28) + 1, cap=0), L.FT_ERR_TOO_LONG, b"2^28")):
            st, untouched, _ = _push(eng, h, x[300:600], **dict(dict(n=300, final=False, cap=bound), **change))
            assert st == status and untouched, change
            assert word in eng.lib.ft_last_error(eng._h), (change, eng.lib.ft_last_error(eng._h))
            again = L.ft_flac_info()
            assert eng.lib.ft_codec_flac_stream_info(h, C.byref(again)) == L.FT_OK and bytes(again) == bytes(info), change
        assert _push(eng, None, x, 1, False, 1 << 16)[0] == L.FT_ERR_ARG
        st, _, b = _push(eng, h, x[300:600], 300, False, bound)
        assert st == L.FT_OK
        st, _, c = _push(eng, h, x[600:], len(x) - 600, True, 1 << 16)
        assert st == L.FT_OK
        assert a + b + c == want[42:]                                    # the refused pushes changed no byte of the later ones
        head = (C.c_uint8 * 42)()
        assert eng.lib.ft_codec_flac_stream_head(h, head) == L.FT_OK and bytes(head) == want[:42]
        # a push after the final one, empty or not
        for n in (0, 5):
            st, untouched, _ = _push(eng, h, x, n, n == 0, 1 << 16)
            assert st == L.FT_ERR_STATE and untouched and b"after the final" in eng.lib.ft_last_error(eng._h)
        assert eng.lib.ft_codec_flac_stream_head(h, head) == L.FT_OK and bytes(head) == want[:42]
    finally:
        eng.lib.ft_codec_flac_stream_end(h)


def test_begin_checks_in_the_one_shot_calls_order(eng):
    from fish_tts_amd import _lib as L
    for args, word in (((1, 2, 44100, 256, 0), b"fmt"), ((3, 0, 44100, 256, 0), b"channels"), ((2, 0, 7999, 256, 0), b"sample rate"),
                       ((1, 1, 44100, 300, 0), b"blocksize"), ((1, 1, 44100, 256, 1), b"reserved"), ((3, 2, 1, 7, 1), b"fmt"),
                       ((3, 1, 1, 7, 1), b"channels")):
        ch, fmt, rate, B, reserved = args
        fp = L.ft_flac_params(B, reserved)
        h = C.c_void_p()
        assert eng.lib.ft_codec_flac_stream_begin(eng._h, ch, fmt, rate, C.byref(fp), C.byref(h)) == L.FT_ERR_ARG and not h.value, args
        assert word in eng.lib.ft_last_error(eng._h), (args, eng.lib.ft_last_error(eng._h))
    assert eng.lib.ft_codec_flac_stream_begin(eng._h, 1, 0, 44100, None, C.byref(C.c_void_p())) == L.FT_ERR_ARG
    eng.lib.ft_codec_flac_stream_end(None)


def test_engine_methods_check_their_arguments(eng):
    for bad in (dict(blocksize=300), dict(blocksize=True), dict(channels=3), dict(channels=0), dict(dtype=np.int32),
                dict(dtype=np.float64), dict(sample_rate=7000)):
        with pytest.raises(ValueError):
            eng.flac_stream(**bad)
    with eng.flac_stream(channels=2, blocksize=256, dtype=np.int16) as fs:
        for bad in (np.zeros(10, dtype=np.int16), np.zeros((10, 3), dtype=np.int16), np.zeros((10, 2), dtype=np.float32),
                    np.zeros((10, 2), dtype=np.int32)):
            with pytest.raises(ValueError):
                fs.push(bad)
        assert fs.push(None) == b"" and fs.push(np.zeros((0, 2), dtype=np.int16)) == b""
        data = fs.push(np.zeros((300, 2), dtype=np.int16)) + fs.push(final=True)
        assert fs.head() + data == R.encode(np.zeros((300, 2), dtype=np.int32), 44100, 256)
        with pytest.raises(Exception):
            fs.push(np.zeros((1, 2), dtype=np.int16))                   # FT_ERR_STATE: the stream has ended
    with pytest.raises(RuntimeError):
        fs.push(None)
    with pytest.raises(RuntimeError):
        fs.head()
