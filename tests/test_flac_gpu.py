"""GPU: the FLAC stage through the C ABI (include/fishtts_hip.h: "FLAC"; ft_codec_flac, CodecHipEngine.flac) against its
restatement tests/flac_ref.py, over the cases of tests/flac_cases.py.  Every comparison is exact: the stream's bytes, and
ft_flac_info against the reference's census."""
import ctypes as C

import numpy as np
import pytest

from tests import flac_cases as FC
from tests import flac_ref as R
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec(tiny_codec_shape())
    yield e
    e.close()


def _first_difference(got: bytes, want: bytes) -> str:
    if got == want:
        return ""
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}; first difference at byte {at}: {got[at:at + 8].hex()} against {want[at:at + 8].hex()}"


@pytest.mark.parametrize("name", [c[0] for c in FC.CASES])
def test_stream_is_the_references(eng, name):
    _, x, rate, B = FC.BY_NAME[name]
    want, census, pcm = FC.reference(name)
    got, rep = eng.flac(x, rate, B)
    assert got == want, _first_difference(got, want)
    assert (rep.frames, rep.bytes, rep.min_frame, rep.max_frame) == (census.frames, census.bytes, census.min_frame, census.max_frame)
    assert rep.kinds == census.kinds and rep.assignments == census.assignments
    assert sum(rep.kinds) == census.frames * (1 if pcm.ndim == 1 else 2) and sum(rep.assignments) == census.frames


def test_int16_and_float_inputs_of_the_same_samples_agree(eng):
    """fmt 1 takes the samples as they are: the quantised samples of a float case, given as int16, give that case's stream."""
    _, x, rate, B = FC.BY_NAME["speech_B1024"]
    pcm = R.quantise(x).astype(np.int16)
    got16, _ = eng.flac(pcm, rate, B)
    assert got16 == FC.reference("speech_B1024")[0]


def test_a_repeated_call_gives_the_same_bytes(eng):
    for name in ("st_speech_pair", "speech_B256", "frames130"):
        _, x, rate, B = FC.BY_NAME[name]
        first, rep1 = eng.flac(x, rate, B)
        again, rep2 = eng.flac(x, rate, B)
        assert first == again and rep1 == rep2, name


def _call(eng, x, fmt, n, channels, rate, B, cap, reserved=0, null=None):
    from fish_tts_amd import _lib as L
    out = np.full(min(max(cap, 1), 1 << 16) + 16, 0xA5, dtype=np.uint8)       # (a refused call's capacity need not be there)
    total = C.c_int64(-7)
    info = L.ft_flac_info()
    info.frames = -7
    fp = L.ft_flac_params(B, reserved)
    args = dict(x=x.ctypes.data_as(C.c_void_p), fp=C.byref(fp), out=out.ctypes.data_as(C.c_void_p), total=C.byref(total),
                info=C.byref(info))
    if null:
        args[null] = None
    st = eng.lib.ft_codec_flac(eng._h, args["x"], fmt, n, channels, rate, args["fp"], args["out"], cap, args["total"], args["info"])
    untouched = bool((out == 0xA5).all()) and total.value == -7 and info.frames == -7
    return st, untouched, out, total.value


def test_refusals_write_nothing(eng):
    from fish_tts_amd import _lib as L
    x = np.zeros(600, dtype=np.float32)
    bound = int(eng.lib.ft_flac_bound(300, 2, 256))
    assert bound == 42 + 2 * 19 + 4 * 300
    ok = dict(fmt=0, n=300, channels=2, rate=44100, B=256, cap=bound)
    st, untouched, out, total = _call(eng, x, **ok)
    assert st == L.FT_OK and not untouched and 42 < total <= bound
    assert (out[bound:] == 0xA5).all()
    want = R.encode(np.zeros((300, 2), dtype=np.int32), 44100, 256)
    assert out[:total].tobytes() == want
    # a capacity one byte short
    st, untouched, _, _ = _call(eng, x, **dict(ok, cap=bound - 1))
    assert st == L.FT_ERR_ARG and untouched
    assert b"capacity" in eng.lib.ft_last_error(eng._h)
    # every other refusal, each alone
    for change, status, word in ((dict(fmt=2), L.FT_ERR_ARG, b"fmt"), (dict(fmt=-1), L.FT_ERR_ARG, b"fmt"),
                                 (dict(channels=0), L.FT_ERR_ARG, b"channels"), (dict(channels=3), L.FT_ERR_ARG, b"channels"),
                                 (dict(rate=7999), L.FT_ERR_ARG, b"sample rate"), (dict(rate=48001), L.FT_ERR_ARG, b"sample rate"),
                                 (dict(B=0), L.FT_ERR_ARG, b"blocksize"), (dict(B=300), L.FT_ERR_ARG, b"blocksize"),
                                 (dict(B=8192), L.FT_ERR_ARG, b"blocksize"), (dict(reserved=1), L.FT_ERR_ARG, b"reserved"),
                                 (dict(n=0), L.FT_ERR_ARG, b"n < 1"), (dict(n=-1), L.FT_ERR_ARG, b"n < 1"),
                                 (dict(n=(1 << 28) + 1, cap=1 << 40), L.FT_ERR_TOO_LONG, b"2^28"),
                                 (dict(cap=0), L.FT_ERR_ARG, b"capacity"), (dict(cap=-1), L.FT_ERR_ARG, b"capacity")):
        st, untouched, _, _ = _call(eng, x, **dict(ok, **change))
        assert st == status and untouched, change
        assert word in eng.lib.ft_last_error(eng._h), (change, eng.lib.ft_last_error(eng._h))
    for null in ("x", "fp", "out", "total", "info"):
        st, untouched, _, _ = _call(eng, x, **ok, null=null)
        assert st == L.FT_ERR_ARG and untouched, null
    # the order: the earlier reason wins
    st, _, _, _ = _call(eng, x, **dict(ok, fmt=5, channels=9, rate=1, B=7, n=0, cap=0))
    assert st == L.FT_ERR_ARG and b"fmt" in eng.lib.ft_last_error(eng._h)
    st, _, _, _ = _call(eng, x, **dict(ok, B=7, n=(1 << 28) + 1, cap=0))
    assert st == L.FT_ERR_ARG and b"blocksize" in eng.lib.ft_last_error(eng._h)
    # ... and the engine still encodes
    st, untouched, out, total = _call(eng, x, **ok)
    assert st == L.FT_OK and out[:total].tobytes() == want


def test_engine_method_checks_its_arguments(eng):
    x = np.zeros(10, dtype=np.float32)
    for bad in (dict(blocksize=300), dict(blocksize=True), dict(blocksize=4096.0), dict(sample_rate=7000)):
        with pytest.raises(ValueError):
            eng.flac(x, **bad)
    for bad in (np.zeros((10, 3), dtype=np.float32), np.zeros((2, 2, 2), dtype=np.float32), np.zeros(0, dtype=np.float32),
                np.zeros(10, dtype=np.int32), np.zeros(10, dtype=complex)):
        with pytest.raises(ValueError):
            eng.flac(bad)
    data, rep = eng.flac(np.zeros(10, dtype=np.float64))                # float64 is brought to float32
    assert R.decode(data).n == 10 and rep.frames == 1
