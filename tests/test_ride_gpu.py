"""GPU: the ride stage (ride_hop_kernel, ride_node_kernel, ride_apply_kernel).  ft_codec_ride against the float64
restatement tests/ride_ref.py at five rates; carried streams of the stage alone (ft_test_ride_streams) against ft_codec_ride,
bit for bit, whatever the chunking and the neighbours; codec streams with a live target against ride() over the same stream
without it, bit for bit; and the refusals.

Bounds (from the issue that asked for the stage; the level stage's own, profiles/r14_level.txt): every node within 4e-7
relative of the restatement's (1.2e-7 from the measure, two float32 roundings); every sample within (4e-7 + 2^-23) |y_ref|
(the node bound plus the roundings of the interpolation and the product); silence returned bit for bit; max |y| at most
c (1 + 2^-22); a repeated call the same bits.  Every input has a gate distance of at least 1e-6 LU in the restatement
(asserted), so that no block of any node's measure can change sides through rounding."""
import ctypes as CT

import numpy as np
import pytest

from tests import ride_ref as RR
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.level_ref import RATES
from tests.test_codec_gpu import make_codec
from tests.test_timescale_gpu import _codes

pytestmark = pytest.mark.gpu

A = RR.A
LONG_HOPS = 2 * 64 + 5     # ride_node_kernel's 64 threads take the blocks of a measure in three passes; ride_hop_kernel runs three workgroups
MAX_FRAMES = 9600          # ft_codec_ride takes 2 * max_frames * frame_len * 48000 / 44100 samples: the long input at 48 kHz
TARGET = -1600


@pytest.fixture(scope="module")
def tiny():
    eng, _ = make_codec(tiny_codec_shape(), max_frames=MAX_FRAMES)
    yield eng
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def lengths(H):
    return (0, 1, H - 1, H, 4 * H - 1, 4 * H, (A + 1) * H - 1, (A + 1) * H, (A + 1) * H + 1, LONG_HOPS * H)


def inputs(rate):
    """name -> x float32.  Seeds were picked on the CPU for a gate distance >= 1e-6 LU (asserted by the tests)."""
    H = RR.hop(rate)
    rng = np.random.default_rng(rate + 1)
    xs = {}
    for n in lengths(H):
        xs[f"noise {n}"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    n = int(2.5 * rate)
    t = np.arange(n) / rate
    env = np.zeros(n)
    env[(t >= 0.1) & (t < 0.9)] = 0.2
    env[(t >= 1.1) & (t < 1.7)] = 0.2 * 10.0 ** (-15.0 / 20.0)
    env[(t >= 1.9) & (t < 2.4)] = 0.2
    xs["bursts"] = (env * rng.standard_normal(n) + 0.05).astype(np.float32)
    xs["silence"] = np.zeros(13 * H + 3, dtype=np.float32)
    x = 1e-3 * rng.standard_normal(14 * H + 5)
    x[::H // 3] = 0.97
    x[5 * H + 11] = -0.97
    xs["impulses"] = x.astype(np.float32)
    xs["step"] = RR.step_signal(rate, seed=rate)
    return xs


@pytest.fixture(scope="module")
def refs():
    """The restatement of every input at TARGET, computed once."""
    return {(rate, name): (x, RR.ride(x, rate, TARGET)) for rate in RATES for name, x in inputs(rate).items()}


@pytest.mark.parametrize("rate", RATES)
def test_ride_against_the_restatement(tiny, refs, rate):
    H = RR.hop(rate)
    capped = 0
    for (r, name), (x, ref) in refs.items():
        if r != rate:
            continue
        assert ref.margin >= 1e-6, (rate, name, ref.margin)
        y, g = tiny.ride(x, rate, TARGET / 100.0, nodes=True)
        assert len(g) == -(-len(x) // H) + 1 and len(y) == len(x), (rate, name)
        rel = float(np.max(np.abs(g.astype(np.float64) / ref.g - 1.0)))
        err = float(np.max(np.abs(y.astype(np.float64) - ref.y) / np.maximum(np.abs(ref.y.astype(np.float64)), 1e-30))) if len(x) else 0.0
        print(f"{rate} {name}: nodes {len(g)}, node err {rel:.2e}, sample err {err:.2e}, capped {ref.capped}, "
              f"peak/c - 1 {(np.max(np.abs(y)) / RR.CEILING - 1) if len(y) else -1:.2e}, margin {ref.margin:.3g}")
        assert RR.check(g, y, ref) == [], (rate, name)
        if name == "silence":
            assert np.all(g == 1.0) and np.array_equal(_bits(y), _bits(x)), (rate, name)
        y2, g2 = tiny.ride(x, rate, TARGET / 100.0, nodes=True)
        assert np.array_equal(_bits(y2), _bits(y)) and np.array_equal(_bits(g2), _bits(g)), (rate, name)
        capped += ref.capped
    assert capped > 0, "no input reached the peak guard"


def _chunkings(H, longest, seed):
    rng = np.random.default_rng(seed)
    cuts = sorted(int(c) for c in rng.integers(0, longest, 9))
    rand = cuts[:3] + [cuts[2]] + cuts[3:] + [cuts[-1]] + [longest + 5, longest + 5]     # empty chunks, a tail-only final
    alt, at = [], 0
    while at < longest:
        at += H + (1 if len(alt) % 2 else -1)
        alt.append(at)
    return {"one": [], "hops": list(range(H, longest + H, H)), "H+-1": alt, "random": rand}


@pytest.mark.parametrize("rate", RATES)
def test_streams_equal_the_whole_call(tiny, rate):
    H = RR.hop(rate)
    xs_all = inputs(rate)
    xs = [xs_all["step"], xs_all["bursts"], xs_all[f"noise {(A + 1) * H + 1}"]]
    whole = [tiny.ride(x, rate, TARGET / 100.0, nodes=True) for x in xs]
    longest = max(len(x) for x in xs)
    for name, cuts in _chunkings(H, longest, rate).items():
        ys, gs, emitted = tiny.test_ride_streams(xs, rate, TARGET, cuts)
        for b, (x, (y, g)) in enumerate(zip(xs, whole)):
            assert np.array_equal(_bits(ys[b]), _bits(y)), (rate, name, b)
            assert np.array_equal(_bits(gs[b]), _bits(g)), (rate, name, b)
            seen = 0
            for j, c in enumerate(cuts + [None]):
                now = len(x) if c is None else min(c, len(x))
                want = tiny.ride_plan(rate, now, c is None)[1] - tiny.ride_plan(rate, seen, False)[1]
                assert emitted[j, b] == want, (rate, name, b, j)
                assert tiny.ride_plan(rate, now, c is None) == RR.plan(now, H, c is None)
                seen = now
            assert emitted[:, b].sum() == len(x)
    # a stream's result does not change when its neighbours do
    others = [xs[0], xs_all["impulses"], xs_all["silence"]]
    ys, gs, _ = tiny.test_ride_streams(others, rate, TARGET, _chunkings(H, longest, rate)["random"])
    assert np.array_equal(_bits(ys[0]), _bits(whole[0][0])) and np.array_equal(_bits(gs[0]), _bits(whole[0][1]))
    assert np.array_equal(_bits(ys[2]), _bits(others[2]))


def test_codec_streams_with_a_live_target(tiny):
    shape = tiny_codec_shape()
    fl = tiny.frame_len
    for kw in ({"sample_rate": 16000}, {"speed": 1.25, "pitch": 3}):
        rate = kw.get("sample_rate", 44100)
        H = RR.hop(rate)
        T = int(-(-(A + 3) * H * 44100 * kw.get("speed", 1.0) // (rate * fl))) + 7     # at least A + 3 hops of output
        codes = _codes(shape, T, 11)
        live, bare, plain = tiny.stream(live_loudness=TARGET / 100.0, **kw), tiny.stream(**kw), tiny.stream()
        got, ref, direct = [], [], []
        cuts = [0, 5, 5 + T // 3, T - 2, T]
        for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            final = j == len(cuts) - 2
            out = tiny.decode_streams([live, plain, bare], [codes[:, a:b]] * 3, [final, False, final])
            got.append(out[0]); direct.append(out[1]); ref.append(out[2])
        got, ref = np.concatenate(got), np.concatenate(ref)
        assert len(got) == len(ref) >= (A + 3) * H and live.finished
        want = tiny.ride(ref, rate, TARGET / 100.0)
        assert np.array_equal(_bits(got), _bits(want)), kw
        assert not np.array_equal(_bits(got), _bits(ref)), kw
        whole = tiny.stream()
        assert np.array_equal(_bits(np.concatenate(direct)), _bits(whole.decode(codes))), kw
        for s in (live, bare, plain, whole):
            s.close()


def test_refusals_before_device_work(tiny):
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import HipError
    lib = tiny.lib
    x = np.zeros(64, dtype=np.float32)
    y = np.full(64, 7.0, dtype=np.float32)
    for bad in (-5001, -499, 1, 100, -1):
        assert lib.ft_codec_ride(tiny._h, x.ctypes.data_as(CT.c_void_p), 64, 16000, bad, y.ctypes.data_as(CT.c_void_p), None) == L.FT_ERR_ARG
        h = CT.c_void_p()
        assert lib.ft_codec_stream_begin_live(tiny._h, 16000, 100, 0, bad, CT.byref(h)) == L.FT_ERR_ARG and not h
    assert np.all(y == 7.0)
    assert lib.ft_codec_ride(tiny._h, x.ctypes.data_as(CT.c_void_p), 64, 44101, TARGET, y.ctypes.data_as(CT.c_void_p), None) == L.FT_ERR_ARG
    assert lib.ft_codec_ride(tiny._h, None, 64, 16000, TARGET, y.ctypes.data_as(CT.c_void_p), None) == L.FT_ERR_ARG
    assert lib.ft_codec_ride(tiny._h, x.ctypes.data_as(CT.c_void_p), 64, 16000, TARGET, None, None) == L.FT_ERR_ARG
    assert lib.ft_ride_plan(44101, 5, 0, None, None) == L.FT_ERR_ARG and lib.ft_ride_plan(16000, -1, 0, None, None) == L.FT_ERR_ARG
    for bad in (-50.01, -4.99, 0, float("nan"), True, "loud"):
        with pytest.raises(ValueError):
            tiny.stream(live_loudness=bad)
    # the two plain stream calls refuse a live stream; a chunk after final is refused
    shape = tiny_codec_shape()
    codes = _codes(shape, 4, 3)
    live = tiny.stream(live_loudness=-16)
    audio = np.zeros(4 * tiny.frame_len, dtype=np.float32)
    lens = np.array([4], dtype=np.int32)
    handles = (CT.c_void_p * 1)(live._h.value)
    assert lib.ft_codec_stream_decode(tiny._h, live._h, codes.ctypes.data_as(CT.c_void_p), 4, audio.ctypes.data_as(CT.c_void_p)) == L.FT_ERR_STATE
    assert lib.ft_codec_stream_decode_many(tiny._h, 1, handles, codes.ctypes.data_as(CT.c_void_p), lens.ctypes.data_as(CT.c_void_p),
                                           audio.ctypes.data_as(CT.c_void_p)) == L.FT_ERR_STATE
    assert live.frames == 0
    out = live.decode(codes, final=True)
    assert len(out) == 4 * tiny.frame_len and live.finished
    with pytest.raises(HipError, match="final chunk went out"):
        live.decode(codes)
    live.close()
