"""GPU: the join stage behind synthesize_long (join_edges_kernel, join_layout_kernel, join_assemble_kernel) - through the
test hook ft_test_join against the numpy restatement tests/join_ref.py, compared as bit patterns, with the total, the cuts
and the sentinel past the output; then ft_codec_decode_join with the identity parameters against the rows of
ft_codec_decode_fxp, and CodecHipEngine.decode_join's grouping into native calls.  All comparisons are exact."""
import ctypes as CT

import numpy as np
import pytest

from tests import join_ref as J
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec
from tests.test_timescale_gpu import _codes

pytestmark = pytest.mark.gpu

THR = 0.1
P44 = (THR, 220, 1323, 220)        # synthesize_long's parameters at 44100 Hz ...
P8 = (THR, 40, 240, 40)            # ... and at 8000 Hz
SENTINEL = 0xFFFFFFFE


@pytest.fixture(scope="module")
def tiny():
    eng, _ = make_codec(tiny_codec_shape(), max_frames=2048)
    yield eng
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _quiet(rng, n, loud=()):
    """n samples well below THR, with samples of 0.5 at `loud`."""
    x = rng.uniform(-0.01, 0.01, n).astype(np.float32)
    for i in loud:
        x[i] = 0.5 if i % 2 else -0.5
    return x


def _check(eng, items, params, gaps, started=0, what=None):
    y, total, cuts = eng.test_join(items, params, gaps, started)
    want, wcuts, s = J.join(items, params[0], params[1], params[2], params[3], gaps, started)
    assert total == len(want), (what, total, len(want))
    assert cuts.tolist() == wcuts.tolist(), (what, cuts.tolist(), wcuts.tolist())
    assert np.array_equal(_bits(y[:total]), _bits(want)), (what, int(np.argmax(_bits(y[:total]) != _bits(want))))
    assert np.all(_bits(y[total:]) == SENTINEL), (what, "the stage wrote past its output")
    return y[:total], cuts, s


@pytest.mark.parametrize("params", [P44, P8], ids=["44k", "8k"])
def test_lengths_and_batches(tiny, params):
    H = params[1]
    lengths = [0, 1, H - 1, H, 3 * H + 7, 20 * H + 3]
    rng = np.random.default_rng(H)
    for B in range(1, 6):
        for rot in range(len(lengths)):
            ns = [lengths[(rot + b) % len(lengths)] for b in range(B)]
            items = [rng.uniform(-0.12, 0.12, n).astype(np.float32) for n in ns]      # about one sample in six is loud
            gaps = [int(g) for g in rng.integers(0, 3, B)]
            for started in (0, 1):
                _check(tiny, items, params, gaps, started, (B, ns, gaps, started))
            _check(tiny, items, (0.5, H, params[2], params[3]), gaps, 0, ("all silent", B, ns))


@pytest.mark.parametrize("params", [P44, P8], ids=["44k", "8k"])
def test_edges_fades_and_alignment(tiny, params):
    thr, H, keep, F = params
    rng = np.random.default_rng(7)
    n = 20 * H + 3
    last = n - 1
    cases = {
        "first window only": [_quiet(rng, n, [H - 1])],
        "last window only": [_quiet(rng, n, [last])],
        "first and last": [_quiet(rng, n, [0, last])],
        "short pieces": [_quiet(rng, n, [9 * H + 1]), _quiet(rng, H - 1, [3]), _quiet(rng, 1, [0]), _quiet(rng, 3, [1])],
        "odd cuts": [_quiet(rng, n, [(keep // H + 2) * H + 5, 15 * H]), _quiet(rng, n, [(keep // H + 3) * H])],
        "nan": [_quiet(rng, n, [10 * H])],
    }
    cases["nan"][0][10 * H + H // 2] = np.nan            # not loud; it lies between the ramps and comes through as it is
    cases["nan"][0][2] = np.nan
    for name, items in cases.items():
        for kp, fd in ((keep, F), (0, F), (keep, 0), (1, 1), (0, 10 * H)):
            if name == "nan" and kp == 0:
                continue                                 # (a one-window piece is faded throughout)
            _, cuts, _ = _check(tiny, items, (thr, H, kp, fd), [1] * len(items), 0, (name, kp, fd))
            if name == "short pieces" and kp == 0:
                assert all(e - a < 2 * fd for a, e in cuts.tolist())       # f = m / 2: the ramps meet
    a = J.edges(cases["odd cuts"][0], thr, H, 1)[0]
    assert a > 0 and a % 4 != 0, a                       # (keep = 1) the source offset is not a multiple of 16 bytes
    # a sample exactly at the threshold is loud, one ulp below is not
    t32 = np.float32(thr)
    for v, loud in ((t32, True), (np.nextafter(t32, np.float32(0), dtype=np.float32), False)):
        x = np.zeros(5 * H, dtype=np.float32)
        x[2 * H + 1] = -v
        _, cuts, _ = _check(tiny, [x], (thr, H, 0, 0), [0], 0, ("threshold", loud))
        assert cuts.tolist() == ([[2 * H, 3 * H]] if loud else [[0, 0]])


def test_64_short_items_and_gaps(tiny):
    rng = np.random.default_rng(3)
    items = [rng.uniform(-0.3, 0.3, int(n)).astype(np.float32) for n in rng.integers(1, 51, 64)]
    for params in (P44, P8, (THR, 4, 3, 2)):
        for gaps in ([0] * 64, [1] * 64, [int(g) for g in rng.integers(0, 2, 64)]):
            _check(tiny, items, params, gaps, 0, ("64 items", params))
    _check(tiny, items, (THR, 4, 3, 2), [5] * 64, 1, "64 items, started")


def test_identity_parameters_concatenate(tiny):
    rng = np.random.default_rng(4)
    items = [rng.standard_normal(n).astype(np.float32) for n in (221, 0, 1, 4403, 7)]
    gaps = [3, 1, 0, 1, 2]
    y, cuts, _ = _check(tiny, items, (0.0, 220, 0, 0), gaps, 0, "identity")
    want = np.concatenate([items[0], items[2], np.zeros(1, np.float32), items[3], np.zeros(2, np.float32), items[4]])
    assert np.array_equal(_bits(y), _bits(want))
    assert cuts.tolist() == [[0, len(x)] for x in items]


def test_one_call_equals_two_with_started_carried(tiny):
    rng = np.random.default_rng(5)
    H = 220
    items = [_quiet(rng, 8 * H, []), _quiet(rng, 20 * H + 3, [7 * H + 1, 12 * H]), _quiet(rng, 3 * H + 7, [H]),
             _quiet(rng, 5 * H, []), _quiet(rng, 9 * H + 1, [8 * H + 9])]
    gaps = [4, 1000, 0, 7, 441]
    for started in (0, 1):
        whole, cuts, _ = _check(tiny, items, P44, gaps, started)
        a, ca, s = _check(tiny, items[:2], P44, gaps[:2], started)
        b, cb, _ = _check(tiny, items[2:], P44, gaps[2:], s)
        assert np.array_equal(_bits(np.concatenate([a, b])), _bits(whole))
        assert np.concatenate([ca, cb]).tolist() == cuts.tolist()


def test_bad_arguments_are_refused_with_y_untouched(tiny):
    from fish_tts_amd import _lib as L
    lib, h = tiny.lib, tiny._h
    x = np.full((65, 8), 0.5, dtype=np.float32)
    n = np.full(65, 8, dtype=np.int64)
    gaps = np.ones(65, dtype=np.int64)
    y = np.full(2048, 123.0, dtype=np.float32)
    total, cuts = CT.c_int64(-7), np.full((65, 2), -7, dtype=np.int64)
    jp = L.ft_join_params(0.1, 4, 2, 2)
    P = lambda a: a.ctypes.data_as(CT.c_void_p)      # noqa: E731

    def call(B=2, stride=8, n=n, jp=jp, gaps=gaps, started=0, y=y, cap=2048, x=x, total=total, cuts=cuts):
        return lib.ft_test_join(h, P(x) if x is not None else None, B, stride, P(n) if n is not None else None,
                                CT.byref(jp) if jp is not None else None, P(gaps) if gaps is not None else None, started,
                                P(y) if y is not None else None, cap, CT.byref(total) if total is not None else None,
                                P(cuts) if cuts is not None else None)

    neg_gap, neg_n = gaps.copy(), n.copy()
    neg_gap[1], neg_n[0] = -1, -1
    bad = [dict(B=0), dict(B=65), dict(B=-1), dict(cap=17), dict(gaps=neg_gap), dict(n=neg_n), dict(x=None), dict(n=None),
           dict(jp=None), dict(gaps=None), dict(y=None), dict(total=None), dict(cuts=None), dict(started=2), dict(stride=7),
           dict(jp=L.ft_join_params(-0.1, 4, 2, 2)), dict(jp=L.ft_join_params(float("nan"), 4, 2, 2)),
           dict(jp=L.ft_join_params(0.1, 0, 2, 2)), dict(jp=L.ft_join_params(0.1, 4, -1, 2)),
           dict(jp=L.ft_join_params(0.1, 4, 2, -1))]
    for kw in bad:
        assert call(**kw) != L.FT_OK, kw
        assert np.all(y == 123.0) and total.value == -7 and np.all(cuts == -7), kw
    assert call(cap=18) == L.FT_OK and total.value == 17          # room for 8 + 1 + 8 + 1; the first gap is dropped


RATES = [(44100, 100, 0), (16000, 100, 0), (44100, 125, 300)]


def _rows_fxp(eng, block, lens, rate, pct, cents):
    """The rows of ft_codec_decode_fxp, cut to out_lens."""
    B, R, T = block.shape
    out_lens = np.zeros(B, dtype=np.int64)
    P = lambda a: a.ctypes.data_as(CT.c_void_p)      # noqa: E731
    lib = eng.lib                                    # the rows lie at the stride of the longest output
    stride = max(int(lib.ft_resampled_len(rate, lib.ft_timescaled_len(pct, int(t) * eng.frame_len))) for t in lens)
    audio = np.zeros((B, max(stride, 1)), dtype=np.float32)
    eng._check(lib.ft_codec_decode_fxp(eng._h, P(block), B, T, P(lens), rate, pct, cents, P(audio), P(out_lens)),
               "ft_codec_decode_fxp")
    return [audio[b, :int(out_lens[b])].copy() for b in range(B)]


@pytest.fixture(scope="module")
def blocks(tiny):
    shape = tiny_codec_shape()
    lens = np.array([3, 7, 12], dtype=np.int32)
    block = np.zeros((3, shape.n_codebooks + 1, 12), dtype=np.int32)
    for b, T in enumerate(lens):
        block[b, :, :T] = _codes(shape, int(T), 40 + b)
    return block, lens


@pytest.mark.parametrize("rate,pct,cents", RATES)
def test_decode_join_identity_equals_the_rows_of_decode_fxp(tiny, blocks, rate, pct, cents):
    from fish_tts_amd import _lib as L
    block, lens = blocks
    rows = _rows_fxp(tiny, block, lens, rate, pct, cents)
    gaps = np.array([5, 0, 3], dtype=np.int64)
    cap = sum(len(r) for r in rows) + int(gaps.sum())
    audio = np.full(cap + 16, 123.0, dtype=np.float32)
    total, cuts = CT.c_int64(0), np.zeros((3, 2), dtype=np.int64)
    jp = L.ft_join_params(0.0, 220, 0, 0)
    P = lambda a: a.ctypes.data_as(CT.c_void_p)      # noqa: E731
    tiny._check(tiny.lib.ft_codec_decode_join(tiny._h, P(block), 3, 12, P(lens), rate, pct, cents, CT.byref(jp), P(gaps), 0,
                                              P(audio), cap, CT.byref(total), P(cuts)), "ft_codec_decode_join")
    want = np.concatenate([rows[0], rows[1], np.zeros(3, np.float32), rows[2]])
    assert total.value == len(want) and np.array_equal(_bits(audio[:len(want)]), _bits(want))
    assert np.all(audio[len(want):] == 123.0)
    assert cuts.tolist() == [[0, len(r)] for r in rows]
    # refusals, before any device work: nothing is written
    for kw in (dict(cap=cap - 1), dict(B=0), dict(B=65), dict(rate=12345), dict(pct=49), dict(cents=1201), dict(started=2)):
        a2 = np.full(cap + 16, 123.0, dtype=np.float32)
        st = tiny.lib.ft_codec_decode_join(tiny._h, P(block), kw.get("B", 3), 12, P(lens), kw.get("rate", rate), kw.get("pct", pct),
                                           kw.get("cents", cents), CT.byref(jp), P(gaps), kw.get("started", 0), P(a2),
                                           kw.get("cap", cap), CT.byref(total), P(cuts))
        assert st != L.FT_OK and np.all(a2 == 123.0), kw


def test_engine_decode_join_groups_calls(tiny):
    """70 one-frame items take two native calls (64 + 6): trimmed, faded and laid out as one call would."""
    shape = tiny_codec_shape()
    codes = [_codes(shape, 1 if i % 5 else 2, 100 + i) for i in range(70)]
    rows = [tiny.decode(c)[0] for c in codes]
    peak = max(float(np.abs(r).max()) for r in rows)
    params = (0.5 * peak, 4, 3, 2)
    gaps = [i % 3 for i in range(70)]
    for started in (False, True):
        audio, cuts = tiny.decode_join(codes, params=params, gaps=gaps, started=started)
        want, wcuts, _ = J.join(rows, *params, gaps, int(started))
        assert np.array_equal(_bits(audio), _bits(want)) and cuts.tolist() == wcuts.tolist()
    assert any(a > 0 or e < len(r) for (a, e), r in zip(wcuts.tolist(), rows))     # something was trimmed
    plain, cuts = tiny.decode_join(codes[:3])
    assert np.array_equal(_bits(plain), _bits(np.concatenate(rows[:3])))
    for bad in (dict(gaps=[0]), dict(gaps=[-1] * 70), dict(params=(-1.0, 4, 3, 2)), dict(params=(0.1, 0, 3, 2)),
                dict(sample_rate=12345), dict(speed=3.0), dict(pitch=13)):
        with pytest.raises(ValueError):
            tiny.decode_join(codes, **bad)


def test_new_symbols_resolve(tiny):
    for name in ("ft_codec_decode_join", "ft_test_join", "ft_join_groups"):
        assert getattr(tiny.lib, name) is not None
    lens = np.array([3, 0, 2045, 4, 1], dtype=np.int32)
    ends = np.zeros(5, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(CT.c_void_p)      # noqa: E731
    assert tiny.lib.ft_join_groups(P(lens), 5, 2048, P(ends)) == 2 and ends[:2].tolist() == [3, 5]
    assert tiny.lib.ft_join_groups(P(lens), 5, 2044, P(ends)) == -1
