"""CPU: tests/join_ref.py - the numpy restatement of the join stage (include/fishtts_hip.h: ft_codec_decode_join) - pinned
on cases worked out by hand, so that the GPU tests compare the kernels against a reference that is itself checked."""
import numpy as np

from tests import join_ref as J


def _item(n, loud=(), value=0.5):
    x = np.zeros(n, dtype=np.float32)
    for i in loud:
        x[i] = value
    return x


def test_threshold_is_inclusive_in_float32():
    thr = np.float32(0.1)
    below = np.nextafter(thr, np.float32(0), dtype=np.float32)
    x = _item(30)
    x[12] = thr                                   # exactly at the threshold: loud
    assert J.edges(x, thr, 10, 0) == (10, 20)
    x[12] = -thr
    assert J.edges(x, thr, 10, 0) == (10, 20)
    x[12] = below                                 # one ulp below: not loud
    assert J.edges(x, thr, 10, 0) == (0, 0)
    x[12] = np.nan                                # a NaN is never loud, not even at threshold 0
    assert J.edges(x, thr, 10, 0) == (0, 0)
    assert J.edges(np.array([np.nan, np.nan], dtype=np.float32), 0.0, 10, 0) == (0, 0)
    assert J.edges(np.array([np.nan, 0.0, np.nan], dtype=np.float32), 0.0, 2, 0) == (0, 2)
    # the comparison is made in float32: a float64 threshold a hair above float32(0.1) rounds onto it
    assert J.edges(_item(30, [12], thr), float(thr) + 1e-12, 10, 0) == (10, 20)


def test_clamps_at_zero_and_at_n():
    x = _item(47, [13, 31])                       # windows of 10: first = 1, last = 3; the last window is [40, 47)
    assert J.edges(x, 0.25, 10, 0) == (10, 40)
    assert J.edges(x, 0.25, 10, 4) == (6, 44)
    assert J.edges(x, 0.25, 10, 10) == (0, 47)    # 10 - 10 = 0 exactly; 40 + 10 clamps to n
    assert J.edges(x, 0.25, 10, 1000) == (0, 47)
    assert J.edges(_item(47, [45]), 0.25, 10, 0) == (40, 47)      # the short last window ends at n
    assert J.edges(_item(47, [0]), 0.25, 10, 3) == (0, 13)
    assert J.edges(_item(0), 0.0, 10, 3) == (0, 0)
    assert J.edges(_item(1), 0.0, 10, 0) == (0, 1)                # threshold 0: every sample is loud


def test_fades_with_odd_m_and_f_of_half_m():
    x = np.arange(1, 8, dtype=np.float32)         # m = 7, fade 5 -> f = 3: ramps 1/6, 3/6, 5/6; sample 3 untouched
    r = [np.float32(1 / 6), np.float32(3 / 6), np.float32(5 / 6)]
    want = np.array([1 * r[0], 2 * r[1], 3 * r[2], 4, 5 * r[2], 6 * r[1], 7 * r[0]], dtype=np.float32)
    got = J.piece(x, 0, 7, 5)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert J.piece(x, 0, 7, 0).tobytes() == x.tobytes()
    assert J.piece(x, 2, 3, 9).tobytes() == x[2:3].tobytes()      # m = 1: f = 0
    two = J.piece(x, 2, 4, 9)                                     # m = 2: f = 1, both samples halved
    assert two.tobytes() == np.array([1.5, 2.0], dtype=np.float32).tobytes()
    big = J.piece(np.ones(1000, dtype=np.float32), 100, 900, 220)
    assert big[0] == np.float32(1 / 440) and big[219] == np.float32(439 / 440) and big[220] == 1 and big[579] == 1
    assert big[580] == np.float32(439 / 440) and big[799] == np.float32(1 / 440) and len(big) == 800


def test_silent_items_and_started():
    loud, silent = _item(20, [5]), _item(20)
    kw = dict(threshold=0.25, hop=10, keep=0, fade=0)
    for where in (0, 1, 2):
        items = [loud, loud, loud]
        items[where] = silent
        gaps = [3, 4, 5]
        for started in (0, 1):
            audio, cuts, s = J.join(items, gaps=gaps, started=started, **kw)
            want, first = [], not started
            for b in range(3):
                if b == where:
                    continue
                if not first:
                    want.append(np.zeros(gaps[b], dtype=np.float32))
                want.append(loud[0:10])
                first = False
            assert audio.tobytes() == np.concatenate(want).tobytes(), (where, started)
            assert cuts.tolist() == [[0, 0] if b == where else [0, 10] for b in range(3)] and s == 1
    audio, cuts, s = J.join([silent, silent], gaps=[7, 7], started=0, **kw)
    assert len(audio) == 0 and s == 0 and cuts.tolist() == [[0, 0], [0, 0]]
    audio, cuts, s = J.join([silent], gaps=[7], started=1, **kw)
    assert len(audio) == 0 and s == 1


def test_identity_parameters_concatenate_with_gaps():
    rng = np.random.default_rng(0)
    items = [rng.standard_normal(n).astype(np.float32) for n in (5, 0, 1, 17)]
    audio, cuts, _ = J.join(items, 0.0, 1, 0, 0, [9, 2, 1, 3], started=0)
    want = np.concatenate([items[0], np.zeros(1, np.float32), items[2], np.zeros(3, np.float32), items[3]])
    assert audio.tobytes() == want.tobytes() and cuts.tolist() == [[0, 5], [0, 0], [0, 1], [0, 17]]


def test_splitting_the_items_over_calls_gives_the_same_samples():
    rng = np.random.default_rng(1)
    items = [(rng.standard_normal(n) * (0.0 if n == 90 else 0.3)).astype(np.float32) for n in (90, 130, 64, 90, 257)]
    gaps = [11, 0, 1, 5, 8]
    kw = dict(threshold=0.2, hop=16, keep=20, fade=16)
    for started in (0, 1):
        whole, cuts, s_all = J.join(items, gaps=gaps, started=started, **kw)
        for cut in (1, 2, 4):
            a, ca, s = J.join(items[:cut], gaps=gaps[:cut], started=started, **kw)
            b, cb, s2 = J.join(items[cut:], gaps=gaps[cut:], started=s, **kw)
            assert np.concatenate([a, b]).tobytes() == whole.tobytes() and s2 == s_all
            assert np.concatenate([ca, cb]).tolist() == cuts.tolist()
