"""GPU: ft_codec_decode_join_items - the join of items that each go through a chain of their own (speed, pitch, level), as
FishTTS.synthesize_script needs it.  Its result is stated as a composition of calls that are checked element-wise
elsewhere: ft_test_join over the rows of one ft_codec_decode_level call per item.  Everything here is an equality of bit
patterns; there is no tolerance.

Shapes: five items of 3, 7, 0, 12 and 19 frames of 32 samples with the chains (speed_pct, pitch_cents, loudness)
(100,0,0) (150,0,0) (100,300,0) (80,-200,-2300) (100,0,-1600) - no chain, each stage alone, two stages with a level,
levelled and unlevelled items in one launch of the level stage, an empty item in the middle.  In that layout the pitch-only
chain falls on the empty item, so a second layout gives it frames and puts an empty levelled item between two levelled ones.
Rates 44100 and 16000; no trimming, and a threshold just above the largest sample in the first two windows of the last
item, which therefore loses its front (or, if its peak lies there, everything): a cut moves whatever the samples are."""
import ctypes as CT

import numpy as np
import pytest

from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import make_codec
from tests.test_timescale_gpu import _codes

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "issue": ([3, 7, 0, 12, 19], [(100, 0, 0), (150, 0, 0), (100, 300, 0), (80, -200, -2300), (100, 0, -1600)]),
    "rotated": ([7, 12, 0, 19, 3], [(100, 300, 0), (80, -200, -2300), (100, 0, -1600), (100, 0, -1600), (150, 0, 0)]),
}
RATES = [44100, 16000]
HOP, KEEP, FADE = 8, 4, 4
GAPS = [5, 0, 9, 7, 3]
EMPTY = (float("-inf"), 0.0, 1.0, 0, 0, 0)


@pytest.fixture(scope="module")
def tiny():
    eng, _ = make_codec(tiny_codec_shape(), max_frames=2048)
    assert eng.frame_len == 32
    yield eng
    eng.close()


def P(a):
    return a.ctypes.data_as(CT.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _block(lens):
    shape = tiny_codec_shape()
    b = np.zeros((len(lens), shape.n_codebooks + 1, max(1, max(lens))), dtype=np.int32)
    for i, T in enumerate(lens):
        if T:
            b[i, :, :T] = _codes(shape, T, 40 + i)
    return b


def _info(i):
    return (np.float64(i.lufs).view(np.uint64).item(), np.float32(i.peak).view(np.uint32).item(),
            np.float32(i.gain).view(np.uint32).item(), i.blocks, i.gated, i.capped)


def _rows(eng, block, lens, rate, chains):
    """One ft_codec_decode_level call per item: (its samples, its ft_level_info as bit patterns)."""
    from fish_tts_amd import _lib as L
    rows, infos = [], []
    T = block.shape[2]
    for b, (Tb, (pct, cents, level)) in enumerate(zip(lens, chains)):
        width = max(1, int(eng.lib.ft_resampled_len(rate, eng.lib.ft_timescaled_len(pct, Tb * eng.frame_len))))
        audio = np.zeros(width, dtype=np.float32)
        n = np.zeros(1, dtype=np.int64)
        info = (L.ft_level_info * 1)()
        one = np.ascontiguousarray(block[b:b + 1])
        eng._check(eng.lib.ft_codec_decode_level(eng._h, P(one), 1, T, P(np.array([Tb], dtype=np.int32)), rate, pct, cents, level,
                                                 P(audio), P(n), info), "ft_codec_decode_level")
        rows.append(audio[:int(n[0])].copy())
        infos.append(_info(info[0]))
    return rows, infos


def _items(eng, block, lens, rate, chains, params, gaps, started=0, capacity=None, fx=True):
    """The native call itself: (status, audio, total, cuts, infos); buffers pre-filled so that a refused call shows."""
    from fish_tts_amd import _lib as L
    B, _, T = block.shape
    native = (L.ft_item_fx * B)(*[L.ft_item_fx(*c) for c in chains])
    cap = sum(int(eng.lib.ft_resampled_len(rate, eng.lib.ft_timescaled_len(max(50, min(200, c[0])), t * eng.frame_len)))
              for t, c in zip(lens, chains)) + sum(gaps) if capacity is None else capacity
    audio = np.full(max(cap, 1) + 8, 123.0, dtype=np.float32)
    total, cuts = CT.c_int64(-7), np.full((B, 2), -7, dtype=np.int64)
    infos = (L.ft_level_info * B)(*[L.ft_level_info(7.0, 7.0, 7.0, 7, 7, 7) for _ in range(B)])
    jp = eng._join_params(params)
    st = eng.lib.ft_codec_decode_join_items(eng._h, P(block), B, T, P(np.array(lens, dtype=np.int32)), rate, native if fx else None,
                                            CT.byref(jp), P(np.array(gaps, dtype=np.int64)), started, P(audio), cap,
                                            CT.byref(total), P(cuts), infos)
    return st, audio, total.value, cuts, [_info(i) for i in infos]


def _untouched(res):
    _, audio, total, cuts, infos = res
    return bool(np.all(audio == 123.0)) and total == -7 and bool(np.all(cuts == -7)) and all(i[3] == 7 for i in infos)


def _threshold(rows):
    """Just above the largest magnitude in the last item's first two windows."""
    head = np.abs(rows[-1][:2 * HOP]).astype(np.float32)
    return float(np.nextafter(head.max(), np.float32(np.inf), dtype=np.float32))


@pytest.fixture(scope="module")
def want(tiny):
    """The reference rows of every layout and rate, computed once and left unchanged."""
    out = {}
    for name, (lens, chains) in LAYOUTS.items():
        block = _block(lens)
        for rate in RATES:
            out[name, rate] = (block, *_rows(tiny, block, lens, rate, chains))
    return out


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_items_equal_the_join_of_the_levelled_rows(tiny, want, layout, rate):
    from fish_tts_amd import _lib as L
    lens, chains = LAYOUTS[layout]
    block, rows, infos = want[layout, rate]
    assert [len(r) for r in rows][lens.index(0)] == 0
    for (_, _, level), info, T in zip(chains, infos, lens):
        if level == 0 or T == 0:
            assert info == _info(L.ft_level_info(*EMPTY))
        else:
            assert info[3] >= 1 and np.isfinite(np.uint64(info[0]).view(np.float64))     # measured
    moved = False
    for trim in (False, True):
        params = (_threshold(rows), HOP, KEEP, FADE) if trim else (0.0, HOP, 0, 0)
        for started in (0, 1):
            st, audio, total, cuts, got = _items(tiny, block, lens, rate, chains, params, GAPS, started)
            assert st == L.FT_OK, tiny.lib.ft_last_error(tiny._h)
            y, wtotal, wcuts = tiny.test_join(rows, params, GAPS, started)
            assert total == wtotal > 0
            assert cuts.tolist() == wcuts.tolist(), (cuts.tolist(), wcuts.tolist())
            assert np.array_equal(_bits(audio[:total]), _bits(y[:total]))
            assert np.all(audio[total:] == 123.0), "the call wrote past its output"
            assert got == infos, (got, infos)
            if trim:
                moved = moved or cuts.tolist() != [[0, len(r)] for r in rows]
            else:
                assert cuts.tolist() == [[0, len(r)] for r in rows]
            # the same bits again
            again = _items(tiny, block, lens, rate, chains, params, GAPS, started)
            assert again[2] == total and np.array_equal(_bits(again[1]), _bits(audio)) and again[3].tolist() == cuts.tolist()
            assert again[4] == got
    assert moved, "the threshold moved no cut"


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("chain", [(100, 0, 0), (100, 0, -1600), (80, -200, -2300), (150, 0, 0)])
def test_equal_chains_are_the_level_join(tiny, want, rate, chain):
    from fish_tts_amd import _lib as L
    lens, _ = LAYOUTS["issue"]
    block = want["issue", rate][0]
    B, _, T = block.shape
    rows, _ = _rows(tiny, block, lens, rate, [chain] * B)
    params = (_threshold(rows), HOP, KEEP, FADE)
    st, audio, total, cuts, infos = _items(tiny, block, lens, rate, [chain] * B, params, GAPS)
    assert st == L.FT_OK, tiny.lib.ft_last_error(tiny._h)
    ref = np.full(len(audio), 123.0, dtype=np.float32)
    rtotal, rcuts = CT.c_int64(-7), np.full((B, 2), -7, dtype=np.int64)
    rinfos = (L.ft_level_info * B)(*[L.ft_level_info(*EMPTY) for _ in range(B)])
    jp = tiny._join_params(params)
    tiny._check(tiny.lib.ft_codec_decode_join_level(tiny._h, P(block), B, T, P(np.array(lens, dtype=np.int32)), rate, *chain,
                                                    CT.byref(jp), P(np.array(GAPS, dtype=np.int64)), 0, P(ref), len(ref) - 8,
                                                    CT.byref(rtotal), P(rcuts), rinfos), "ft_codec_decode_join_level")
    assert total == rtotal.value > 0 and cuts.tolist() == rcuts.tolist()
    assert np.array_equal(_bits(audio), _bits(ref))
    assert infos == [_info(i) for i in rinfos]       # (without a level the older call leaves infos alone: the empty result)


def test_refusals_name_the_item_and_change_nothing(tiny, want):
    from fish_tts_amd import _lib as L
    lens, chains = LAYOUTS["issue"]
    rate = 16000
    block, rows, _ = want["issue", rate]
    params = (0.0, HOP, 0, 0)
    good = _items(tiny, block, lens, rate, chains, params, GAPS)
    assert good[0] == L.FT_OK
    need = sum(len(r) for r in rows) + sum(GAPS)

    def bad_at(i, c):
        return [c if b == i else x for b, x in enumerate(chains)]

    cases = [
        ("a bad chain in item 3", dict(chains=bad_at(3, (49, 0, -2300))), ["item 3", "speed"]),
        ("a bad pitch in item 0", dict(chains=bad_at(0, (100, 1201, 0))), ["item 0", "pitch"]),
        ("a bad pair", dict(chains=bad_at(1, (200, -100, 0))), ["item 1", "ratio"]),
        ("a bad level", dict(chains=bad_at(4, (100, 0, -400))), ["item 4", "loudness"]),
        ("the first bad item is named", dict(chains=bad_at(2, (100, 0, 5))[:4] + [(300, 0, 0)]), ["item 2", "loudness"]),
        ("the rate goes first", dict(rate=12345, chains=bad_at(3, (49, 0, 0))), ["12345"]),
        ("a null fx", dict(fx=False), ["bad argument"]),
        ("a too-small capacity", dict(capacity=need - 1), ["capacity"]),
    ]
    for what, change, words in cases:
        kw = dict(rate=rate, chains=chains, capacity=None, fx=True)
        kw.update(change)
        res = _items(tiny, block, lens, kw["rate"], kw["chains"], params, GAPS, 0, kw["capacity"], kw["fx"])
        msg = tiny.lib.ft_last_error(tiny._h).decode()
        assert res[0] == L.FT_ERR_ARG, (what, res[0], msg)
        assert msg.startswith("ft_codec_decode_join_items") and all(w in msg for w in words), (what, msg)
        assert (": item " in msg) == any(w.startswith("item") for w in words), (what, msg)
        assert _untouched(res), what
        after = _items(tiny, block, lens, rate, chains, params, GAPS)
        assert after[0] == L.FT_OK and after[2] == good[2], what
        assert np.array_equal(_bits(after[1]), _bits(good[1])) and after[3].tolist() == good[3].tolist() and after[4] == good[4], what
    # exactly enough room is enough
    assert _items(tiny, block, lens, rate, chains, params, GAPS, 0, need)[0] == L.FT_OK


def test_the_engine_wrapper_carries_every_items_chain(tiny, want):
    from fish_tts_amd.codec_engine import LevelInfo, OutputFx
    lens, chains = LAYOUTS["rotated"]
    rate = 16000
    block, rows, _ = want["rotated", rate]
    codes = [block[b, :, :T] for b, T in enumerate(lens)]
    fxs = [OutputFx(rate, None if p == 100 else p, c or None, lv or None) for p, c, lv in chains]
    params = (_threshold(rows), HOP, KEEP, FADE)
    levels = []
    audio, cuts = tiny.decode_join(codes, params=params, gaps=GAPS, item_fx=fxs, levels=levels)
    y, total, wcuts = tiny.test_join(rows, params, GAPS)
    assert len(audio) == total and np.array_equal(_bits(audio), _bits(y[:total])) and cuts.tolist() == wcuts.tolist()
    assert len(levels) == len(lens) and all(isinstance(i, LevelInfo) for i in levels)
    assert [i.blocks > 0 for i in levels] == [bool(lv and T) for T, (_, _, lv) in zip(lens, chains)]
    # each item decoded by the engine through its own chain gives the same rows
    for b, (c, f) in enumerate(zip(codes, fxs)):
        if lens[b]:
            assert np.array_equal(_bits(tiny.decode(c, fx=f)[0][:len(rows[b])]), _bits(rows[b])), b
    # the items split over two calls, `started` carried; and over the wrapper's own groups
    a, ca = tiny.decode_join(codes[:2], params=params, gaps=GAPS[:2], item_fx=fxs[:2])
    b2, cb = tiny.decode_join(codes[2:], params=params, gaps=GAPS[2:], item_fx=fxs[2:], started=len(a) > 0)
    assert np.array_equal(_bits(np.concatenate([a, b2])), _bits(audio)) and np.concatenate([ca, cb]).tolist() == cuts.tolist()
    for bad in (fxs[:4], fxs[:4] + [OutputFx(22050)], fxs[:4] + [OutputFx(rate, live=-2000)],
                fxs[:4] + [None]):
        with pytest.raises(ValueError):
            tiny.decode_join(codes, params=params, gaps=GAPS, item_fx=bad)
    # without item_fx the method is what it was
    p0, c0 = tiny.decode_join(codes, params=params, gaps=GAPS, sample_rate=rate, speed=1.5)
    p1, c1 = tiny.decode_join(codes, params=params, gaps=GAPS, item_fx=[OutputFx(rate, 150)] * len(codes))
    assert np.array_equal(_bits(p0), _bits(p1)) and c0.tolist() == c1.tolist()
