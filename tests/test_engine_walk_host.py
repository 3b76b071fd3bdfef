"""Host only: the census of the frame engine's K/V walk (tests/engine_walk.py) pinned at the edges of the rolling window, and
the case lists of tests/test_engine_long_context_gpu.py (imported, not copied) held to the whole required event set per form
of the kernel, so that a later edit of the lists cannot silently drop an edge."""
import pytest

from tests import engine_walk as W
from tests import test_engine_long_context_gpu as G


def deep(nsplit, pos):
    c = W.census(nsplit, pos)
    return [c.deepest(gw) for gw in range(4)]


def has(nsplit, pos, *ev):
    return set(ev) <= W.census(nsplit, pos).events


def skipped(nsplit, pos):
    return sorted(e[1] for e in W.census(nsplit, pos).events if e[0] == "refill_skipped")


def test_geometry_and_split_rule():
    assert W.geometry(128) == (4, 16) and W.geometry(64) == (8, 32)
    assert W.KVST * W.geometry(128)[1] == 96
    assert W.splits(32, 2)[:4] == [(0, 1), (1, 2), (2, 3), (3, 3)]                  # chunk 1: split 2 holds only the new row
    assert [W.census(32, p).chunk for p in (31, 32, 63, 64, 3071, 3072, 8191)] == [1, 2, 2, 3, 96, 97, 256]
    assert W.splits(16, 3071)[15] == (2880, 3072) and W.splits(1, 511) == [(0, 512)]


@pytest.mark.parametrize("nsplit,wrap,new_row_blk1,all_wrap,blk2", [(32, 3072, 3103, 3456, 6144), (16, 1536, 1551, 1728, 3072),
                                                                     (1, 96, 96, 108, 192)])
def test_census_at_the_edges_of_the_window(nsplit, wrap, new_row_blk1, all_wrap, blk2):
    assert deep(nsplit, wrap - 1) == [0, 0, 0, 0] and deep(nsplit, wrap) == [1, 0, 0, 0]                # first wrap, wave 0 only
    # the first row behind the window: refilled - unless it is the new row itself (one split: rows [0, 96] at pos 96)
    assert not has(nsplit, wrap - 1, ("refill", 0, 0)) and has(nsplit, wrap + 1, ("refill", 0, 0))
    assert has(nsplit, wrap, ("refill", 0, 0)) == (nsplit > 1) and (nsplit > 1 or skipped(nsplit, wrap) == [0])
    assert not has(nsplit, new_row_blk1 - 1, ("new_row", 1)) and has(nsplit, new_row_blk1, ("new_row", 1), ("refill_skipped", 0))
    assert min(deep(nsplit, all_wrap - 1)) == 0 and min(deep(nsplit, all_wrap)) == 1                    # all four waves wrap
    assert max(deep(nsplit, blk2 - 1)) == 1 and deep(nsplit, blk2) == [2, 1, 1, 1]                      # blk 2
    assert has(nsplit, blk2 + 1, ("refill", 1, 0)) and not has(nsplit, blk2 + 1, ("refill", 2, 0))
    assert has(nsplit, blk2, ("refill", 1, 0)) == (nsplit > 1) and (nsplit > 1 or skipped(nsplit, blk2) == [0])


def test_census_at_the_ends():
    assert deep(32, 8191) == [2, 2, 2, 2] and has(32, 8191, ("new_row", 2)) and skipped(32, 8191) == [3]
    assert not any(e[0] == "refill" and e[1] == 2 for e in W.census(32, 8191).events)      # 256 rows per split: no third refill
    assert deep(16, 3071) == [1, 1, 1, 1]                        # the last frame ft_ar_decode gives 16 splits: two full blocks
    assert deep(1, 511) == [5, 5, 5, 5] and has(1, 511, ("refill", 2, 3), ("refill", 4, 0), ("new_row", 5))
    assert has(32, 2, ("empty_split",), ("new_row_only",)) and has(32, 31, ("new_row_only",)) and not has(32, 31, ("empty_split",))
    assert has(8, 9, ("empty_split",)) and not has(8, 9, ("new_row_only",))
    assert not has(32, 3071, ("partial_step",)) and has(32, 3072, ("partial_step",))
    # the skipped refill, register by register: the new row sits 96 + 16 st (+ 0 .. 15) behind the start of its split
    assert [skipped(1, 96 + 16 * st) for st in range(8)] == [[0], [1], [2], [3], [4], [5], [0], [1]]
    assert skipped(1, 95) == [] and skipped(32, 3102) == []


@pytest.mark.parametrize("hd", [128, 64])
def test_census_is_consistent_everywhere_it_is_cheap(hd):
    """census() asserts that every position of [0, pos] is consumed exactly once and every register step holds the row read
    from it, for a prefetched turn and for one that was not."""
    for nsplit in (1, 2, 4, 8):
        for pos in list(range(0, 330)) + [383, 384, 511, 767, 768, 1023]:
            a = W.census(nsplit, pos, hd, prefetched=True)
            b = W.census(nsplit, pos, hd, prefetched=False)
            assert a.events == b.events
    for nsplit, pos in ((16, 1535), (16, 1536), (16, 3071), (16, 4095), (32, 3103), (32, 6151), (32, 8191)):
        W.census(nsplit, pos, hd, prefetched=False)


def test_case_lists_keep_what_the_issue_set():
    """The contexts each list must hold (a later edit may add cases, not drop these)."""
    xl = {(c.max_seq_len, c.Lp) for c in G.XL_CASES}
    assert {(8192, 2), (8192, 3064), (8192, 3096), (8192, 3448), (8192, 6136), (8192, 8176), (4096, 4080)} <= xl
    assert all(c.form == "xl" and not c.env and not c.over and all(ns == 32 for _, ns in c.calls) for c in G.XL_CASES)
    g = {c.name: c for c in G.GENERAL_CASES}
    assert all(c.form == "general" and (c.env or dict(c.over).get("n_local_heads") == 4) for c in g.values())
    for name, max_seq_len, Lp, calls in (("g1-88", 512, 88, ((40, 1),)), ("g1-184", 512, 184, ((16, 1),)), ("g1-496-end", 512, 496, ((24, 1),)),
                                         ("g16-1528", 4096, 1528, ((32, 16),)), ("g16-3040", 4096, 3040, ((24, 16),)),
                                         ("g32-3060", 4096, 3060, ((24, 32),)), ("g8to16-740", 1024, 740, ((16, 8), (32, 16))),
                                         ("f2-300", 1024, 300, ((16, 2),)), ("f4-300", 1024, 300, ((16, 4),)), ("f8-1000", 2048, 1000, ((16, 8),)),
                                         ("kv4-1528", 4096, 1528, ((16, 16),)), ("kv4-3096", 4096, 3096, ((16, 32),)),
                                         ("turns-9x8", 1024, 300, ((16, 8),)), ("turns-5x16", 4096, 1600, ((16, 16),)),
                                         ("turns-kv4-5x16", 4096, 1600, ((16, 16),))):
        assert (g[name].max_seq_len, g[name].Lp, g[name].calls) == (max_seq_len, Lp, calls), name
    assert dict(g["turns-9x8"].over) == {"n_layer": 9} and dict(g["turns-5x16"].over) == {"n_layer": 5}
    assert dict(g["turns-kv4-5x16"].over) == {"n_layer": 5, "n_local_heads": 4}
    # the two cache ends are asked for 24 frames and run 16
    assert [len(c.frames()) for c in G.XL_CASES if c.name.endswith("-end")] == [16, 16] and len(g["g1-496-end"].frames()) == 16
    assert {(form, Lp) for _, form, _, Lp, _, _ in G.LAST_ROW_CASES} == {("xl", 3096), ("general", 1528)}


@pytest.mark.parametrize("form", ["xl", "general"])
def test_case_lists_reach_the_required_events(form):
    """Exceptions (engine_walk.required_events names them): the XCD-local form cannot issue a refill in blk 2 - that takes a
    split of more than 288 positions, and 32 splits of an 8192-row cache hold 256.  The general form has none."""
    cases = G.XL_CASES if form == "xl" else G.GENERAL_CASES
    pairs = [p for c in cases for p in c.pairs()]
    ev = W.events_of(pairs)
    need = W.required_events(form)
    assert not need - ev, sorted(need - ev)
    full = W.required_events("general")
    assert need == (full - {("refill", 2, gw) for gw in range(4)} if form == "xl" else full)
    if form == "xl":
        assert max(hi - lo for lo, hi in W.splits(32, 8191)) == 256 < 2 * 96 + 96 + 1
        assert {ns for ns, _ in pairs} == {32}
    else:
        assert {ns for ns, _ in pairs} == {1, 2, 4, 8, 16, 32}


def test_what_each_case_reaches():
    """The events the issue names per case, as the census derives them from the case's own frames."""
    ev = {c.name: W.events_of(c.pairs()) for c in G.XL_CASES + G.GENERAL_CASES}
    assert {("empty_split",), ("new_row_only",)} <= ev["xl-2"] and {W.census(32, p).chunk for _, p in G.XL_CASES[0].pairs()} == {1, 2, 3}
    assert ("blk", 1, 0) in ev["xl-3064"] and ("blk", 1, 1) not in ev["xl-3064"]
    assert {("new_row", 1), ("refill_skipped", 0)} <= ev["xl-3096"]
    assert ("blk", 1, 3) in ev["xl-3448"] and ("blk", 1, 3) not in ev["xl-3096"]
    assert ("refill_skipped", 2) in ev["xl-4592"] and ("refill_skipped", 4) in ev["xl-5616"]
    assert ("blk", 2, 0) in ev["xl-6136"] and ("blk", 2, 0) not in ev["xl-5616"]
    assert {("blk", 2, 3), ("new_row", 2)} <= ev["xl-8176-end"]
    assert {("new_row", 0), ("new_row", 1), ("blk", 1, 3), ("refill_skipped", 0), ("refill_skipped", 1)} <= ev["g1-88"]
    assert {("refill_skipped", st) for st in range(1, 6)} <= ev["g1-120"]
    assert {("blk", 2, 0), ("new_row", 2)} <= ev["g1-184"] and ("blk", 5, 3) in ev["g1-496-end"] and ("refill", 2, 3) in ev["g1-496-end"]
    assert {("empty_split",), ("new_row_only",)} <= ev["g8-2"]
    assert ("blk", 1, 0) in ev["g16-1528"] and {W.census(16, p).chunk for _, p in G.GENERAL_CASES[6].pairs()} == {191, 192}
    assert all(("blk", 1, 0) not in ev[n] for n in ("f4-300", "turns-9x8")) and ("blk", 1, 0) in ev["f8-1000"] and ("blk", 1, 3) in ev["f2-300"]
    assert ("blk", 1, 0) in ev["turns-5x16"] and ("blk", 1, 0) in ev["kv4-3096"]
