"""A census of the K/V walk of the frame engine's slow-stack attention turn (csrc/frame_engine.h, slow_engine_kernel: kv_issue
and the blk / st loop), restated in plain Python integers.  No floats: it decides nothing about correctness.  It says which
corners of the walk a frame at (nsplit, pos, hd) reaches, so that the bit-identity tests of
tests/test_engine_long_context_gpu.py can prove they executed them, and it names the wave, blk and step to look at when a
frame differs.

The kernel's rule, per attention workgroup (one kv head, one KV split):
    chunk = (pos + nsplit) // nsplit;  lo = split * chunk;  hi = min(lo + chunk, pos + 1)      (pos = the new row)
    four gathering waves gw; a lane group grp of a wave owns one position per step: PPW = 64 / (hd / 8) positions per wave
    and step, NSLOT = 4 PPW positions per step of the workgroup
    kv_issue (the prefetch):  register st  <-  row lo + st NSLOT + gw PPW + grp   if it is < hi and is not pos
    walk: for blk while lo + gw PPW + blk KVST NSLOT < hi:  for st in 0 .. KVST - 1:
              base = lo + gw PPW + (blk KVST + st) NSLOT;   skipped unless base < hi;   j = base + grp
              the row comes from: the new row's LDS copy (j == pos), register st (a prefetched turn, or blk > 0), a direct
              load (blk 0 of a turn that was not prefetched)
              refill: register st <- row j + KVST NSLOT if that is < hi and is not pos, else zeros
              the row is consumed if j < hi
Events (the keys of Census.events, each a tuple):
    ("empty_split",)            a split with lo >= hi
    ("new_row_only",)           a split that holds the new row and nothing else
    ("blk", b, gw)              wave gw ran block b (deepest(gw) = the largest b)
    ("refill", b, gw)           wave gw issued a refill load while consuming block b
    ("new_row", b)              the new row was consumed in block b
    ("refill_skipped", st)      the refill of register st was skipped because its target is the new row
    ("partial_step",)           a wave's last step covered fewer than PPW rows of the split
"""
from dataclasses import dataclass, field

KVST = 6            # ENG_KVST: K/V steps of an attention workgroup held in registers


def geometry(hd):
    lpp = hd // 8
    ppw = 64 // lpp
    return ppw, 4 * ppw             # PPW, NSLOT


def splits(nsplit, pos):
    """[(lo, hi)] of every split of a frame whose new row is pos (hi <= lo: the split is empty)."""
    chunk = (pos + nsplit) // nsplit
    return [(s * chunk, min(s * chunk + chunk, pos + 1)) for s in range(nsplit)]


@dataclass
class Census:
    nsplit: int
    pos: int
    hd: int
    chunk: int = 0
    events: set = field(default_factory=set)
    where: dict = field(default_factory=dict)       # event -> (split, gw, blk, st) of its first occurrence

    def deepest(self, gw):
        return max((e[1] for e in self.events if e[0] == "blk" and e[2] == gw), default=-1)


def walk_split(lo, hi, pos, hd, prefetched, emit):
    """The walk of one split.  Returns the rows consumed, in the order the four waves would list them (wave by wave).
    Asserts that every register read finds the row the walk wants there."""
    ppw, nslot = geometry(hd)
    window = KVST * nslot
    consumed = []
    for gw in range(4):
        for grp in range(ppw):
            reg = [None] * KVST                       # the row index held by register st of this lane group (None: zeros)
            if prefetched:
                for st in range(KVST):
                    j = lo + st * nslot + gw * ppw + grp
                    reg[st] = j if (j < hi and j != pos) else None
            blk = 0
            while lo + gw * ppw + blk * window < hi:
                emit(("blk", blk, gw), gw, blk, 0)
                for st in range(KVST):
                    base = lo + gw * ppw + (blk * KVST + st) * nslot
                    if base >= hi:
                        continue
                    if grp == 0 and hi - base < ppw:
                        emit(("partial_step",), gw, blk, st)
                    j = base + grp
                    if j < hi and j == pos:
                        emit(("new_row", blk), gw, blk, st)
                    elif prefetched or blk > 0:
                        if j < hi:
                            assert reg[st] == j, f"register {st} of wave {gw} group {grp} holds {reg[st]}, the walk reads {j} " \
                                                 f"(lo {lo} hi {hi} pos {pos} blk {blk})"
                    jn = j + window
                    if jn < hi and jn != pos:
                        reg[st] = jn
                        emit(("refill", blk, gw), gw, blk, st)
                    else:
                        if jn < hi and jn == pos:
                            emit(("refill_skipped", st), gw, blk, st)
                        reg[st] = None
                    if j < hi:
                        consumed.append(j)
                blk += 1
    return consumed


def census(nsplit, pos, hd=128, prefetched=True):
    """The events of one frame at (nsplit, pos, hd), with the census's own consistency checked: every position of [0, pos] is
    consumed exactly once over the splits, and every register step holds the row that is read from it (walk_split)."""
    assert nsplit >= 1 and pos >= 0 and hd % 8 == 0 and 64 % (hd // 8) == 0
    c = Census(nsplit, pos, hd, (pos + nsplit) // nsplit)
    seen = []
    for s, (lo, hi) in enumerate(splits(nsplit, pos)):
        def emit(ev, gw, blk, st, s=s):
            if ev not in c.events:
                c.events.add(ev)
                c.where[ev] = (s, gw, blk, st)
        if lo >= hi:
            emit(("empty_split",), 0, 0, 0)
            continue
        if lo == pos:
            emit(("new_row_only",), 0, 0, 0)
        got = walk_split(lo, hi, pos, hd, prefetched, emit)
        assert sorted(got) == list(range(lo, hi)), f"split {s} [{lo}, {hi}) consumed {sorted(got)[:8]}.. ({len(got)} rows)"
        seen += got
    assert sorted(seen) == list(range(pos + 1)), f"nsplit {nsplit} pos {pos}: {len(seen)} rows consumed of {pos + 1}"
    return c


def events_of(pairs, hd=128):
    """Union of the events of (nsplit, pos) pairs."""
    ev = set()
    for nsplit, pos in sorted(set(pairs)):
        ev |= census(nsplit, pos, hd).events
    return ev


def required_events(form):
    """The events the long-context tests must reach per form of the kernel: "xl" = the XCD-local form (32 splits, up to 8192
    cache rows), "general" = the general form over all its split counts (1, 2, 4, 8, 16, 32).  Everything the census can
    report, less what a form cannot reach at its split count:
      xl: a refill issued in blk 2 needs a split of more than 2 x 96 + 96 = 288 positions; 32 splits of at most 8192 rows hold
          at most 256.
    The general form reaches all of them (the one-split walk of a 512-row cache goes to blk 5)."""
    ev = {("empty_split",), ("new_row_only",), ("partial_step",)}
    ev |= {("blk", b, gw) for b in range(3) for gw in range(4)}
    ev |= {("refill", b, gw) for b in range(3) for gw in range(4)}
    ev |= {("new_row", b) for b in range(3)}
    ev |= {("refill_skipped", st) for st in range(KVST)}
    if form == "xl":
        ev -= {("refill", 2, gw) for gw in range(4)}
    return ev


def describe(nsplit, pos, hd=128):
    """One line for a failure report: the events of the frame with the (split, wave, blk, st) where each first occurs."""
    c = census(nsplit, pos, hd)
    parts = [f"{'/'.join(str(x) for x in ev)}@split{w[0]}.gw{w[1]}.blk{w[2]}.st{w[3]}" for ev, w in sorted(c.where.items())
             if ev[0] != "blk" or ev[1] == c.deepest(ev[2])]
    return f"nsplit {nsplit} pos {pos} chunk {c.chunk}: " + ", ".join(parts)
