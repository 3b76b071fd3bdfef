"""Inputs of the draw tests, shared by tests/test_draw_kernels_gpu.py (which runs them on the device) and
tests/test_draw_ref_host.py (which checks, on the reference alone, that they satisfy the band, normaliser and probe-validity
conditions of tests/draw_ref.py): shapes and models, row configurations, probe rows, their packing into launches, the plan of
every probe test, the rows of the counter-noise test and the exact-tie row of the noise-rounding test.  Nothing here needs a
GPU or the library."""
import dataclasses

import numpy as np
import torch

from tests import draw_ref as D
from tests.shapes import tiny_shape

FMTS = ("bf16", "fp16", "f32")
NEW = 8                                                                    # max_new_tokens: cap = 32
EDGES = {0, 1, 2, 16, 17, 18, NEW + 23, NEW + 24}                          # nf = 0, both sides of ws = 0 | it - 16, cap - 1, cap
NEW_ROWS66 = 42                                                            # cap = 66: the rows of one launch differ in nf, 0 .. cap - 1 and cap


def new_for(kind):
    """max_new_tokens of a plan's context."""
    return NEW_ROWS66 if kind == "rows66" else NEW


def shape_for(V=2319, cbsize=2048, ncb=10, wide=False, n_slots=128):
    if wide:
        from tests.test_ar_gpu import medium_shape
        over = dict(fast_n_head=16, fast_n_local_heads=16, fast_head_dim=128) if wide == 6144 else {}   # fast q k v width 6144
        return medium_shape(n_text=17, n_layer=1, n_fast_layer=1, max_seq_len=n_slots, **over)
    s = tiny_shape()
    sem_end = min(V - 1, s.semantic_begin_id + 2047)
    return dataclasses.replace(s, vocab_size=V, codebook_size=cbsize, num_codebooks=ncb, semantic_end_id=sem_end)


def model_of(fmt, shape, MB, new=NEW, weights=None, eng=None):
    if weights is None:
        fe = np.zeros((shape.codebook_size, shape.fast_dim), dtype=np.float32)
    else:
        fe = weights["fast_embeddings.weight"].to(D.DT[fmt]).to(torch.float32).numpy()
    m = D.DrawModel(fmt=fmt, V=shape.vocab_size, fastV=min(1024, shape.codebook_size), ncb=shape.num_codebooks, cap=new + 24,
                    sem_begin=shape.semantic_begin_id, im_end=shape.im_end_id, cbsize=shape.codebook_size, fast_emb=fe, MB=MB)
    if eng is not None and "MFMA launches" in eng.frame_path():
        m.xo_pair = (MB + 15) // 16 * 16
        m.qkv0_tab = eng.test_qkv0_tab(0, m.fastV)
    return m



def configs_for(model, cb, n, seed, variants=("plain", "top3", "cut40", "plain", "plain", "plain"), t0=False):
    """n row configurations (logits, Ctl, window ids, {1: reference at nf > 0, 0: reference at nf = 0, "spread", "skipped"}):
    the five controls in turn (then T = 0), variants cycling, ban_eos on every other one; the window ids hold a duplicate, an id
    outside [0, V) where the row allows one, and im_end.
    The spread of a configuration: 0.3, 1, 3, 8 are tried in turn from a seeded start.  A spread at which the reference raises
    BandTooWide or NormaliserTooClose is a bad input and is passed over (the float32 chain sum of 155 776 probabilities is
    uncertain by ~3e-5, more than eight ranks of a flat row's tail).  Of the admitted spreads the first with at most 10 % of its
    probes invalid is taken, else the one with the fewest invalid.  None admitted: BandTooWide.  All of this is decided by the
    reference alone.  "spread" is the one used, "skipped" the (spread, reason) pairs passed over; tests/test_draw_ref_host.py
    pins which spreads each kind of test ends up with."""
    V = model.width(cb)
    zeros = np.zeros((model.R, model.cap), dtype=np.int32)
    out = []
    for i in range(n):
        tp, T, rep = D.CONTROLS[i % 5]
        if t0 and i == n - 1:
            tp, T, rep = 0.8, 0.0, 1.1
        var = variants[i % len(variants)]
        if var == "big" and V < 140000:
            var = "plain"
        n_ids = model.R if cb == 0 else 16
        ctl = D.Ctl(tp, T, rep, ban_eos=i % 2 == 0)
        best, skipped = None, []
        for k in range(4):
            lg = D.family_logits(model.fmt, V, D.SPREADS[(i + seed + k) % 4], 1000 * seed + i, var, tp)
            ids = D.pick_ids(lg, n_ids, tp, np.random.default_rng(1000 * seed + i))
            if cb >= 1:
                ids[2] = 1023 if V < 1024 else ids[2]                      # a code the fast vocabulary does not hold
                ids[3] = -1
            elif model.im_end < V and i % 3 == 0:
                ids[2] = model.im_end
            try:
                rows = {nf: D.Row(logits=lg, ctl=ctl, nf=nf, hist=D.hist_for(model, cb, nf, ids, zeros)) for nf in (1, 0)}
                refs = {nf: D.reference(model, cb, r) for nf, r in rows.items()}
            except D.BandTooWide as err:
                skipped.append((D.SPREADS[(i + seed + k) % 4], type(err).__name__))
                continue
            pr = D.probe_list(model, refs[1], rows[1], cb)
            bad = sum(not D.probe_valid(model, refs[1], j) for _, j in pr) / len(pr)
            if best is None or bad < best[0]:
                best = (bad, lg, ids, dict(refs, spread=D.SPREADS[(i + seed + k) % 4], skipped=skipped))
            if bad <= 0.1:
                break
        if best is None:
            raise D.BandTooWide(f"no spread admits control {ctl} at V = {V}")
        _, lg, ids, refs = best
        out.append((lg, ctl, ids, refs))
    return out


def rows_for(model, cb, configs, seed):
    """The probe rows of the configurations, plus up to two probes at nf = 0 per configuration; -> (rows without nf / hist yet,
    probes, left out, the history filler)."""
    filler = D.random_hist(model, seed)
    rows, total, left = [], 0, 0
    for lg, ctl, ids, refs in configs:
        for nf in (1, 0):
            ref = refs[nf]
            base = D.Row(logits=lg, ctl=ctl, nf=nf, hist=D.hist_for(model, cb, nf, ids, filler))
            probes = D.probe_list(model, ref, base, cb)
            if nf == 0:
                probes = probes[:2]
            if ctl.temperature == 0:
                # T = 0 (Tc = 1e-5): every probability but the top one underflows to 0, so no probe but the argmax can be
                # valid by construction; the configuration runs that probe and three rows of random noise (whatever the noise,
                # the top token wins), and is not part of the left-out share
                probes = [p for p in probes if p[0] == "argmax"]
                if nf == 1:
                    g = torch.Generator().manual_seed(seed)
                    for _ in range(3):
                        q = torch.empty(len(lg)).exponential_(1.0, generator=g).clamp_min_(1e-6).numpy()
                        rows.append((D.Row(logits=lg, ctl=ctl, nf=nf, hist=None, noise=q, tag="random noise at T = 0", ref=ref), ids))
            for kind, j in probes:
                total += 1
                if not D.probe_valid(model, ref, j):
                    left += 1
                    continue
                rows.append((D.Row(logits=lg, ctl=ctl, nf=nf, hist=None, probe=j, tag=kind, ref=ref), ids))
    return rows, total, left, filler


def frames(cap, start=0):
    """nf of the rows of one launch: the edges of the window rule first (cap, cap - 1, 18, 17, 16, 2, 1), rotated by `start` so
    that short launches (1 to 5 rows) reach every one of them in turn, then the frames in between."""
    first = [cap, cap - 1, 18, 17, 16, 2, 1]
    k = start % len(first)
    return first[k:] + first[:k] + [n for n in range(3, cap - 1) if n not in first]


def launches(model, cb, rows, sizes, filler, shuffle_seed=0):
    """Packs the rows into launches of the given sizes (cycling; mixed configurations in one launch), nf distinct inside one."""
    g = np.random.default_rng(shuffle_seed)
    rows = [rows[i] for i in g.permutation(len(rows))]
    zeros, rest = [r for r in rows if r[0].nf == 0], [r for r in rows if r[0].nf != 0]
    out, s = [], 0
    at = 0                                                                 # where the next launch starts in the list of edges
    while zeros or rest:
        M = min(sizes[s % len(sizes)], model.MB)
        s += 1
        fr_all = frames(model.cap, at)
        part = []
        if zeros:                                                          # nf = 0 once per launch: nf is distinct inside one
            row, _ = zeros.pop()
            row.hist = filler.copy()
            part.append(row)
        for nf in fr_all:
            if not rest or len(part) >= M:
                break
            row, ids = rest.pop()
            row.nf, row.hist = nf, D.hist_for(model, cb, nf, ids, filler)
            part.append(row)
            at += 1
        for i, row in enumerate(part):
            row.pos = 7 + i
        out.append(part)
    return out


def frames_used(parts):
    return {r.nf for part in parts for r in part}



SMALL_V = (5, 63, 64, 65, 255, 257, 1021, 1024)
FOUR_V = (1025, 2048, 2319, 16384, 16385, 32784, 49152, 65540, 155776)
BLOCK_V = (1025, 2319, 4097)


FOUR_VARIANTS = ("plain", "top3", "cut40", "big")


def plan(kind, fmt, size=None):
    """(context arguments, max_batch, [(cb, configurations, seed, configs_for arguments)], launch sizes) of one test: the GPU
    tests below run it, tests/test_draw_ref_host.py checks the caps on the very same inputs."""
    # T = 0 (the clamp to 1e-5) runs in bf16 and f32.  In fp16 the reference itself has no defined draw there: l / 1e-5 leaves
    # fp16's range for |l| > 0.655, inf - inf makes every probability NaN and torch.argmax of NaNs names an arbitrary index
    t0 = fmt != "fp16"
    if kind == "small":
        return dict(cbsize=size), 33, [(cb, 5, size + cb, {}) for cb in (1, 2, 9)], (33, 1, 4, 5)
    if kind == "rows66":
        # the small path beyond the 33 rows of "small": max_batch = 66, launches of 66, 65 and 5 rows (grid rows 33 .. 65 of
        # sample_small_kernel and finish_draw); ten configurations per codebook give the rows of one launch of each size
        return dict(cbsize=257), 66, [(cb, 10, 70 + cb, {}) for cb in (1, 9)], (66, 65, 5)
    if kind == "semantic":
        return dict(V=1024, cbsize=512), 33, [(0, 6, 3, dict(t0=t0))], (5, 33, 4)
    if kind == "block":
        return dict(V=size), 3, [(0, 6, size % 97, dict(t0=t0))], (3, 1)
    if kind == "block_real":
        return dict(V=155776), 3, [(0, 2, 5, {})], (3, 1)
    if kind == "four":
        return dict(V=size), 5, [(0, 6, size % 97, dict(t0=True, variants=FOUR_VARIANTS))], (5, 1, 2)
    if kind == "wide":
        return dict(wide=True), 8, [(cb, 3, 11 + cb, {}) for cb in (0, 1, 9)], (8, 5, 6)
    if kind == "wide6144":
        return dict(wide=6144), 8, [(1, 3, 17, {})], (8, 5, 6)
    raise KeyError(kind)


def plans():
    return ([("small", f, v) for f in FMTS for v in SMALL_V] + [("rows66", f, None) for f in FMTS] + [("semantic", f, None) for f in FMTS] +
            [("block", f, v) for f in ("fp16", "f32") for v in BLOCK_V] + [("block_real", f, None) for f in ("fp16", "f32")] +
            [("four", "bf16", v) for v in FOUR_V] + [("wide", f, None) for f in ("bf16", "fp16")] + [("wide6144", "bf16", None)])


def family_cases():
    """(name, DrawModel, [(cb, configurations, seed)]) of every probe test below, on models without a context."""
    for kind, fmt, size in plans():
        kw, MB, parts, _ = plan(kind, fmt, size)
        m = model_of(fmt, shape_for(**kw), MB, new_for(kind))
        yield f"{kind} {fmt} {size}", m, [(cb, configs_for(m, cb, n, seed, **ckw), seed) for cb, n, seed, ckw in parts]



def counter_rows(model, fmt, V):
    """Launches of 8 rows: seeds with non-zero high words, nf in 0..700, every codebook of the path once (nine launches on the
    small path, cb = 1 .. ncb - 1; eight at cb = 0 on the others), the controls in turn (the next one where the band rule does
    not admit the row)."""
    cbs = [0] * 8 if V > 1024 else list(range(1, model.ncb))
    g = np.random.default_rng(V + len(fmt))
    for i, cb in enumerate(cbs):
        lg = D.family_logits(fmt, model.width(cb), D.SPREADS[i % 4], 50 + i)
        part = []
        for m in range(8):
            seed = (int(g.integers(1, 2 ** 32)) << 32) | int(g.integers(0, 2 ** 32))
            nf, hist = int(g.integers(0, 701)), D.random_hist(model, i * 8 + m)
            for k in range(5):
                tp, T, rep = D.CONTROLS[(i + m + k) % 5]
                r = D.Row(logits=lg, ctl=D.Ctl(tp, T, rep, seed=seed), nf=nf, hist=hist)
                try:
                    r.ref = D.reference(model, cb, r)
                    break
                except D.BandTooWide:
                    assert k < 4
            part.append(r)
        yield cb, part


def discriminating(row):
    """A draw that can expose wrong noise: the second-largest kept probability is at least a tenth of the largest (where one
    token holds nearly all the mass it wins whatever q is)."""
    p = np.sort(row.ref.probs)[::-1]
    return len(p) > 1 and p[1] >= 0.1 * p[0]


def strict_q_row(model, fmt):
    """Two exactly tied logits that hold all the mass (p = 1/2 each).  q of the lower index lies just above 1, q of the higher
    just below, both round to 1 in fmt: the ratios tie and the lower index wins.  With q unrounded the ratios 0.5 / q round to
    two different values of the type (below 0.5 the step is half the step above 1) and the higher index wins."""
    up, dn = {"bf16": (0.0035, 0.0018), "fp16": (0.00045, 0.0002)}[fmt]
    lg = np.full(1024, -30000.0, dtype=np.float32)
    lg[[100, 900]] = 4.0
    q = np.full(1024, 1.0, dtype=np.float32)
    q[100], q[900] = 1.0 + up, 1.0 - dn
    row = D.Row(logits=lg, ctl=D.Ctl(1.0, 1.0, 1.0), nf=0, hist=D.random_hist(model, 0), noise=q, strict=True)
    row.ref = D.reference(model, 1, row)
    return row
