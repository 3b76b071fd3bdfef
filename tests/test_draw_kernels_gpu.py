"""GPU: every draw launch (csrc/ar_kernels.h: sample_small_kernel, sample_block_kernel, samp_cut / samp_count / samp_race /
samp_finish_kernel, and finish_draw behind all of them) ONE LAUNCH AT A TIME through the product's own host routine
(ft_test_draw -> enqueue_sample), several rows per launch, judged field by field against tests/draw_ref.py: the kept set as a
band observed through probe noise, the counter-based noise against its integer restatement, the SampCut record, the penalised
row left behind bit for bit, finish_draw's bookkeeping exactly, every sentinel intact.  tests/test_draw_ref_host.py proves
that judge() flags the faults this is for, and that the inputs (tests/draw_cases.py) satisfy the band and probe-validity caps on the reference
alone.  A flag names the row, the field, the rank and the class.

Contexts are tests/shapes.py's tiny widths with the vocabulary and the codebook size varied (the draw kernels see only V),
and one context at the real widths with 1 + 1 layers for the lock-step forms."""
import os

import numpy as np
import pytest
import torch

from tests import draw_ref as D
from tests.draw_cases import (BLOCK_V, EDGES, FMTS, FOUR_V, NEW, SMALL_V, configs_for, counter_rows, discriminating, frames_used,
                              launches, model_of, new_for, plan, rows_for, shape_for, strict_q_row)

pytestmark = pytest.mark.gpu

PREC = {"bf16": "bf16", "fp16": "fp16", "f32": "fp32"}
_ENG = {}
TALLY = {0: D.Tally(), 1: D.Tally(), 2: D.Tally()}
SEEN, RECENT = set(), set()                                                # (path, what & 28): of the file, of the running test
FRAMES_SEEN = {}                                                           # (fmt, cb, V) -> nf values its launches used
RAN = set()                                                                # test functions of this file that ran


# ------------------------------------------------------------------------------------------------------------ contexts
def context(fmt, MB, new=NEW, env=(), **kw):
    """(engine, DrawModel) shared by the tests of this module, created without the frame engine."""
    k = (fmt, MB, new, env, tuple(sorted(kw.items())))
    if k not in _ENG or not _ENG[k][0]._h:
        from fish_tts_amd.ar_engine import ARHipEngine
        from tests.hip_util import args_from_shape, cached_random_weights
        shape = shape_for(**kw)
        sets = dict((("FT_NO_ENGINE", "1"),) + tuple(env))
        saved = {n: os.environ.get(n) for n in sets}
        os.environ.update(sets)
        try:
            eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                              precision=PREC[fmt], device=0, max_batch=MB, max_new_tokens=new)
            w = cached_random_weights(shape, seed=0)
            eng.load_state_dict({n: v.to(D.DT[fmt]) for n, v in w.items()})
        finally:
            for n, v in saved.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
        _ENG[k] = (eng, model_of(fmt, shape, MB, new, w, eng))
    return _ENG[k]


def drop_contexts():
    for eng, _ in _ENG.values():
        eng.close()
    _ENG.clear()


REACH = {"test_small_kernel", "test_block_kernel", "test_four_launch_draw", "test_lock_step_launches", "test_table_row_wider_than_two_steps"}


@pytest.fixture(autouse=True)
def _note_test(request):
    RAN.add(request.node.originalname)
    yield


@pytest.fixture(scope="module", autouse=True)
def _close_engines_and_sum_up():
    """At the end of the file: the per-path figures (DESIGN.md section 2 quotes those of one MI355X run) and, if the tests that define the reach
    all ran (a selection with -k sums up nothing), what they reached: the three paths, both lock-step forms, the table, and every
    frame edge on every path and type."""
    yield
    drop_contexts()
    for p, name in ((0, "sample_small_kernel"), (1, "sample_block_kernel"), (2, "four-launch draw")):
        t = TALLY[p]
        print(f"\n{name}: {t.probes} probes, {t.left_out} left out, widest band {t.widest_band} ranks, {t.draws} noise draws, "
              f"{t.allowed} needed the allowance", end="")
    if REACH <= RAN:
        assert {p for p, _ in SEEN} == {0, 1, 2}, SEEN
        assert {w for _, w in SEEN} >= {0, 4, 8, 20}, SEEN
        short = {k: sorted(EDGES - v) for k, v in FRAMES_SEEN.items() if not EDGES <= v}
        assert not short, f"frame edges not reached: {short}"


# ------------------------------------------------------------------------------------------------------------ configurations
def run(eng, model, cb, parts, last=False):
    fl = []
    for part in parts:
        got = eng.test_draw(np.stack([r.logits for r in part]), cb, [eng._sampling(r.ctl.temperature, r.ctl.top_p, r.ctl.rep, r.ctl.seed, r.ctl.ban_eos) for r in part],
                            [r.nf for r in part], np.stack([r.hist for r in part]), last=last, pos=[r.pos for r in part],
                            done=[r.done for r in part], noise=D.noise_block(model, cb, part))
        t = TALLY[got["path"]]
        SEEN.add((got["path"], got["what"] & 28))
        RECENT.add((got["path"], got["what"] & 28))
        f = D.judge(model, cb, last, part, got, t)
        fl += [f"M {len(part)} cb {cb} {x} [{part[x.row].tag if x.row >= 0 else ''}; {part[max(x.row, 0)].ctl}; nf {part[max(x.row, 0)].nf}]" for x in f]
    return fl


# ------------------------------------------------------------------------------------------------------------ the cases
def run_plan(kind, fmt, size=None, env=()):
    kw, MB, parts, sizes = plan(kind, fmt, size)
    eng, model = context(fmt, MB, new=new_for(kind), env=env, **kw)
    total = left = 0
    fl = []
    for cb, n, seed, ckw in parts:
        rows, t, l, filler = rows_for(model, cb, configs_for(model, cb, n, seed, **ckw), seed)
        parts_ = launches(model, cb, rows, sizes, filler, seed)
        FRAMES_SEEN.setdefault((model.fmt, cb, model.width(cb)), set()).update(frames_used(parts_))
        fl += run(eng, model, cb, parts_)
        path = 0 if model.width(cb) <= 1024 else 2 if model.fmt == "bf16" else 1
        TALLY[path].probes += t - l
        TALLY[path].left_out += l
        total, left = total + t, left + l
    assert left <= 0.1 * total, f"{left} of {total} probes invalid: a bad input family"
    assert not fl, f"{len(fl)} flags, first: " + "\n".join(fl[:6])
    return eng, model, total - left


@pytest.mark.parametrize("fv", SMALL_V)
@pytest.mark.parametrize("fmt", FMTS)
def test_small_kernel(fmt, fv):
    """sample_small_kernel at a full last thread (1024), a partial one (V % 4 != 0), idle waves (V <= 192) and one lane (5);
    cb in {1, 2, ncb - 1}; launches of 1, 4, 5 and 33 rows with mixed controls and frames."""
    assert run_plan("small", fmt, fv)[2] > 30
    drop_contexts()


@pytest.mark.parametrize("fmt", FMTS)
def test_small_kernel_66_rows(fmt):
    """max_batch = 66 (cap = 66, so that 66 rows of one launch differ in nf): launches of 66, 65 and 5 rows at cb = 1 and
    ncb - 1 - grid rows 33 .. 65 of sample_small_kernel and finish_draw, which a batch beyond the MFMA launches' 64 rows runs."""
    eng, model, n = run_plan("rows66", fmt)
    assert model.MB == 66 and model.cap == 66 and n > 250
    drop_contexts()


@pytest.mark.parametrize("fmt", FMTS)
def test_small_kernel_semantic_draw(fmt):
    """cb = 0 on a vocabulary of 1024: the R-id window, ban_eos, the code clamp below (a text token wins)."""
    run_plan("semantic", fmt)
    drop_contexts()


@pytest.mark.parametrize("V", BLOCK_V)
@pytest.mark.parametrize("fmt", ("fp16", "f32"))
def test_block_kernel(fmt, V):
    run_plan("block", fmt, V)
    drop_contexts()


@pytest.mark.parametrize("fmt", ("fp16", "f32"))
def test_block_kernel_real_vocabulary(fmt):
    run_plan("block_real", fmt)
    drop_contexts()


@pytest.mark.parametrize("V", FOUR_V)
def test_four_launch_draw(V):
    """1025: the second chunk holds one logit; 2319: rows >= 1 unaligned (scalar fall-back); 16384: one vector step, no tail;
    16385; 32784: a second step in flight; 49152: fa reloaded; 65540; 155776 with a class of > 65535 members (the recount)."""
    run_plan("four", "bf16", V)
    drop_contexts()


@pytest.mark.parametrize("env", [(), (("FT_NO_PAIR", "1"),), (("FT_NO_QKV0", "1"),)], ids=["pair", "no_pair", "no_qkv0"])
@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_lock_step_launches(fmt, env):
    """M >= wide_min on the real widths: the octet-major copy (to the paired pass's rows at cb = 0 unless FT_NO_PAIR), the table
    row at cb = 1 (not with FT_NO_QKV0, never at cb = ncb - 1).  fast_head_dim is a multiple of 8 in every model the loader
    accepts for the lock-step path (fqkvN % 32 == 0), so finish_draw's scalar table copy (qkv0_n % 8 != 0) is dead and is not
    tested; qkv0_n = 2048 here: the third copy loop (d >= 2 x 256 x 8 = 4096) is test_table_row_wider_than_two_steps."""
    RECENT.clear()
    eng, model, _ = run_plan("wide", fmt, env=env)
    assert model.xo_pair == 16 and (model.qkv0_tab is None) == (env == (("FT_NO_QKV0", "1"),))
    new = set(RECENT)
    big = 2 if fmt == "bf16" else 1
    assert (big, 4 if env == (("FT_NO_PAIR", "1"),) else 8) in new
    assert (0, 4 if env == (("FT_NO_QKV0", "1"),) else 20) in new and (0, 4) in new
    drop_contexts()


def test_table_row_wider_than_two_steps():
    """A fast stack of 16 heads and 16 KV heads of 128 (H hd = 2048, q k v width 6144), which the loader accepts for the lock-step
    path: finish_draw copies the first 4096 elements of the table row from the two 16-byte pieces it fetched beside the
    embedding row and the last 2048 in its third loop (d >= TQ x T x 8).  cb = 1, the table in use."""
    RECENT.clear()
    eng, model, _ = run_plan("wide6144", "bf16")
    assert model.qkv0_tab is not None and model.qkv0_tab.shape == (model.fastV, 6144)
    assert (0, 20) in RECENT, RECENT                                        # (a last launch of fewer than 5 rows is no lock-step one)
    drop_contexts()


@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_layer0_qkv_table(fmt):
    """The table the draw copies rows of is judged once: rows {0, 1, 63, 64, 65, fastV - 1} and 64 seeded ones against
    tests/wide_ref.py's fused-norm Linear of the embedding rows (the launch that built them), acceptance as there."""
    from tests import wide_ref as WR
    from tests.hip_util import cached_random_weights
    eng, model = context(fmt, 8, wide=True)
    shape = shape_for(wide=True)
    w = cached_random_weights(shape, seed=0)
    cast = lambda n: w[n].to(D.DT[fmt]).to(torch.float64)
    g = np.random.default_rng(5)
    rows = sorted(set([0, 1, 63, 64, 65, model.fastV - 1] + g.integers(0, model.fastV, size=64).tolist()))
    assert model.qkv0_tab is not None and model.qkv0_tab.shape == (model.fastV, 2048)
    ref = WR.linear_ref(fmt, WR.STORE, X=cast("fast_embeddings.weight")[rows], W=cast("fast_layers.0.attention.wqkv.weight"),
                        gain=cast("fast_layers.0.attention_norm.weight"), eps=shape.norm_eps, seed=3)
    ver = WR.check(model.qkv0_tab[rows], ref.ref, ref.err, fmt)
    print(f"layer-0 q k v table {fmt}: {ver.checked} elements, largest |got - ref| / bound {ver.worst:.3f}, r_stage {ref.r_stage:.2e}")
    assert ver.flagged == 0 and ver.checked == len(rows) * 2048, (ver.flagged, ver.worst, ver.rows[:8], ver.cols[:8])
    assert eng.test_qkv0_tab(model.fastV - 1, 1).shape == (1, 2048)
    drop_contexts()


@pytest.mark.parametrize("fmt", FMTS)
def test_last_draw_of_a_frame(fmt):
    """last = 1 on one launch mixing a live row that draws a code above the clamp, one that draws a text token, a frozen row, a
    row at nf = cap and a row whose probe forces im_end; then at cb = ncb - 1, where the product sets it."""
    eng, model = context(fmt, 6, V=4097, cbsize=1024)
    lg = D.family_logits(fmt, 4097, 1.0, 12)
    filler = D.random_hist(model, 3)
    c = D.Ctl(1.0, 1.0, 1.0)
    mk = lambda cb, j, nf, done=0: D.Row(logits=lg[: model.width(cb)], ctl=c, nf=nf, hist=filler.copy(), pos=40 + nf, done=done, probe=j)
    rows = [mk(0, 4000, 3), mk(0, 17, 4), mk(0, 600, 5, done=1), mk(0, 700, model.cap), mk(0, model.im_end, 6), mk(0, 2000, model.cap - 1)]
    for cb, part in ((0, rows), (model.ncb - 1, [mk(model.ncb - 1, 1000, 3), mk(model.ncb - 1, 3, model.cap, done=1), mk(model.ncb - 1, 77, model.cap - 1)])):
        for r in part:
            r.ref = D.reference(model, cb, r)
            assert D.probe_valid(model, r.ref, r.probe)
        fl = run(eng, model, cb, [part], last=True)
        assert not fl, "\n".join(fl[:6])
    drop_contexts()


@pytest.mark.parametrize("fmt,V", [("bf16", 1024), ("fp16", 1024), ("f32", 1024), ("f32", 2319), ("fp16", 2319), ("bf16", 2319)])
def test_counter_based_noise(fmt, V):
    """No injected noise: q comes from philox4 on (index / 4, codebook, frame, 0) keyed by the row's 64-bit seed.  At least 64
    draws per path and type over seeds with non-zero high words, nf up to 700, every codebook; the rows of one launch differ in
    seed and frame.  At least half of the draws must be discriminating (see above): the others pass under any noise.  At most
    2 % of the draws may need the logf allowance (tests/draw_ref.py)."""
    eng, model = context(fmt, 8, new=700, V=2319)
    t0 = (TALLY[0 if V <= 1024 else 2 if fmt == "bf16" else 1].draws, TALLY[0 if V <= 1024 else 2 if fmt == "bf16" else 1].allowed)
    fl, n, hard, cbs = [], 0, 0, set()
    for cb, part in counter_rows(model, fmt, V):
        fl += run(eng, model, cb, [part])
        n += len(part)
        hard += sum(discriminating(r) for r in part)
        cbs.add(cb)
    t = TALLY[0 if V <= 1024 else 2 if fmt == "bf16" else 1]
    assert n >= 64 and cbs == ({0} if V > 1024 else set(range(1, model.ncb))), (n, cbs)
    assert hard >= n // 2, f"only {hard} of {n} draws are discriminating"
    assert not fl, "\n".join(fl[:6])
    assert t.allowed - t0[1] <= 0.02 * (t.draws - t0[0]), (t.allowed - t0[1], t.draws - t0[0])
    drop_contexts()


@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_noise_is_rounded_to_the_type(fmt):
    """Two tied logits whose q differ by less than half a step of the type: equal once rounded, so the lower index wins."""
    eng, model = context(fmt, 8, V=2319)
    fl = run(eng, model, 1, [[strict_q_row(model, fmt)]])
    assert not fl, fl
    drop_contexts()


def test_what_the_hook_refuses():
    from fish_tts_amd.ar_engine import HipError
    eng, model = context("f32", 3, V=1025)
    lg = np.zeros((1, 1025), dtype=np.float32)
    sp = [eng._sampling(0.7, 0.8, 1.1)]
    hist = np.zeros((1, model.R, model.cap), dtype=np.int32)
    ok = eng.test_draw(lg, 0, sp, [0], hist)
    assert ok["path"] == 1
    big = (np.zeros((4, 1025), dtype=np.float32), 0, sp * 4, [0] * 4, np.zeros((4, model.R, model.cap), dtype=np.int32))
    for kw, args in ((dict(), (lg, model.ncb, sp, [0], hist)), (dict(), (lg, -1, sp, [0], hist)), (dict(), (lg, 0, sp, [model.cap + 1], hist)),
                     (dict(), (lg, 0, sp, [-1], hist)), (dict(noise=np.ones((1, model.V + (model.ncb - 1) * model.fastV))), (lg, 0, sp, [1], hist)),
                     (dict(noise=np.ones((2, 100))), (lg, 0, sp, [1], hist)),
                     (dict(), big),                                          # M = 4 > max_batch = 3
                     (dict(last=2), (lg, 0, sp, [0], hist)), (dict(last=-1), (lg, 0, sp, [0], hist)),
                     (dict(omit="logits"), (lg, 0, sp, [0], hist)), (dict(omit="seq"), (lg, 0, sp, [0], hist)),
                     (dict(omit="cut"), (lg, 0, sp, [0], hist))):
        with pytest.raises(HipError, match="ft_test_draw"):                  # the hook's own refusal, nothing raised on the way to it
            eng.test_draw(*args, **kw)
    again = eng.test_draw(lg, 0, sp, [0], hist)                              # a refusal leaves the context usable
    assert again["path"] == 1 and np.array_equal(again["tokn"], ok["tokn"])
    drop_contexts()


