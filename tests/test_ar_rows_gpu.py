"""GPU: the multi-row decode launches from 5 to 256 rows - what every lock-step batch runs that the MFMA launches do not take
(65..256 rows, any fp32 batch, fast-stack biases, fast_dim != dim, FT_NO_WIDE): gemv_mb_kernel over ceil(M / MB) groups,
gemv_kernel with grid.y = M, attn_decode_kernel with grid.z = M, gemv_attn_combine_kernel with grid.y = M and
fast_attn_kernel writing f32 rows - ONE LAUNCH AT A TIME through the hooks of tests/test_ar_kernels_gpu.py (ft_test_gemv,
ft_test_decode_attn, ft_test_fast_attn form 0), judged by the same float64 restatement (tests/ar_ref.py) under the same bound

    |got - ref| <= half a ulp of the stored format at max(|got|, |ref|) + err

on every element of every written row: nothing left out, nothing flagged, every sentinel and NaN region intact, every cache
row but the appended one bit-unchanged, the launch's <MB, R, NT> the one tests/ar_ref.want_id restates.  On top of that row m
of an M-row launch must equal the 1-row launch of the same row bit for bit (the claim of gemv_mb_kernel's comment and of
DESIGN.md section 2).  tests/test_ar_ref_host.py proves that the checker flags a tail group's dead rows stored, its live rows
computed from row M - 1, a group reading the group before it, and a merge reading row m mod 4's partials.

Then the seam, end to end: a 66-row bf16 batch at the real widths equals its single runs bit for bit, one frame of the same
state at 64 rows (MFMA launches) and at 66 rows (these launches) agree in their vocabulary logits within the project's
slow-logit rule (0.02 x the row's logit range), and nine fp32 utterances in lock step equal their single
runs.

The product hook takes its sizes from the call: one tiny context per type with max_batch = 256 serves every product."""
import os

import numpy as np
import pytest
import torch

from oracle import ar as O
from tests import ar_ref as A
from tests import wide_ref as WR
from tests.codec_stage_ref import F32, F64
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import make_prompt, tiny_shape
from tests.test_ar_gpu import medium_shape
from tests.test_ar_kernels_gpu import nan_from, sentinel, shape_of

pytestmark = pytest.mark.gpu

PREC = {"bf16": "bf16", "fp16": "fp16", "f32": "fp32"}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
MS = (5, 6, 7, 8, 9, 63, 64, 65, 66, 67, 255, 256)           # every M mod 4, the 63 | 64 step of R at N = 1024, the largest grid
K16 = (512, 1024, 2048, 3072, 4096)                          # NT 1, 2, 4, 6 and 8 (the last is no gemv_mb class)
K32 = (256, 1024, 3072)                                      # NT 1, 4, 12
NK_CAP, MN_CAP = 1 << 22, 1 << 18                            # operands stay small: N K <= 2^22, M N <= 2^18
EQ_ROWS = lambda M: sorted({0, 3, 4, M - 2, M - 1})
_ENG, _IN = {}, {}
STATS, IDS, EQ, NSPLITS = {}, set(), {}, set()


def engine(fmt, key="tiny", n_slots=128, max_batch=256, env=()):
    """A context shared by the tests of this module, created without the frame engine (the hooks need none)."""
    k = (fmt, key, n_slots, max_batch, env)
    if k not in _ENG or not _ENG[k]._h:
        from fish_tts_amd.ar_engine import ARHipEngine
        shape = shape_of(key, n_slots)
        sets = dict((("FT_NO_ENGINE", "1"),) + tuple(env))
        saved = {n: os.environ.get(n) for n in sets}
        os.environ.update(sets)
        try:
            eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                              precision=PREC[fmt], device=0, max_batch=max_batch, max_new_tokens=8)
            eng.load_state_dict({n: v.to(DT[fmt]) for n, v in cached_random_weights(shape, seed=0).items()})
        finally:
            for n, v in saved.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
        _ENG[k] = eng
    return _ENG[k]


def drop_engines():
    for eng in _ENG.values():
        eng.close()
    _ENG.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    drop_engines()
    _IN.clear()


def note(kind, worst, r_stage, n):
    s = STATS.setdefault(kind, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], worst), max(s[1], r_stage or 0.0), s[2] + n
    return f"{kind}: largest |got - ref| / bound {s[0]:.3f}, largest r_stage {s[1]:.2e}, {s[2]} elements so far"


def kind_of(ids):
    return f"gemv_mb_kernel<R {ids[1]}, MB {ids[0]}>" if ids[0] else f"gemv_kernel<R {ids[1]}>, grid.y = M"


# ------------------------------------------------------------------------------------------------------ products
def n_max(K):
    return min(NK_CAP // K, 16384)


def n_values(M, K):
    """1, 5, both sides of R = 1 | 2 (N M = 2048) and of R = 2 | 4 (N M = 65536), 1024 - where inside the caps."""
    t2, t4 = -(-2048 // M), -(-65536 // M)
    return [N for N in dict.fromkeys((1, 5, t2 - 1, t2, t4 - 1, t4, 1024)) if 1 <= N <= n_max(K) and M * N <= MN_CAP]


def gemv_case(fmt, K):
    """Inputs of 256 rows x n_max(K) weight rows, made once; the float64 contractions (with and without the fused norm) are
    computed once per prologue: a launch of M rows and N weight rows reads the prefixes, whose sums are the prefixes of these."""
    key = ("gemv", fmt, K)
    if key not in _IN:
        _IN.clear()                                                        # one case's operands at a time
        x, W, gain, bias, resid = A.seeded_gemv_inputs(fmt, 256, n_max(K), K, seed=7000 + K)
        _IN[key] = (x, W, gain, bias, resid, {0: None, 1: None, "bits": tuple(A.wbits(t, fmt) for t in (W, gain, bias))})
    return _IN[key]


def launch(fmt, K, pro, epi, rows, N, with_bias, alias, nt, pad_x, pad_o):
    """One ft_test_gemv call on the rows `rows` (a slice or a list of one) of the case."""
    x, _, _, _, resid, pres = gemv_case(fmt, K)
    Wb, gb, bb = pres["bits"]                                              # the patterns of the whole case, made once
    oc = N // 2 if epi == A.EPI_SWIGLU else N
    ldo = oc + (-oc) % 4 + pad_o
    return engine(fmt).test_gemv(pro, epi, x[rows].numpy(), Wb[:N], gb if pro else None, bb[:N] if with_bias else None,
                                 resid[rows, :N].numpy() if epi == A.EPI_RESID else None, alias=alias, nt=nt, ldx=K + pad_x, ldo=ldo)


def run_gemv(fmt, K, pro, epi, M, N, with_bias, alias=False, nt=True, pad_x=0, pad_o=0):
    x, W, gain, bias, resid, pres = gemv_case(fmt, K)
    if pres[pro] is None:
        pres[pro] = A.gemv_pre(fmt, pro, x, W, gain)
    acc, E, r, _ = pres[pro]
    oc = N // 2 if epi == A.EPI_SWIGLU else N
    out, pad, tail, ids = launch(fmt, K, pro, epi, slice(0, M), N, with_bias, alias, nt, pad_x, pad_o)
    what = f"{fmt} pro {pro} epi {epi} M {M} N {N} K {K} bias {with_bias} alias {alias} nt {nt} ldx +{pad_x} ldo +{pad_o} <MB, R, NT> {ids}"
    IDS.add(ids)
    assert ids == A.want_id(fmt, epi, M, N, K), what
    assert sentinel(pad) and sentinel(tail), "written outside the rows and columns of the product: " + what
    assert bool(np.isfinite(out).all()), what
    ref = A.gemv_ref(fmt, pro, epi, bias=bias[:N] if with_bias else None, resid=resid[:M, :N] if epi == A.EPI_RESID else None,
                     pre=(acc[:M, :N], E[:M, :N], r, None))
    ver = A.check(out, ref.ref, ref.err, fmt)
    line = note(kind_of(ids), ver.worst, r, ver.checked)
    assert ver.flagged == 0 and ver.checked == M * oc, f"{what}: {ver.flagged} flagged, worst {ver.worst:.3f}, rows {ver.rows[:12]}, cols {ver.cols[:12]}"
    # rows equal their single runs: once per (type, class, epilogue, K) AND row count - every M of MS, so every tail group
    # (1, 2, 3 live rows of MB = 4; 1 of MB = 2), the third and the last group and rows M - 2, M - 1 up to 256 rows, in every
    # class that M reaches - five 1-row launches of the same operands
    ek = (fmt, ids, epi, K, M)
    if ek not in EQ:
        differ = []
        for m in EQ_ROWS(M):
            one, pad1, tail1, _ = launch(fmt, K, pro, epi, [m], N, with_bias, alias, nt, pad_x, pad_o)
            assert sentinel(pad1) and sentinel(tail1), what
            if not np.array_equal(one[0].view(np.uint32), out[m].view(np.uint32)):
                differ.append((m, int((one[0].view(np.uint32) != out[m].view(np.uint32)).sum())))
        EQ[ek] = differ
        assert not differ, f"{what}: rows (row, differing elements) {differ} differ from their 1-row launches"
    return line


def products(fmt, K):
    line, i = "", 0
    for M in MS:
        for N in n_values(M, K):
            i += 1
            line = run_gemv(fmt, K, 1, A.EPI_STORE, M, N, with_bias=bool(i & 1), nt=bool(i & 2), pad_x=8 * (i % 3 == 0), pad_o=4 * (i % 2))
            line = run_gemv(fmt, K, 0, A.EPI_RESID, M, N, with_bias=not (i & 1), alias=bool(i & 2), nt=bool(i & 4), pad_x=4 * (i % 5 == 0))
        for N in (6, 14, 2048):
            if N <= n_max(K) and M * N <= MN_CAP:
                line = run_gemv(fmt, K, 1, A.EPI_SWIGLU, M, N, with_bias=False, nt=bool(M & 1), pad_o=4 * (M & 1))
    return line


@pytest.mark.parametrize("fmt,K", [(f, K) for f in ("bf16", "fp16") for K in K16] + [("f32", K) for K in K32])
def test_products_of_five_to_256_rows(fmt, K):
    """Every M of MS at N = 1, 5, both sides of the two R thresholds and 1024 (63 | 64 rows: R 2 -> 4, gemv_mb_kernel<2, 2> ->
    gemv_kernel<R = 4> from NT 4 on), the fused norm with the store and with SwiGLU (N = 6, 14: odd N / 2; 2048), no norm with
    the residual epilogue aliased and not, bias on and off, ldx > K, ldo past the columns, both load policies."""
    line = products(fmt, K)
    print(f"\n{fmt} K {K}: {line}; classes so far {sorted(IDS)}")


def want_classes():
    """What want_id can return for M >= 5 at the widths above (pinned on the CPU: test_dispatch_restated)."""
    mb = {(MB, R, nt) for MB, R in ((4, 1), (4, 2)) for nt in (1, 2)} | {(2, R, nt) for R in (1, 2) for nt in (4, 6)} | {(2, 4, 1), (2, 4, 2)}
    plain = {(0, 4, 4), (0, 4, 6)} | {(0, R, nt) for R in (1, 2, 4) for nt in (8, 1, 4, 12)}
    return mb | plain


def planned_classes():
    """(<MB, R, NT> -> the M at which it is launched) over exactly the launches products() makes, by want_id alone: no state
    of another test is read, and every launch asserts on the device that it ran the class want_id names."""
    out = {}
    for fmt, Ks in (("bf16", K16), ("fp16", K16), ("f32", K32)):
        for K in Ks:
            for M in MS:
                cases = [(A.EPI_STORE, N) for N in n_values(M, K)] + [(A.EPI_RESID, N) for N in n_values(M, K)]
                cases += [(A.EPI_SWIGLU, N) for N in (6, 14, 2048) if N <= n_max(K) and M * N <= MN_CAP]
                for epi, N in cases:
                    out.setdefault(A.want_id(fmt, epi, M, N, K), set()).add(M)
    return out


def test_every_product_class_of_the_multi_row_path_is_reached():
    """gemv_mb_kernel<R, MB> for (1, 4), (1, 2), (2, 4), (2, 2), (4, 2) and gemv_kernel<R> for R in 1, 2, 4 with grid.y = M: the
    launches of test_products_of_five_to_256_rows cover the whole set, each gemv_mb class at a row count with a tail group
    and at one with three groups or more.  Derived from the case list itself (each launch asserts its class on the device),
    so the test holds alone, in any order and in any selection; what this run's launches reached is printed, with the
    bit-equality of rows and single runs per class, and must lie inside the set."""
    plan = planned_classes()
    assert set(plan) == want_classes(), (sorted(set(plan) - want_classes()), sorted(want_classes() - set(plan)))
    for (MB, R, nt), Ms in plan.items():
        if MB:
            assert any(M % MB for M in Ms) and any(-(-M // MB) >= 3 for M in Ms) and max(Ms) >= 255, ((MB, R, nt), sorted(Ms))
            assert R == 4 or {M % MB for M in Ms} == set(range(MB)), ((MB, R, nt), sorted(Ms))     # every tail of 1 .. MB - 1 live rows
    assert IDS <= want_classes(), sorted(IDS - want_classes())
    print(f"\nclasses reached by this run <MB, R, NT>: {sorted(IDS)}")
    for kind, (worst, r, n) in sorted(STATS.items()):
        print(f"  {kind}: largest |got - ref| / bound {worst:.3f}, largest r_stage {r:.2e}, {n} elements")
    held = {}
    for (fmt, ids, epi, K, M), differ in EQ.items():
        h = held.setdefault((ids[0], ids[1]), [0, 0, set()])
        h[0] += 1
        h[1] += bool(differ)
        h[2].add(M)
    for (MB, R), (n, bad, Ms) in sorted(held.items()):
        print(f"  rows equal their 1-row launches, {kind_of((MB, R))}: {n - bad} of {n} (type, NT, epilogue, M) cases, M in {sorted(Ms)}")


# ------------------------------------------------------------------------------------------------------ decode attention
def attn_inputs(fmt, key, n_slots, dim, rows):
    k = ("attn", fmt, key, n_slots, rows)
    if k not in _IN:
        _IN.clear()
        sh = shape_of(key, n_slots)
        H, Hkv, hd = sh.n_head, sh.n_local_heads, sh.head_dim
        g = torch.Generator().manual_seed(4100 + H + Hkv + hd)
        r = lambda t: A.store(t.to(F64), fmt).to(F32)
        qkv = r(torch.randn(rows, (H + 2 * Hkv) * hd, generator=g))
        qkv[3] = r(qkv[3] * 8.0)
        qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.0 + 0.1 * torch.randn(hd, generator=g))
        kc = A.wbits(torch.randn(rows, Hkv, n_slots, hd, generator=g), fmt)
        vc = A.wbits(torch.randn(rows, Hkv, n_slots, hd, generator=g), fmt)
        wo, bo = r(0.03 * torch.randn(dim, H * hd, generator=g)), r(0.1 * torch.randn(dim, generator=g))
        resid = r(torch.randn(rows, dim, generator=g))
        _IN[k] = (qkv, qn, kn, kc, vc, wo, bo, resid, O.rope_table(n_slots, hd, sh.rope_base).to(F32), (H, Hkv, hd))
    return _IN[k]


def call_attn(fmt, eng, inp, rows, pos, with_bo):
    qkv, qn, kn, kc0, vc0, wo, bo, resid, tab, _ = inp
    b = lambda t: A.wbits(t, fmt)
    kc, vc = kc0[rows].copy(), vc0[rows].copy()
    nan = np.float32(np.nan) if fmt == "f32" else A.SENT16
    for i, p in enumerate(pos):                          # NaN patterns from the appended row on: the kernel masks them by construction
        kc[i, :, p:] = nan
        vc[i, :, p:] = nan
    return (kc, vc) + eng.test_decode_attn(qkv[rows].numpy(), np.array(pos, dtype=np.int32), b(qn), b(kn), kc, vc, b(wo),
                                           b(bo) if with_bo else None, resid[rows].numpy())


def run_attn(fmt, key, eng, n_slots, pos, rows_total, with_bo=False, want_nsplit=None):
    """One ft_test_decode_attn call of len(pos) rows, judged whole: partials or y, x_out, the caches; then rows EQ_ROWS against
    their 1-row calls where those pick the same split count (always, where it is pinned)."""
    dim, eps = eng.args.dim, eng.args.norm_eps
    inp = attn_inputs(fmt, key, n_slots, dim, rows_total)
    qkv, qn, kn, _, _, wo, bo, resid, tab, (H, Hkv, hd) = inp
    M = len(pos)
    kc, vc, ns, y, po, pml, x_out, kc1, vc1 = call_attn(fmt, eng, inp, slice(0, M), pos, with_bo)
    what = f"{fmt} {key} M {M} nsplit {ns} lengths {sorted({p + 1 for p in pos})}"
    NSPLITS.add(ns)
    if want_nsplit is not None:
        assert ns == want_nsplit, what
    HD = H * hd
    assert sentinel(y[:, HD:]), "y written past its columns: " + what
    assert bool(np.isfinite(x_out).all()), what
    if ns == 1:
        if fmt == "f32":
            pr = A.decode_attn_ref(fmt, qkv[:M], pos, qn, kn, kc, vc, tab, H, Hkv, hd, 1, eps)
            yref, kref, vref, r_st = WR.Ref(pr.y[:, :, 0].reshape(M, -1), pr.y_err[:, :, 0].reshape(M, -1), None), pr.k, pr.v, pr.r_stage
        else:
            ar = WR.attn_ref(fmt, qkv[:M], pos, qn, kn, kc, vc, tab, H, Hkv, hd, eps, splits=1)
            yref, kref, vref, r_st = ar.y, ar.k, ar.v, ar.y.r_stage
        vy = A.check(y[:, :HD], yref.ref, yref.err, fmt)
        line = note("attn_decode_kernel (1 split, y), grid.z = M", vy.worst, r_st, vy.checked)
        assert vy.flagged == 0 and vy.checked == M * HD, f"{what}: y {vy.flagged} flagged, worst {vy.worst:.3f}, rows {vy.rows[:12]}, cols {vy.cols[:12]}"
        xr = A.gemv_ref(fmt, 0, A.EPI_RESID, torch.from_numpy(y[:, :HD].copy()), wo, bias=bo if with_bo else None, resid=resid[:M])
        wo_kind = "Wo after one split (gemv), M rows"
    else:
        assert sentinel(y), "y written although the partials carry the output: " + what
        pr = A.decode_attn_ref(fmt, qkv[:M], pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns, eps)
        kref, vref = pr.k, pr.v
        vp = A.check_parts(po, pml, pr)
        line = note("attn_decode_kernel (partials), grid.z = M", vp.worst, pr.r_stage, vp.checked)
        assert vp.checked == po.size + pml.size
        assert vp.flagged == 0, f"{what}: partials flagged at (row, head, split) {vp.where[:12]}, worst {vp.worst:.3f}"
        _, _, yr, er = A.merge_ref(po, pml, fmt)
        xr = A.gemv_ref(fmt, 0, A.EPI_RESID, yr, wo, bias=bo if with_bo else None, resid=resid[:M], dx_in=er)
        wo_kind = "gemv_attn_combine_kernel, grid.y = M"
    vx = A.check(x_out, xr.ref, xr.err, fmt)
    line2 = note(wo_kind, vx.worst, xr.r_stage, vx.checked)
    assert vx.flagged == 0 and vx.checked == M * dim, f"{what}: x_out {vx.flagged} flagged, worst {vx.worst:.3f}, rows {vx.rows[:12]}, cols {vx.cols[:12]}"
    vk, v_ok, same = A.check_cache(fmt, kc, vc, kc1, vc1, pos, kref, vref)
    assert vk.flagged == 0 and vk.checked == M * Hkv * hd, f"{what}: appended K rows {vk.rows[:12]}, worst {vk.worst:.3f}"
    assert v_ok, "the appended V rows are copies: " + what
    assert same, "a cache row other than the appended one changed: " + what
    compared = 0
    for m in EQ_ROWS(M):
        one = call_attn(fmt, eng, inp, slice(m, m + 1), [pos[m]], with_bo)
        if one[2] != ns:
            continue                                                       # another split count: another order of the sums
        compared += 1
        assert np.array_equal(one[6][0].view(np.uint32), x_out[m].view(np.uint32)), f"{what}: row {m} differs from its 1-row call"
        bits = lambda t: np.ascontiguousarray(t).view(np.uint8)            # (patterns: the rows behind pos hold NaN)
        assert np.array_equal(bits(one[7][0]), bits(kc1[m])) and np.array_equal(bits(one[8][0]), bits(vc1[m])), f"{what}: row {m}'s caches differ from its 1-row call"
    return f"{line}; {line2}; appended K worst {vk.worst:.3f}", compared


TINY_LENS = (1, 2, 31, 32, 33, 127)


@pytest.mark.parametrize("M", (5, 66, 256))
@pytest.mark.parametrize("split", (32, 1))
@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_decode_attention_tiny_geometry(fmt, split, M):
    """4/2 x 16 heads, 128 cache rows, 32 splits (FT_ATTN_NSPLIT) and unsplit; every launch mixes the context lengths 1, 2, 31,
    32, 33 and 127 over its rows: part_o / part_ml at m H nsplit hd for m up to 255, grid.z = M, the Wo launch's grid.y = M."""
    eng = engine(fmt, "tiny", 128, env=(("FT_ATTN_NSPLIT", "32"),) if split > 1 else ())
    pos = [TINY_LENS[(5 * m + m // 6) % 6] - 1 for m in range(M)]
    assert {p + 1 for p in pos} == set(TINY_LENS) or M < 6
    line, compared = run_attn(fmt, "tiny", eng, 128, pos, 256, with_bo=bool(M & 1), want_nsplit=split)
    assert compared == len(EQ_ROWS(M))                                     # the split count is pinned: every row is compared
    print(f"\n{fmt} tiny M {M} nsplit {split}: {line}")


@pytest.mark.parametrize("env", [(), (("FT_NO_XL", "1"),), (("FT_ATTN_NSPLIT", "8"),)], ids=["chip", "no_xl", "pinned8"])
@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_decode_attention_real_heads_nine_rows(fmt, env):
    """16/8 x 128 heads, 1024 cache rows, 9 rows of lengths 1, 129, 257, 400 and 1023.  The split count is what the context
    picks: fixed where ft_test_ar_attn_plan reports 32 (one kv head per XCD on this chip), else 8 up to 768 positions and 16
    beyond, as ft_ar_decode picks it for the longest context of the call.  Rows are compared with their 1-row calls where those
    pick the same count: all five with FT_ATTN_NSPLIT=8 (pinned on every chip) and where the chip pins 32."""
    eng = engine(fmt, "16/8x128", 1024, max_batch=9, env=env)
    plan_ns, _, slots = eng.attn_plan()
    assert slots == 1024
    lens = (1, 129, 257, 400, 1023)
    pos = [lens[(2 * m) % 5] - 1 for m in range(9)]
    pinned = env == (("FT_ATTN_NSPLIT", "8"),)
    want = 8 if pinned else 32 if plan_ns == 32 else 16
    if env:
        assert plan_ns == 8, plan_ns                                       # not XCD-local: 8 until a call's longest context passes 768
    line, compared = run_attn(fmt, "16/8x128", eng, 1024, pos, 9, with_bo=True, want_nsplit=want)
    assert compared == (5 if pinned or plan_ns == 32 else sum(pos[m] + 1 > 768 for m in EQ_ROWS(9))) and compared >= 1
    print(f"\n{fmt} 16/8x128 M 9 nsplit {want} ({compared} rows compared with their 1-row calls): {line}")


# ------------------------------------------------------------------------------------------------------ fast attention
def fast_inputs(fmt, key, rows):
    k = ("fast", fmt, key, rows)
    if k not in _IN:
        _IN.clear()
        s = shape_of(key)
        H, Hkv, hd, ncb = s.fast_n_head, s.fast_n_local_heads, s.fast_head_dim, s.num_codebooks
        g = torch.Generator().manual_seed(6100 + H + hd)
        r = lambda t: A.store(t.to(F64), fmt).to(F32)
        qkv = r(1.5 * torch.randn(rows, (H + 2 * Hkv) * hd, generator=g))
        qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.2 + 0.1 * torch.randn(hd, generator=g))
        kc, vc = A.wbits(torch.randn(rows, Hkv, ncb, hd, generator=g), fmt), A.wbits(torch.randn(rows, Hkv, ncb, hd, generator=g), fmt)
        _IN[k] = (qkv, qn, kn, kc, vc, O.rope_table(ncb, hd, s.rope_base).to(F32), (H, Hkv, hd, ncb))
    return _IN[k]


@pytest.mark.parametrize("key", ("tiny", "16/8x128", "fast128"))
@pytest.mark.parametrize("fmt", ("bf16", "fp16", "f32"))
def test_fast_attention_f32_rows(fmt, key):
    """fast_attn_kernel writing f32 rows (form 0) at M = 5 and 65, codebook positions 0, 1 and ncb - 1; head widths 16, 64, 128."""
    eng = engine(fmt, key, 400 if key != "tiny" else 128, max_batch=65)
    qkv, qn, kn, kc, vc, tab, (H, Hkv, hd, ncb) = fast_inputs(fmt, key, 65)
    b = lambda t: A.wbits(t, fmt)
    line = ""
    for M in (5, 65):
        for c in (0, 1, ncb - 1):
            norm = bool((M + c) & 1)
            what = f"{fmt} {key} f32 rows M {M} c {c} qk-norm {norm}"
            y, pad, tail, kc1, vc1 = eng.test_fast_attn(0, qkv[:M].numpy(), c, b(qn) if norm else None, b(kn) if norm else None, kc[:M], vc[:M])
            assert sentinel(pad) and sentinel(tail), "y written outside its rows and columns: " + what
            assert bool(np.isfinite(y).all()), what
            kin, vin = nan_from(kc[:M], vc[:M], c, fmt)
            ref = A.fast_attn_ref(fmt, qkv[:M], c, qn if norm else None, kn if norm else None, kin, vin, tab, H, Hkv, hd, eng.args.norm_eps)
            vy = A.check(y, ref.y.ref, ref.y.err, fmt)
            line = note(f"fast_attn_kernel (f32 rows, hd {hd})", vy.worst, None, vy.checked)
            assert vy.flagged == 0 and vy.checked == M * H * hd, f"{what}: y {vy.flagged} flagged, worst {vy.worst:.3f}, rows {vy.rows[:12]}, cols {vy.cols[:12]}"
            vk, v_ok, same = A.check_cache(fmt, kin, vin, kc1, vc1, [c] * M, ref.k, ref.v)
            assert vk.flagged == 0 and vk.checked == M * Hkv * hd and v_ok, f"{what}: appended K rows {vk.rows[:12]} worst {vk.worst:.3f}, V copies {v_ok}"
            assert same, "a cache row other than the appended one changed: " + what
    print(f"\n{fmt} {key}: {line}")


# ------------------------------------------------------------------------------------------------------ the seam, end to end
def product_engine(shape, fmt, max_batch, **wkw):
    """A context as the product creates it (the frame engine where it runs), on the seeded weights."""
    from fish_tts_amd.ar_engine import ARHipEngine
    eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                      precision=PREC[fmt], device=0, max_batch=max_batch, max_new_tokens=64)
    eng.load_state_dict({n: v.to(DT[fmt]) for n, v in cached_random_weights(shape, seed=0, **wkw).items()})
    return eng


def test_66_rows_equal_their_single_runs_and_meet_64_rows_at_the_seam():
    """bf16, the real widths at 2 + 2 layers, max_batch = 66, 66 prompts of 5..27 positions, top_p = 1e-6.  (a) All 66 slots
    prefilled, five lock-step frames of 66 rows: every utterance equals its own single-slot run bit for bit.  (b) From the same
    prefilled state one frame at 64 rows (the MFMA launches) and one at 66 (the multi-row launches): the vocabulary logits of
    slots 0, 31 and 63 agree within 0.02 x the row's logit range - the two paths differ in the order of their sums only."""
    drop_engines()
    shape = medium_shape(n_text=1009)
    B = 66
    kw = dict(temperature=0.7, top_p=1e-6, repetition_penalty=1.1)
    prompts = [make_prompt(shape, 5 + (7 * i) % 23, seed=500 + i, n_vq=i % 4).numpy() for i in range(B)]
    eng = product_engine(shape, "bf16", B, std=0.05)
    try:
        assert "MFMA launches" in eng.frame_path(), eng.frame_path()
        singles = [eng.generate(p, 6, **kw) for p in prompts]
        sp = eng._sampling(0.7, 1e-6, 1.1)
        fill = lambda: [eng.prefill(p, sp, slot=i) for i, p in enumerate(prompts)]
        logits = {}
        for rows in (64, 66):
            firsts = fill()
            eng.decode(1, [sp] * rows, poll=1)
            logits[rows] = {s: eng.debug_state(s)[0].copy() for s in (0, 31, 63)}
        worst, moved = 0.0, False
        for s in (0, 31, 63):
            a, b = logits[64][s], logits[66][s]
            assert bool(np.isfinite(a).all()) and bool(np.isfinite(b).all())
            rng = float(b.max() - b.min())
            d = float(np.abs(a - b).max())
            worst = max(worst, d / rng)
            print(f"\nslot {s}: logits at 64 rows and at 66 rows differ by at most {d:.4g}, {d / rng:.5f} of the range {rng:.4g}")
            assert d <= 0.02 * rng, (s, d, rng)
            moved = moved or d > 0.0
        assert moved, "64 rows and 66 rows gave the same logits in every slot: the 64-row frame did not run the MFMA launches"
        firsts = fill()
        frames, n = eng.decode(5, [sp] * B, poll=5)
        for i, p in enumerate(prompts):
            got = np.concatenate([p, firsts[i][:, None], frames[i, : n[i]].T], axis=1)
            assert np.array_equal(got[:, : singles[i].shape[1]], singles[i]), f"utterance {i} differs from its single-slot run"
        print(f"\n66 rows: every utterance equals its single run; the seam's largest distance {worst:.5f} of the logit range")
    finally:
        eng.close()


def test_nine_fp32_rows_equal_their_single_runs():
    """fp32 has no MFMA path: nine utterances in one lock-step decode run gemv_kernel with grid.y = 9 and equal their single
    runs bit for bit."""
    shape = tiny_shape()
    B = 9
    kw = dict(temperature=0.7, top_p=1e-6, repetition_penalty=1.1)
    prompts = [make_prompt(shape, 5 + (7 * i) % 23, seed=700 + i, n_vq=i % 4).numpy() for i in range(B)]
    eng = product_engine(shape, "f32", B)
    try:
        assert "MFMA launches" not in eng.frame_path(), eng.frame_path()
        singles = [eng.generate(p, 12, **kw) for p in prompts]
        sp = eng._sampling(0.7, 1e-6, 1.1)
        firsts = [eng.prefill(p, sp, slot=i) for i, p in enumerate(prompts)]
        frames, n = eng.decode(11, [sp] * B, poll=4)
        for i, p in enumerate(prompts):
            got = np.concatenate([p, firsts[i][:, None], frames[i, : n[i]].T], axis=1)
            assert np.array_equal(got[:, : singles[i].shape[1]], singles[i]), f"utterance {i} differs from its single-slot run"
    finally:
        eng.close()


def test_print_the_figures():
    """Last in file order: the largest ratio and r_stage per kernel kind, the product classes and the split counts reached by
    the tests of this run (what DESIGN.md section 2 records)."""
    print(f"\nproduct classes <MB, R, NT>: {sorted(IDS)}; split counts: {sorted(NSPLITS)}")
    for kind, (worst, r, n) in sorted(STATS.items()):
        print(f"  {kind}: largest |got - ref| / bound {worst:.3f}, largest r_stage {r:.2e}, {n} elements")
        assert worst <= 1.0, kind
