"""GPU: the decode launches of 1..4 rows (5..256 rows: tests/test_ar_rows_gpu.py) (csrc/ar_kernels.h: gemv_kernel, gemv_mb_kernel, attn_decode_kernel with its f32
output and its split partials, gemv_attn_combine_kernel, fast_attn_kernel, embed_kernel) called ONE LAUNCH AT A TIME through
the product's own host dispatchers (ft_test_gemv, ft_test_decode_attn, ft_test_fast_attn, ft_test_embed) on seeded inputs,
every element of every written row against the float64 restatement of tests/ar_ref.py:

    |got - ref| <= half a ulp of the stored format at max(|got|, |ref|) + err

with err derived there.  Every sentinel and NaN region must be intact, every cache row but the appended one bit-unchanged,
every output finite.  tests/test_ar_ref_host.py proves the checker flags the subtle faults this is for.  No frame is traced:
the wiring between the launches stays the job of the oracle-following tests (test_ar_gpu.py).

Contexts are cheap: real widths with 1 + 1 layers and a small vocabulary, and tests/shapes.py's tiny shapes.  The product
hook takes its sizes from the call, so the tiny contexts serve every product and embedding case."""
import os

import numpy as np
import pytest
import torch

from oracle import ar as O
from tests import ar_ref as A
from tests import wide_ref as WR
from tests.codec_stage_ref import F32, F64
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import tiny_shape, tiny_shape_b
from tests.test_ar_gpu import medium_shape
from tests.test_ar_ref_host import embed_case

pytestmark = pytest.mark.gpu

PREC = {"bf16": "bf16", "fp16": "fp16", "f32": "fp32"}
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
K16 = (8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 3072, 3080, 4096, 4104, 6144)      # pairs: the two sides of an NT step
K32 = (8, 248, 256, 264, 1024, 1032, 3072)
CTX_LENS = (1, 2, 31, 32, 33, 127, 128, 129, 257, 400)
GEOS = {"16/8x128": (16, 8, 128), "8/8x128": (8, 8, 128), "16/4x128": (16, 4, 128), "16/2x128": (16, 2, 128), "16/8x64": (16, 8, 64)}
_ENG, _IN = {}, {}
STATS, IDS, NSPLITS = {}, set(), set()


def shape_of(key, n_slots=400):
    """key: "tiny", "tiny_b", a GEOS name (slow-stack heads at the real widths) or "fast128" (fast heads 8/4 x 128)."""
    if key == "tiny":
        return tiny_shape()
    if key == "tiny_b":
        return tiny_shape_b()
    kw = dict(n_text=17, n_layer=1, n_fast_layer=1, max_seq_len=n_slots)
    if key == "fast128":
        kw.update(fast_n_head=8, fast_n_local_heads=4, fast_head_dim=128)
    else:
        H, Hkv, hd = GEOS[key]
        kw.update(n_head=H, n_local_heads=Hkv, head_dim=hd)
    return medium_shape(**kw)


def engine(fmt, key="tiny", n_slots=400, max_batch=4, env=()):
    """A context shared by the tests of this module, created without the frame engine (the hooks need none, and a cached
    context must not hold the device's one frame-engine seat).  env: ((name, value), ...) set while it is created."""
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


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENG.values():
        eng.close()
    _ENG.clear()
    _IN.clear()


def note(kind, worst, r_stage, n):
    s = STATS.setdefault(kind, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], worst), max(s[1], r_stage or 0.0), s[2] + n
    return f"{kind}: largest |got - ref| / bound {s[0]:.3f}, largest r_stage {s[1]:.2e}, {s[2]} elements so far"


def sentinel(a):
    return bool((np.asarray(a).view(np.uint32) == A.SENT32).all())


# ------------------------------------------------------------------------------------------------------ products
def gemv_case(fmt, K, Nmax, seed=0):
    """Inputs of 4 rows x Nmax weight rows and their two float64 contractions (with and without the fused norm), computed
    once: a launch of M rows and N weight rows reads the prefixes, whose sums are the prefixes of these."""
    key = ("gemv", fmt, K, Nmax)
    if key not in _IN:
        _IN.clear()                                                        # one case's operands at a time
        x, W, gain, bias, resid = A.seeded_gemv_inputs(fmt, 4, Nmax, K, seed=2000 + K + Nmax + seed)
        _IN[key] = (x, W, gain, bias, resid, {1: A.gemv_pre(fmt, 1, x, W, gain), 0: None})
    return _IN[key]


def run_gemv(fmt, K, Nmax, pro, epi, M, N, with_bias, alias=False, nt=True, pad_x=0, pad_o=0):
    x, W, gain, bias, resid, pres = gemv_case(fmt, K, Nmax)
    if pres[pro] is None:
        pres[pro] = A.gemv_pre(fmt, pro, x, W, gain)
    acc, E, r, _ = pres[pro]
    b = lambda t: A.wbits(t, fmt)
    oc = N // 2 if epi == A.EPI_SWIGLU else N
    ldo = oc + (-oc) % 4 + pad_o
    out, pad, tail, ids = engine(fmt).test_gemv(pro, epi, x[:M].numpy(), b(W[:N]), b(gain) if pro else None, b(bias[:N]) if with_bias else None,
                                                resid[:M, :N].numpy() if epi == A.EPI_RESID else None, alias=alias, nt=nt, ldx=K + pad_x, ldo=ldo)
    what = f"{fmt} pro {pro} epi {epi} M {M} N {N} K {K} bias {with_bias} alias {alias} ldx +{pad_x} ldo {ldo} <MB, R, NT> {ids}"
    IDS.add(ids)
    assert ids == A.want_id(fmt, epi, M, N, K), what
    assert sentinel(pad) and sentinel(tail), "written outside the rows and columns of the product: " + what
    assert bool(np.isfinite(out).all()), what
    ref = A.gemv_ref(fmt, pro, epi, bias=bias[:N] if with_bias else None, resid=resid[:M, :N] if epi == A.EPI_RESID else None,
                     pre=(acc[:M, :N], E[:M, :N], r, None))
    ver = A.check(out, ref.ref, ref.err, fmt)
    line = note("gemv_mb_kernel" if ids[0] else "gemv_kernel", ver.worst, r, ver.checked)
    assert ver.flagged == 0 and ver.checked == M * oc, f"{what}: {ver.flagged} flagged, worst {ver.worst:.3f}, rows {ver.rows[:12]}, cols {ver.cols[:12]}"
    return line


def n_values(M):
    t = -(-2048 // M)                                                       # the smallest N with N M >= 2048: R = 2 from here
    return (1, 3, 4, 5, 1024, 2047, t - 1, t, 2048)


@pytest.mark.parametrize("fmt,K", [(f, K) for f in ("bf16", "fp16") for K in K16] + [("f32", K) for K in K32])
def test_products_both_sides_of_every_nt_step(fmt, K):
    """Every M in 1..4 at N = 1, 3, 4, 5 (one partial workgroup), 1024, 2047 (a partial last workgroup of R = 1 or 2) and both
    sides of the R = 1 | 2 threshold; the fused norm with the store and the SwiGLU epilogue (N = 2, 6, 14: odd N / 2), no norm
    with the residual epilogue aliased and not; with and without bias, ldx > K, ldo past the columns, both load policies."""
    line, i = "", 0
    for M in (1, 2, 3, 4):
        for N in n_values(M):
            i += 1
            line = run_gemv(fmt, K, 2048, 1, A.EPI_STORE, M, N, with_bias=bool(i & 1), nt=bool(i & 2), pad_x=8 * (i % 3 == 0), pad_o=4 * (i % 2))
            line = run_gemv(fmt, K, 2048, 0, A.EPI_RESID, M, N, with_bias=not (i & 1), alias=bool(i & 2), nt=bool(i & 4), pad_x=4 * (i % 5 == 0))
        for N in (2, 6, 14):
            line = run_gemv(fmt, K, 2048, 1, A.EPI_SWIGLU, M, N, with_bias=False, nt=bool(M & 1))
        line = run_gemv(fmt, K, 2048, 0, A.EPI_STORE, M, 5, with_bias=True)
    print(f"\n{fmt} K {K}: {line}; classes so far {sorted(IDS)}")


@pytest.mark.parametrize("fmt,K", [("bf16", 1024), ("bf16", 1032), ("fp16", 1024), ("f32", 1024)])
def test_swiglu_at_the_ffn_width(fmt, K):
    line = ""
    for M in (1, 2, 3, 4):
        line = run_gemv(fmt, K, 6144, 1, A.EPI_SWIGLU, M, 6144, with_bias=False)
    print(f"\n{fmt} K {K} SwiGLU N 6144: {line}")


# four weight rows per wave: N M >= 65536.  (fmt, M, N, K); N x K <= 2^25 but for <NT 12, R 4>, which no smaller product reaches
R4_CASES = [("bf16", 4, 16384, 512), ("bf16", 4, 16384, 1024), ("bf16", 4, 16384, 1536), ("fp16", 4, 16384, 2048), ("bf16", 1, 65540, 8),
            ("bf16", 1, 65540, 504), ("fp16", 1, 65540, 512), ("f32", 4, 16384, 512), ("f32", 4, 16384, 768), ("f32", 4, 16384, 1536),
            ("f32", 4, 16384, 2048), ("f32", 4, 16384, 2056), ("f32", 1, 65540, 256)]


@pytest.mark.parametrize("fmt,M,N,K", R4_CASES)
def test_products_four_rows_per_wave(fmt, M, N, K):
    line = run_gemv(fmt, K, N, 1, A.EPI_STORE, M, N, with_bias=True, pad_x=8)
    line = run_gemv(fmt, K, N, 0, A.EPI_RESID, M, N, with_bias=False, alias=True)
    if M == 4:
        run_gemv(fmt, K, N, 0, A.EPI_RESID, 3, N, with_bias=False, alias=False)      # 3 x 16384 < 65536: R = 2 on the same weights
    assert A.want_id(fmt, A.EPI_STORE, M, N, K)[1] == 4
    print(f"\n{fmt} M {M} N {N} K {K}: {line}")


def test_every_product_class_is_reached():
    """The classes the tests above reached are exactly those the dispatcher can pick: gemv_kernel<NT, R> for every NT and
    R in 1, 2, 4; gemv_mb_kernel<R, MB> for (1, 2) (1, 4) (2, 2) (2, 4) (4, 2) at the NT the register rule allows.  (The R >= 8
    branch of gemv has no caller that passes 8.)  Runs after them in file order; on its own it reaches them with zeros."""
    if not IDS:
        for fmt, Ks in (("bf16", K16), ("f32", K32)):
            z = lambda *s: np.zeros(s, dtype=np.float32 if fmt == "f32" else np.uint16)
            for K in Ks:
                for M, N in ((1, 4), (1, 2048), (2, 4), (2, 1024), (3, 4), (3, 1024)):
                    IDS.add(engine(fmt).test_gemv(0, 0, np.zeros((M, K), np.float32), z(N, K))[3])
        for fmt, M, N, K in R4_CASES:
            z = lambda *s: np.zeros(s, dtype=np.float32 if fmt == "f32" else np.uint16)
            IDS.add(engine(fmt).test_gemv(0, 0, np.zeros((M, K), np.float32), z(N, K))[3])
    plain = {(0, R, nt) for R in (1, 2, 4) for nt in A.NT_OPTS}
    mb = {(MB, R, nt) for (R, MB) in ((1, 2), (1, 4), (2, 2), (2, 4)) for nt in ((1, 2, 4, 6) if MB == 2 else (1, 2))} | {(2, 4, 1), (2, 4, 2)}
    print(f"\nclasses reached <MB, R, NT>: {sorted(IDS)}")
    for kind, (worst, r, n) in sorted(STATS.items()):
        print(f"  {kind}: largest |got - ref| / bound {worst:.3f}, largest r_stage {r:.2e}, {n} elements")
    assert IDS == plain | mb, (sorted(IDS - plain - mb), sorted((plain | mb) - IDS))


# ------------------------------------------------------------------------------------------------------ decode attention
def attn_inputs(fmt, key, n_slots, dim):
    k = ("attn", fmt, key, n_slots)
    if k not in _IN:
        _IN.clear()
        sh = shape_of(key)
        H, Hkv, hd = sh.n_head, sh.n_local_heads, sh.head_dim
        g = torch.Generator().manual_seed(4000 + H + Hkv + hd)
        r = lambda t: A.store(t.to(F64), fmt).to(F32)
        qkv = r(torch.randn(4, (H + 2 * Hkv) * hd, generator=g))
        qkv[3] = r(qkv[3] * 8.0)
        qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.0 + 0.1 * torch.randn(hd, generator=g))
        kc = A.wbits(torch.randn(4, Hkv, n_slots, hd, generator=g), fmt)
        vc = A.wbits(torch.randn(4, Hkv, n_slots, hd, generator=g), fmt)
        wo, bo = r(0.03 * torch.randn(dim, H * hd, generator=g)), r(0.1 * torch.randn(dim, generator=g))
        resid = r(torch.randn(4, dim, generator=g))
        _IN[k] = (qkv, qn, kn, kc, vc, wo, bo, resid, O.rope_table(n_slots, hd, sh.rope_base).to(F32), (H, Hkv, hd))
    return _IN[k]


def run_attn(fmt, key, eng, n_slots, dev_pos, pos_off=0, qk_norm=True, with_bo=False, want_nsplit=None):
    """One ft_test_decode_attn call of len(dev_pos) rows, judged whole: partials or y, x_out, the caches."""
    dim, eps = eng.args.dim, eng.args.norm_eps
    qkv, qn, kn, kc0, vc0, wo, bo, resid, tab, (H, Hkv, hd) = attn_inputs(fmt, key, n_slots, dim)
    M = len(dev_pos)
    pos = [p + pos_off for p in dev_pos]
    b = lambda t: A.wbits(t, fmt)
    kc, vc = kc0[:M].copy(), vc0[:M].copy()
    nan = np.float32(np.nan) if fmt == "f32" else A.SENT16
    for m in range(M):                                   # NaN patterns from the appended row on: the kernel masks them by construction
        kc[m, :, pos[m]:] = nan
        vc[m, :, pos[m]:] = nan
    ns, y, po, pml, x_out, kc1, vc1 = eng.test_decode_attn(qkv[:M].numpy(), np.array(dev_pos, dtype=np.int32), b(qn) if qk_norm else None,
                                                           b(kn) if qk_norm else None, kc, vc, b(wo), b(bo) if with_bo else None,
                                                           resid[:M].numpy(), pos_off=pos_off)
    what = f"{fmt} {key} M {M} pos {pos} nsplit {ns}"
    NSPLITS.add(ns)
    if want_nsplit is not None:
        assert ns == want_nsplit, what
    qn_, kn_ = (qn, kn) if qk_norm else (None, None)
    HD = H * hd
    assert sentinel(y[:, HD:]), "y written past its columns: " + what
    assert bool(np.isfinite(x_out).all()), what
    if ns == 1:
        if fmt == "f32":
            pr = A.decode_attn_ref(fmt, qkv[:M], pos, qn_, kn_, kc, vc, tab, H, Hkv, hd, 1, eps)
            yref, kref, vref, r_st = WR.Ref(pr.y[:, :, 0].reshape(M, -1), pr.y_err[:, :, 0].reshape(M, -1), None), pr.k, pr.v, pr.r_stage
        else:
            ar = WR.attn_ref(fmt, qkv[:M], pos, qn_, kn_, kc, vc, tab, H, Hkv, hd, eps, splits=1)
            yref, kref, vref, r_st = ar.y, ar.k, ar.v, ar.y.r_stage
        vy = A.check(y[:, :HD], yref.ref, yref.err, fmt)
        line = note("attn_decode_kernel (1 split, y)", vy.worst, r_st, vy.checked)
        assert vy.flagged == 0 and vy.checked == M * HD, f"{what}: y {vy.flagged} flagged, worst {vy.worst:.3f}, rows {vy.rows}, cols {vy.cols[:12]}"
        xr = A.gemv_ref(fmt, 0, A.EPI_RESID, torch.from_numpy(y[:, :HD].copy()), wo, bias=bo if with_bo else None, resid=resid[:M])
        wo_kind = "Wo after one split (gemv)"
    else:
        assert sentinel(y), "y written although the partials carry the output: " + what
        pr = A.decode_attn_ref(fmt, qkv[:M], pos, qn_, kn_, kc, vc, tab, H, Hkv, hd, ns, eps)
        kref, vref = pr.k, pr.v
        vp = A.check_parts(po, pml, pr)
        line = note(f"attn_decode_kernel (partials)", vp.worst, pr.r_stage, vp.checked)
        assert vp.flagged == 0, f"{what}: partials flagged at (row, head, split) {vp.where[:12]}, worst {vp.worst:.3f}"
        _, _, yr, er = A.merge_ref(po, pml, fmt)
        xr = A.gemv_ref(fmt, 0, A.EPI_RESID, yr, wo, bias=bo if with_bo else None, resid=resid[:M], dx_in=er)
        wo_kind = "gemv_attn_combine_kernel"
    vx = A.check(x_out, xr.ref, xr.err, fmt)
    line2 = note(wo_kind, vx.worst, xr.r_stage, vx.checked)
    assert vx.flagged == 0 and vx.checked == M * dim, f"{what}: x_out {vx.flagged} flagged, worst {vx.worst:.3f}, rows {vx.rows}, cols {vx.cols[:12]}"
    vk, v_ok, same = A.check_cache(fmt, kc, vc, kc1, vc1, pos, kref, vref)
    assert vk.flagged == 0 and vk.checked == M * Hkv * hd, f"{what}: appended K rows {vk.rows}, worst {vk.worst:.3f}"
    assert v_ok, "the appended V rows are copies: " + what
    assert same, "a cache row other than the appended one changed: " + what
    return f"{line}; {line2}; appended K worst {vk.worst:.3f}"


def mixed_positions(M, i):
    return [CTX_LENS[(3 * m + i) % len(CTX_LENS)] - 1 for m in range(M)]


@pytest.mark.parametrize("key", ["tiny", "tiny_b"] + list(GEOS))
@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_decode_attention_every_geometry(fmt, key):
    """A context of 400 slots: one split (32 where the real 16/8 x 128 shape pins them on this chip - asserted as returned).
    M in 1, 3, 4; every launch mixes context lengths; pos_off 0 and 5; qk-norm on and off; with and without the Wo bias."""
    slots = {"tiny": 128, "tiny_b": 96}.get(key, 400)                       # (a tiny shape's cache: lengths above it end in its last slot)
    eng = engine(fmt, key, slots)
    line, i = "", 0
    for M in (1, 3, 4):
        for pos_off in (0, 5):
            for lens_i in range(0, 10, 3 if M > 1 else 1):
                i += 1
                dev = [max(0, min(p, slots - 1) - pos_off) for p in mixed_positions(M, lens_i)]
                line = run_attn(fmt, key, eng, slots, dev, pos_off, qk_norm=bool(i % 4), with_bo=bool(i & 1))
    print(f"\n{fmt} {key}: {line}; split counts so far {sorted(NSPLITS)}")


@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_decode_attention_split_counts(fmt):
    """8 splits from a 1024-slot context, 8 / 16 / 32 from a 4096-slot one as the longest context of the call grows (the
    choice ft_ar_decode makes), 32 from FT_ATTN_NSPLIT and whatever the real shape picks here."""
    noxl = (("FT_NO_XL", "1"),)
    e1, e4 = engine(fmt, "16/8x128", 1024, env=noxl), engine(fmt, "16/8x128", 4096, env=noxl)
    line = ""
    for M in (1, 3, 4):
        line = run_attn(fmt, "16/8x128", e1, 1024, mixed_positions(M, M), want_nsplit=8)
    for M in (1, 3, 4):
        line = run_attn(fmt, "16/8x128", e4, 4096, mixed_positions(M, M + 1), want_nsplit=8)
    line = run_attn(fmt, "16/8x128", e4, 4096, [1000, 5, 769], want_nsplit=16)
    line = run_attn(fmt, "16/8x128", e4, 4096, [3100, 0, 31, 3095], pos_off=5, want_nsplit=32)
    e32 = engine(fmt, "16/4x128", env=(("FT_ATTN_NSPLIT", "32"),))
    for M in (1, 3, 4):
        for pos_off in (0, 5):
            line = run_attn(fmt, "16/4x128", e32, 400, [max(0, p - pos_off) for p in mixed_positions(M, M + pos_off)], pos_off, want_nsplit=32)
    t32 = engine(fmt, "tiny", 128, env=(("FT_ATTN_NSPLIT", "32"),))
    line = run_attn(fmt, "tiny", t32, 128, [0, 1, 31, 127], want_nsplit=32)
    run_attn(fmt, "16/8x128", engine(fmt, "16/8x128"), 400, mixed_positions(4, 2))        # whatever the real shape picks on this chip
    print(f"\n{fmt}: {line}; split counts reached {sorted(NSPLITS)}")
    assert {8, 16, 32} <= NSPLITS


def test_decode_attention_long_contexts():
    """bf16 at the 16/8 x 128 geometry, at the lengths where tests/test_engine_long_context_gpu.py holds the frame engine to
    these launches bit for bit: a context of 8192 slots with pos 6143, 6144 and 8191 (32 splits of up to 256 positions, the
    last row of the cache), and pos 1535, 1536 of a 4096-slot context at 16 splits (96 | 97 positions per split).  Bounds as
    everywhere in this file."""
    noxl = (("FT_NO_XL", "1"),)
    e4 = engine("bf16", "16/8x128", 4096, env=noxl)
    line16 = run_attn("bf16", "16/8x128", e4, 4096, [1535, 1536], want_nsplit=16)
    run_attn("bf16", "16/8x128", e4, 4096, [1535], want_nsplit=16)
    e8 = engine("bf16", "16/8x128", 8192, env=noxl)
    line32 = run_attn("bf16", "16/8x128", e8, 8192, [6143, 6144, 8191], want_nsplit=32)
    run_attn("bf16", "16/8x128", e8, 8192, [8186], pos_off=5, want_nsplit=32, qk_norm=False, with_bo=True)
    print(f"\n16 splits: {line16}\n32 splits: {line32}")


# ------------------------------------------------------------------------------------------------------ fast attention
def fast_inputs(fmt, key, rows):
    k = ("fast", fmt, key)
    if k not in _IN:
        _IN.clear()
        s = shape_of(key)
        H, Hkv, hd, ncb = s.fast_n_head, s.fast_n_local_heads, s.fast_head_dim, s.num_codebooks
        g = torch.Generator().manual_seed(6000 + H + hd)
        r = lambda t: A.store(t.to(F64), fmt).to(F32)
        qkv = r(1.5 * torch.randn(128, (H + 2 * Hkv) * hd, generator=g))
        qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.2 + 0.1 * torch.randn(hd, generator=g))
        kc, vc = A.wbits(torch.randn(64, Hkv, ncb, hd, generator=g), fmt), A.wbits(torch.randn(64, Hkv, ncb, hd, generator=g), fmt)
        _IN[k] = (qkv, qn, kn, kc, vc, O.rope_table(ncb, hd, s.rope_base).to(F32), (H, Hkv, hd, ncb))
    return _IN[k]


def check_fast(fmt, what, kind, y, ref, kc_in, vc_in, kc1, vc1, c, M):
    vy = A.check(y, ref.y.ref, ref.y.err, fmt)
    line = note(kind, vy.worst, None, vy.checked)
    assert vy.flagged == 0 and vy.checked == ref.y.ref.numel(), f"{what}: y {vy.flagged} flagged, worst {vy.worst:.3f}, rows {vy.rows[:12]}, cols {vy.cols[:12]}"
    vk, v_ok, same = A.check_cache(fmt, kc_in, vc_in, kc1, vc1, [c] * M, ref.k, ref.v)
    assert vk.flagged == 0 and v_ok, f"{what}: appended K rows {vk.rows[:12]} worst {vk.worst:.3f}, V copies {v_ok}"
    assert same, "a cache row other than the appended one changed: " + what
    return line


def nan_from(kc, vc, first, fmt):
    kc, vc = kc.copy(), vc.copy()
    if fmt == "f32":
        kc[:, :, first:].view(np.uint32)[...] = 0xFFFFFFFF
        vc[:, :, first:].view(np.uint32)[...] = 0xFFFFFFFF
    else:
        kc[:, :, first:], vc[:, :, first:] = 0xFFFF, 0xFFFF
    return kc, vc


@pytest.mark.parametrize("fmt,key", [("bf16", "tiny"), ("f32", "tiny"), ("bf16", "tiny_b"), ("bf16", "16/8x128"), ("f32", "16/8x128"), ("fp16", "16/8x128"),
                                     ("bf16", "fast128"), ("f32", "fast128")])
def test_fast_attention_single(fmt, key):
    """M in 1, 2, 4 with the f32 y; c in 0, 1, 2, ncb - 1; qk-norm on and off; head widths 16, 64 and 128."""
    eng = engine(fmt, key)
    qkv, qn, kn, kc, vc, tab, (H, Hkv, hd, ncb) = fast_inputs(fmt, key, 4)
    b = lambda t: A.wbits(t, fmt)
    line = ""
    for M in (1, 2, 4):
        for c in (0, 1, 2, ncb - 1):
            for norm in (True, False):
                what = f"{fmt} {key} single M {M} c {c} qk-norm {norm}"
                y, pad, tail, kc1, vc1 = eng.test_fast_attn(0, qkv[:M].numpy(), c, b(qn) if norm else None, b(kn) if norm else None, kc[:M], vc[:M])
                assert sentinel(pad) and sentinel(tail), "y written outside its rows and columns: " + what
                assert bool(np.isfinite(y).all()), what
                kin, vin = nan_from(kc[:M], vc[:M], c, fmt)
                ref = A.fast_attn_ref(fmt, qkv[:M], c, qn if norm else None, kn if norm else None, kin, vin, tab, H, Hkv, hd, eng.args.norm_eps)
                line = check_fast(fmt, what, f"fast_attn_kernel (single, hd {hd})", y, ref, kin, vin, kc1, vc1, c, M)
    print(f"\n{fmt} {key}: {line}")


@pytest.mark.parametrize("fmt,key", [("bf16", "16/8x128"), ("fp16", "16/8x128"), ("bf16", "fast128")])
def test_fast_attention_wide_and_paired(fmt, key):
    """The 16-bit octet-major output of a lock-step batch: single M in 5, 16, 17, 64; paired M in 5, 16, 64, where the
    position-1 block rebuilds cache row 0 from the position-0 row: position 1 is recomputed from row 0 AS RETURNED and must
    pass; recomputed from the reference's row 0 it must pass too unless the returned row differs from the reference's
    (a boundary flip inside the key's bound, which then shows in both blocks or in neither)."""
    eng = engine(fmt, key, max_batch=64)
    qkv, qn, kn, kc, vc, tab, (H, Hkv, hd, ncb) = fast_inputs(fmt, key, 128)
    b = lambda t: A.wbits(t, fmt)
    HD, line = H * hd, ""
    for norm in (True, False):
        q_, k_ = (qn, kn) if norm else (None, None)
        for M in (5, 16, 17, 64):
            for c in (0, 1, 2, ncb - 1):
                what = f"{fmt} {key} wide M {M} c {c} qk-norm {norm}"
                yb, kc1, vc1 = eng.test_fast_attn(1, qkv[:M].numpy(), c, None if q_ is None else b(q_), None if k_ is None else b(k_), kc[:M], vc[:M])
                assert bool((yb[:, M:, :] == A.SENT16).all()), "rows past M written: " + what
                kin, vin = nan_from(kc[:M], vc[:M], c, fmt)
                ref = A.fast_attn_ref(fmt, qkv[:M], c, q_, k_, kin, vin, tab, H, Hkv, hd)
                line = check_fast(fmt, what, f"fast_attn_kernel (wide, hd {hd})", A.xo_rows(yb, M, HD), ref, kin, vin, kc1, vc1, c, M)
        for M in (5, 16, 64):
            what = f"{fmt} {key} paired M {M} qk-norm {norm}"
            q2 = torch.cat([qkv[:M], qkv[64:64 + M]])
            yb, kc1, vc1 = eng.test_fast_attn(2, q2.numpy(), 0, None if q_ is None else b(q_), None if k_ is None else b(k_), kc[:M], vc[:M])
            xp = yb.shape[1] // 2
            keep = np.ones(yb.shape[1], dtype=bool)
            keep[:M] = keep[xp:xp + M] = False
            assert bool((yb[:, keep, :] == A.SENT16).all()), "rows of no utterance written: " + what
            kin, vin = nan_from(kc[:M], vc[:M], 0, fmt)
            r0 = A.fast_attn_ref(fmt, q2[:M], 0, q_, k_, kin, vin, tab, H, Hkv, hd)
            # position 0: y rows [0, M), cache row 0 appended
            vy0 = A.check(A.xo_rows(yb, M, HD), r0.y.ref, r0.y.err, fmt)
            vk0 = A.check(kc1[:, :, 0], r0.k.ref, r0.k.err, fmt)
            assert vy0.flagged == 0 and vk0.flagged == 0, f"{what}: position 0 rows {vy0.rows[:12]}, key rows {vk0.rows[:12]}"
            assert np.array_equal(vc1[:, :, 0], b(r0.v)), what
            # position 1: from row 0 as returned (rows 1.. of the cache must come back as they went in, but for row 1)
            y1 = A.xo_rows(yb[:, xp:, :], M, HD)
            k_ret, v_ret = kin.copy(), vin.copy()
            k_ret[:, :, 0], v_ret[:, :, 0] = kc1[:, :, 0], vc1[:, :, 0]
            r1 = A.fast_attn_ref(fmt, q2[M:], 1, q_, k_, k_ret, v_ret, tab, H, Hkv, hd)
            line = check_fast(fmt, what, f"fast_attn_kernel (paired, hd {hd})", y1, r1, k_ret, v_ret, kc1, vc1, 1, M)
            k_ref = kin.copy()
            k_ref[:, :, 0] = b(r0.k.rnd)
            flips = int((k_ref[:, :, 0] != kc1[:, :, 0]).sum())
            if flips == 0:
                continue                                                   # both recomputations are the same one
            r1b = A.fast_attn_ref(fmt, q2[M:], 1, q_, k_, k_ref, v_ret, tab, H, Hkv, hd)
            v1b = A.check(y1, r1b.y.ref, r1b.y.err, fmt)
            print(f"{what}: {flips} boundary flips in cache row 0; position 1 against the reference's row 0: {v1b.flagged} flagged")
    print(f"\n{fmt} {key}: {line}")


# ------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("D", (8, 248, 256, 264, 1024))
@pytest.mark.parametrize("fmt", ("bf16", "fp16", "f32"))
def test_embedding(fmt, D):
    """ncb 1, 10, 16; M 1, 4, 33; tokens on both sides of the semantic range, -1 and vocab; codes -1 and cbsize; scale on and
    off; with and without the octet-major copy (xo_ldm 32 and 128), which must equal the f32 value's pattern exactly."""
    eng = engine(fmt)
    line = ""
    for ncb in (1, 10, 16):
        for M in (1, 4, 33):
            emb, cbe, toks, cbsize, sb, se = embed_case(fmt, D, ncb, M)
            for scale in (True, False):
                for xo_ldm in ((0,) if fmt == "f32" else (0, 32, 128) if M <= 32 else (0, 128)):
                    what = f"{fmt} D {D} ncb {ncb} M {M} scale {scale} xo_ldm {xo_ldm}"
                    # row-major tokens: codes follow their token; the strides are the hook's to take
                    x, pad, tail, xo = eng.test_embed(A.wbits(emb, fmt), A.wbits(cbe, fmt), toks, M, ncb, cbsize, sb, se, scale,
                                                      tok_row_stride=1, tok_m_stride=ncb + 1, ldx=D + 4 * (M & 1), xo_ldm=xo_ldm)
                    assert sentinel(pad) and sentinel(tail), "x written outside its rows and columns: " + what
                    assert bool(np.isfinite(x).all()), what
                    ref = A.embed_ref(fmt, emb, cbe, toks, ncb, cbsize, sb, se, scale)
                    ver = A.check(x, ref.ref, ref.err, fmt)
                    line = note("embed_kernel", ver.worst, None, ver.checked)
                    assert ver.flagged == 0 and ver.checked == M * D, f"{what}: {ver.flagged} flagged, worst {ver.worst:.3f}, rows {ver.rows[:12]}, cols {ver.cols[:12]}"
                    if xo_ldm:
                        assert np.array_equal(A.xo_rows(xo, M, D), A.wbits(torch.from_numpy(x), fmt)), "the 16-bit copy differs: " + what
                        assert bool((xo[:, M:, :] == A.SENT16).all()), "octet-major rows past M written: " + what
    print(f"\n{fmt} D {D}: {line}")


# ------------------------------------------------------------------------------------------------------ refusals
def test_what_the_hooks_refuse():
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import HipError

    def refused(code, fn, *a, **kw):
        with pytest.raises(HipError) as e:
            fn(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)

    bf, f32 = engine("bf16"), engine("f32")
    zf = lambda *s: np.zeros(s, dtype=np.float32)
    zu = lambda *s: np.zeros(s, dtype=np.uint16)
    refused(L.FT_ERR_ARG, bf.test_gemv, 0, 0, zf(1, 6152), zu(4, 6152))                       # pick_nt < 0
    refused(L.FT_ERR_ARG, f32.test_gemv, 0, 0, zf(1, 3080), zf(4, 3080))
    refused(L.FT_ERR_ARG, bf.test_gemv, 0, 0, zf(1, 12), zu(4, 12))                           # K no multiple of 8
    refused(L.FT_ERR_ARG, bf.test_gemv, 0, 0, zf(5, 8), zu(4, 8))                             # M outside 1..max_batch (4 here)
    assert bf.max_batch == 4 and engine("bf16", max_batch=64).test_gemv(0, 0, zf(64, 8), zu(4, 8))[3] == A.want_id("bf16", 0, 64, 4, 8)
    refused(L.FT_ERR_ARG, engine("bf16", max_batch=64).test_gemv, 0, 0, zf(65, 8), zu(4, 8))
    refused(L.FT_ERR_ARG, bf.test_gemv, 1, 0, zf(1, 8), zu(4, 8))                             # the norm without a gain
    refused(L.FT_ERR_ARG, bf.test_gemv, 0, 1, zf(1, 8), zu(4, 8))                             # the residual epilogue without one
    refused(L.FT_ERR_ARG, bf.test_gemv, 0, 2, zf(1, 8), zu(5, 8))                             # SwiGLU on an odd N
    refused(L.FT_ERR_ARG, bf.test_gemv, 0, 0, zf(1, 8), zu(4, 8), ldx=10)
    a = bf.args
    qkvN, n_slots = (a.n_head + 2 * a.n_local_heads) * a.head_dim, a.max_seq_len + (-a.max_seq_len) % 8
    cache = zu(1, a.n_local_heads, n_slots, a.head_dim)
    wo, res = zu(a.dim, a.n_head * a.head_dim), zf(1, a.dim)
    refused(L.FT_ERR_ARG, bf.test_decode_attn, zf(1, qkvN), [n_slots], None, None, cache, cache, wo, None, res)
    refused(L.FT_ERR_ARG, bf.test_decode_attn, zf(1, qkvN), [-1], None, None, cache, cache, wo, None, res)
    refused(L.FT_ERR_ARG, bf.test_decode_attn, zf(1, qkvN), [n_slots - 3], None, None, cache, cache, wo, None, res, pos_off=5)
    c5 = zu(5, a.n_local_heads, n_slots, a.head_dim)
    refused(L.FT_ERR_ARG, bf.test_decode_attn, zf(5, qkvN), [0] * 5, None, None, c5, c5, wo, None, zf(5, a.dim))
    fq = (a.fast_n_head + 2 * a.fast_n_local_heads) * a.fast_head_dim
    fc = lambda M: zu(M, a.fast_n_local_heads, a.num_codebooks, a.fast_head_dim)
    refused(L.FT_ERR_ARG, bf.test_fast_attn, 0, zf(5, fq), 0, None, None, fc(5), fc(5))       # the f32 y form takes 1..max_batch rows
    refused(L.FT_ERR_ARG, bf.test_fast_attn, 0, zf(1, fq), a.num_codebooks, None, None, fc(1), fc(1))
    refused(L.FT_ERR_STATE, bf.test_fast_attn, 1, zf(5, fq), 0, None, None, fc(5), fc(5))     # a tiny context has no lock-step MFMA path
    refused(L.FT_ERR_STATE, bf.test_fast_attn, 2, zf(10, fq), 0, None, None, fc(5), fc(5))
    f32fc = lambda M: zf(M, a.fast_n_local_heads, a.num_codebooks, a.fast_head_dim)
    refused(L.FT_ERR_ARG, f32.test_fast_attn, 1, zf(5, fq), 0, None, None, f32fc(5), f32fc(5))
    toks = np.zeros(3, dtype=np.int32)
    refused(L.FT_ERR_ARG, bf.test_embed, zu(4, 8), zu(2 * 3, 8), toks, 2, 2, 3, 1, 2, True, tok_row_stride=1, tok_m_stride=3)   # strides past toks
    refused(L.FT_ERR_ARG, bf.test_embed, zu(4, 8), zu(2 * 3, 8), toks, 1, 2, 3, 1, 2, True, tok_row_stride=1, tok_m_stride=3, ldx=4)
    refused(L.FT_ERR_ARG, f32.test_embed, zf(4, 8), zf(2 * 3, 8), toks, 1, 2, 3, 1, 2, True, tok_row_stride=1, tok_m_stride=3, xo_ldm=32)


def test_print_the_figures():
    """Last in file order: the largest ratio and r_stage per kernel kind, the product classes and the split counts reached by
    the tests of this run (what DESIGN.md section 2 records)."""
    print(f"\nproduct classes <MB, R, NT>: {sorted(IDS)}; split counts: {sorted(NSPLITS)}")
    for kind, (worst, r, n) in sorted(STATS.items()):
        print(f"  {kind}: largest |got - ref| / bound {worst:.3f}, largest r_stage {r:.2e}, {n} elements")
        assert worst <= 1.0, kind
