"""GPU: the lock-step batch kernels (csrc/wide_kernels.h: wide_gemm_kernel, wide_head_kernel; csrc/ar_kernels.h:
attn_wide_kernel, and the split fall-back attn_decode_kernel + attn_combine_rows_kernel) called ONE LAUNCH AT A TIME
through the product's own dispatchers (ft_test_wide_linear, ft_test_wide_attn) on seeded inputs, every element of every
written row against the float64 restatement of tests/wide_ref.py:

    |got - ref| <= half a ulp of the stored format at max(|got|, |ref|) + err

with err derived there.  Rows past M must still hold the sentinel, cache rows other than the appended one must be
bit-unchanged.  tests/test_wide_ref_host.py proves the checker flags the subtle faults this is for.  No frame is traced:
the wiring between the launches stays the job of the oracle-following tests (test_ar_gpu.py, test_wide_fp16_gpu.py).

A subset runs once more on a max_batch = 256 context, whose octet-major operands lie at xo_ldm = 512 (the contexts above have
32 and 128): the launches a 5..64-row batch runs on an engine sized for 256 rows, where the paired codebook pass never holds."""
import os

import numpy as np
import pytest
import torch

from oracle import ar as O
from tests import wide_ref as R
from tests.codec_stage_ref import F32, h16_bits
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import tiny_shape
from tests.test_ar_gpu import medium_shape

pytestmark = pytest.mark.gpu

FMTS = ("bf16", "fp16")
MS = (1, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)     # both sides of every 16-row tile, of M > 16 and of the head's M <= 32
HEAD_MS = (1, 5, 16, 17, 31, 32)
N_SLOTS = 400
CTX_LENS = (1, 2, 127, 128, 129, 255, 256, 257, 385, N_SLOTS)   # pos + 1: both sides of every 128-position chunk, the last slot
SENT16, SENT32 = 0xFFFE, 0xFFFFFFFE
_ENG, _PRE, _IN = {}, {}, {}
STATS = {}                                                  # kernel kind -> [worst ratio, largest r_stage, elements]
IDS = set()


def ctx_shape(H=16, Hkv=8):
    """s1-mini widths at one slow layer and the smallest vocabulary the MFMA launches take (a multiple of 32 above the
    semantic range); 400 cache slots, so a context can end in the last one."""
    return medium_shape(n_text=17, n_layer=1, n_head=H, n_local_heads=Hkv, max_seq_len=N_SLOTS)


def engine(fmt, H=16, Hkv=8, max_batch=64, env=None):
    """A context shared by the tests of this module.  Created with FT_NO_ENGINE: the hooks need no frame engine, and a
    cached context must not hold the device's one frame-engine seat against the tests that run after this module."""
    key = (fmt, H, Hkv, max_batch, env)
    if key not in _ENG or not _ENG[key]._h:                 # (a failed test's engines are closed by tests/conftest.py)
        from fish_tts_amd.ar_engine import ARHipEngine
        shape = ctx_shape(H, Hkv)
        saved = {n: os.environ.get(n) for n in ("FT_NO_ENGINE", env) if n}
        os.environ.update({n: "1" for n in saved})
        try:
            eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                              precision=fmt, device=0, max_batch=max_batch, max_new_tokens=8)
            eng.load_state_dict({k: v.to(R.FMT_DT[fmt]) for k, v in cached_random_weights(shape, seed=0).items()})
        finally:
            for n, v in saved.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
        assert "MFMA launches" in eng.frame_path(), eng.frame_path()
        _ENG[key] = eng
    return _ENG[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENG.values():
        eng.close()
    _ENG.clear()
    _PRE.clear()
    _IN.clear()


def note(kind, ver, r_stage):
    s = STATS.setdefault(kind, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], ver.worst), max(s[1], r_stage or 0.0), s[2] + ver.checked
    return f"{kind}: largest |got - ref| / bound {s[0]:.3f}, largest r_stage {s[1]:.2e}, {s[2]} elements so far"


def inputs(fmt, N, K, w_std=0.03):
    key = (fmt, N, K, w_std)
    if key not in _IN:
        _IN[key] = R.seeded_linear_inputs(fmt, 64, N, K, seed=1000 + N + K, w_std=w_std)
    return _IN[key]


def pre(fmt, epi, N, K):
    """The 64-row float64 contraction of a case, computed once and shared by every M, bias choice and context."""
    key = (fmt, epi, N, K)
    if key not in _PRE:
        X, W, gain, _, _ = inputs(fmt, N, K)
        _PRE[key] = R.linear_pre(fmt, epi, X, W, None if epi == R.RESID else gain)
    return _PRE[key]


def want_id(epi, M, N, head=False, head_stream=True):
    if epi == R.RESID:
        return R.ID_R11
    if epi == R.SWIGLU:
        return R.ID_G22 if M > 16 else R.ID_G12
    if head and head_stream and M <= 32 and N >= 4096:
        return R.ID_HEAD
    if N >= 32768:
        return R.ID_S22 if M > 16 else R.ID_S12
    return R.ID_S12 if N >= 4096 and M > 16 else R.ID_S11


def run_linear(eng, fmt, epi, M, N, K, with_bias, alias=False, head=False, head_stream=True, kind=None):
    X, W, gain, bias, resid = inputs(fmt, N, K)
    b = lambda t: h16_bits(t, fmt)
    out, tail, var = eng.test_wide_linear(epi, M, b(X[:M]), b(W), None if epi == R.RESID else b(gain),
                                          bias.numpy() if with_bias else None, b(resid[:M]) if epi == R.RESID else None,
                                          alias=alias, vocab_head=head)
    IDS.add(var)
    assert var == want_id(epi, M, N, head, head_stream), (epi, M, N, var)
    assert tail.shape[0] == -M % 32
    sent = SENT32 if epi == R.STORE else SENT16
    assert bool((tail.view(np.uint32 if epi == R.STORE else np.uint16) == sent).all()), ("rows past M were written", epi, M, N, K)
    ref = R.linear_ref(fmt, epi, bias=bias if with_bias else None, resid=resid, pre=pre(fmt, epi, N, K), rows=M)
    ver = R.check(out, ref.ref, ref.err, fmt)
    line = note(kind or f"linear id {var}", ver, ref.r_stage)
    assert ver.flagged == 0 and ver.checked == out.size, (
        f"{fmt} epi {epi} M {M} N {N} K {K} bias {with_bias} alias {alias} id {var}: {ver.flagged} flagged, worst {ver.worst:.3f}, "
        f"rows {ver.rows[:12]}, cols {ver.cols[:12]}")
    return line


@pytest.mark.parametrize("K", (1024, 2048, 3072))
@pytest.mark.parametrize("epi,N", [(R.STORE, 64), (R.STORE, 4096), (R.SWIGLU, 64), (R.RESID, 1024)])
@pytest.mark.parametrize("fmt", FMTS)
def test_linear_every_class_every_k(fmt, epi, N, K):
    """<1,1> / <1,2> store, <1,2> / <2,2> SwiGLU and the <1,1> residual epilogue at the smallest N that selects each, over
    every M, with and without bias, the residual epilogue aliased and not; at K = 1024 also on a max_batch = 5 context
    (xo_ldm = 32 instead of 128)."""
    line = ""
    for eng, ms in [(engine(fmt), MS)] + ([(engine(fmt, max_batch=5), [m for m in MS if m <= 32])] if K == 1024 and N <= 1024 else []):
        for M in ms:
            for with_bias in (True, False):
                for alias in ((False, True) if epi == R.RESID else (False,)):
                    line = run_linear(eng, fmt, epi, M, N, K, with_bias, alias)
    print(f"\n{fmt} epi {epi} N {N} K {K}: {line}; ids so far {sorted(IDS)}")


@pytest.mark.parametrize("fmt", FMTS)
def test_linear_store_at_the_vocabulary_width(fmt):
    """N = 32768 (K = 1024): <1,2,norm,store> up to 16 rows and <2,2,norm,store> beyond - the form only a 33..64-row batch at
    s1-mini's 155 776-row vocabulary reaches in the product."""
    line = ""
    for M in MS:
        for with_bias in (True, False):
            line = run_linear(engine(fmt), fmt, R.STORE, M, 32768, 1024, with_bias)
    print(f"\n{fmt} N 32768: {line}")


@pytest.mark.parametrize("N", (4096, 5120, 32784))
@pytest.mark.parametrize("fmt", FMTS)
def test_vocabulary_head(fmt, N):
    """wide_head_kernel at 256 tiles (most of its 2048 waves idle), 320, and 2049 (one wave takes a second tile step), and
    the same shapes on the general launch (FT_NO_HEAD_STREAM); each against the reference on its own.  The general launch
    takes two 16-row weight tiles per workgroup from 17 rows on: it refuses N = 32784, as the product's load-time check
    (vocab_size % 32) does."""
    eng, gen = engine(fmt), engine(fmt, env="FT_NO_HEAD_STREAM")
    from fish_tts_amd.ar_engine import HipError
    line = ""
    for M in HEAD_MS:
        line = run_linear(eng, fmt, R.STORE, M, N, 1024, False, head=True, kind="vocabulary head (wide_head_kernel)")
        if N % 32 and (M > 16 or N >= 32768):
            with pytest.raises(HipError, match="whole number"):
                run_linear(gen, fmt, R.STORE, M, N, 1024, False, head=True, head_stream=False)
        else:
            run_linear(gen, fmt, R.STORE, M, N, 1024, False, head=True, head_stream=False)
    print(f"\n{fmt} N {N}: {line}")


def test_fp16_overflow_stores_infinity_where_the_reference_does():
    """Weights large enough that accumulators pass 65504: device and reference must store infinity at the same elements
    (R.check: infinity exactly where the reference passes the threshold by more than err, finite where it stays below)."""
    fmt, M, N, K = "fp16", 17, 64, 1024
    X, W, gain, _, _ = R.seeded_linear_inputs(fmt, M, N, K, seed=77, w_std=2000.0)
    b = lambda t: h16_bits(t, fmt)
    out, tail, var = engine(fmt).test_wide_linear(R.STORE, M, b(X), b(W), b(gain))
    ref = R.linear_ref(fmt, R.STORE, X, W, gain)
    ver = R.check(out, ref.ref, ref.err, fmt)
    n_inf = int(np.isinf(out).sum())
    print(f"\nfp16 overflow: {n_inf} of {out.size} elements are infinite, worst finite ratio {ver.worst:.3f}")
    assert var == R.ID_S11 and 0 < n_inf < out.size
    assert ver.flagged == 0, (ver.rows, ver.cols)
    assert int((ref.ref.abs() >= R.OVERFLOW[fmt]).sum()) == n_inf or bool(((ref.ref.abs() - R.OVERFLOW[fmt]).abs() <= ref.err).any())


def test_what_the_dispatcher_refuses():
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import HipError
    from tests.hip_util import make_pair
    eng = engine("bf16", max_batch=5)
    z = lambda *s: np.zeros(s, dtype=np.uint16)
    for epi, M, N, K in ((R.STORE, 0, 64, 1024), (R.STORE, 33, 64, 1024), (R.STORE, 5, 64, 512), (R.STORE, 5, 64, 4096),
                         (R.STORE, 5, 24, 1024), (R.SWIGLU, 5, 48, 1024)):
        with pytest.raises(HipError) as e:
            eng.test_wide_linear(epi, M, z(M, K), z(N, K), z(K))
        assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    f32, _ = make_pair(tiny_shape(), "fp32")
    with pytest.raises(HipError) as e:
        f32.test_wide_linear(R.STORE, 5, z(5, 1024), z(64, 1024), z(1024))
    assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    f32.close()


# ------------------------------------------------------------------------------------------------------ attention
def attn_inputs(fmt, H, Hkv):
    key = ("attn", fmt, H, Hkv)
    if key not in _IN:
        g = torch.Generator().manual_seed(4000 + H + Hkv)
        hd = 128
        r = lambda t: R.round16(t.to(F32), fmt)
        qkv = r(torch.randn(64, (H + 2 * Hkv) * hd, generator=g))
        qkv[3] = r(qkv[3] * 64.0)
        qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.0 + 0.1 * torch.randn(hd, generator=g))
        pos = np.array([CTX_LENS[(3 * m) % 10] - 1 for m in range(64)], dtype=np.int32)
        kc = h16_bits(torch.randn(64, Hkv, N_SLOTS, hd, generator=g), fmt)
        vc = h16_bits(torch.randn(64, Hkv, N_SLOTS, hd, generator=g), fmt)
        for m in range(64):                               # NaN patterns from the new position on: the kernels mask them by construction
            kc[m, :, pos[m]:] = SENT16
            vc[m, :, pos[m]:] = SENT16
        _IN[key] = (qkv, qn, kn, pos, kc, vc, O.rope_table(N_SLOTS, hd, 1e6).to(F32))
    return _IN[key]


@pytest.mark.parametrize("M", (5, 15, 16, 33, 64))
@pytest.mark.parametrize("H,Hkv", [(16, 8), (8, 8), (16, 4)])
@pytest.mark.parametrize("fmt", FMTS)
def test_attention(fmt, H, Hkv, M):
    """attn_wide_kernel<2>, <1> and <4> from 128 (row, kv head) blocks on, the split fall-back below: one launch mixing the
    context lengths of CTX_LENS; y, the appended K and V rows, and every other cache row bit-unchanged."""
    check_attention(engine(fmt, H, Hkv), fmt, H, Hkv, M)


def check_attention(eng, fmt, H, Hkv, M):
    hd = 128
    qkv, qn, kn, pos, kc, vc, tab = attn_inputs(fmt, H, Hkv)
    b = lambda t: h16_bits(t, fmt)
    y, kc2, vc2, splits = eng.test_wide_attn(qkv[:M].numpy(), pos[:M], b(qn), b(kn), kc[:M], vc[:M])
    if M * Hkv >= 128:
        assert splits == 0, splits
    else:
        ctx_splits = 32 if (H, Hkv) == (16, 8) else 1          # one kv head per XCD at 16/8 on 256 CUs (engine.hip: ar_alloc), else n_slots <= 512: 1
        want = 1
        while want < ctx_splits and M * Hkv * want < 256:
            want *= 2
        assert splits == want, (splits, want)
        if (H, Hkv) == (16, 8):
            assert splits > 1                                  # the combine kernel runs
    ref = R.attn_ref(fmt, qkv[:M], pos[:M], qn, kn, kc[:M], vc[:M], tab, H, Hkv, hd, splits=splits)
    kind = f"attn_wide_kernel<{H // Hkv}>" if splits == 0 else "attn_decode + combine" if splits > 1 else "attn_decode (1 split)"
    vy = R.check(y, ref.y.ref, ref.y.err, fmt)
    rows = np.arange(M)
    k_new, v_new = kc2[rows, :, pos[:M]], vc2[rows, :, pos[:M]]              # [M, Hkv, hd]
    vk = R.check(k_new, ref.k.ref, ref.k.err, fmt)
    print(f"\n{fmt} {H}/{Hkv} M {M} splits {splits}: {note(kind, vy, ref.y.r_stage)}; appended K rows worst {vk.worst:.3f}")
    assert vy.flagged == 0 and vy.checked == M * H * hd, (vy.flagged, vy.worst, vy.rows[:12], vy.cols[:12])
    assert vk.flagged == 0 and vk.checked == M * Hkv * hd, (vk.flagged, vk.worst, vk.rows[:12])
    assert np.array_equal(v_new, b(ref.v)), "the appended V rows are copies"
    for got, was, new in ((kc2, kc[:M], k_new), (vc2, vc[:M], v_new)):
        was = was.copy()
        was[rows, :, pos[:M]] = new
        assert np.array_equal(got, was), "a cache row other than pos[m] changed"


# ------------------------------------------------------------------------------------------------------ a 256-row context
BIG = 256                                                       # xo_pair = 256, xo_ldm = 512


@pytest.mark.parametrize("epi,N,head", [(R.STORE, 64, False), (R.STORE, 4096, False), (R.STORE, 32768, False), (R.STORE, 4096, True),
                                        (R.SWIGLU, 64, False), (R.RESID, 1024, False)])
@pytest.mark.parametrize("fmt", FMTS)
def test_linear_at_xo_ldm_512(fmt, epi, N, head):
    """Every epilogue and tile class (<1,1>, <1,2>, <2,2> store, the vocabulary head, <1,2> / <2,2> SwiGLU, the residual
    epilogue aliased and not) at K = 1024 and M = 5, 17, 33, 64 with the operands at row stride 512: same verdicts, same
    sentinel rows."""
    eng = engine(fmt, max_batch=BIG)
    line = ""
    for M in (5, 17, 33, 64):
        for alias in ((False, True) if epi == R.RESID else (False,)):
            line = run_linear(eng, fmt, epi, M, N, 1024, with_bias=bool(M & 1) and not head, alias=alias, head=head,
                              kind="vocabulary head (wide_head_kernel)" if head and M <= 32 else None)
    print(f"\n{fmt} epi {epi} N {N} head {head} on a {BIG}-row context: {line}")


@pytest.mark.parametrize("M", (16, 64))
@pytest.mark.parametrize("fmt", FMTS)
def test_attention_at_xo_ldm_512(fmt, M):
    check_attention(engine(fmt, max_batch=BIG), fmt, 16, 8, M)


@pytest.mark.parametrize("fmt", FMTS)
def test_fast_attention_and_draw_at_xo_ldm_512(fmt):
    """fast_attn_kernel's octet-major output (form 1) at M = 5 and 64 on the 256-row context, judged as
    tests/test_ar_kernels_gpu.py judges it; the paired form is refused (xo_pair = 256: xo_pair + M <= 64 holds for no M, the
    product never pairs there), and a lock-step draw at cb = 0 sends its octet-major copy to xo_femb, never to the paired rows."""
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import HipError
    from tests import ar_ref as A
    from tests import test_ar_kernels_gpu as AK
    eng = engine(fmt, max_batch=BIG)
    qkv, qn, kn, kc, vc, tab, (H, Hkv, hd, ncb) = AK.fast_inputs(fmt, "16/8x128", 128)
    b = lambda t: A.wbits(t, fmt)
    HD, line = H * hd, ""
    for M in (5, 64):
        for c in (0, 1, ncb - 1):
            norm = bool((M + c) & 1)
            q_, k_ = (qn, kn) if norm else (None, None)
            what = f"{fmt} wide M {M} c {c} qk-norm {norm} xo_ldm 512"
            yb, kc1, vc1 = eng.test_fast_attn(1, qkv[:M].numpy(), c, None if q_ is None else b(q_), None if k_ is None else b(k_), kc[:M], vc[:M])
            assert yb.shape[1] == 2 * BIG and bool((yb[:, M:, :] == A.SENT16).all()), "rows past M written: " + what
            kin, vin = AK.nan_from(kc[:M], vc[:M], c, fmt)
            ref = A.fast_attn_ref(fmt, qkv[:M], c, q_, k_, kin, vin, tab, H, Hkv, hd)
            line = AK.check_fast(fmt, what, f"fast_attn_kernel (wide, hd {hd}, xo_ldm 512)", A.xo_rows(yb, M, HD), ref, kin, vin, kc1, vc1, c, M)
    for M in (5, 64):
        with pytest.raises(HipError) as e:
            eng.test_fast_attn(2, torch.cat([qkv[:M], qkv[64:64 + M]]).numpy(), 0, None, None, kc[:M], vc[:M])
        assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    a = eng.args
    g = np.random.default_rng(9)
    for M in (5, 64):
        for cb in (0, 1):
            V = a.vocab_size if cb == 0 else min(1024, a.codebook_size)
            got = eng.test_draw(g.standard_normal((M, V)).astype(np.float32), cb, [eng._sampling(0.7, 0.8, 1.1, seed=3 + m) for m in range(M)],
                                [1 + m % 20 for m in range(M)], np.zeros((M, a.num_codebooks + 1, 8 + 24), dtype=np.int32))
            assert got["what"] >= 0 and not got["what"] & 8, (M, cb, got["what"])
            assert got["what"] & 4, (M, cb, got["what"])                   # the lock-step form: the copy goes to xo_femb
    print(f"\n{line}")


def test_every_class_is_reachable():
    """One launch per instantiation class, through the dispatcher's own thresholds: the set of ids reached, printed."""
    eng, seen = engine("bf16"), set()
    z = lambda *s: np.zeros(s, dtype=np.uint16)
    for epi, M, N, head in ((R.STORE, 16, 4096, False), (R.STORE, 17, 4096, False), (R.STORE, 16, 32768, False),
                            (R.STORE, 17, 32768, False), (R.SWIGLU, 16, 64, False), (R.SWIGLU, 17, 64, False),
                            (R.RESID, 5, 1024, False), (R.STORE, 32, 4096, True), (R.STORE, 33, 4096, True)):
        _, _, var = eng.test_wide_linear(epi, M, z(M, 1024), z(N, 1024), None if epi == R.RESID else z(1024),
                                         resid=z(M, N) if epi == R.RESID else None, vocab_head=head)
        assert var == want_id(epi, M, N, head), (epi, M, N, head, var)
        seen.add(var)
    print(f"\ninstantiation ids reached: {sorted(seen)} (all tests of this run: {sorted(IDS | seen)})")
    for kind, (worst, r, n) in sorted(STATS.items()):
        print(f"  {kind}: largest |got - ref| / bound {worst:.3f}, largest r_stage {r:.2e}, {n} elements")
    assert seen == set(range(7)), seen
