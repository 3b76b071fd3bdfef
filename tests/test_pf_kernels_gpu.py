"""GPU: the launches of the bf16 prompt pass (csrc/engine.hip: prefill_gemm) - pf_gemm's kernel classes (skinny_gemm_kernel<TS>,
lingemm_kernel<128,128> and <64,64>, the two tapgemm64_kernel tiles, the tapgemm_kernel fall-backs), rmsnorm_llama_rows_kernel,
prefill_rope_append_kernel and flash_prefill_kernel<HD, NG> (and attn_decode_kernel position by position) - called ONE LAUNCH AT
A TIME through the product's own host dispatchers (ft_test_pf_linear, ft_test_pf_norm, ft_test_pf_attn) on seeded inputs,
every element of every written row against the float64 restatement of tests/pf_ref.py:

    |got - ref| <= half a ulp of bf16 at max(|got|, |ref|) + err

with err derived there.  Rows past S must still hold the sentinel, cache rows other than the appended ones must be
bit-unchanged (the hook's NaN fill behind every sequence and in unused slots included), every y must be finite.
tests/test_pf_ref_host.py proves the checker flags the subtle faults this is for.  These hooks trace no prompt pass: the wiring between
the launches is held to float64 launch by launch in tests/test_prompt_launches_gpu.py (the launch trace of a whole prompt call),
beside the oracle-following tests (test_ar_gpu.py: test_prefill_gemm_paths_vs_oracle, test_ragged_prompt_pass_vs_oracle)."""
import os

import numpy as np
import pytest
import torch

from tests import pf_ref as P
from tests.codec_stage_ref import h16_bits
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import tiny_shape
from tests.test_ar_gpu import medium_shape

pytestmark = pytest.mark.gpu

FMT = P.FMT
SKINNY_S = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)     # both sides of the 16-row tiles of TS = 1, 2, 4 and of the skinny limit
LIN64_S = (129, 191, 192, 193, 511)                              # first row past the skinny limit, both sides of a 64-row tile, last below the 128 tile
LIN128_S = (512, 513, 640, 641)                                  # first row of the 128 x 128 tile, both sides of its row-tile edges
FORMS = ((P.WQKV, False), (P.RESID, False), (P.RESID, True), (P.W13, False))          # (form, in place)
GEOMS = ((16, 8, 128), (8, 8, 128), (16, 4, 128), (16, 8, 64))
LPS_A = (16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)          # NG = 4: query tiles of 32, the 128-key step and the 256-key pair
LPS_B = (255, 256, 257, 320, 321, 385)                           # ... the NG threshold (320 / 321) and NG = 2 (query tiles of 64)
POS0S = (0, 1, 31, 100)
MAX_SEQ, MB, SLOT = 768, 9, 5
_ENG, _PRE, _IN, _APP = {}, {}, {}, {}
STATS = {}                                                       # kernel kind -> [worst ratio, largest r_stage, elements]
IDS = set()
PATHS = set()


def engine(H=16, Hkv=8, hd=128, max_batch=1, mode=None):
    """A bf16 context at s1-mini widths with one slow layer, shared by the tests of this module; FT_NO_ENGINE: the hooks need
    no frame engine.  mode: FT_PREFILL_GEMM of the context (read when it is created)."""
    key = (H, Hkv, hd, max_batch, mode)
    if key not in _ENG or not _ENG[key]._h:                 # (a failed test's engines are closed by tests/conftest.py)
        from fish_tts_amd.ar_engine import ARHipEngine
        shape = medium_shape(n_text=17, n_layer=1, n_head=H, n_local_heads=Hkv, head_dim=hd, max_seq_len=MAX_SEQ)
        env = {"FT_NO_ENGINE": "1"}
        if mode is not None:
            env["FT_PREFILL_GEMM"] = str(mode)
        saved = {n: os.environ.get(n) for n in env}
        os.environ.update(env)
        try:
            eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                              precision="bf16", device=0, max_batch=max_batch, max_new_tokens=8)
            eng.load_state_dict({k: v.to(torch.bfloat16) for k, v in cached_random_weights(shape, seed=0).items()})
        finally:
            for n, v in saved.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
        _ENG[key] = eng
    return _ENG[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENG.values():
        eng.close()
    for d in (_ENG, _PRE, _IN, _APP):
        d.clear()


def note(kind, ver, r_stage):
    s = STATS.setdefault(kind, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], ver.worst), max(s[1], r_stage or 0.0), s[2] + ver.checked
    return f"{kind}: largest |got - ref| / bound {s[0]:.3f}, largest r_stage {s[1]:.2e}, {s[2]} elements so far"


def summary():
    return "\n".join(f"  {kind}: largest |got - ref| / bound {w:.3f}, largest r_stage {r:.2e}, {n} elements"
                     for kind, (w, r, n) in sorted(STATS.items()))


# ------------------------------------------------------------------------------------------------------ linear
def lin_case(N, K, rows):
    """Inputs and the float64 contraction of a width, computed once for `rows` rows and shared by every S, form and bias."""
    key = (N, K)
    if key not in _PRE or _PRE[key][0][0].shape[0] < rows:
        X, W, bias, resid = P.seeded_linear_inputs(rows, N, K, seed=2000 + N + K)
        _PRE[key] = ((X, W, bias, resid), P.linear_pre(X, W))
    return _PRE[key]


def run_linear(eng, mode, form, alias, S, N, K, with_bias, rows):
    (X, W, bias, resid), pre = lin_case(N, K, rows)
    b = lambda t: h16_bits(t, FMT)
    out, tail, var = eng.test_pf_linear(form, b(X[:S]), b(W), bias.numpy() if with_bias else None,
                                        resid[:S].numpy() if form == P.RESID else None, alias=alias)
    IDS.add(var)
    what = f"mode {mode} form {form} S {S} N {N} K {K} bias {with_bias} in place {alias} id {var}"
    assert var == P.want_id(2 if mode is None else mode, S, N, K), what
    assert tail.shape[0] == -S % 128
    sent = P.SENT16 if form == P.W13 else P.SENT32
    assert bool((tail.view(np.uint16 if form == P.W13 else np.uint32) == sent).all()), "rows past S were written: " + what
    ref = P.linear_ref(form, pre, bias=bias if with_bias else None, resid=resid if form == P.RESID else None, rows=S)
    ver = P.check(out, ref.ref, ref.err)
    line = note(f"linear {P.ID_NAMES[var]}", ver, ref.r_stage)
    print(f"  {what}: worst {ver.worst:.3f}")
    assert ver.flagged == 0 and ver.checked == out.size, (
        f"{what}: {ver.flagged} flagged, worst {ver.worst:.3f}, rows {ver.rows[:12]}, cols {ver.cols[:12]}")
    return line


def run_all_forms(eng, mode, Ss, N, K):
    line = ""
    for S in Ss:
        for form, alias in FORMS:
            for with_bias in (True, False):
                line = run_linear(eng, mode, form, alias, S, N, K, with_bias, max(Ss))
    print(f"\nN {N} K {K}: {line}; ids so far {sorted(IDS)}")


@pytest.mark.parametrize("K", (128, 1024))
@pytest.mark.parametrize("N", (64, 1024))
def test_linear_skinny(N, K):
    """skinny_gemm_kernel<1>, <2>, <4> (one and two 64-row block rows): all four forms, with and without bias."""
    run_all_forms(engine(), None, SKINNY_S, N, K)


@pytest.mark.parametrize("K", (256, 512, 1024))
@pytest.mark.parametrize("N", (128, 1024, 1152))
def test_linear_lingemm64(N, K):
    """lingemm_kernel<64,64> (DEPTH = 4 K-steps in flight): K = 256 is one DEPTH round, 512 one round past it, 1024 the model's."""
    run_all_forms(engine(), None, LIN64_S, N, K)


@pytest.mark.parametrize("K", (256, 512, 1024))
@pytest.mark.parametrize("N", (1152, 2048))
def test_linear_lingemm128(N, K):
    """lingemm_kernel<128,128> from 512 rows at N > 1024."""
    run_all_forms(engine(), None, LIN128_S, N, K)


@pytest.mark.parametrize("S,N", ((129, 1152), (513, 1152), (513, 2048)))
def test_linear_tapgemm64_at_k_192(S, N):
    """K = 192 (K % 256 != 0): tapgemm64_kernel<64,64> below 512 rows, <128,128> from there."""
    run_all_forms(engine(), None, (S,), N, 192)


@pytest.mark.parametrize("mode,N", ((1, 1024), (0, 1024), (0, 64)))
def test_linear_other_dispatch_modes(mode, N):
    """The same S edges under FT_PREFILL_GEMM = 1 (no skinny kernel: lingemm from the first row) and = 0 (the tapgemm_kernel
    fall-backs alone, <128,128> and at N = 64 <128,64>: 128-row tiles)."""
    run_all_forms(engine(mode=mode), mode, SKINNY_S + LIN64_S + (513,), N, 1024)


@pytest.mark.parametrize("D", (64, 1024))
def test_norm(D):
    g = torch.Generator().manual_seed(3000 + D)
    x = P.round16(torch.randn(129, D, generator=g), FMT)
    x[3] *= 64.0
    gain = P.round16(1.0 + 0.1 * torch.randn(D, generator=g), FMT)
    line = ""
    for S in (1, 17, 129):
        out, tail = engine().test_pf_norm(x[:S].numpy(), h16_bits(gain, FMT))
        assert bool((tail == P.SENT16).all()), "the row past S was written"
        ref = P.norm_ref(x[:S], gain, 1e-6)
        ver = P.check(out, ref.ref, ref.err)
        line = note("rmsnorm_llama_rows_kernel", ver, None)
        assert ver.flagged == 0 and ver.checked == S * D, (S, D, ver.flagged, ver.worst, ver.rows[:12], ver.cols[:12])
    print(f"\nD {D}: {line}")


def test_what_the_linear_hook_refuses():
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import HipError
    from tests.hip_util import make_pair
    eng = engine()
    z = lambda *s: np.zeros(s, dtype=np.uint16)
    for form, S, N, K in ((P.WQKV, MAX_SEQ + 1, 64, 128), (P.WQKV, 5, 64, 48), (P.WQKV, 5, 24, 128), (3, 5, 64, 128)):
        with pytest.raises(HipError) as e:
            eng.test_pf_linear(form, z(S, K), z(N, K))
        assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    with pytest.raises(HipError) as e:
        eng.test_pf_linear(P.RESID, z(5, 128), z(64, 128))                     # no residual
    assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    f32, _ = make_pair(tiny_shape(), "fp32")
    try:
        with pytest.raises(HipError) as e:
            f32.test_pf_linear(P.WQKV, z(5, 128), z(64, 128))
        assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    finally:
        f32.close()


# ------------------------------------------------------------------------------------------------------ attention
def attn_inputs(H, Hkv, hd):
    key = (H, Hkv, hd)
    if key not in _IN:
        _IN[key] = P.seeded_attn_inputs(640, H, Hkv, hd, MAX_SEQ, MB, seed=5000 + H + Hkv + hd)
    return _IN[key]


def append_of(H, Hkv, hd, pos0, rows=385):
    """The float64 append of rows 0 .. rows - 1 of the geometry's inputs at positions pos0 + row: shared by every prompt
    length at that pos0 (a shorter prompt is a prefix of it)."""
    key = (H, Hkv, hd, pos0)
    if key not in _APP:
        qkv, qn, kn, _, _, tab = attn_inputs(H, Hkv, hd)
        _APP[key] = P.append_ref(qkv[:rows], range(pos0, pos0 + rows), qn, kn, tab, H, Hkv, hd)
    return _APP[key]


def rows_of(app, rows):
    cut = lambda r: P.Ref(r.ref[rows], r.err[rows], r.rnd[rows])
    return P.AppendRef(cut(app.q), cut(app.k), app.v[rows])


def run_attn(H, Hkv, hd, seqs, app, want_path, env=None):
    """One pass through the hook and every assertion of an attention case.  want_path: "ragged" = the n_seq form of the hook
    (NG follows the longest sequence), else the single-prompt form of seqs[0] and the path it must take."""
    qkv, qn, kn, kc, vc, tab = attn_inputs(H, Hkv, hd)
    eng = engine(H, Hkv, hd, MB)
    S = sum(s.rows for s in seqs)
    b = lambda t: h16_bits(t, FMT)
    single = want_path != "ragged"
    saved = os.environ.get(env) if env else None
    if env:
        os.environ[env] = "1"
    try:
        if single:
            y, q, kc1, vc1, tail, path = eng.test_pf_attn(qkv[:S].numpy(), b(qn), b(kn), kc, vc, pos0=seqs[0].pos0, slot=seqs[0].slot)
        else:
            y, q, kc1, vc1, tail, path = eng.test_pf_attn(qkv[:S].numpy(), b(qn), b(kn), kc, vc,
                                                          seqs=[[s.row0, s.rows, s.pos0, s.slot] for s in seqs])
    finally:
        if env:
            os.environ.pop(env, None) if saved is None else os.environ.__setitem__(env, saved)
    PATHS.add((hd, path))
    what = f"{H}/{Hkv} x {hd} seqs {[(s.rows, s.pos0, s.slot) for s in seqs]} path {path}"
    max_lp = max(s.rows for s in seqs)
    assert path == (want_path if isinstance(want_path, int) else (4 if max_lp <= 320 else 2)), what
    assert bool((tail == P.SENT16).all()), "the row past S of y or q was written: " + what
    cv = P.check_cache(kc, vc, kc1, vc1, seqs, app, Hkv, hd)
    assert cv.k.flagged == 0 and cv.k.checked == S * Hkv * hd, (what, "appended K rows", cv.k.flagged, cv.k.worst, cv.k.rows[:12])
    assert cv.v_equal, what + ": the appended V rows are copies"
    assert cv.untouched, what + ": a cache row that was not appended changed"
    if path == 0:
        assert bool((q == P.SENT16).all()), what                                   # the decode kernel keeps its queries in LDS
        a = P.decode_ref(qkv, kc1, vc1, seqs[0], qn, kn, tab, H, Hkv, hd)
        ref, kind, vq = a.y, f"attn_decode_kernel position by position (hd {hd})", None
    else:
        vq = P.check(q, app.q.ref, app.q.err)
        note(f"prefill_rope_append_kernel<{hd}> (q, k)", vq, None)
        assert vq.flagged == 0 and vq.checked == S * H * hd, (what, "finished queries", vq.flagged, vq.worst, vq.rows[:12])
        ref, kind = P.attn_ref(q, kc1, vc1, seqs, path, H, Hkv, hd), f"flash_prefill_kernel<{hd}, {path}>"
    note(f"prefill_rope_append_kernel<{hd}> (q, k)" if path else f"attn_decode_kernel append (hd {hd})", cv.k, None)
    assert bool(np.isfinite(P.values(y, FMT).numpy()).all()), what + ": y is not finite"
    vy = P.check(y, ref.ref, ref.err)
    line = note(kind, vy, ref.r_stage)
    print(f"  {what}: y worst {vy.worst:.3f}, k {cv.k.worst:.3f}" + ("" if vq is None else f", q {vq.worst:.3f}"))
    assert vy.flagged == 0 and vy.checked == S * H * hd, (what, vy.flagged, vy.worst, vy.rows[:12], vy.cols[:12])
    return line


@pytest.mark.parametrize("lps", (LPS_A, LPS_B), ids=("to129", "from255"))
@pytest.mark.parametrize("pos0", POS0S)
@pytest.mark.parametrize("H,Hkv,hd", GEOMS)
def test_attention_single_prompt(H, Hkv, hd, pos0, lps):
    """flash_prefill_kernel<hd, 4> up to 320 rows and <hd, 2> beyond, behind a restored prefix of pos0 rows."""
    app, line = append_of(H, Hkv, hd, pos0), ""
    for Lp in lps:
        line = run_attn(H, Hkv, hd, [P.Seq(0, Lp, pos0, SLOT)], rows_of(app, slice(0, Lp)), 4 if Lp <= 320 else 2)
    print(f"\n{H}/{Hkv} x {hd} pos0 {pos0}: {line}")


@pytest.mark.parametrize("H,Hkv,hd", GEOMS)
def test_attention_position_by_position(H, Hkv, hd):
    """Fewer than 16 rows, and longer prompts under FT_PREFILL_ATTN_V0: attn_decode_kernel per position."""
    line = ""
    for pos0 in POS0S:
        app = append_of(H, Hkv, hd, pos0)
        for Lp in (1, 2, 15):
            line = run_attn(H, Hkv, hd, [P.Seq(0, Lp, pos0, SLOT)], rows_of(app, slice(0, Lp)), 0)
    for Lp, pos0 in ((16, 0), (33, 31)):
        line = run_attn(H, Hkv, hd, [P.Seq(0, Lp, pos0, SLOT)], rows_of(append_of(H, Hkv, hd, pos0), slice(0, Lp)), 0, env="FT_PREFILL_ATTN_V0")
    print(f"\n{H}/{Hkv} x {hd}: {line}")


RAGGED = {   # lengths in launch order; pos0 and slots below, one of the nine slots unused
    "5 to 130": (33, 1, 130, 15, 64), "5 to 321": (2, 321, 15, 64, 1),
    "8 to 130": (130, 1, 2, 15, 33, 64, 130, 64), "8 to 321": (15, 321, 1, 2, 33, 64, 130, 33),
}
RAGGED_POS0 = (0, 31, 1, 100, 0, 7, 64, 3)
RAGGED_SLOTS = (6, 2, 8, 0, 5, 1, 7, 3)                            # slot 4 is never named


@pytest.mark.parametrize("case", sorted(RAGGED))
@pytest.mark.parametrize("H,Hkv,hd", GEOMS)
def test_attention_ragged(H, Hkv, hd, case):
    """Several sequences in one launch (grid.z): mixed lengths and pos0, slots in shuffled order, max_lp on both sides of 320."""
    lens = RAGGED[case]
    qkv, qn, kn, _, _, tab = attn_inputs(H, Hkv, hd)
    seqs, row0 = [], 0
    for i, n in enumerate(lens):
        seqs.append(P.Seq(row0, n, RAGGED_POS0[i], RAGGED_SLOTS[i]))
        row0 += n
    key = (H, Hkv, hd, case)
    if key not in _APP:
        _APP[key] = P.append_ref(qkv[:row0], [s.pos0 + i for s in seqs for i in range(s.rows)], qn, kn, tab, H, Hkv, hd)
    line = run_attn(H, Hkv, hd, seqs, _APP[key], "ragged")
    print(f"\n{H}/{Hkv} x {hd} {case}: {line}")


def test_what_the_attention_hook_refuses():
    from fish_tts_amd import _lib as L
    from fish_tts_amd.ar_engine import HipError
    H, Hkv, hd = GEOMS[0]
    qkv, qn, kn, kc, vc, _ = attn_inputs(H, Hkv, hd)
    eng, b = engine(H, Hkv, hd, MB), lambda t: h16_bits(t, FMT)
    bad = ([[0, 5, 0, 9]], [[0, 5, 0, 1], [5, 5, 0, 1]], [[0, 5, 0, 1], [6, 4, 0, 2]], [[0, 0, 0, 1]], [[0, 5, MAX_SEQ - 5, 1]])
    for seqs in bad:
        with pytest.raises(HipError) as e:
            eng.test_pf_attn(qkv[:10].numpy(), b(qn), b(kn), kc, vc, seqs=seqs)
        assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)
    for pos0, slot in ((MAX_SEQ - 10, 0), (0, MB), (-1, 0)):
        with pytest.raises(HipError) as e:
            eng.test_pf_attn(qkv[:10].numpy(), b(qn), b(kn), kc, vc, pos0=pos0, slot=slot)
        assert f"({L.FT_ERR_ARG})" in str(e.value), str(e.value)


def test_every_class_is_reachable():
    """One launch per kernel class of pf_gemm through the dispatcher's own thresholds, both NG forms at both head widths and the
    per-position path: the ids the dispatchers reported."""
    z = lambda *s: np.zeros(s, dtype=np.uint16)
    seen = set()
    for mode, S, N, K, want in ((None, 16, 64, 128, P.ID_SKINNY1), (None, 17, 64, 128, P.ID_SKINNY2), (None, 33, 64, 128, P.ID_SKINNY4),
                                (None, 512, 1152, 256, P.ID_LIN128), (None, 129, 128, 256, P.ID_LIN64), (None, 512, 128, 192, P.ID_TAP64_128),
                                (None, 129, 128, 192, P.ID_TAP64_64), (0, 5, 128, 128, P.ID_TAP_128), (None, 129, 64, 128, P.ID_TAP_64)):
        _, _, var = engine(mode=mode).test_pf_linear(P.WQKV, z(S, K), z(N, K))
        assert var == want == P.want_id(2 if mode is None else mode, S, N, K), (mode, S, N, K, var)
        seen.add(var)
    paths = set()
    for H, Hkv, hd in ((16, 8, 128), (16, 8, 64)):
        qkv, qn, kn, kc, vc, _ = attn_inputs(H, Hkv, hd)
        b = lambda t: h16_bits(t, FMT)
        for Lp, want in ((15, 0), (16, 4), (320, 4), (321, 2)):
            path = engine(H, Hkv, hd, MB).test_pf_attn(qkv[:Lp].numpy(), b(qn), b(kn), kc, vc, slot=SLOT)[-1]
            assert path == want, (hd, Lp, path)
            paths.add((hd, path))
    print(f"\nkernel class ids reached: {sorted(seen)} (all tests of this run: {sorted(IDS | seen)}); "
          f"attention (hd, NG or 0) reached: {sorted(paths)} (all tests of this run: {sorted(PATHS | paths)})")
    print(summary())
    assert seen == set(range(9)), seen
    assert paths == {(hd, ng) for hd in (128, 64) for ng in (0, 2, 4)}, paths
