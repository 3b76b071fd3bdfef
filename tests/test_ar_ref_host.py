"""Pins tests/ar_ref.py on the CPU: (1) launch by launch on oracle/ar.py's own intermediates of one decode step (one slow
layer, the head, two fast steps) it passes with NO element flagged, bit for bit where float32 is exact, the boundary flips
counted; (2) its checkers pass an honest float32 emulation of the device's work split and flag every one of a list of
emulated kernel faults at the right rows and columns - the proof that tests/test_ar_kernels_gpu.py (1..4 rows) and
tests/test_ar_rows_gpu.py (5..256 rows: MB-row tiles over several groups, a tail group, partials of rows >= 4) would fail if
a decode kernel were subtly wrong.

Two of the listed faults are roundings left out ("residual added before the rounding", "one norm rounding for two").  An f32
model has no rounding (RND_NONE), so there they are no faults; they are asserted in bf16 and fp16.  "One element two ulp
off" is asserted in f32 where the bound is about half a float32 ulp (a copied text embedding); after a contraction the f32
order error of the sum is itself many float32 ulp of the result, and no checker could tell."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

from oracle import ar as O
from tests import ar_ref as A
from tests import wide_ref as WR
from tests.codec_stage_ref import F32, F64, half_ulp
from tests.shapes import make_prompt, tiny_shape

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
FLIPS = {}


def _two_ulp(t, i, j, fmt):
    t = t.clone()
    t[i, j] += 4 * half_ulp(t[i, j].abs(), fmt == "f32", fmt) * (1 if t[i, j] >= 0 else -1)
    return t


# ------------------------------------------------------------------------------------------------- pinned to the oracle
@pytest.mark.parametrize("fmt", ("f32", "bf16"))
def test_restatement_passes_the_oracle_launch_by_launch(fmt):
    """A 13-position prompt fills the caches, then ONE decode step at position 13 on a VQ column: every launch of the step
    (embedding, norm + Wqkv, decode attention, Wo + residual, norm + W13 + SwiGLU, W2 + residual, norm + head; fast layer 0 at
    codebook positions 0 and 1) restated on the oracle's own input of that launch and judged against what the oracle
    computed from it.  The intermediates are rebuilt from the oracle's functions and must end in its logits and hidden
    state bit for bit."""
    dt = DT[fmt]
    c = tiny_shape()
    orc = O.AROracle(c, O.random_weights(c, seed=0), dt)
    prompt = make_prompt(c, 14, seed=300, n_vq=2)
    prompt[:, 13] = prompt[:, 2]                                         # the decode column is a VQ position
    T = 13
    w, p, fp = orc.w, "layers.0", "fast_layers.0"
    H, Hkv, hd = c.n_head, c.n_local_heads, c.head_dim
    Hf, Hkvf, hdf = c.fast_n_head, c.fast_n_local_heads, c.fast_head_dim
    G = H // Hkv
    with torch.inference_mode(), sdpa_kernel(SDPBackend.MATH):
        orc.slow_forward(prompt[:, :T].view(1, c.num_codebooks + 1, -1), torch.arange(T))
        kc0, vc0 = orc.slow_cache[0].k.clone(), orc.slow_cache[0].v.clone()
        inp, pos = prompt[:, T:T + 1].view(1, c.num_codebooks + 1, 1), torch.tensor([T])
        x = orc.embed(inp)
        qkv = F.linear(O.rms_norm(x, w[f"{p}.attention_norm.weight"], c.norm_eps), w[f"{p}.attention.wqkv.weight"])
        q, k, v = qkv.split([H * hd, Hkv * hd, Hkv * hd], dim=-1)
        tab = orc.tab[pos]
        q = O.rope(F.rms_norm(q.view(1, 1, H, hd), (hd,), w[f"{p}.attention.q_norm.weight"], c.norm_eps), tab).transpose(1, 2)
        k = O.rope(F.rms_norm(k.view(1, 1, Hkv, hd), (hd,), w[f"{p}.attention.k_norm.weight"], c.norm_eps), tab).transpose(1, 2)
        v = v.view(1, 1, Hkv, hd).transpose(1, 2)
        kk, vv = kc0.clone(), vc0.clone()
        kk[:, :, pos], vv[:, :, pos] = k, v
        y = F.scaled_dot_product_attention(q, kk.repeat_interleave(G, dim=1), vv.repeat_interleave(G, dim=1),
                                           attn_mask=orc.tril[None, None, pos, :orc.n_slots])
        y = y.transpose(1, 2).contiguous().view(1, 1, H * hd)
        h = x + F.linear(y, w[f"{p}.attention.wo.weight"])
        hn = O.rms_norm(h, w[f"{p}.ffn_norm.weight"], c.norm_eps)
        g = F.silu(F.linear(hn, w[f"{p}.feed_forward.w1.weight"])) * F.linear(hn, w[f"{p}.feed_forward.w3.weight"])
        x1 = h + F.linear(g, w[f"{p}.feed_forward.w2.weight"])
        x2 = orc._block("layers.1", x1, tab, orc.tril[None, None, pos, :orc.n_slots], pos, orc.slow_cache[1], H, Hkv, hd, True, True)
        lg = F.linear(O.rms_norm(x2, w["norm.weight"], c.norm_eps), w["embeddings.weight"])
        orc.slow_cache[0].k.copy_(kc0); orc.slow_cache[0].v.copy_(vc0)
        k1c = orc.slow_cache[1].k.clone()
        logits, hidden = orc.slow_forward(inp, pos)
        assert torch.equal(lg, logits) and torch.equal(x2, hidden) and torch.equal(orc.slow_cache[1].k, k1c)
        # fast layer 0: codebook position 0 on the hidden state, position 1 on a code's embedding
        fq, fy, fx = [], [], [hidden, F.embedding(torch.tensor([[7]]), w["fast_embeddings.weight"])]
        fk = torch.zeros(1, Hkvf, c.num_codebooks, hdf, dtype=dt)
        fv = torch.zeros_like(fk)
        for cb in (0, 1):
            qkvf = F.linear(O.rms_norm(fx[cb], w[f"{fp}.attention_norm.weight"], c.norm_eps), w[f"{fp}.attention.wqkv.weight"])
            q_, k_, v_ = qkvf.split([Hf * hdf, Hkvf * hdf, Hkvf * hdf], dim=-1)
            ft = orc.fast_tab[torch.tensor([cb])]
            q_ = O.rope(q_.view(1, 1, Hf, hdf), ft).transpose(1, 2)
            fk[:, :, cb], fv[:, :, cb] = O.rope(k_.view(1, 1, Hkvf, hdf), ft).transpose(1, 2)[:, :, 0], v_.view(1, 1, Hkvf, hdf).transpose(1, 2)[:, :, 0]
            yy = O._explicit_attention(q_, fk.repeat_interleave(Hf // Hkvf, dim=1), fv.repeat_interleave(Hf // Hkvf, dim=1),
                                       orc.tril[None, None, torch.tensor([cb]), :c.num_codebooks])
            fq.append(qkvf); fy.append(yy.transpose(1, 2).contiguous().view(1, Hf * hdf))
    W = {n: t.to(F64) for n, t in w.items()}
    d = lambda t: t.reshape(-1, t.shape[-1]).to(F64)
    bits = lambda t: A.wbits(t, fmt)
    flips = {}

    def judge(name, ref, want, exact=False):
        want = d(want)
        ver = A.check(bits(want), ref.ref, ref.err, fmt)
        differ = int((bits(ref.rnd) != bits(want)).sum())
        flips[name] = differ
        print(f"{fmt} {name}: {differ} of {want.numel()} patterns differ, worst ratio {ver.worst:.3f}")
        assert ver.flagged == 0 and ver.checked == want.numel(), (name, ver.flagged, ver.rows[:8], ver.cols[:8])
        if exact:
            assert differ == 0, (name, differ)
        elif fmt != "f32":
            lam = float((ref.err / half_ulp(ref.ref.abs(), False, fmt)).clamp(max=1.0).sum())
            assert differ <= lam + 3 * lam ** 0.5 + 1, (name, differ, lam)

    toks = prompt[:, T].numpy().reshape(1, -1)
    judge("embed", A.embed_ref(fmt, W["embeddings.weight"], W["codebook_embeddings.weight"], toks, c.num_codebooks, c.codebook_size,
                               c.semantic_begin_id, c.semantic_end_id, c.scale_codebook_embeddings), x)
    judge("norm + wqkv", A.gemv_ref(fmt, 1, A.EPI_STORE, d(x), W[f"{p}.attention.wqkv.weight"], W[f"{p}.attention_norm.weight"],
                                    eps=c.norm_eps), qkv)
    kcb, vcb = bits(kc0), bits(vc0)
    qn, kn = W[f"{p}.attention.q_norm.weight"], W[f"{p}.attention.k_norm.weight"]
    if fmt == "f32":
        a = A.decode_attn_ref(fmt, d(qkv), [T], qn, kn, kcb, vcb, orc.tab, H, Hkv, hd, 1, c.norm_eps)
        judge("decode attention", WR.Ref(a.y[:, :, 0].reshape(1, -1), a.y_err[:, :, 0].reshape(1, -1), A.store(a.y[:, :, 0].reshape(1, -1), fmt)), y)
        judge("appended k", a.k, k.transpose(1, 2).reshape(1, -1).view(1, Hkv, hd)[0])
    else:
        a = WR.attn_ref(fmt, d(qkv), [T], qn, kn, kcb, vcb, orc.tab, H, Hkv, hd, c.norm_eps, splits=1)
        judge("decode attention", a.y, y)
        assert np.array_equal(bits(a.k.rnd[0]), bits(k[0, :, 0])), "the appended K row is exact in float32"
    assert torch.equal(a.v[0].to(dt), v[0, :, 0])
    # split four ways, the same step's partials merged in float64 give the same attention output
    a4 = A.decode_attn_ref(fmt, d(qkv), [T], qn, kn, kcb, vcb, orc.tab, H, Hkv, hd, 4, c.norm_eps)
    po, pml, _, _, _ = A.emulate_decode_attn(fmt, d(qkv), [T], qn, kn, kcb, vcb, orc.tab.to(F32), H, Hkv, hd, 4, c.norm_eps)
    assert A.check_parts(po, pml, a4).flagged == 0
    ym, em, _, _ = A.merge_ref(po, pml, fmt)
    ya = a.y.ref if fmt != "f32" else a.y[:, :, 0].reshape(1, -1)
    ea = a.y.err if fmt != "f32" else a.y_err[:, :, 0].reshape(1, -1)
    assert bool(((ym - ya).abs() <= em + ea + a4.y_err.sum(dim=2).reshape(1, -1)).all())
    judge("wo + residual", A.gemv_ref(fmt, 0, A.EPI_RESID, d(y), W[f"{p}.attention.wo.weight"], resid=d(x)), h)
    w13 = WR.interleave_w13(W[f"{p}.feed_forward.w1.weight"], W[f"{p}.feed_forward.w3.weight"])
    judge("norm + w13 + swiglu", A.gemv_ref(fmt, 1, A.EPI_SWIGLU, d(h), w13, W[f"{p}.ffn_norm.weight"], eps=c.norm_eps), g)
    judge("w2 + residual", A.gemv_ref(fmt, 0, A.EPI_RESID, d(g), W[f"{p}.feed_forward.w2.weight"], resid=d(h)), x1)
    judge("norm + head", A.gemv_ref(fmt, 1, A.EPI_STORE, d(x2), W["embeddings.weight"], W["norm.weight"], eps=c.norm_eps), lg)
    fkb, fvb = bits(fk), bits(fv)
    for cb in (0, 1):
        judge(f"fast norm + wqkv c{cb}", A.gemv_ref(fmt, 1, A.EPI_STORE, d(fx[cb]), W[f"{fp}.attention.wqkv.weight"],
                                                    W[f"{fp}.attention_norm.weight"], eps=c.norm_eps), fq[cb])
        fa = A.fast_attn_ref(fmt, d(fq[cb]), cb, None, None, fkb, fvb, orc.fast_tab, Hf, Hkvf, hdf, c.norm_eps)
        judge(f"fast attention c{cb}", fa.y, fy[cb])
        if fmt != "f32":
            assert np.array_equal(bits(fa.k.rnd[0]), fkb[0, :, cb]), "the appended fast K row is exact in float32"
    FLIPS[fmt] = flips
    print(f"{fmt} boundary flips per launch: {flips}")


# ------------------------------------------------------------------------------------------------- products
# (pro, epi, M, N, K): MB = 4 tiles at M = 4, a partial last workgroup (N no multiple of 4 R), every epilogue
GEMV_CASES = {"bf16": [(1, A.EPI_STORE, 4, 23, 520), (1, A.EPI_SWIGLU, 3, 30, 1032), (0, A.EPI_RESID, 4, 21, 1024)],
              "f32": [(1, A.EPI_STORE, 4, 23, 264), (1, A.EPI_SWIGLU, 3, 30, 512), (0, A.EPI_RESID, 4, 21, 520)]}
GEMV_CASES["fp16"] = GEMV_CASES["bf16"]


@pytest.mark.parametrize("fmt", A.FMTS)
def test_checker_passes_the_honest_product_and_flags_each_product_fault(fmt):
    for pro, epi, M, N, K in GEMV_CASES[fmt]:
        x, W, gain, bias, resid = A.seeded_gemv_inputs(fmt, M, N, K, seed=11)
        kw = dict(x=x, W=W, gain=gain if pro else None, bias=bias, resid=resid if epi == A.EPI_RESID else None)
        ref = A.gemv_ref(fmt, pro, epi, **kw)
        clean = A.emulate_gemv(fmt, pro, epi, **kw)
        v = A.check(clean.to(F32).numpy(), ref.ref, ref.err, fmt)
        MB, R, NT = A.want_id(fmt, epi, M, N, K)
        print(f"{fmt} pro {pro} epi {epi} M {M} N {N} K {K} <MB {MB}, R {R}, NT {NT}>: clean worst ratio {v.worst:.3f}, r_stage {ref.r_stage:.2e}")
        assert v.checked == ref.ref.numel() and v.flagged == 0, (epi, v.flagged, v.rows[:8], v.cols[:8])
        cols = ref.ref.shape[1]
        bugs = ["last_wg", "drop_piece", "twice_piece", "drop_bias"]
        if fmt != "f32":
            bugs += ["two_ulp"] + (["mb_row"] if M == 4 else [])
        if pro:
            bugs += ["norm_other_row"] + (["single_round"] if fmt != "f32" else [])
        if epi == A.EPI_SWIGLU:
            bugs.append("swap_gate_up")
        if epi == A.EPI_RESID:
            bugs += ["resid_after_store"] + (["resid_before_round"] if fmt != "f32" else [])
        for bug in bugs:
            got = _two_ulp(clean, M - 1, 5, fmt) if bug == "two_ulp" else A.emulate_gemv(fmt, pro, epi, bug=bug, **kw)
            b = A.check(got.to(F32).numpy(), ref.ref, ref.err, fmt)
            differs = got != clean
            assert b.flagged > 0, (fmt, epi, bug)
            if bug not in ("resid_before_round",):                        # (an unrounded store is flagged by the type rule wherever it is)
                assert not bool((b.bad & ~differs).any()), (fmt, epi, bug)
            oc4 = 4 * R // (2 if epi == A.EPI_SWIGLU else 1)               # output columns of one workgroup
            if bug == "two_ulp":
                assert b.flagged == 1 and b.rows == [M - 1] and b.cols == [5], (b.rows, b.cols)
            elif bug == "last_wg":
                n0 = (N - 1) // (4 * R) * (4 * R) // (2 if epi == A.EPI_SWIGLU else 1)
                assert b.cols and set(b.cols) <= set(range(n0, cols)) and len(b.cols) >= (cols - n0 + 1) // 2, (bug, b.cols, n0, oc4)
                assert len(b.rows) == M
            elif bug == "mb_row":
                assert b.rows == [2], (bug, b.rows)                        # row 2 of the tile alone took row 3's activation
                assert len(b.cols) >= (cols * 9) // 10
            elif bug == "norm_other_row":
                assert len(b.rows) == M, (bug, b.rows)
            elif bug == "resid_after_store":
                assert b.cols and set(b.cols) <= set(range(cols - 3, cols)), (bug, b.cols)
            elif bug in ("single_round", "resid_before_round"):
                assert len(b.rows) >= 1, bug
            elif bug in ("drop_piece", "twice_piece"):
                # 8 (4) of K terms: above half a step of the output only where the piece's share is large; M x N elements
                assert len(b.rows) >= 1 and len(b.cols) >= 1, (bug, b.rows, b.cols)
            else:                                                          # drop_bias, swap_gate_up: everywhere but the loud row
                assert len(b.rows) >= M - 1 and len(b.cols) >= (cols * 8) // 10, (bug, len(b.rows), len(b.cols))


# (M, N, K): MB = 4 in groups of 4 + 3 (NT 2, R 1); MB = 2 in groups of 2 + 2 + 1 (NT 4 takes no four-row tile)
TILE_CASES = [(7, 23, 520, 4), (5, 21, 1544, 2)]


@pytest.mark.parametrize("fmt", A.FMTS)
def test_checker_passes_the_honest_tiles_and_flags_each_tile_fault(fmt):
    """More rows than one tile: the emulation of ceil(M / MB) groups passes with no flag, the row behind row M - 1 unwritten;
    each fault of the split is flagged at the rows it moves and nowhere else.  gemv_mb_kernel exists in bf16 and fp16; an
    f32 launch is gemv_kernel with grid.y = M (MB = 0), which has no tile to get wrong: there the honest launch alone."""
    for M, N, K, MB in TILE_CASES:
        for pro, epi in ((1, A.EPI_STORE), (0, A.EPI_RESID)):
            x, W, gain, bias, resid = A.seeded_gemv_inputs(fmt, M, N, K, seed=17)
            kw = dict(x=x, W=W, gain=gain if pro else None, bias=bias, resid=resid if epi == A.EPI_RESID else None)
            ref = A.gemv_ref(fmt, pro, epi, **kw)
            assert A.want_id(fmt, epi, M, N, K)[0] == (0 if fmt == "f32" else MB)
            clean = A.emulate_gemv(fmt, pro, epi, tail=True, **kw)
            v = A.check(clean[:M].to(F32).numpy(), ref.ref, ref.err, fmt)
            assert v.checked == M * N and v.flagged == 0, (fmt, M, epi, v.rows, v.cols[:8])
            assert bool(torch.isnan(clean[M]).all()), "the honest launch stores nothing behind row M - 1"
            if fmt == "f32":
                continue
            src, dst = A.tile_rows(M, MB)
            assert len(src) == MB * -(-M // MB) and [d for d in dst if d >= 0] == list(range(M)) and dst.count(-1) == len(dst) - M
            assert all(s == min(i, M - 1) for i, s in enumerate(src))
            g_last = (M - 1) // MB * MB                                    # first row of the tail group
            want = {"tail_store": [], "tail_from_last": list(range(g_last, M - 1)), "group_prev": list(range(MB, M))}
            for bug, rows in want.items():
                got = A.emulate_gemv(fmt, pro, epi, bug=bug, tail=True, **kw)
                b = A.check(got[:M].to(F32).numpy(), ref.ref, ref.err, fmt)
                assert b.rows == rows, (fmt, M, MB, epi, bug, b.rows)
                assert not bool((b.bad & (got[:M] == clean[:M])).any()), (fmt, bug)
                if rows:
                    assert len(b.cols) >= (N * 9) // 10, (bug, len(b.cols))
                # the sentinel row: written by the fault that stores dead rows, by no other
                assert bool(torch.isnan(got[M]).all()) == (bug != "tail_store"), (fmt, M, bug)
            # (MB = 2, M = 5: the tail group's one live row IS row M - 1, so "tail_from_last" moves nothing there - by
            # construction, as the empty row list above says; at MB = 4, M = 7 it is rows 4 and 5)
    assert A.tile_rows(3, 0) == ([0, 1, 2], [0, 1, 2])


def test_dispatch_restated():
    """want_id over the issue's axes reaches exactly the set the dispatcher can pick."""
    seen = set()
    for fmt, Ks in (("bf16", (8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 3072, 3080, 4096, 4104, 6144)),
                    ("f32", (8, 248, 256, 264, 1024, 1032, 3072))):
        for K in Ks:
            for M in (1, 2, 3, 4):
                for N in (1, 3, 4, 5, 1024, 2047, 2048 // M, 16384, 65540):
                    seen.add(A.want_id(fmt, A.EPI_STORE, M, N, K))
    plain = {(0, R, nt) for R in (1, 2, 4) for nt in A.NT_OPTS}
    mb = {(MB, R, nt) for (R, MB) in ((1, 2), (1, 4), (2, 2), (2, 4)) for nt in ((1, 2, 4, 6) if MB == 2 else (1, 2))} | {(2, 4, 1), (2, 4, 2)}
    assert seen == plain | mb, (sorted(seen - plain - mb), sorted((plain | mb) - seen))
    # five rows and more (tests/test_ar_rows_gpu.py): gemv_mb_kernel<R, MB> for (1, 4), (1, 2), (2, 4), (2, 2), (4, 2) at the NT the
    # register rule allows, gemv_kernel<R> with grid.y = M for every other NT and for f32; R = 4 with NT > 2 is (0, 4, NT)
    for nt, K in ((4, 2048), (6, 3072)):
        assert A.want_id("bf16", A.EPI_STORE, 64, 1024, K) == (0, 4, nt) and A.want_id("bf16", A.EPI_STORE, 63, 1024, K) == (2, 2, nt)
    assert A.want_id("bf16", A.EPI_STORE, 64, 1024, 1024) == (2, 4, 2) and A.want_id("bf16", A.EPI_STORE, 63, 1024, 1024) == (4, 2, 2)
    assert A.want_id("bf16", A.EPI_STORE, 256, 256, 4096) == (0, 4, 8) and A.want_id("f32", A.EPI_STORE, 256, 256, 256) == (0, 4, 1)
    assert A.want_id("fp16", A.EPI_SWIGLU, 5, 6, 512) == (4, 2, 1) and A.want_id("bf16", A.EPI_SWIGLU, 5, 6, 2048) == (2, 2, 4)
    big = {A.want_id(f, A.EPI_STORE, M, N, K) for f, Ks in (("bf16", (512, 1024, 2048, 3072, 4096)), ("f32", (256, 1024, 3072)))
           for K in Ks for M in (5, 7, 63, 64, 256) for N in (1, 5, -(-2048 // M), -(-65536 // M), 1024)}
    assert big == ({(MB, R, nt) for MB, R in ((4, 1), (4, 2)) for nt in (1, 2)} | {(2, R, nt) for R in (1, 2) for nt in (4, 6)} |
                   {(2, 4, 1), (2, 4, 2), (0, 4, 4), (0, 4, 6)} | {(0, R, nt) for R in (1, 2, 4) for nt in (8, 1, 4, 12)}), sorted(big)
    assert A.pick_nt(6152, "bf16") < 0 and A.pick_nt(3080, "f32") < 0 and A.pick_nt(6144, "bf16") == 12


# ------------------------------------------------------------------------------------------------- decode attention
def _attn_inputs(fmt, M, H, Hkv, hd, n_slots, seed=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda t: A.store(t.to(F64), fmt).to(F32)
    qkv = r(torch.randn(M, (H + 2 * Hkv) * hd, generator=g))
    qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.0 + 0.1 * torch.randn(hd, generator=g))
    kc = A.wbits(torch.randn(M, Hkv, n_slots, hd, generator=g), fmt)
    vc = A.wbits(torch.randn(M, Hkv, n_slots, hd, generator=g), fmt)
    tab = O.rope_table(n_slots, hd, 1e6).to(F32)
    return qkv, qn, kn, kc, vc, tab


@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_checker_passes_the_honest_decode_attention_and_flags_each_fault(fmt):
    M, H, Hkv, hd, n_slots, ns = 4, 4, 2, 64, 264, 16
    qkv, qn, kn, kc, vc, tab = _attn_inputs(fmt, M, H, Hkv, hd, n_slots)
    pos = [0, 9, 128, 262]                            # 16 splits: row 0 leaves 15 ranges empty, row 1 six, row 2 one; cache rows >= pos are finite here
    ref = A.decode_attn_ref(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns)
    assert int((~ref.on).sum()) == (15 + 6 + 1) * H
    po, pml, k, kc1, vc1 = A.emulate_decode_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns)
    vp = A.check_parts(po, pml, ref)
    vk, v_ok, same = A.check_cache(fmt, kc, vc, kc1, vc1, pos, ref.k, ref.v)
    print(f"{fmt} decode attention: clean worst ratio partials {vp.worst:.3f}, k {vk.worst:.3f}, r_stage {ref.r_stage:.2e}")
    assert vp.flagged == 0 and vk.flagged == 0 and v_ok and same, (vp.where[:8], vk.rows)
    # faults of the attention launch: charged to the partials (row, head, split) or to the cache
    chunk = lambda p: (p + ns) // ns
    for bug, rows in (("miss_pos", [1, 2, 3]), ("stale_pos1", [0, 1, 2, 3])):
        po_b, pml_b, _, _, _ = A.emulate_decode_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns, bug=bug)
        b = A.check_parts(po_b, pml_b, ref)
        assert sorted({w[0] for w in b.where}) == rows, (bug, b.where[:8])
        for (m, h, s) in b.where:                                          # only the split whose range holds pos
            assert s == pos[m] // chunk(pos[m]), (bug, m, h, s)
    po_b, pml_b, _, _, _ = A.emulate_decode_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns, bug="empty_m0")
    b = A.check_parts(po_b, pml_b, ref)
    assert b.flagged == (15 + 6 + 1) * H and all(not bool(ref.on[w]) for w in b.where)
    _, _, _, kc_b, vc_b = A.emulate_decode_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns, bug="append_wrong_split")
    vk, v_ok, same = A.check_cache(fmt, kc, vc, kc_b, vc_b, pos, ref.k, ref.v)
    assert vk.rows == [0, 1, 2, 3] and not v_ok
    kc_b = kc1.copy(); kc_b[2, 1, 5, 7] = kc_b[2, 1, 5, 8]                              # another cache row touched
    assert not A.check_cache(fmt, kc, vc, kc_b, vc1, pos, ref.k, ref.v)[2]
    # faults of the merge inside the Wo launch: the partials are the honest ones, x_out is judged from them
    D = 24
    g = torch.Generator().manual_seed(5)
    r = lambda t: A.store(t.to(F64), fmt).to(F32)
    wo, bo, resid = r(0.05 * torch.randn(D, H * hd, generator=g)), r(0.1 * torch.randn(D, generator=g)), r(torch.randn(M, D, generator=g))

    def x_out(y):
        return A.emulate_gemv(fmt, 0, A.EPI_RESID, y.to(F32), wo, bias=bo, resid=resid)

    _, _, yr, er = A.merge_ref(po, pml, fmt)
    xr = A.gemv_ref(fmt, 0, A.EPI_RESID, yr, wo, bias=bo, resid=resid, dx_in=er)
    clean = x_out(A.emulate_merge(fmt, po, pml))
    v = A.check(clean.to(F32).numpy(), xr.ref, xr.err, fmt)
    print(f"{fmt} merge + wo: clean worst ratio {v.worst:.3f}")
    assert v.flagged == 0 and v.checked == M * D, (v.rows, v.cols)
    for bug in ("weight_one", "chunk2_twice"):
        b = A.check(x_out(A.emulate_merge(fmt, po, pml, bug=bug)).to(F32).numpy(), xr.ref, xr.err, fmt)
        # row 0 has one visible split: no second weight, no second chunk; rows 1..3 have 10, 15 and 16
        assert b.rows == [1, 2, 3] and len(b.cols) >= D // 2, (bug, b.rows, b.cols)
    # an empty split that came back with m = 0 shifts the merge's maximum: judged from the recorded partials the merge is
    # still right - the fault was charged to the attention above, not to the Wo launch
    xo_b = x_out(A.emulate_merge(fmt, po_b, pml_b))
    _, _, yr_b, er_b = A.merge_ref(po_b, pml_b, fmt)
    xr_b = A.gemv_ref(fmt, 0, A.EPI_RESID, yr_b, wo, bias=bo, resid=resid, dx_in=er_b)
    assert A.check(xo_b.to(F32).numpy(), xr_b.ref, xr_b.err, fmt).flagged == 0
    if fmt != "f32":
        b = A.check(_two_ulp(clean, 2, 7, fmt).to(F32).numpy(), xr.ref, xr.err, fmt)
        assert b.flagged == 1 and b.rows == [2] and b.cols == [7]


@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_merge_reading_another_rows_partials_is_flagged(fmt):
    """Seven rows, 16 splits: the merge of row m must read the partials at m H nsplit (hd).  Read at row m mod 4's offset, rows
    0..3 are right and rows 4, 5, 6 take the partials of rows 0, 1, 2: flagged there, in most columns, and nowhere else."""
    M, H, Hkv, hd, n_slots, ns, D = 7, 4, 2, 64, 264, 16, 24
    qkv, qn, kn, kc, vc, tab = _attn_inputs(fmt, M, H, Hkv, hd, n_slots, seed=8)
    pos = [0, 9, 128, 262, 40, 3, 200]
    ref = A.decode_attn_ref(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns)
    po, pml, _, kc1, vc1 = A.emulate_decode_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, ns)
    assert A.check_parts(po, pml, ref).flagged == 0
    vk, v_ok, same = A.check_cache(fmt, kc, vc, kc1, vc1, pos, ref.k, ref.v)
    assert vk.flagged == 0 and vk.checked == M * Hkv * hd and v_ok and same
    g = torch.Generator().manual_seed(6)
    r = lambda t: A.store(t.to(F64), fmt).to(F32)
    wo, bo, resid = r(0.05 * torch.randn(D, H * hd, generator=g)), r(0.1 * torch.randn(D, generator=g)), r(torch.randn(M, D, generator=g))
    _, _, yr, er = A.merge_ref(po, pml, fmt)
    xr = A.gemv_ref(fmt, 0, A.EPI_RESID, yr, wo, bias=bo, resid=resid, dx_in=er)
    x_out = lambda y: A.emulate_gemv(fmt, 0, A.EPI_RESID, y.to(F32), wo, bias=bo, resid=resid)
    v = A.check(x_out(A.emulate_merge(fmt, po, pml)).to(F32).numpy(), xr.ref, xr.err, fmt)
    assert v.flagged == 0 and v.checked == M * D, (v.rows, v.cols)
    b = A.check(x_out(A.emulate_merge(fmt, po, pml, bug="row_mod4")).to(F32).numpy(), xr.ref, xr.err, fmt)
    assert b.rows == [4, 5, 6] and len(b.cols) >= D // 2, (b.rows, b.cols)


# ------------------------------------------------------------------------------------------------- fast attention
@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_checker_passes_the_honest_fast_attention_and_flags_each_fault(fmt):
    M, H, Hkv, hd, ncb = 4, 4, 2, 64, 10
    g = torch.Generator().manual_seed(9)
    r = lambda t: A.store(t.to(F64), fmt).to(F32)
    qkv = r(2.0 * torch.randn(2 * M, (H + 2 * Hkv) * hd, generator=g))
    qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.3 + 0.1 * torch.randn(hd, generator=g))
    kc, vc = A.wbits(torch.randn(M, Hkv, ncb, hd, generator=g), fmt), A.wbits(torch.randn(M, Hkv, ncb, hd, generator=g), fmt)
    tab = O.rope_table(ncb, hd, 1e6).to(F32)
    for c in (0, 1, 2, ncb - 1):
        ref = A.fast_attn_ref(fmt, qkv[:M], c, qn, kn, kc, vc, tab, H, Hkv, hd)
        y, k = A.emulate_fast_attn(fmt, qkv[:M], c, qn, kn, kc, vc, tab, H, Hkv, hd)
        vy, vk = A.check(A.wbits(y, fmt), ref.y.ref, ref.y.err, fmt), A.check(A.wbits(k, fmt), ref.k.ref, ref.k.err, fmt)
        print(f"{fmt} fast attention c {c}: clean worst ratio y {vy.worst:.3f}, k {vk.worst:.3f}")
        assert vy.flagged == 0 and vk.flagged == 0 and vy.checked == M * H * hd
        if c > 0:                                                            # position c - 1's rotation: the appended key carries it too
            yb, kb = A.emulate_fast_attn(fmt, qkv[:M], c, qn, kn, kc, vc, tab, H, Hkv, hd, bug="rot_prev")
            b = A.check(A.wbits(yb, fmt), ref.y.ref, ref.y.err, fmt)
            assert A.check(A.wbits(kb, fmt), ref.k.ref, ref.k.err, fmt).rows == list(range(M))
            assert len(b.rows) >= M - 1, (c, b.rows)
    # the paired pass: position 0's block appends cache row 0, position 1's block rebuilds it from the position-0 row
    r0 = A.fast_attn_ref(fmt, qkv[:M], 0, qn, kn, kc, vc, tab, H, Hkv, hd)
    _, k0 = A.emulate_fast_attn(fmt, qkv[:M], 0, qn, kn, kc, vc, tab, H, Hkv, hd)
    kc1, vc1 = np.array(kc), np.array(vc)
    kc1[:, :, 0], vc1[:, :, 0] = A.wbits(k0, fmt), A.wbits(r0.v, fmt)
    ref1 = A.fast_attn_ref(fmt, qkv[M:], 1, qn, kn, kc1, vc1, tab, H, Hkv, hd)       # from the row as returned
    y1, _ = A.emulate_fast_attn(fmt, qkv[M:], 1, qn, kn, kc, vc, tab, H, Hkv, hd, k0_from=qkv[:M])
    assert A.check(A.wbits(y1, fmt), ref1.y.ref, ref1.y.err, fmt).flagged == 0
    y1b, _ = A.emulate_fast_attn(fmt, qkv[M:], 1, qn, kn, kc, vc, tab, H, Hkv, hd, k0_from=qkv[:M], bug="pair_no_kn")
    b = A.check(A.wbits(y1b, fmt), ref1.y.ref, ref1.y.err, fmt)
    assert len(b.rows) >= M - 1, b.rows
    if fmt != "f32":
        b = A.check(A.wbits(_two_ulp(y1, 1, 9, fmt), fmt), ref1.y.ref, ref1.y.err, fmt)
        assert b.flagged == 1 and b.rows == [1] and b.cols == [9]


def test_fast_attention_without_rb_d_is_flagged():
    """Dropping rb(d) moves a score only where the rounding of d scale lands elsewhere than that of rb(d) scale.  At head
    widths 16 and 64 the scale is a power of two and rb(d) changes nothing; at 128 (scale 2^-3.5) it shows over 4 rows x 4
    heads x 10 positions in bf16 with scores of a few units."""
    fmt, M, H, Hkv, hd, ncb, c = "bf16", 4, 4, 2, 128, 10, 9
    g = torch.Generator().manual_seed(21)
    r = lambda t: A.store(t.to(F64), fmt).to(F32)
    qkv = r(1.5 * torch.randn(M, (H + 2 * Hkv) * hd, generator=g))
    kc, vc = A.wbits(1.5 * torch.randn(M, Hkv, ncb, hd, generator=g), fmt), A.wbits(torch.randn(M, Hkv, ncb, hd, generator=g), fmt)
    tab = O.rope_table(ncb, hd, 1e6).to(F32)
    ref = A.fast_attn_ref(fmt, qkv, c, None, None, kc, vc, tab, H, Hkv, hd)
    y, _ = A.emulate_fast_attn(fmt, qkv, c, None, None, kc, vc, tab, H, Hkv, hd)
    assert A.check(A.wbits(y, fmt), ref.y.ref, ref.y.err, fmt).flagged == 0
    yb, _ = A.emulate_fast_attn(fmt, qkv, c, None, None, kc, vc, tab, H, Hkv, hd, bug="no_rb_d")
    b = A.check(A.wbits(yb, fmt), ref.y.ref, ref.y.err, fmt)
    assert b.flagged > 0 and not bool((b.bad & (yb == y)).any())


# ------------------------------------------------------------------------------------------------- embedding
def embed_case(fmt, D, ncb, M, seed=0):
    """Tables and tokens of the embedding tests (host and GPU): every token edge of the issue, codes -1 and cbsize."""
    vocab, cbsize, sb, se = 40, 6, 20, 30
    g = torch.Generator().manual_seed(seed + D + ncb)
    r = lambda t: A.store(t.to(F64), fmt).to(F32)
    emb, cbe = r(torch.randn(vocab, D, generator=g)), r(torch.randn(ncb * cbsize, D, generator=g))
    edge = [sb - 1, sb, se, se + 1, -1, vocab, 25, 3]
    toks = np.zeros((M, ncb + 1), dtype=np.int32)
    for m in range(M):
        toks[m, 0] = edge[m % len(edge)]
        toks[m, 1:] = torch.randint(0, cbsize, (ncb,), generator=g).numpy()
        toks[m, 1 + m % ncb] = -1 if m % 2 else cbsize
    return emb, cbe, toks, cbsize, sb, se


@pytest.mark.parametrize("fmt", ("bf16", "f32"))
def test_checker_passes_the_honest_embedding_and_flags_each_fault(fmt):
    D, ncb, M = 264, 10, 8
    emb, cbe, toks, cbsize, sb, se = embed_case(fmt, D, ncb, M)
    for scale in (True, False):
        ref = A.embed_ref(fmt, emb, cbe, toks, ncb, cbsize, sb, se, scale)
        x = A.emulate_embed(fmt, emb, cbe, toks, ncb, cbsize, sb, se, scale)
        v = A.check(x.to(F32).numpy(), ref.ref, ref.err, fmt)
        assert v.flagged == 0 and v.checked == M * D, (v.rows, v.cols)
        b = A.check(A.emulate_embed(fmt, emb, cbe, toks, ncb, cbsize, sb, se, scale, bug="vq_past_end").to(F32).numpy(), ref.ref, ref.err, fmt)
        assert b.rows == [3], b.rows                                           # the row whose token is sem_end + 1
        if scale:
            b = A.check(A.emulate_embed(fmt, emb, cbe, toks, ncb, cbsize, sb, se, scale, bug="scale_text").to(F32).numpy(), ref.ref, ref.err, fmt)
            assert b.rows == [0, 3, 4, 5, 7], b.rows                          # every text token
        b = A.check(_two_ulp(x, 0, 5, fmt).to(F32).numpy(), ref.ref, ref.err, fmt)  # row 0 is a copied text embedding
        assert b.flagged == 1 and b.rows == [0] and b.cols == [5]
