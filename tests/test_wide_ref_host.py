"""Pins tests/wide_ref.py on the CPU: (1) chained over one layer and the vocabulary head with its own rounded outputs it
IS the model (oracle/ar.py's bf16 and fp16 taps, bit for bit); (2) its checker passes an honest float32 / 16-bit emulation
of the lock-step kernels with no element flagged and flags every one of a list of subtle emulated kernel bugs at the
right rows and columns - the proof that tests/test_wide_kernels_gpu.py would fail if a kernel were subtly wrong."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

from oracle import ar as O
from tests import wide_ref as R
from tests.codec_stage_ref import F32, F64, h16_bits, half_ulp
from tests.shapes import make_prompt
from tests.test_ar_gpu import medium_shape

FMTS = ("bf16", "fp16")


def test_fp16_formats():
    m = torch.tensor([1.0, 1.999, 2.0, 0.75, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 0.0, 65504.0], dtype=F64)
    want = [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** 4]
    assert half_ulp(m, False, "fp16").tolist() == want
    assert half_ulp(torch.tensor([1.0, 3e-3], dtype=F64), False).tolist() == [2.0 ** -8, 2.0 ** -17]      # bf16 unchanged
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 65519.0, 65520.0, -1e6])
    assert h16_bits(x, "fp16").tolist() == [0x3C00, 0x3C00, 0x3C02, 0x0001, 0x0000, 0x0002, 0x7BFF, 0x7C00, 0xFC00]
    back = R.values(h16_bits(x, "fp16"), "fp16")
    assert back.tolist()[:6] == [1.0, 1.0, 1.0 + 2.0 ** -9, 2.0 ** -24, 0.0, 2.0 ** -23]
    assert R.values(h16_bits(x[:3], "bf16"), "bf16").tolist() == [1.0, 1.0, 1.0]
    r, e = R.reach(torch.tensor([1.0 + 2.0 ** -11, 1.25], dtype=F64), torch.tensor([1e-6, 1e-6], dtype=F64), "fp16")
    assert e.tolist() == [2.0 ** -10, 0.0]                                   # a boundary inside the interval: one step


# ------------------------------------------------------------------------------------------------- pinned to the oracle
@pytest.mark.parametrize("fmt", FMTS)
def test_restatement_reproduces_the_oracle_taps(fmt):
    """One prompt, one frame, one layer and the head: every launch of the restatement (fused norm + Wqkv, attention with
    the K / V append, Wo + residual, fused norm + W13 + SwiGLU, W2 + residual, final norm + head) on the oracle's own
    inputs of that launch, against what the oracle computed from them; the oracle's intermediates are rebuilt here from
    its functions and must end in its hidden-state and logit taps bit for bit.

    What is exact in float32 is reproduced bit for bit: both norms, the q / k norm, the rotation, the appended K and V
    rows and the attention output.  A contraction is not: the oracle's matmul accumulates in float32 and the restatement
    in float64, so an element whose sum lies within the accumulation error of a rounding boundary lands on the other
    neighbour (measured: 2 of 53 248 q k v elements in bf16, 121 in fp16).  For those launches the oracle's output must
    pass the checker with NO element flagged, and the patterns that differ must be no more than the bound itself
    predicts: an error spread over [-err, err] crosses a boundary with probability err / (half a step), summed over the
    elements, plus three standard deviations of that count."""
    dt = R.FMT_DT[fmt]
    shape = medium_shape(n_text=1009, n_layer=1)
    orc = O.AROracle(shape, O.random_weights(shape, seed=0, std=0.05), dt)
    prompt = make_prompt(shape, 13, seed=300, n_vq=2)
    T = prompt.shape[1]
    c, p, w = shape, "layers.0", orc.w
    H, Hkv, hd = c.n_head, c.n_local_heads, c.head_dim
    inp = prompt.view(1, c.num_codebooks + 1, -1)
    with torch.inference_mode(), sdpa_kernel(SDPBackend.MATH):          # the backend of the oracle's decode frames (AROracle._frames)
        logits, hidden = orc.slow_forward(inp, torch.arange(T))
        x = orc.embed(inp)
        qkv = F.linear(O.rms_norm(x, w[f"{p}.attention_norm.weight"], c.norm_eps), w[f"{p}.attention.wqkv.weight"])
        q, k, v = qkv.split([H * hd, Hkv * hd, Hkv * hd], dim=-1)
        tab = orc.tab[torch.arange(T)]
        q = O.rope(F.rms_norm(q.view(1, T, H, hd), (hd,), w[f"{p}.attention.q_norm.weight"], c.norm_eps), tab).transpose(1, 2)
        k = O.rope(F.rms_norm(k.view(1, T, Hkv, hd), (hd,), w[f"{p}.attention.k_norm.weight"], c.norm_eps), tab).transpose(1, 2)
        v = v.view(1, T, Hkv, hd).transpose(1, 2)
        y = F.scaled_dot_product_attention(q, k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1),
                                           attn_mask=orc.tril[None, None, torch.arange(T), :T])
        y = y.transpose(1, 2).contiguous().view(1, T, H * hd)
        h = x + F.linear(y, w[f"{p}.attention.wo.weight"])
        hn = O.rms_norm(h, w[f"{p}.ffn_norm.weight"], c.norm_eps)
        g = F.silu(F.linear(hn, w[f"{p}.feed_forward.w1.weight"])) * F.linear(hn, w[f"{p}.feed_forward.w3.weight"])
        x2 = h + F.linear(g, w[f"{p}.feed_forward.w2.weight"])
        lg = F.linear(O.rms_norm(x2[:, -1:], w["norm.weight"], c.norm_eps), w["embeddings.weight"])
    assert torch.equal(x2[:, -1:], hidden) and torch.equal(lg, logits)   # the intermediates above are the oracle's
    W = {n: t.to(F64) for n, t in w.items()}
    d = lambda t: t[0].to(F64)

    def contraction(name, ref, want):
        ver = R.check(h16_bits(want, fmt), ref.ref, ref.err, fmt)
        differ = int((h16_bits(ref.rnd, fmt) != h16_bits(want, fmt)).sum())
        lam = float((ref.err / half_ulp(ref.ref.abs(), False, fmt)).clamp(max=1.0).sum())
        print(f"{fmt} {name}: {differ} of {want.numel()} patterns differ (allowed {lam + 3 * lam ** 0.5 + 1:.0f}), "
              f"worst ratio {ver.worst:.3f}, r_stage {ref.r_stage:.2e}")
        assert ver.flagged == 0 and ver.checked == want.numel(), (name, ver.flagged, ver.rows[:8], ver.cols[:8])
        assert differ <= lam + 3 * lam ** 0.5 + 1, (name, differ, lam)

    contraction("norm + wqkv", R.linear_ref(fmt, R.STORE, d(x), W[f"{p}.attention.wqkv.weight"], W[f"{p}.attention_norm.weight"],
                                            eps=c.norm_eps), d(qkv))
    # the attention of every position on the oracle's cache rows: K, V and y bit for bit
    kc, vc = h16_bits(k, fmt), h16_bits(v, fmt)                         # [1, Hkv, T, hd]: rows < t are what position t reads
    for t in range(T):
        a = R.attn_ref(fmt, d(qkv)[t:t + 1], [t], W[f"{p}.attention.q_norm.weight"], W[f"{p}.attention.k_norm.weight"],
                       kc, vc, orc.tab, H, Hkv, hd, c.norm_eps)
        assert np.array_equal(h16_bits(a.k.rnd[0], fmt), kc[0, :, t]) and np.array_equal(h16_bits(a.v[0], fmt), vc[0, :, t]), t
        ydiff = int((h16_bits(a.y.rnd[0], fmt) != h16_bits(d(y)[t], fmt)).sum())
        lam = float((a.y.err / half_ulp(a.y.ref.abs(), False, fmt)).clamp(max=1.0).sum())
        assert R.check(h16_bits(d(y)[t:t + 1], fmt), a.y.ref, a.y.err, fmt).flagged == 0, t
        assert ydiff <= lam + 3 * lam ** 0.5 + 1, (t, ydiff, lam)   # the oracle's softmax sums in float32 (measured: 0 in bf16, <= 15 of 2048 in fp16)
    contraction("wo + residual", R.linear_ref(fmt, R.RESID, d(y), W[f"{p}.attention.wo.weight"], resid=d(x)), d(h))
    w13 = R.interleave_w13(W[f"{p}.feed_forward.w1.weight"], W[f"{p}.feed_forward.w3.weight"])
    contraction("norm + w13 + swiglu", R.linear_ref(fmt, R.SWIGLU, d(h), w13, W[f"{p}.ffn_norm.weight"], eps=c.norm_eps), d(g))
    contraction("w2 + residual", R.linear_ref(fmt, R.RESID, d(g), W[f"{p}.feed_forward.w2.weight"], resid=d(h)), d(x2))
    contraction("norm + head", R.linear_ref(fmt, R.STORE, d(x2)[-1:], W["embeddings.weight"], W["norm.weight"], eps=c.norm_eps), d(lg))
    # the fused norm alone is exact: round16(round16(x inv) gain) equals the oracle's rms_norm bit for bit
    t_ = d(h) * R.rms_inv(d(h), c.norm_eps)
    assert np.array_equal(h16_bits(R.round16(R.round16(t_, fmt) * W[f"{p}.ffn_norm.weight"][None], fmt), fmt), h16_bits(d(hn), fmt))


# ------------------------------------------------------------------------------------------------- the checker
# (epilogue, M, N, K, NW waves, TS): every epilogue, every K form, a TS = 2 class, a ragged last tile
LIN_CASES = [(R.STORE, 33, 64, 1024, 8, 2), (R.SWIGLU, 40, 64, 2048, 8, 2), (R.RESID, 17, 64, 3072, 12, 1)]


def _lin(fmt, epi, M, N, K, seed=7):
    X, W, gain, bias, resid = R.seeded_linear_inputs(fmt, M, N, K, seed)
    return dict(X=X, W=W, gain=None if epi == R.RESID else gain, bias=bias, resid=resid if epi == R.RESID else None)


@pytest.mark.parametrize("fmt", FMTS)
def test_checker_passes_the_honest_emulation_and_flags_each_linear_bug(fmt):
    for epi, M, N, K, NW, TS in LIN_CASES:
        kw = _lin(fmt, epi, M, N, K)
        ref = R.linear_ref(fmt, epi, **kw)
        clean = R.emulate_linear(fmt, epi, NW=NW, TS=TS, **kw)
        v = R.check(h16_bits(clean, fmt), ref.ref, ref.err, fmt)
        print(f"{fmt} epi {epi} K {K}: clean worst ratio {v.worst:.3f}, r_stage {ref.r_stage:.2e}, "
              f"ambiguous norm operands per row <= {0 if ref.amb is None else int(ref.amb.max())}")
        assert v.checked == ref.ref.numel() and v.flagged == 0, (epi, v.flagged, v.rows[:8], v.cols[:8])
        cols = ref.ref.shape[1]
        bugs = ["drop_wave", "drop_bias", "two_ulp"]
        if epi != R.RESID:
            bugs += ["norm_neighbour", "single_round"]
        if TS == 2:
            bugs.append("ts2_rows")
        if epi == R.SWIGLU:
            bugs.append("swap_gate_up")
        if epi == R.RESID:
            bugs.append("resid_after_store")
        for bug in bugs:
            if bug == "two_ulp":
                got = clean.clone()
                got[M - 1, 5] += 4 * half_ulp(got[M - 1, 5].abs(), False, fmt) * (1 if got[M - 1, 5] >= 0 else -1)
            else:
                got = R.emulate_linear(fmt, epi, NW=NW, TS=TS, bug=bug, **kw)
            b = R.check(h16_bits(got, fmt), ref.ref, ref.err, fmt)
            differs = (got != clean)
            assert b.flagged > 0, (fmt, epi, bug)
            # never outside the elements the bug changed
            assert not bool((b.bad & ~differs).any()), (fmt, epi, bug)
            if bug == "two_ulp":
                assert b.flagged == 1 and b.rows == [M - 1] and b.cols == [5], (b.rows, b.cols)
            elif bug == "ts2_rows":
                want = [m for m in range(M) if m % 32 >= 16]
                assert b.rows == want, (bug, b.rows)                            # every row of every second tile, no other
                assert len(b.cols) >= cols // 2
            elif bug == "norm_neighbour":
                assert len(b.rows) == M, (bug, b.rows)                           # row statistics differ by percents, the loud row's by 64 x
            elif bug == "resid_after_store":
                assert b.cols and set(b.cols) <= {8, 9, 10, 11}, (bug, b.cols)
                assert len(b.rows) >= M // 2
            elif bug == "single_round":
                assert len(b.rows) >= 1, bug                                     # a few double-rounding cases per launch
            else:                                                                # drop_wave, drop_bias, swap_gate_up: everywhere
                # (a 0.1 bias is below the bf16 step of the loud row's sums, which are 64 x larger)
                assert len(b.rows) >= M - 1 and len(b.cols) >= (cols * 9) // 10, (bug, len(b.rows), len(b.cols))


def _attn_inputs(fmt, M, H, Hkv, hd, n_slots, seed=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda t: R.round16(t.to(F32), fmt)
    qkv = r(torch.randn(M, (H + 2 * Hkv) * hd, generator=g))
    qn, kn = r(1.0 + 0.1 * torch.randn(hd, generator=g)), r(1.0 + 0.1 * torch.randn(hd, generator=g))
    kc = h16_bits(torch.randn(M, Hkv, n_slots, hd, generator=g), fmt)
    vc = h16_bits(torch.randn(M, Hkv, n_slots, hd, generator=g), fmt)
    tab = O.rope_table(n_slots, hd, 1e6).to(F32)
    return qkv, qn, kn, kc, vc, tab


@pytest.mark.parametrize("fmt", FMTS)
def test_checker_passes_the_honest_attention_and_flags_each_attention_bug(fmt):
    M, H, Hkv, hd, n_slots = 5, 4, 2, 128, 264
    qkv, qn, kn, kc, vc, tab = _attn_inputs(fmt, M, H, Hkv, hd, n_slots)
    pos = [0, 1, 128, 200, 263]                       # cache rows >= pos hold finite values here: a stale read then shows as a wrong number
    ref = R.attn_ref(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd)
    y, k = R.emulate_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd)
    vy, vk = R.check(h16_bits(y, fmt), ref.y.ref, ref.y.err, fmt), R.check(h16_bits(k, fmt), ref.k.ref, ref.k.err, fmt)
    print(f"{fmt} attention: clean worst ratio y {vy.worst:.3f}, k {vk.worst:.3f}")
    assert vy.flagged == 0 and vk.flagged == 0 and vy.checked == M * H * hd, (vy.rows, vk.rows)
    for bug, rows in (("miss_pos", [1, 2, 3, 4]), ("miss_128", [2, 3, 4]), ("stale_pos1", [0, 1, 2, 3])):
        yb, _ = R.emulate_attn(fmt, qkv, pos, qn, kn, kc, vc, tab, H, Hkv, hd, bug=bug)
        b = R.check(h16_bits(yb, fmt), ref.y.ref, ref.y.err, fmt)
        # (the emulation keeps the only position of row 0; a walk past the cache's last slot, row 4, has nothing to read)
        assert b.rows == rows, (fmt, bug, b.rows)
    yb = y.clone()
    yb[2, 77] += 4 * half_ulp(yb[2, 77].abs(), False, fmt) * (1 if yb[2, 77] >= 0 else -1)
    b = R.check(h16_bits(yb, fmt), ref.y.ref, ref.y.err, fmt)
    assert b.flagged == 1 and b.rows == [2] and b.cols == [77]


def test_check_overflow_rule():
    ref = torch.tensor([[70000.0, 65519.0, 65521.0, -70000.0, 60000.0]], dtype=F64)
    err = torch.full_like(ref, 4.0)
    inf = float("inf")
    ok = torch.tensor([[inf, 65504.0, inf, -inf, 60000.0]])
    assert R.check(h16_bits(ok, "fp16"), ref, err, "fp16").flagged == 0
    assert R.check(h16_bits(torch.tensor([[inf, inf, 65504.0, -inf, 60000.0]]), "fp16"), ref, err, "fp16").flagged == 0   # within err of the threshold: either
    bad = R.check(h16_bits(torch.tensor([[65504.0, 65504.0, inf, inf, inf]]), "fp16"), ref, err, "fp16")
    assert bad.cols == [0, 3, 4], bad.cols
