"""Pins tests/pf_ref.py on the CPU: (1) on oracle/ar.py's own intermediates of one bf16 prompt pass (one layer) every launch of
the restatement reproduces the oracle - bit for bit where float32 is exact (both norms, the q / k norm, the rotation, the
appended rows), otherwise with no element flagged and a stated, small count of boundary flips; (2) its checker passes an
honest float32 / bf16 emulation of the device's work split (K in 64-steps, 32-key tiles in NG groups with an online softmax
and the merge, P as two planes) with no element flagged and (3) flags each of fourteen emulated kernel faults at the right
rows and columns - the proof that tests/test_pf_kernels_gpu.py would fail if a prompt-pass kernel were subtly wrong."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

from oracle import ar as O
from tests import pf_ref as P
from tests.codec_stage_ref import F32, F64, h16_bits, half_ulp
from tests.shapes import make_prompt
from tests.test_ar_gpu import medium_shape

FMT = P.FMT


# ------------------------------------------------------------------------------------------------- pinned to the oracle
def test_restatement_reproduces_the_oracle_prompt_pass():
    """One 37-position prompt, one layer, bf16: norm, wqkv, append (q / k norm, RoPE, K / V rows), attention, wo + residual,
    norm, w13 + SwiGLU, w2 + residual - each on the oracle's own inputs of that launch.  A contraction accumulates in float32
    in the oracle and in float64 here, so an element within the accumulation error of a rounding boundary lands on the other
    neighbour: no element may be flagged, and the patterns that differ may be no more than the bound itself predicts (an error
    spread over [-err, err] crosses a boundary with probability err / (half a step), summed, plus three standard deviations;
    measured: 13 of 151 552 for wqkv, 25 of 75 776 for the attention, 2, 19 and 1 for wo, w13 and w2)."""
    shape = medium_shape(n_text=1009, n_layer=1)
    orc = O.AROracle(shape, O.random_weights(shape, seed=0, std=0.05), torch.bfloat16)
    prompt = make_prompt(shape, 37, seed=300, n_vq=2)
    T = prompt.shape[1]
    c, p, w = shape, "layers.0", orc.w
    H, Hkv, hd = c.n_head, c.n_local_heads, c.head_dim
    inp = prompt.view(1, c.num_codebooks + 1, -1)
    with torch.inference_mode(), sdpa_kernel(SDPBackend.MATH):
        logits, hidden = orc.slow_forward(inp, torch.arange(T))
        x = orc.embed(inp)
        xn = O.rms_norm(x, w[f"{p}.attention_norm.weight"], c.norm_eps)
        qkv = F.linear(xn, w[f"{p}.attention.wqkv.weight"])
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
    assert torch.equal(x2[:, -1:], hidden)                               # the intermediates above are the oracle's
    W = {n: t.to(F64) for n, t in w.items()}
    d = lambda t: t[0].to(F64)
    bits = lambda t: h16_bits(t, FMT)

    def contraction(name, ref, want):
        ver = P.check(bits(want), ref.ref, ref.err)
        differ = int((bits(ref.rnd) != bits(want)).sum())
        lam = float((ref.err / half_ulp(ref.ref.abs(), False, FMT)).clamp(max=1.0).sum())
        print(f"{name}: {differ} of {want.numel()} patterns differ (allowed {lam + 3 * lam ** 0.5 + 1:.0f}), "
              f"worst ratio {ver.worst:.3f}, r_stage {ref.r_stage:.2e}")
        assert ver.flagged == 0 and ver.checked == want.numel(), (name, ver.flagged, ver.rows[:8], ver.cols[:8])
        assert differ <= lam + 3 * lam ** 0.5 + 1, (name, differ, lam)

    # both norms: bit for bit
    assert np.array_equal(bits(P.norm_ref(d(x), W[f"{p}.attention_norm.weight"], c.norm_eps).rnd), bits(d(xn)))
    assert np.array_equal(bits(P.norm_ref(d(h), W[f"{p}.ffn_norm.weight"], c.norm_eps).rnd), bits(d(hn)))
    contraction("wqkv", P.linear_ref(P.WQKV, P.linear_pre(d(xn), W[f"{p}.attention.wqkv.weight"])), d(qkv))
    # the append: finished queries, K and V rows bit for bit
    app = P.append_ref(d(qkv), range(T), W[f"{p}.attention.q_norm.weight"], W[f"{p}.attention.k_norm.weight"], orc.tab, H, Hkv, hd, c.norm_eps)
    q_rows = q[0].transpose(0, 1).reshape(T, H * hd)
    assert np.array_equal(bits(app.q.rnd), bits(q_rows))
    assert np.array_equal(bits(app.k.rnd), bits(k[0].transpose(0, 1).reshape(T, Hkv * hd)))
    assert np.array_equal(bits(app.v), bits(v[0].transpose(0, 1).reshape(T, Hkv * hd)))
    # the attention on the oracle's queries and cache rows
    n_slots = 40
    kc, vc = np.full((1, Hkv, n_slots, hd), P.SENT16, dtype=np.uint16), np.full((1, Hkv, n_slots, hd), P.SENT16, dtype=np.uint16)
    kc[0, :, :T], vc[0, :, :T] = bits(k[0]), bits(v[0])
    a = P.attn_ref(bits(q_rows), kc, vc, [P.Seq(0, T, 0, 0)], 4, H, Hkv, hd)
    ydiff = int((bits(a.rnd) != bits(d(y))).sum())
    lam = float((a.err / half_ulp(a.ref.abs(), False, FMT)).clamp(max=1.0).sum())
    ver = P.check(bits(d(y)), a.ref, a.err)
    print(f"attention: {ydiff} of {a.ref.numel()} patterns differ (allowed {lam + 3 * lam ** 0.5 + 1:.0f}), worst ratio {ver.worst:.3f}")
    assert ver.flagged == 0 and ver.checked == T * H * hd, (ver.rows[:8], ver.cols[:8])
    assert ydiff <= lam + 3 * lam ** 0.5 + 1, (ydiff, lam)
    contraction("wo + residual", P.linear_ref(P.RESID, P.linear_pre(d(y), W[f"{p}.attention.wo.weight"]), resid=d(x)), d(h))
    w13 = P.WR.interleave_w13(W[f"{p}.feed_forward.w1.weight"], W[f"{p}.feed_forward.w3.weight"])
    contraction("w13 + swiglu", P.linear_ref(P.W13, P.linear_pre(d(hn), w13)), d(g))
    contraction("w2 + residual", P.linear_ref(P.RESID, P.linear_pre(d(g), W[f"{p}.feed_forward.w2.weight"]), resid=d(h)), d(x2))


# ------------------------------------------------------------------------------------------------- the checker: linear
# (form, S, N, K, row tile): every form; a ragged last row tile; K = 256 (one DEPTH round), 512 and 1024
LIN_CASES = [(P.WQKV, 150, 64, 256, 64), (P.RESID, 70, 64, 512, 64), (P.W13, 141, 64, 1024, 128)]
F32_STORE = (P.WQKV, P.RESID)


def _stored(form, v):
    """What the hook returns: float32 values for the two float32 forms, bf16 patterns for w13."""
    return v.to(F32).numpy() if form in F32_STORE else h16_bits(v, FMT)


def test_checker_passes_the_honest_linear_and_flags_each_linear_fault():
    for form, S, N, K, BM in LIN_CASES:
        X, W, bias, resid = P.seeded_linear_inputs(S, N, K, seed=7)
        kw = dict(bias=bias, resid=resid if form == P.RESID else None)
        ref = P.linear_ref(form, P.linear_pre(X, W), **kw)
        clean = P.emulate_linear(form, X, W, BM=BM, **kw)
        v = P.check(_stored(form, clean), ref.ref, ref.err)
        print(f"form {form} K {K}: clean worst ratio {v.worst:.3f}, r_stage {ref.r_stage:.2e}")
        assert v.checked == ref.ref.numel() and v.flagged == 0, (form, v.flagged, v.rows[:8], v.cols[:8])
        cols = ref.ref.shape[1]
        faults = ["last_tile_stale", "drop_kstep", "last_kstep_twice", "drop_bias", "two_ulp"]
        if form == P.RESID:
            faults.append("resid_after_round")
        if form == P.W13:
            faults.append("swap_gate_up")
        for bug in faults:
            if bug == "two_ulp":
                got = clean.clone()
                got[S - 1, 5] += 4 * half_ulp(got[S - 1, 5].abs(), False, FMT) * (1 if got[S - 1, 5] >= 0 else -1)
            else:
                got = P.emulate_linear(form, X, W, BM=BM, bug=bug, **kw)
            b = P.check(_stored(form, got), ref.ref, ref.err)
            assert b.flagged > 0, (form, bug)
            assert not bool((b.bad & (got == clean)).any()), (form, bug)         # never outside the elements the fault changed
            if bug == "two_ulp":
                assert b.flagged == 1 and b.rows == [S - 1] and b.cols == [5], (b.rows, b.cols)
            elif bug == "last_tile_stale":
                assert b.rows == list(range(S // BM * BM, S)), (bug, b.rows)      # every row of the last partial tile, no other
                assert len(b.cols) >= (cols * 9) // 10
            elif bug == "resid_after_round":
                # the unrounded sum is CLOSER to the reference than the rounded one: only the demand that a float32 store
                # holds a bf16 value sees it (the sum of two bf16 values of like magnitude is one itself about half the time)
                assert len(b.rows) == S and len(b.cols) == cols and b.flagged >= (S * cols) // 4, (bug, b.flagged)
            else:                      # a dropped or doubled K-step, the bias, gate and up: everywhere
                # (a 0.1 bias is below the bf16 step of the loud row's sums, which are 64 x larger)
                assert len(b.rows) >= S - 1 and len(b.cols) >= (cols * 9) // 10, (bug, len(b.rows), len(b.cols))


def test_norm_emulation_passes_and_a_neighbour_row_statistic_is_flagged():
    g = torch.Generator().manual_seed(5)
    x = P.round16(torch.randn(19, 1024, generator=g), FMT)
    x[3] *= 64.0
    gain = P.round16(1.0 + 0.1 * torch.randn(1024, generator=g), FMT)
    ref = P.norm_ref(x, gain, 1e-6)
    clean = P.emulate_norm(x, gain, 1e-6)
    v = P.check(h16_bits(clean, FMT), ref.ref, ref.err)
    assert v.flagged == 0 and v.checked == x.numel(), (v.rows, v.cols[:8])
    b = P.check(h16_bits(torch.roll(clean, 1, dims=0), FMT), ref.ref, ref.err)
    assert len(b.rows) == 19


# ------------------------------------------------------------------------------------------------- the checker: attention
H, HKV, HD, N_SLOTS, MB = 4, 2, 128, 328, 3
# two sequences in slots 2 and 0 (slot 1 unused): 161 rows behind a 31-row prefix (keys past 128, NG * 32 and 2 * NG * 32), 40 rows at pos0 = 3
SEQS = [P.Seq(0, 161, 31, 2), P.Seq(161, 40, 3, 0)]


def _attn_case():
    S = sum(s.rows for s in SEQS)
    qkv, qn, kn, kc, vc, tab = P.seeded_attn_inputs(S, H, HKV, HD, N_SLOTS, MB, seed=11)
    pos = [s.pos0 + i for s in SEQS for i in range(s.rows)]
    return qkv, qn, kn, kc, vc, tab, pos


@pytest.mark.parametrize("NG", (4, 2))
def test_checker_passes_the_honest_attention_and_flags_each_attention_fault(NG):
    qkv, qn, kn, kc, vc, tab, pos = _attn_case()
    app = P.append_ref(qkv, pos, qn, kn, tab, H, HKV, HD)
    q, kc1, vc1 = P.emulate_append(qkv, kc, vc, SEQS, qn, kn, tab, H, HKV, HD)
    vq = P.check(h16_bits(q, FMT), app.q.ref, app.q.err)
    cv = P.check_cache(kc, vc, kc1, vc1, SEQS, app, HKV, HD)
    assert vq.flagged == 0 and cv.k.flagged == 0 and cv.v_equal and cv.untouched, (vq.rows, cv.k.rows, cv.v_equal, cv.untouched)
    ref = P.attn_ref(h16_bits(q, FMT), kc1, vc1, SEQS, NG, H, HKV, HD)
    y = P.emulate_attn(q, kc1, vc1, SEQS, NG, H, HKV, HD)
    vy = P.check(h16_bits(y, FMT), ref.ref, ref.err)
    print(f"NG {NG}: clean worst ratio y {vy.worst:.3f}, q {vq.worst:.3f}, k {cv.k.worst:.3f}, r {ref.r_stage:.2e}")
    assert vy.flagged == 0 and vy.checked == y.numel() and bool(torch.isfinite(y).all()), (vy.flagged, vy.rows[:8])
    s0, s1 = SEQS
    rows0, rows1 = list(range(s0.rows)), list(range(s0.rows, s0.rows + s1.rows))
    want = {
        # hi alone carries 2^-9 of every probability: a few elements per row pass half a step + err, spread over the rows
        "drop_lo": None,
        # key pos0 + 128 exists only for rows at or behind it: sequence 0 from row 128 on, never sequence 1
        "miss_key_128": [r for r in rows0 if r >= 128],
        # a row loses its own key: every row (row 0 of sequence 1 at pos0 = 3 keeps three keys; a row with nothing visible is NaN)
        "mask_off_by_one": rows0 + rows1,
        # keys (row, pos0 + row] are lost: every row of both sequences (pos0 = 31 and 3)
        "mask_without_pos0": rows0 + rows1,
        # the last group's tiles: rows that see a key of tile NG - 1 (keys from 32 (NG - 1) on)
        "drop_group": [r for r in rows0 if s0.pos0 + r >= 32 * (NG - 1)] + [r for r in rows1 if s1.pos0 + (r - s0.rows) >= 32 * (NG - 1)],
        # slot w + 1: sequence 0 (slot 2 -> 0) reads sequence 1's rows and NaN behind them, sequence 1 (slot 0 -> 1) an unused slot: NaN
        "neighbour_slot": rows0 + rows1,
    }
    for bug, rows in want.items():
        yb = P.emulate_attn(q, kc1, vc1, SEQS, NG, H, HKV, HD, bug=bug)
        b = P.check(h16_bits(yb, FMT), ref.ref, ref.err)
        assert b.flagged > 0, (NG, bug)
        assert not bool((b.bad & (yb == y)).any()), (NG, bug)
        if rows is None:
            assert len(b.rows) >= (len(rows0) + len(rows1)) // 2, (bug, len(b.rows))
        else:
            assert b.rows == rows, (NG, bug, [r for r in rows if r not in b.rows][:8], [r for r in b.rows if r not in rows][:8])
    yb = y.clone()
    yb[170, 77] += 4 * half_ulp(yb[170, 77].abs(), False, FMT) * (1 if yb[170, 77] >= 0 else -1)
    b = P.check(h16_bits(yb, FMT), ref.ref, ref.err)
    assert b.flagged == 1 and b.rows == [170] and b.cols == [77]


def test_an_append_one_row_late_is_flagged():
    """The cache row written at pos + 1: every appended K row but the first of a sequence holds its predecessor, the first the
    NaN fill... and the row behind the sequence's end is no longer the fill."""
    qkv, qn, kn, kc, vc, tab, pos = _attn_case()
    app = P.append_ref(qkv, pos, qn, kn, tab, H, HKV, HD)
    _, kc1, vc1 = P.emulate_append(qkv, kc, vc, SEQS, qn, kn, tab, H, HKV, HD, bug="append_pos_plus_1")
    cv = P.check_cache(kc, vc, kc1, vc1, SEQS, app, HKV, HD)
    assert cv.k.rows == list(range(len(pos))) and not cv.v_equal and not cv.untouched
    # and the fill itself: a hook or kernel that clears a row it does not own
    _, kc2, vc2 = P.emulate_append(qkv, kc, vc, SEQS, qn, kn, tab, H, HKV, HD)
    kc2[1, 0, 7, 0] = 0
    assert not P.check_cache(kc, vc, kc2, vc2, SEQS, app, HKV, HD).untouched


def test_want_id_restates_the_dispatcher():
    assert [P.want_id(2, S, 1024, 1024) for S in (16, 17, 32, 33, 128, 129)] == [0, 1, 1, 2, 2, 4]
    assert P.want_id(2, 512, 1152, 1024) == P.ID_LIN128 and P.want_id(2, 512, 1024, 1024) == P.ID_LIN64
    assert P.want_id(2, 511, 2048, 256) == P.ID_LIN64 and P.want_id(2, 129, 1152, 192) == P.ID_TAP64_64
    assert P.want_id(2, 513, 1152, 192) == P.ID_TAP64_128 and P.want_id(1, 16, 1024, 1024) == P.ID_LIN64
    assert P.want_id(0, 16, 1024, 1024) == P.ID_TAP_128 and P.want_id(0, 129, 64, 1024) == P.ID_TAP_64
    assert P.want_id(2, 129, 64, 1024) == P.ID_TAP_64
