"""CPU: tests/draw_ref.py against itself and against the oracle.

1. Philox4x32-10 on its three published answers; the restatement equals oracle.ar.sample on the existing sampler cases.
2. An emulation of the device's work split (the bitwise search on order_key, the class histogram with its wrap and saturating
   recount, nk by bisection, ranks by index across 1024-chunks, four Philox draws per call) passes judge() with no flag.
3. Each planted fault is flagged at the row and the field where it was planted.
4. The inputs of tests/test_draw_kernels_gpu.py (tests/draw_cases.py) satisfy the band cap and the probe-validity caps on the reference alone."""
import numpy as np
import pytest
import torch

from oracle import ar as O
from tests import draw_ref as D
from tests.draw_cases import EDGES, family_cases, frames_used, launches, plan, rows_for, strict_q_row

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ emulation
def small_model(fmt, V=2319, fastV=1024, ncb=4, cap=64, MB=6, sem_begin=271, cbsize=None, seed=0, tab=False, xo=False):
    cbsize = cbsize or max(fastV, 1024)
    g = torch.Generator().manual_seed(seed)
    fe = torch.randn(cbsize, 16, generator=g).to(D.DT[fmt]).to(torch.float32).numpy()
    t = None
    if tab:
        t = D.bits16(torch.randn(fastV, 24, generator=g).numpy(), fmt if fmt != "f32" else "bf16")
    return D.DrawModel(fmt=fmt, V=V, fastV=fastV, ncb=ncb, cap=cap, sem_begin=sem_begin, im_end=260, cbsize=cbsize, fast_emb=fe,
                       MB=MB, xo_pair=16 if xo else 0, qkv0_tab=t)


def emu_row(model, cb, row, m, rows, path, fault):
    """One row as the device's work split computes it, in float32.  Returns (winner, logits left, cut record or None)."""
    fmt = model.fmt
    rbf = lambda x: D.rb(np.asarray(x, dtype=F32), fmt)
    V = model.width(cb)
    src = rows[0] if fault in ("ctl_row0", "nf_row0") and m == 1 else row
    ctl = src.ctl if fault == "ctl_row0" and m == 1 else row.ctl
    nf = src.nf if fault == "nf_row0" and m == 1 else row.nf
    L = np.array(row.logits, dtype=F32)
    ids = D.window_ids(row.hist, cb, nf, fault=fault)
    rep = F32(ctl.rep)
    if ids is not None:
        ids = [int(i) for i in ids if 0 <= i < V]
        pen = lambda s: rbf(s * rep) if s < 0 else rbf(s / rep)
        if fault == "scatter_first":
            for i in ids:
                L[i] = pen(L[i])
        else:
            vals = [pen(L[i]) for i in ids]
            for i, v in zip(ids, vals):
                L[i] = v
    ban_here = cb == 0 if fault != "ban_cb1" else cb in (0, 1)
    if ban_here and ctl.ban_eos and fault != "ban_ignored" and model.im_end < V:
        L[model.im_end] = -np.inf
    cmask = np.uint32(0xFFFF0000 if fmt == "bf16" else 0xFFFFFFFF)
    key = D.order_key(L) & cmask
    am = int(np.flatnonzero(L == L.max())[0])
    Lmax = L[am]
    with np.errstate(all="ignore"):
        ex = np.exp((L - Lmax).astype(F32)).astype(F32)
        Z = ex.sum(dtype=F32)
        prob = rbf(ex / Z)
        tp = rbf(F32(ctl.top_p))
        removed = lambda c: rbf(F32(c)) > tp
        kstar, nk, all_kept, cut = np.uint32(0), 0, False, None
        only_top = path != 2 and bool(removed(prob[am]))
        if not only_top:
            if path == 2:                                                # class histogram in packed u16 counters
                k16 = (key >> np.uint32(16)).astype(np.int64)
                cnt = np.bincount(k16, minlength=65536)
                packed = cnt % 65536
                if packed.sum() != V:                                    # a counter wrapped: saturating recount + side table
                    packed = np.minimum(cnt, 65535)
                    side = {int(k): int(cnt[k]) for k in np.flatnonzero(cnt >= 65535)}
                    assert len(side) <= 8
                    cnt = np.array([side.get(int(k), int(packed[k])) if packed[k] == 65535 else packed[k] for k in range(65536)])
                else:
                    cnt = packed
                occ = np.flatnonzero(cnt)[::-1]
                kv = (occ.astype(np.uint32) << np.uint32(16))
                vals = np.where(kv & np.uint32(0x80000000), kv & np.uint32(0x7FFFFFFF), ~(kv | np.uint32(0xFFFF))).astype(np.uint32).view(F32)
                pc = rbf(np.exp((vals - Lmax).astype(F32)).astype(F32) / Z)
                run, found = F32(0), None
                for i, k in enumerate(occ):
                    nxt = F32(F32(cnt[k]) * pc[i] + run)
                    if removed(nxt):
                        found = (int(k), run, int(cnt[k]), pc[i])
                        break
                    run = nxt
                if found is None:
                    all_kept = True
                else:
                    k, above, icnt, pk = found
                    lo_n, hi_n = 0, icnt
                    while lo_n < hi_n:
                        mid = (lo_n + hi_n + 1) >> 1
                        if removed(F32(F32(mid) * pk + above)):
                            hi_n = mid - 1
                        else:
                            lo_n = mid
                    if k == occ[0] and lo_n < 1 and fault != "rank0_dropped":
                        lo_n = 1
                    kstar, nk = np.uint32(k << 16), lo_n
            else:
                if not removed(prob.sum(dtype=F32)):
                    all_kept = True
                else:
                    for bit in range(31, 15 if fmt == "bf16" else -1, -1):
                        cand = kstar | np.uint32(1 << bit)
                        if removed(prob[key >= cand].sum(dtype=F32)):
                            kstar = cand
                    above, icnt = prob[key > kstar].sum(dtype=F32), int((key == kstar).sum())
                    ub = (kstar & np.uint32(0x7FFFFFFF)) if kstar & np.uint32(0x80000000) else ~(kstar | ~cmask)
                    pk = rbf(np.exp(np.array([ub], dtype=np.uint32).view(F32) - Lmax).astype(F32) / Z)[0]
                    lo_n, hi_n = 0, icnt
                    while lo_n < hi_n:
                        mid = (lo_n + hi_n + 1) >> 1
                        if removed(F32(F32(mid) * pk + above)):
                            hi_n = mid - 1
                        else:
                            lo_n = mid
                    nk = lo_n
        if fault == "nk_plus1" and not all_kept and not only_top:
            nk += 1
        member = (key == kstar) & (not all_kept)
        # ranks of the cut class by index, chunk by chunk of 1024 logits
        nchunk = (V + 1023) // 1024
        chunk_cnt = np.array([int(member[c * 1024:(c + 1) * 1024].sum()) for c in range(nchunk)])
        rank = np.zeros(V, dtype=np.int64)
        for c in range(nchunk):
            base = int(chunk_cnt[:c - 1].sum()) if fault == "chunk_base_prev" and c >= 1 else int(chunk_cnt[:c].sum())
            mc = member[c * 1024:(c + 1) * 1024]
            rank[c * 1024:(c + 1) * 1024] = base + np.cumsum(mc) - mc
        if fault == "ties_from_top":
            rank = np.where(member, int(member.sum()) - 1 - rank, rank)
        keep = np.ones(V, dtype=bool) if all_kept else (key > kstar) | (member & (rank < nk))
        if fault in ("cut_wide", "cut_narrow") and not all_kept and not only_top:
            order = np.lexsort((np.arange(V), -L.astype(np.float64)))
            n = int(keep.sum())
            if fault == "cut_wide" and n < V:
                keep[order[n]] = True
            if fault == "cut_narrow" and n > 1:
                keep[order[n - 1]] = False
        winner = am
        Tc = F32(ctl.temperature) if fault == "no_t_clamp" else max(F32(ctl.temperature), F32(1e-5))
        Mt = rbf(Lmax / Tc)
        if not only_top:
            et = np.where(keep, np.exp((rbf(L / Tc) - Mt).astype(F32)).astype(F32), F32(0))
            Z2 = et.sum(dtype=F32)
            p = np.where(keep, rbf(et / Z2), F32(0))
            if row.probe is not None or row.noise is not None:
                q = D.noise_of(model, cb, rows[0] if fault == "nf_row0" and m == 1 else row)
            else:
                q = D.draw_noise(V, cb, nf, ctl.seed, slot=m, fault=fault)
            if not (fault == "no_rb_q"):
                q = rbf(q)
            ratio = rbf(p / q)
            ratio = np.where(np.isnan(ratio), F32(-2), ratio)
            winner = int(np.argmax(ratio))
        if path == 2:
            cut = np.zeros(8, dtype=np.uint32)
            cut[0], cut[1], cut[2] = int(kstar) >> 16, nk, int(all_kept)
            cut[4:8] = np.array([Lmax, Mt, 0, Tc], dtype=F32).view(np.uint32)
            return winner, L, (cut, chunk_cnt)
    return winner, L, None


def emulate(model, cb, last, rows, fault=None, what_extra=0):
    V, R, cap, MB, M = model.width(cb), model.R, model.cap, model.MB, len(rows)
    path = 0 if V <= 1024 else 2 if model.fmt == "bf16" else 1
    S = D.SENT
    nchunk = (model.V + 1023) // 1024
    n_tab = 0 if model.qkv0_tab is None else model.qkv0_tab.shape[1]
    got = dict(tokn=np.full((MB, R), S, np.int32), tok=np.full((MB, R), S, np.int32), seq=np.full((MB, R, cap), S, np.int32),
               pos=np.full(MB, S, np.int32), nf=np.full(MB, S, np.int32), done=np.full(MB, S, np.int32),
               femb=np.full((MB, model.fast_emb.shape[1]), np.nan, F32).view(np.uint32) | np.uint32(0xFFFFFFFF),
               qkvf=np.full((32, max(n_tab, 8)), 0xFFFFFFFF, np.uint32).view(F32),
               xo_femb=np.full((2, 32, 8), 0xFFFF, np.uint16) if model.xo_pair else None,
               xo_x=np.full((2, 32, 8), 0xFFFF, np.uint16) if model.xo_pair else None,
               cut=np.full((MB, 8), 0xFFFFFFFF, np.uint32), chunk_cnt=np.full(MB * nchunk, -1, np.int32),
               part_idx=np.full(MB * nchunk, -1, np.int32), logits=np.full((MB, V), 0xFFFFFFFF, np.uint32).view(F32))
    got["femb"] = got["femb"].view(F32)
    what = path | what_extra
    ncl = (V + 1023) // 1024
    for m, row in enumerate(rows):
        got["seq"][m], got["pos"][m], got["nf"][m], got["done"][m] = row.hist, row.pos, row.nf, row.done
        w, L, cut = emu_row(model, cb, row, m, rows, path, fault)
        got["logits"][m] = L if path else row.logits
        if cut is not None:
            got["cut"][m] = cut[0]
            got["chunk_cnt"][m * ncl:(m + 1) * ncl] = cut[1]
            got["part_idx"][m * ncl:(m + 1) * ncl] = 0
        code = w
        tokn = got["tokn"][m]
        if cb == 0:
            tokn[0] = w
            code = w - model.sem_begin
            if fault != "no_clamp_lo":
                code = max(code, 0)
            if fault != "no_clamp_hi":
                code = min(code, model.cbsize - 1)
            tokn[1] = code
        else:
            tokn[cb + 1] = w
        src = w if fault == "femb_winner" and cb == 0 else code
        fe = model.fast_emb[src % model.cbsize]
        got["femb"][m] = fe
        if what & 4:
            got["xo_femb"][:, m, :] = D.bits16(fe, model.fmt).reshape(2, 8)
        if what & 8:
            got["xo_x"][:, model.xo_pair + m, :] = D.bits16(fe, model.fmt).reshape(2, 8)
        if what & 16:
            t = torch.from_numpy(model.qkv0_tab[code % model.fastV].view(np.int16).copy()).view(D.DT[model.fmt]).to(torch.float32).numpy()
            got["qkvf"].reshape(-1)[m * n_tab:(m + 1) * n_tab] = t
        if last:
            frozen = row.done != 0 and fault != "frozen_advanced"
            got["tok"][m] = tokn
            col = row.nf + 1 if fault == "seq_nf_plus1" else row.nf
            if (col < cap or (fault == "seq_at_cap" and col == cap)) and not frozen:
                got["seq"][m].reshape(-1)[np.arange(R) * cap + col if col < cap else np.arange(R - 1) * cap + col] = tokn[:R if col < cap else R - 1]
            if not frozen:
                got["pos"][m] += 1
                got["nf"][m] = row.nf + 1
                if tokn[0] == model.im_end and fault != "done_not_set":
                    got["done"][m] = 1
    got["what"] = what
    return got


# ------------------------------------------------------------------------------------------------------------ helpers
def rows_of_config(model, cb, logits, ctl, nf0, seed=0, ids=None, extra=()):
    """The probes of one configuration as the rows of launches: nf distinct (nf0, nf0 + 1, ...), every row's history block laid
    out so that its window holds the same ids."""
    g = np.random.default_rng(seed)
    filler = D.random_hist(model, seed)
    n_ids = model.R if cb == 0 else 16
    if ids is None:
        ids = D.pick_ids(np.asarray(logits), n_ids, ctl.top_p, g)
    base = D.Row(logits=logits, ctl=ctl, nf=max(nf0, 1), hist=D.hist_for(model, cb, max(nf0, 1), ids, filler))
    base.ref = D.reference(model, cb, base)
    rows, left = [], 0
    probes = D.probe_list(model, base.ref, base, cb)
    nf = max(nf0, 1)
    for kind, j in probes:
        if not D.probe_valid(model, base.ref, j):
            left += 1
            continue
        while nf in extra:
            nf += 1
        rows.append(D.Row(logits=logits, ctl=ctl, nf=nf, hist=D.hist_for(model, cb, nf, ids, filler), probe=j, tag=kind, ref=base.ref))
        nf += 1
    return rows, left, len(probes)


def flags_of(model, cb, last, rows, fault=None, **kw):
    fl = []
    for i in range(0, len(rows), model.MB):
        part = rows[i:i + model.MB]
        fl += [(i + f.row if f.row >= 0 else -1, f.field, f.msg) for f in D.judge(model, cb, last, part, emulate(model, cb, last, part, fault, **kw))]
    return fl


def ctl(i, **kw):
    tp, T, rep = D.CONTROLS[i]
    return D.Ctl(top_p=tp, temperature=T, rep=rep, **kw)


# ------------------------------------------------------------------------------------------------------------ pins
def test_philox_known_answers():
    hx = lambda w: [f"{int(x):08x}" for x in w]
    assert hx(D.philox4(0, 0, 0, 0, 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert hx(D.philox4(f, f, f, f, f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hx(D.philox4(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    i = np.arange(11, dtype=np.uint32)
    four = np.stack(D.philox4(i >> 2, 3, 5, 0, 7, 9), axis=-1)[np.arange(11), i & 3]
    assert np.array_equal(D.philox_word(i, 3, 5, 0, 7, 9), four)
    q = D.draw_noise(11, 3, 5, (9 << 32) | 7)
    assert np.array_equal(q, D.exp1_from_word(four)[0]) and q.dtype == np.float32 and (q > 0).all()
    assert D.exp1_from_word(np.array([0xFFFFFFFF], dtype=np.uint32))[0][0] == np.float32(1e-30)


@pytest.mark.parametrize("fmt", ["bf16", "fp16", "f32"])
def test_restatement_equals_the_oracle_on_the_sampler_cases(fmt):
    """The cases of test_sampling_kernel_vs_oracle: same penalised row, kept set = probs > 0 wherever the band is empty (else
    the oracle's count lies in the band), and the same winner under the same noise."""
    dt = D.DT[fmt]
    model = small_model(fmt, V=2319, fastV=1024, ncb=10, cap=32)
    g = torch.Generator().manual_seed(11)
    n_empty = 0
    for trial in range(24):
        cb = 0 if trial % 3 == 0 else 1 + trial % 9
        V = model.width(cb)
        logits = (D.SPREADS[trial % 4] * torch.randn(V, generator=g)).to(dt)
        if trial % 5 == 0:
            logits[torch.randint(0, V, (3,), generator=g)] = logits.max()
        window = torch.randint(0, 1024, (11, 16), generator=g).int()
        window[:, :4] = 0
        window[0] = torch.randint(0, 2319, (16,), generator=g).int()
        q = torch.empty(V).exponential_(1.0, generator=g).clamp_min_(1e-6)
        hist = np.zeros((11, 32), dtype=np.int32)
        hist[:, 1:17] = window.numpy()
        for tp, T, rep in D.CONTROLS:
            prev = window[:, 0] if cb == 0 else window[cb + 1]
            lg = logits.clone()
            want, probs = O.sample(lg[None, None], torch.tensor(T), torch.tensor(tp), torch.tensor(rep), prev, noise=lambda p: q.to(p.dtype))
            row = D.Row(logits=logits.float().numpy(), ctl=D.Ctl(tp, T, rep), nf=1, hist=hist, noise=q.numpy())
            try:
                ref = row.ref = D.reference(model, cb, row)
            except D.BandTooWide:                                          # an input the band rule does not admit
                continue
            assert np.array_equal(ref.after.view(np.uint32), lg.float().numpy().view(np.uint32)), "penalised row"
            assert np.array_equal(ref.ref_probs, probs.double().numpy())
            at1 = O.logits_to_probs(torch.from_numpy(ref.after).to(dt), torch.tensor(1.0), torch.tensor(tp), torch.tensor(1.0)).double().numpy()
            kept = at1 > 0
            if at1[ref.order[ref.n_ref - 1]] > 0:                           # nothing kept underflows at T = 1
                assert kept.sum() == ref.n_ref
            assert ref.lo <= ref.n_ref <= ref.hi
            assert np.array_equal(np.sort(ref.probs), np.sort(ref.ref_probs))
            if ref.band == 0 and not ref.one_sided and kept.sum() == ref.n_ref:
                n_empty += 1
                tied_cut = ref.hi < V and ref.after[ref.order[ref.hi]] == ref.after[ref.order[ref.hi - 1]]
                if not tied_cut:
                    assert np.array_equal(ref.rank_of < ref.n_ref, kept)
                    assert np.array_equal(ref.probs, ref.ref_probs)
            t = D.Tally()
            w = int(want.item())
            assert D.expect_winner(model, cb, row, w, t) is None or logits[w] == logits[int(np.argmax(ref.probs / q.to(dt).double().numpy()))]
    assert n_empty > 40


# ------------------------------------------------------------------------------------------------------------ emulation
CASES = [("bf16", 0, 2319), ("bf16", 0, 155776), ("fp16", 0, 2319), ("f32", 0, 2319), ("bf16", 1, 1024), ("fp16", 2, 1021), ("f32", 3, 65)]


@pytest.mark.parametrize("fmt,cb,V", CASES)
def test_clean_emulation_has_no_flag(fmt, cb, V):
    model = small_model(fmt, V=V if cb == 0 else 2319, fastV=1024 if cb == 0 else V, MB=5, xo=fmt != "f32", tab=fmt != "f32")
    n = 0
    for ci in range(len(D.CONTROLS)):
        variant = ("plain", "top3", "cut40", "big" if V > 70000 else "plain", "plain")[ci]
        for k in range(4):                                                   # the first spread whose band the cap admits
            lg = D.family_logits(fmt, V, D.SPREADS[(ci + k) % 4], 100 + ci, variant, D.CONTROLS[ci][0])
            try:
                rows, left, total = rows_of_config(model, cb, lg, ctl(ci, ban_eos=ci % 2 == 0), nf0=(1, 2, 17, 18, 16)[ci], seed=ci)
                break
            except D.BandTooWide:
                assert k < 3
        extra = 0 if fmt == "f32" else (8 if cb == 0 else 4 | (16 if cb + 1 < model.ncb else 0))
        fl = flags_of(model, cb, ci % 2 == 1, rows, what_extra=extra)
        assert not fl, fl[:4]
        n += len(rows)
    assert n >= 20
    # the counter-based generator, every row its own seed and frame
    lg = D.family_logits(fmt, V, 8.0 if V > 70000 else 1.0, 7)
    rows = []
    for i in range(10 if V > 70000 else 40):
        r = D.Row(logits=lg, ctl=ctl(0, seed=(0x9E3779B9 + i << 32) | (i * 77 + 1)), nf=i * 3 % 31, hist=D.random_hist(model, i))
        try:
            r.ref = D.reference(model, cb, r)
        except D.BandTooWide:
            continue
        rows.append(r)
    assert len(rows) >= 5 and not flags_of(model, cb, False, rows)


def planted(model, cb, fault, rows, last=False, **kw):
    assert not flags_of(model, cb, last, rows, **kw), "the clean emulation is flagged"
    return flags_of(model, cb, last, rows, fault, **kw)


@pytest.mark.parametrize("fmt,V", [("bf16", 2319), ("fp16", 2319), ("f32", 2319), ("bf16", 1024)])
@pytest.mark.parametrize("fault,kind", [("cut_wide", "first must-drop"), ("cut_narrow", "last must-keep"), ("nk_plus1", "first must-drop"),
                                        ("ties_from_top", "cut class, highest member")])
def test_kept_set_faults_are_flagged_at_their_probe(fmt, V, fault, kind):
    cb = 0 if V > 1024 else 1
    model = small_model(fmt, V=2319, fastV=min(V, 1024), MB=6)
    for seed in range(5, 25):                                                # the first input the band rule admits with a straddled class
        lg = D.family_logits(fmt, V, 3.0, seed, "cut40", 0.8)
        try:
            rows, _, _ = rows_of_config(model, cb, lg, ctl(0), nf0=3)
        except D.BandTooWide:
            continue
        kinds = [r.tag for r in rows]
        if "cut class, highest member" in kinds:
            break
    fl = planted(model, cb, fault, rows)
    hit = {rows[r].tag for r, f, _ in fl if f == "winner"}
    assert hit and all(f == "winner" or (f == "cut" and fmt == "bf16") for _, f, _ in fl), fl
    if fault == "ties_from_top":                                           # the last must-keep rank IS the class's last kept member
        assert "cut class, highest member" in kinds and hit & {"cut class, highest member", "last must-keep"}, (hit, kinds)
    elif ref_band_allows(rows, fault):
        assert kind in hit or any(k.startswith("cut class") for k in hit), (hit, kinds)


def ref_band_allows(rows, fault):
    """A one-rank fault is visible only if the band is empty at that side (a free rank may go either way)."""
    return rows[0].ref.band == 0


def test_chunk_rank_base_and_rank0():
    """Rank base of chunk c taken from chunk c - 1: the tied class spans chunks, the count kept lands on other members; rank 0
    dropped when p_0 > top_p (the large draw's forced nk = 1)."""
    model = small_model("bf16", V=4097, MB=6)
    lg = D.family_logits("bf16", 4097, 3.0, 9, "plain")
    v = np.sort(lg)[::-1][30]
    lg[[5, 1030, 1040, 2050, 2060, 3070, 4096]] = v                        # a cut class over all five chunks
    tp = float(np.cumsum(np.sort(np.exp(lg.astype(np.float64) - lg.max()) / np.exp(lg.astype(np.float64) - lg.max()).sum())[::-1])[33])
    rows, _, _ = rows_of_config(model, 0, lg, D.Ctl(tp, 1.0, 1.0), nf0=1, ids=np.full(5, 4000))
    fl = planted(model, 0, "chunk_base_prev", rows)
    assert fl and {f for _, f, _ in fl} <= {"winner"}, fl
    lg2 = D.family_logits("bf16", 4097, 8.0, 10)
    rows, _, _ = rows_of_config(model, 0, lg2, D.Ctl(1e-6, 0.7, 1.0), nf0=1, ids=np.full(5, 4000))
    fl = planted(model, 0, "rank0_dropped", rows)
    assert fl and {f for _, f, _ in fl} <= {"winner", "cut"} and any(rows[r].tag in ("argmax", "last must-keep") for r, f, _ in fl if f == "winner"), fl


@pytest.mark.parametrize("fmt", ["bf16", "fp16", "f32"])
@pytest.mark.parametrize("fault", ["scatter_first", "window_early", "window15", "window_row", "ban_ignored", "ban_cb1"])
def test_penalty_and_ban_faults(fmt, fault):
    """cb = 0 on 2319 logits (the block and the large draw leave the penalised row behind: field `logits`) for the faults that
    exist there; cb = 1 (sample_small_kernel writes nothing back: only the probes see it) for the 16-id window and the ban."""
    cb = 1 if fault in ("window15", "window_row", "ban_cb1") else 0
    V = 2319 if cb == 0 else 1024
    model = small_model(fmt, V=2319, fastV=1024, MB=6)
    lg = D.family_logits(fmt, V, 1.0, 3)
    lg[260] = np.float32(lg.max())                                            # im_end would otherwise rarely matter
    rows, _, _ = rows_of_config(model, cb, lg, D.Ctl(0.8, 0.7, 1.5, ban_eos=True), nf0=20, seed=4)
    fl = planted(model, cb, fault, rows)
    assert fl, fault
    fields = {f for _, f, _ in fl}
    assert fields <= {"winner", "logits", "cut"}, fl
    if cb == 0:
        assert "logits" in fields
    else:
        tags = {rows[r].tag for r, f, _ in fl if f == "winner"}
        assert tags & {"penalised id", "banned im_end", "argmax", "last must-keep", "first must-drop"}, tags


def test_temperature_clamp_and_q_rounding():
    model = small_model("bf16", V=2319, MB=6)
    lg = D.family_logits("bf16", 2319, 3.0, 2)
    rows, _, _ = rows_of_config(model, 0, lg, D.Ctl(0.8, 0.0, 1.1), nf0=1)
    fl = planted(model, 0, "no_t_clamp", rows)
    assert fl and {f for _, f, _ in fl} <= {"winner", "cut"}, fl
    # rb(q) dropped: two tied logits, q within half a bf16 step of each other -> equal after rounding, the lower index wins
    for fmt in ("bf16", "fp16"):
        model = small_model(fmt, V=2319, MB=6)
        rows = [strict_q_row(model, fmt)]
        fl = planted(model, 1, "no_rb_q", rows)
        assert [(r, f) for r, f, _ in fl] == [(0, "winner")], fl


@pytest.mark.parametrize("fault", ["philox_slot", "philox_no_cb", "philox_no_hi", "philox_perm"])
def test_philox_faults(fault):
    model = small_model("f32", V=2319, MB=6)
    lg = D.family_logits("f32", 1024, 1.0, 1)
    rows = []
    for i in range(12):
        r = D.Row(logits=lg, ctl=D.Ctl(1.0, 1.0, 1.0, seed=((i + 1) << 32) | (i + 5)), nf=i * 61, hist=D.random_hist(model, i))
        r.ref = D.reference(model, 2, r)
        rows.append(r)
    model.cap = 1024
    for r in rows:
        r.hist = np.zeros((model.R, model.cap), dtype=np.int32)
    fl = planted(model, 2, fault, rows)
    hit = sorted({r for r, f, _ in fl if f == "winner"})
    assert len(hit) >= 6 and {f for _, f, _ in fl} == {"winner"}, fl
    if fault == "philox_slot":
        assert all(r % model.MB != 0 for r in hit), hit                       # slot 0 is the counter's own zero


@pytest.mark.parametrize("fault", ["ctl_row0", "nf_row0"])
def test_a_row_reading_its_neighbour(fault):
    model = small_model("bf16", V=2319, MB=6)
    lg = D.family_logits("bf16", 1024, 3.0, 6)
    a, _, _ = rows_of_config(model, 1, lg, D.Ctl(0.2, 1.0, 1.5), nf0=2, seed=1)
    b, _, _ = rows_of_config(model, 1, lg, D.Ctl(0.95, 0.7, 1.1), nf0=20, seed=2, extra={r.nf for r in a})
    first = next(r for r in b if r.tag == "last must-keep")
    rows = [a[0], first] + a[1:5]
    fl = planted(model, 1, fault, rows)
    assert fl and {r for r, _, _ in fl} == {1}, fl


@pytest.mark.parametrize("fault,field", [("no_clamp_hi", "tokn"), ("no_clamp_lo", "tokn"), ("femb_winner", "femb"), ("frozen_advanced", "seq"),
                                         ("seq_nf_plus1", "seq"), ("done_not_set", "done"), ("seq_at_cap", "seq")])
def test_bookkeeping_faults(fault, field):
    """One launch with last = 1: a live row whose probe draws a code above the clamp, one that draws a text token (below), a
    frozen row, a row at nf = cap, a row that draws im_end."""
    model = small_model("bf16", V=4097, cbsize=1024, MB=6, xo=True)
    lg = D.family_logits("bf16", 4097, 1.0, 12)
    c = D.Ctl(1.0, 1.0, 1.0)
    filler = D.random_hist(model, 3)
    mk = lambda j, nf, done=0: D.Row(logits=lg, ctl=c, nf=nf, hist=filler.copy(), pos=40 + nf, done=done, probe=j)
    rows = [mk(4000, 3), mk(17, 4), mk(600, 5, done=1), mk(700, model.cap), mk(model.im_end, 6)]
    if fault == "seq_at_cap":                                              # the column behind the row's block is the next row's
        rows = [mk(700, model.cap), mk(600, 5)]
    for r in rows:
        r.ref = D.reference(model, 0, r)
        assert D.probe_valid(model, r.ref, r.probe)
    fl = planted(model, 0, fault, rows, last=True, what_extra=8)
    where = {"no_clamp_hi": 0, "no_clamp_lo": 1, "femb_winner": 0, "frozen_advanced": 2, "seq_nf_plus1": 0, "done_not_set": 4, "seq_at_cap": 0}[fault]
    assert (where, field) in {(r, f) for r, f, _ in fl}, fl
    if fault not in ("seq_nf_plus1", "femb_winner", "seq_at_cap", "no_clamp_hi", "no_clamp_lo"):
        assert {r for r, _, _ in fl} == {where}, fl


# ------------------------------------------------------------------------------------------------------------ input conditions
# Pinned, so that a spread dropping out of a kind of test is seen.  bf16 and f32 use all four wherever a test has five or more
# configurations; in fp16 the wide spreads lose to probe validity (probabilities below 3e-8 are 0 in fp16), not to the band.
ALL4 = [0.3, 1.0, 3.0, 8.0]
SPREADS_IN_USE = {("small", "bf16"): ALL4, ("small", "fp16"): ALL4, ("small", "f32"): ALL4, ("rows66", "bf16"): ALL4,
                  ("rows66", "fp16"): ALL4, ("rows66", "f32"): ALL4, ("semantic", "bf16"): ALL4,
                  ("semantic", "fp16"): [0.3, 3.0], ("semantic", "f32"): ALL4, ("block", "fp16"): [0.3, 1.0, 3.0], ("block", "f32"): ALL4,
                  ("block_real", "fp16"): [3.0, 8.0], ("block_real", "f32"): [3.0, 8.0], ("four", "bf16"): ALL4, ("wide", "bf16"): ALL4,
                  ("wide", "fp16"): [0.3, 1.0], ("wide6144", "bf16"): [1.0, 3.0, 8.0]}


def test_input_families_hold_their_caps():
    """Every probe test of the GPU file, on the very inputs it runs: the band cap and the normaliser condition (configs_for
    passes over a spread the reference does not admit and raises if none is left), at most 10 % of the probes invalid, at least
    one valid probe of each side, every frame edge reached by the launches, every control in use.  Which spreads a kind of test
    ends up with is asserted, so that one dropping out is seen: all four everywhere but at the real vocabulary in fp16 / f32
    (two configurations) and on the lock-step contexts (three per codebook); the exclusions are counted and printed (DESIGN.md
    section 2 quotes them)."""
    used, passed_over = {}, {}
    for name, model, parts in family_cases():
        kind, fmt, size = name.split(" ")
        total = left = 0
        kinds = set()
        for cb, configs, seed in parts:
            rows, t, l, filler = rows_for(model, cb, configs, seed)
            total, left = total + t, left + l
            kinds |= {r.tag for r, _ in rows}
            assert all(refs[nf].one_sided or refs[nf].band <= D.MAX_BAND for _, _, _, refs in configs for nf in (0, 1))
            assert {c.top_p for _, c, _, _ in configs} >= {tp for tp, _, _ in D.CONTROLS[:len(configs)]}, name
            for _, c, _, refs in configs:
                used.setdefault((kind, fmt), set()).add(refs["spread"])
                for sp, why in refs["skipped"]:
                    passed_over[(kind, fmt, size, c.top_p, sp, why)] = passed_over.get((kind, fmt, size, c.top_p, sp, why), 0) + 1
            parts_ = launches(model, cb, rows, plan(kind, fmt, None if size == "None" else int(size))[3], filler, seed)
            seen = frames_used(parts_)
            assert EDGES <= seen, (name, cb, sorted(EDGES - seen))
            if kind == "rows66":                                           # the plan is about its row counts: one launch of each size, every nf of a 66-row launch distinct
                assert model.MB == 66 and model.cap == 66 and [len(p) for p in parts_[:3]] == [66, 65, 5], (name, [len(p) for p in parts_])
                assert {model.cap - 1, model.cap} <= seen and all(len({r.nf for r in p}) == len(p) for p in parts_)
        assert left <= 0.1 * total, (name, left, total)
        assert {"last must-keep", "first must-drop"} <= kinds, (name, kinds)   # (the argmax probe is the last must-keep one where lo = 1)
    for key, n in sorted(passed_over.items()):
        print("passed over:", key, n)
    print("spreads in use:", {k: sorted(v) for k, v in used.items()})
    assert {k: sorted(v) for k, v in used.items()} == SPREADS_IN_USE
