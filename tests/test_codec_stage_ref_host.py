"""Pins tests/codec_stage_ref.py on the CPU: (1) chained freely in float64 it IS the codec (the oracle, and through it
the reference project's own output); (2) its checker passes an honest float32 / bf16 emulation of the device with zero
flagged elements and flags every one of a list of subtle emulated kernel bugs at the right stage and rows - the proof
that tests/test_codec_stages_gpu.py would fail if a kernel were subtly wrong."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import codec as C
from tests import codec_stage_ref as R
from tests.golden.make_golden_codec import tiny_codec_shape

G = os.path.join(os.path.dirname(__file__), "golden")


def encode_shape():
    """The shape of tests/test_codec_gpu.py's encode tests (smallest widths the MFMA tiles take)."""
    return C.CodecShape(n_codebooks=3, codebook_size=64, semantic_codebook_size=128, codebook_dim=8, latent_dim=512,
                        n_tf_layer=2, tf_n_head=8, tf_head_dim=64, tf_ffn=768, tf_window=8, tf_block_size=256,
                        upsample=[2, 2], decoder_dim=128, rates=[4, 4], encoder_dim=32, encoder_rates=[2, 2, 2, 2],
                        encoder_tf_layers=[0, 0, 1, 1], enc_tf_window=16, enc_tf_block_size=1024)


def rand_codes(shape, T, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.zeros(shape.n_codebooks + 1, T, dtype=torch.long)
    codes[0] = torch.randint(0, shape.semantic_codebook_size, (T,), generator=g)
    codes[1:] = torch.randint(0, shape.codebook_size, (shape.n_codebooks, T), generator=g)
    return codes


def test_audio(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n).float()
    return (0.4 * torch.sin(2 * np.pi * t / 37.0) + 0.2 * torch.randn(n, generator=g)).numpy()


test_audio.__test__ = False


def rel_rms(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def roundoff_bound(plan):
    """Distance allowed between the float64 chain and the float32 oracle.  One float32 contraction of n terms is off by
    at most n u relative to S (u = 2^-24), the other operations by a few u; the stages are in series and none amplifies
    a relative perturbation by more than O(1) (norms and LayerScale / ConvNeXt gammas of 0.1-0.2 keep the stack at unit
    scale), so the relative RMS distance is bounded by (number of launches) x (largest term count) x u - the worst case,
    linear in both; the measured distance (printed) is three orders of magnitude below it."""
    n_max = max(len(st.p["offs"]) * st.p["K"] for st in plan if st.kind == "gemm")
    return len(plan) * n_max * R.U


def test_free_chain_reproduces_the_oracle_decode_and_the_reference_golden():
    shape = tiny_codec_shape()
    w = C.random_weights(shape, seed=0)
    orc = C.CodecOracle(shape, w)
    gold = np.load(os.path.join(G, "codec_tiny.npz"))
    cases = [("b1", torch.from_numpy(gold["b1.codes"])[0], gold["b1.audio"][0, 0]),
             ("b2[1]", torch.from_numpy(gold["b2.codes"])[1], gold["b2.audio"][1, 0]),
             ("T=40", rand_codes(shape, 40, 9), None), ("T=1", rand_codes(shape, 1, 3), None)]
    for name, codes, golden in cases:
        plan = R.plan_decode(shape, codes)
        env = R.chain_free(plan, w)
        want, _ = orc.decode(codes[None], torch.tensor([codes.shape[1]]))
        bound = roundoff_bound(plan)
        d = rel_rms(env["audio"][:, 0], want[0, 0])
        print(f"decode {name}: float64 chain vs f32 oracle, relative RMS {d:.2e} (bound {bound:.2e})")
        assert env["audio"].shape == (codes.shape[1] * shape.frame_len, 1)
        assert d <= bound, (name, d, bound)
        if golden is not None:     # the oracle equals the golden file bit for bit (test_codec_oracle_golden.py)
            assert rel_rms(env["audio"][:, 0], golden) <= bound, name


def test_free_chain_reproduces_the_oracle_encode_taps():
    shape = encode_shape()
    w = C.random_weights(shape, seed=0)
    w.update(C.random_encoder_weights(shape, seed=1))
    orc = C.CodecOracle(shape, w)
    for frames, cut, seed in ((37, 11, 5), (61, 5, 12)):
        audio = test_audio(frames * shape.enc_frame_len - cut, seed)
        plan = R.plan_encode(shape, audio)
        env = R.chain_free(plan, w, keep=("enc.out",))
        orc.encode(torch.from_numpy(audio)[None, None])
        bound = roundoff_bound(plan)
        d_enc = rel_rms(env["enc.out"]["bf"], orc.taps["enc_out"][0].t())
        d_pre = rel_rms(env["zq"], orc.taps["pre"][0].t())
        print(f"encode {frames} frames: enc_out {d_enc:.2e}, pre {d_pre:.2e} (bound {bound:.2e})")
        assert env["zq"].shape == (frames, shape.latent_dim)
        assert d_enc <= bound and d_pre <= bound, (d_enc, d_pre, bound)


def test_select_rows_meets_the_stated_condition():
    for M, halo, bm in ((4095, 54, 128), (4096, 54, 128), (440320, 54, 256), (30001, 6, 128), (100000, 0, 64)):
        rows = R.select_rows(M, halo, bm, seed=1)
        s = set(rows.tolist())
        assert rows.tolist() == sorted(s) and min(s) >= 0 and max(s) < M
        if M < 4096:
            assert len(s) == M
            continue
        assert set(range(halo + 8)) <= s                                        # start-up padding
        assert set(range(((M - 1) // bm - 1) * bm, M)) <= s                     # the last two row tiles
        nb = (M - 1) // bm
        full = [b for b in range(1, nb + 1) if set(range(b * bm - 4, min(M, b * bm + 4))) <= s]
        assert len(full) >= 8, len(full)                                        # four rows either side of >= 8 boundaries
        assert len(s) >= 1024 + halo + 8
        assert R.select_rows(M, halo, bm, seed=1).tolist() == rows.tolist()     # fixed seed


def test_half_ulp():
    m = torch.tensor([1.0, 1.5, 1.999, 2.0, 0.75, 3e-3, 100.0], dtype=torch.float64)
    want = [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -17, 2.0 ** -2]
    assert R.half_ulp(m, f32=False).tolist() == want
    assert R.half_ulp(m, f32=True).tolist() == [x * 2.0 ** -16 for x in want]
    # the store the checker models rounds to nearest even
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20])
    assert R.from_raw(R.bf16_bits(x)).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]


# ------------------------------------------------------------------------------------------------ sensitivity
def flagged(verdicts):
    return {v.name: v for v in verdicts if v.flagged}


@pytest.fixture(scope="module")
def tiny():
    shape = tiny_codec_shape()
    w = C.random_weights(shape, seed=0)
    codes = rand_codes(shape, 40, 9)
    return shape, w, R.plan_decode(shape, codes)


def test_checker_passes_an_honest_emulation_with_zero_flagged_elements(tiny):
    shape, w, plan = tiny
    vs = R.check_trace(plan, R.chain_emulate(plan, w), w)
    assert len(vs) == len(plan) and all(v.checked == st.rows * st.cols * len(st.dst) for v, st in zip(vs, plan))
    assert not flagged(vs), [(v.name, v.flagged, v.worst) for v in flagged(vs).values()]
    print("emulated decode: largest |got - ref| / bound per kind:",
          {k: round(max(v.worst for v in vs if v.kind == k), 3) for k in sorted({v.kind for v in vs})})
    es = encode_shape()
    we = C.random_weights(es, seed=0)
    we.update(C.random_encoder_weights(es, seed=1))
    for frames, cut in ((37, 11), (6, 3)):
        eplan = R.plan_encode(es, test_audio(frames * es.enc_frame_len - cut))
        vs = R.check_trace(eplan, R.chain_emulate(eplan, we), we)
        assert not flagged(vs), [(v.name, v.flagged, v.worst) for v in flagged(vs).values()]


def scale_act(rows, cols, factor=1.25):
    """Emulated MFMA sub-tile bug: the stored values of `cols` in `rows` at `factor` (re-rounded to bf16)."""
    def f(outs):
        outs = {k: v.copy() for k, v in outs.items()}
        for k, a in outs.items():
            v = R.from_raw(a).clone()
            ri, ci = torch.tensor(rows)[:, None], torch.tensor(cols)[None, :]
            v[ri, ci] = v[ri, ci] * factor
            outs[k] = R.raw_store(k, v)
        return outs
    return f


def stage(plan, name):
    return next(st for st in plan if st.name == name)


def with_p(st, **kw):
    return dataclasses.replace(st, p={**st.p, **kw})


def test_checker_flags_stale_rows_in_place_of_the_causal_padding(tiny):
    """The final k = 7 convolution reads 6 stale rows (O(1) values left by an earlier decode) instead of zeros: a click
    in the first 6 samples, invisible to a whole-waveform relative RMS."""
    shape, w, plan = tiny
    g = torch.Generator().manual_seed(4)
    st = stage(plan, "final")
    stale = R.from_raw(R.bf16_bits(torch.randn(6, st.p["C"], generator=g) * 0.8))
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, override={"final": with_p(st, stale=stale)}), w))
    assert set(bad) == {"final"}, sorted(bad)
    assert bad["final"].rows and set(bad["final"].rows) <= set(range(6)) and 0 in bad["final"].rows, bad["final"].rows
    # the same in a dilated convolution's tap GEMM and in the depthwise convolution
    for name, halo in (("dec.0.u2.c7", 54), ("up.1.dwln", 6)):
        st = stage(plan, name)
        C_in = st.p["K"] if st.kind == "gemm" else st.cols
        stale = R.from_raw(R.bf16_bits(torch.randn(halo, C_in, generator=g) * 0.8))
        bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, override={name: with_p(st, stale=stale)}), w))
        assert set(bad) == {name}, sorted(bad)
        assert bad[name].rows and set(bad[name].rows) <= set(range(halo)) and 0 in bad[name].rows, bad[name].rows


def test_checker_flags_one_bad_sub_tile_per_row_tile(tiny):
    """16 output channels of one row in every 128 at 1.25x in one dilated convolution of block 0; then the same, one row
    in 64, in every k = 7 convolution: each is flagged at exactly those rows, and nothing else is."""
    shape, w, plan = tiny
    st = stage(plan, "dec.0.u1.c7")
    rows = list(range(5, st.rows, 128))
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, mutate={st.name: scale_act(rows, list(range(16, 32)))}), w))
    assert set(bad) == {st.name} and bad[st.name].rows == rows, {k: v.rows for k, v in bad.items()}
    c7 = [s for s in plan if s.name.endswith(".c7") or s.name == "dec.in"]
    mut = {s.name: scale_act(list(range(9, s.rows, 64)), list(range(0, 16))) for s in c7}
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, mutate=mut), w))
    assert set(bad) == {s.name for s in c7}, sorted(bad)
    for s in c7:
        assert bad[s.name].rows == list(range(9, s.rows, 64)), s.name


def test_checker_flags_an_attention_window_off_by_one(tiny):
    shape, w, plan = tiny
    st = stage(plan, "post.1.attn")
    bugged = with_p(st, window=st.p["window"] - 1)
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, override={st.name: bugged}), w))
    assert set(bad) == {st.name}, sorted(bad)
    first = st.p["window"] - 1                                  # rows below it see the same keys either way
    assert bad[st.name].rows and min(bad[st.name].rows) >= first, bad[st.name].rows
    assert len(bad[st.name].rows) >= (st.rows - first) * 3 // 4, len(bad[st.name].rows)


def test_checker_flags_a_dropped_tap_a_dropped_bias_and_two_ulp(tiny):
    shape, w, plan = tiny
    st = stage(plan, "dec.1.u2.c7")                             # dilation 9
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, override={st.name: with_p(st, drop_tap=2)}), w))
    assert set(bad) == {st.name} and len(bad[st.name].rows) > st.rows // 2
    st = stage(plan, "dec.1.u0.c1")                             # a 1x1 convolution
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, override={st.name: with_p(st, drop_bias=True)}), w))
    assert set(bad) == {st.name} and len(bad[st.name].rows) > st.rows // 2
    # one stored element two bf16 ulp off (same binade)
    for name, kind in (("dec.0.u0.c1", "bf"), ("up.0.pw1", "bf"), ("dec.1.u1.c7", "act")):
        st = stage(plan, name)

        def two_ulp(outs, kind=kind, st=st):
            outs = {k: v.copy() for k, v in outs.items()}
            a = outs[kind]
            r, c = st.rows // 3, st.cols // 2
            assert (int(a[r, c]) & 0x7F) < 0x7D                 # stays in its binade
            a[r, c] += 2
            return outs
        bad = flagged(R.check_trace(plan, R.chain_emulate(plan, w, mutate={name: two_ulp}), w))
        assert set(bad) == {name} and bad[name].flagged == 1 and bad[name].rows == [st.rows // 3], (name, sorted(bad))


def test_checker_flags_a_wrong_f32_residual_stream_and_encode_side_bugs():
    """f32 stores are held to half an f32 ulp + the accumulation bound: a relative error of 1e-5 in one element of the
    transformer's residual stream is flagged; on the encode side a strided convolution that drops its bias is."""
    es = encode_shape()
    we = C.random_weights(es, seed=0)
    we.update(C.random_encoder_weights(es, seed=1))
    plan = R.plan_encode(es, test_audio(20 * es.enc_frame_len - 3))

    def nudge(outs):
        outs = {k: v.copy() for k, v in outs.items()}
        outs["f32"][3, 7] *= np.float32(1.00001)
        return outs
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, we, mutate={"pre.0.wo": nudge}), we))
    assert set(bad) == {"pre.0.wo"} and bad["pre.0.wo"].rows == [3] and bad["pre.0.wo"].flagged == 1
    st = stage(plan, "enc.1.sc")
    bad = flagged(R.check_trace(plan, R.chain_emulate(plan, we, override={st.name: with_p(st, drop_bias=True)}), we))
    assert set(bad) == {st.name}


# ------------------------------------------------------------------------------------------------ carried context
STREAM_CHUNKS = (3, 1, 7, 1, 5)      # t0 = 0, 3, 4, 11, 12 at window 8: a fresh chunk, chunks below the halos, nh = 3, 4, 7, 7


def run_stream(shape, w, codes, chunks, mode="emulate"):
    """The stream chunk by chunk on its own carries: per chunk (plan, carries before it, trace or final env)."""
    t0, car, out = 0, {}, []
    for T in chunks:
        plan = R.plan_stream(shape, codes[:, t0:t0 + T], t0, min(t0, shape.tf_window - 1))
        if mode == "emulate":
            env = dict(car)
            res = R.chain_emulate(plan, w, env=env)
        else:
            res = env = R.chain_free(plan, w, env=car)
        out.append((plan, car, res))
        car = R.carries(env)
        t0 += T
    return out


def test_chunked_emulation_equals_the_whole_emulation_bit_for_bit():
    """Emulate mode: every arithmetic launch of every chunk stores what the whole decode stores in those rows, whatever
    the chunking (chunks of one frame are below every halo; window 8 is passed within the stream; [1] * 12 covers the
    first 12 frames: the codec is causal)."""
    shape = tiny_codec_shape()
    w = C.random_weights(shape, seed=0)
    codes = rand_codes(shape, 40, 9)
    wplan = R.plan_decode(shape, codes)
    whole = {st.name: (st, outs) for st, outs in zip(wplan, R.chain_emulate(wplan, w))}
    for chunks in ([40], [3, 7, 1, 20, 9], [1] * 12):
        t0 = 0
        for (plan, _, trace), T in zip(run_stream(shape, w, codes, chunks), chunks):
            for st, outs in zip(plan, trace):
                if st.kind in R.CARRY_KINDS:
                    continue
                wst, wouts = whole[st.name]
                m = wst.rows // 40
                for k, a in outs.items():
                    assert np.array_equal(a, wouts[k][t0 * m:(t0 + T) * m]), (chunks, t0, st.name, k)
            t0 += T


def test_chunked_free_chain_reproduces_the_oracle_decode():
    """Free mode: the streamed plan chained in float64 over its own carries is the codec: the oracle's decode of the
    whole code matrix, within the bound of the one-shot plan."""
    shape = tiny_codec_shape()
    w = C.random_weights(shape, seed=0)
    codes = rand_codes(shape, 40, 9)
    orc = C.CodecOracle(shape, w)
    for chunks in ([40], [3, 7, 1, 20, 9], [1] * 12):
        n = sum(chunks)                                          # ([1] * 12: the first 12 frames of the code matrix)
        want, _ = orc.decode(codes[None, :, :n], torch.tensor([n]))
        bound = roundoff_bound(R.plan_decode(shape, codes[:, :n]))
        audio = torch.cat([env["audio"][:, 0] for _, _, env in run_stream(shape, w, codes, chunks, "free")])
        d = rel_rms(audio, want[0, 0])
        print(f"stream {chunks}: float64 chain vs f32 oracle, relative RMS {d:.2e} (bound {bound:.2e})")
        assert audio.shape == want[0, 0].shape and d <= bound, (chunks, d, bound)


@pytest.fixture(scope="module")
def tiny_stream():
    shape = tiny_codec_shape()
    w = C.random_weights(shape, seed=0)
    codes = rand_codes(shape, sum(STREAM_CHUNKS), 11)
    return shape, w, run_stream(shape, w, codes, STREAM_CHUNKS)


def check_chunk(w, plan, before, trace):
    """The verdicts of one chunk judged on the carries recorded before it (those the honest stream left)."""
    return R.check_trace(plan, trace, w, env=dict(before))


def faulty(tiny_stream, c, override=None, mutate=None, before=None):
    """Chunk c emulated again with a fault (on the honest carries unless `before` says otherwise), judged on the honest
    carries: {stage name: verdict} of the flagged launches."""
    shape, w, runs = tiny_stream
    plan, car, _ = runs[c]
    env = dict(car if before is None else before)
    trace = R.chain_emulate(plan, w, override=override, mutate=mutate, env=env)
    return flagged(check_chunk(w, plan, car, trace)), plan


def test_checker_passes_an_honest_emulated_stream_with_zero_flagged_elements(tiny_stream):
    shape, w, runs = tiny_stream
    kinds = set()
    for c, (plan, car, trace) in enumerate(runs):
        vs = check_chunk(w, plan, car, trace)
        assert len(vs) == len(plan) and all(v.checked == st.rows * st.cols * len(st.dst) for v, st in zip(vs, plan))
        assert not flagged(vs), (c, [(v.name, v.flagged, v.worst) for v in flagged(vs).values()])
        kinds |= {v.kind for v in vs}
        # the same chunk judged as one whose predecessor was not traced: on its own recorded front rows
        assert not flagged(R.check_trace(plan, trace, w, env=R.seed_unlinked(plan, trace)))
    assert {"roll", "kvin", "kvout"} <= kinds


def test_checker_flags_the_carrying_faults(tiny_stream):
    """Each fault of the carrying launches, at the launch, chunk and rows it touches, and nowhere else."""
    shape, w, runs = tiny_stream
    W1 = shape.tf_window - 1
    # chunk 1 (one frame, t0 = 3): 2 rows at up.0 against halo 6
    for bug in ("tail_src_r", "chunk_only"):
        plan = runs[1][0]
        st = stage(plan, "up.0.dwln.roll")
        bad, _ = faulty(tiny_stream, 1, override={st.name: with_p(st, bug=bug)})
        assert set(bad) == {st.name}, (bug, sorted(bad))
        assert bad[st.name].rows and set(bad[st.name].rows) <= set(range(6 - 2)), (bug, bad[st.name].rows)
    # the carried K/V one row off (chunk 2: nh = 4)
    st = stage(runs[2][0], "post.1.kvin")
    bad, _ = faulty(tiny_stream, 2, override={st.name: with_p(st, bug="off_by_one")})
    assert set(bad) == {st.name} and bad[st.name].rows == list(range(4)), {k: v.rows for k, v in bad.items()}
    # kv_out writes all W1 rows when only nh + T = 3 exist (chunk 0)
    st = stage(runs[0][0], "post.0.kvout")
    bad, _ = faulty(tiny_stream, 0, override={st.name: with_p(st, bug="writes_all_rows")})
    assert set(bad) == {st.name} and bad[st.name].rows == list(range(W1 - 3)), {k: v.rows for k, v in bad.items()}
    # chunk z of a batched call reads chunk z - 1's carry: another stream's carry in place of its own
    other = run_stream(shape, w, rand_codes(shape, 9, 12), (4, 5))
    st = stage(runs[4][0], "dec.0.u1.c7.roll")
    key = st.src["prev"]
    bad, _ = faulty(tiny_stream, 4, before={**runs[4][1], key: other[1][1][key]})
    assert set(bad) == {st.name} and bad[st.name].rows == list(range(st.rows)), {k: v.rows[:8] for k, v in bad.items()}


def test_checker_flags_the_carried_context_faults(tiny_stream):
    """Each fault of an arithmetic launch in its carried-context form, at the launch, chunk and rows it touches."""
    shape, w, runs = tiny_stream
    # rope at position 0 instead of t0 (chunk 2, t0 = 4)
    st = stage(runs[2][0], "post.0.rope")
    bad, _ = faulty(tiny_stream, 2, override={st.name: with_p(st, t0=0)})
    assert set(bad) == {st.name} and bad[st.name].rows == list(range(7)), {k: v.rows for k, v in bad.items()}
    # the window counted from the chunk's first row (chunk 4: nh = 7 = window - 1, 5 frames): query 0 sees the same keys
    st = stage(runs[4][0], "post.1.attn")
    bad, _ = faulty(tiny_stream, 4, override={st.name: with_p(st, bug="window_ignores_nh")})
    assert set(bad) == {st.name} and bad[st.name].rows and set(bad[st.name].rows) <= {1, 2, 3, 4}, {k: v.rows for k, v in bad.items()}
    assert len(bad[st.name].rows) >= 3
    # the oldest carried key dropped at nh = window - 1: only query 0 reaches it
    bad, _ = faulty(tiny_stream, 4, override={st.name: with_p(st, bug="drops_oldest")})
    assert set(bad) == {st.name} and bad[st.name].rows == [0], {k: v.rows for k, v in bad.items()}
    # the final convolution reads zeros instead of its carry (chunk 3)
    st = stage(runs[3][0], "final")
    blind = dataclasses.replace(st, src={"x": st.src["x"]})
    bad, _ = faulty(tiny_stream, 3, override={"final": blind})
    assert set(bad) == {"final"} and bad["final"].rows and set(bad["final"].rows) <= set(range(6)) and 0 in bad["final"].rows
    # z * gap left out of one stage's row base: the stage reads the neighbour chunk's last rows where its carry belongs
    other = run_stream(shape, w, rand_codes(shape, 9, 12), (4, 5))
    oplan, _, otrace = other[1]
    st = stage(runs[4][0], "dec.1.u2.c7")                      # dilation 9: halo 54
    src = next(o for s_, o in zip(oplan, otrace) if s_.name == "dec.1.u1.c1")["act"]   # what the neighbour's dec.1.u2.c7 read
    tail = R.from_raw(src[-54:])
    bad, _ = faulty(tiny_stream, 4, override={st.name: dataclasses.replace(st, src={"x": st.src["x"]}, p={**st.p, "stale": tail})})
    assert set(bad) == {st.name} and bad[st.name].rows and set(bad[st.name].rows) <= set(range(54)) and 0 in bad[st.name].rows
    # one element two ulp off in the last, partial row tile of a chunk (chunk 2: 7 frames, 224 rows at dec.0.u0.c1)
    st = stage(runs[2][0], "dec.0.u0.c1")

    def two_ulp(outs, st=st):
        outs = {k: v.copy() for k, v in outs.items()}
        a = outs["bf"]
        assert (int(a[st.rows - 1, 5]) & 0x7F) < 0x7D
        a[st.rows - 1, 5] += 2
        return outs
    bad, _ = faulty(tiny_stream, 2, mutate={st.name: two_ulp})
    assert set(bad) == {st.name} and bad[st.name].flagged == 1 and bad[st.name].rows == [st.rows - 1]


# ------------------------------------------------------------------- the encode's windows at the real head geometry
ENC_TF_ATTN = dict(H=16, hd=64, window=512, rows=520)      # enc.3.tf.*.attn: the window IS window_attn_kernel's capacity
PRE_ATTN = dict(H=C.CodecShape().tf_n_head, hd=C.CodecShape().tf_head_dim, window=C.CodecShape().tf_window, rows=132)


@pytest.mark.parametrize("geo", (ENC_TF_ATTN, PRE_ATTN), ids=("enc_tf", "pre"))
def test_checker_flags_a_window_one_off_at_the_real_head_geometry(geo):
    """ONE attention stage on a seeded bf16 qkv of unit scale, a few rows past the window: the honest emulation passes;
    a window one short is flagged from the first query that has `window` keys to drop one of (row window - 1), a window
    one long from the first query that sees one key too many (row window), and neither at any earlier row."""
    H, hd, win, T = geo["H"], geo["hd"], geo["window"], geo["rows"]
    g = torch.Generator().manual_seed(win)
    env = {"qkv": R.bf16_bits(torch.randn(T, 3 * H * hd, generator=g))}
    st = R.Stage("attn", "attn", T, H * hd, {"x": "qkv"}, {"bf": "y"}, dict(H=H, hd=hd, window=win))
    W = R.Weights({}, dev=True)

    def stored(stage):
        return {"bf": R.raw_store("bf", R.eval_stage(stage, env, W, None, "emulate").ref["bf"])}
    v = R.check_stage(st, env, W, stored(st))
    assert v.checked == T * H * hd and v.flagged == 0, (v.flagged, v.worst, v.rows[:8])
    print(f"window {win}, {T} rows: honest emulation, largest |got - ref| / bound {v.worst:.3f}")
    for w_bug, first in ((win - 1, win - 1), (win + 1, win)):
        v = R.check_stage(st, env, W, stored(with_p(st, window=w_bug)))
        assert v.rows == list(range(first, T)), (w_bug, v.rows)


# ------------------------------------------------------------------------------------------- the quantiser search
def quantiser_weights(shape, seed=3):
    """The tensors the search reads, seeded, in the distributions of oracle.codec.random_weights (the real-width codec has
    10^8 other parameters that a host test of the search has no use for)."""
    g = torch.Generator().manual_seed(seed)
    D, cd, w = shape.latent_dim, shape.codebook_dim, {}
    for q in range(shape.n_codebooks + 1):
        p = R.vq_prefix(q)
        N = shape.semantic_codebook_size if q == 0 else shape.codebook_size
        w[f"{p}.in_proj.weight"] = torch.randn(cd, D, 1, generator=g) / D ** 0.5
        w[f"{p}.in_proj.bias"] = 0.05 * torch.randn(cd, generator=g)
        w[f"{p}.codebook.weight"] = torch.randn(N, cd, generator=g)
        w[f"{p}.out_proj.weight"] = torch.randn(D, cd, 1, generator=g) / cd ** 0.5
        w[f"{p}.out_proj.bias"] = 0.05 * torch.randn(D, generator=g)
    return w


def latents(shape, T, seed=17):
    return torch.randn(T, shape.latent_dim, generator=torch.Generator().manual_seed(seed)).numpy()


@pytest.fixture(scope="module", params=("encode_shape", "real"))
def search(request):
    shape = encode_shape() if request.param == "encode_shape" else C.CodecShape()
    w = quantiser_weights(shape)
    zq = latents(shape, 40)
    return shape, w, zq, R.rvq_search_emulate(shape, w, zq)


def test_search_check_passes_an_honest_float32_search(search):
    shape, w, zq, codes = search
    v = R.rvq_search_check(shape, w, zq, codes)
    print(f"honest float32 search, {shape.latent_dim}-wide, {shape.semantic_codebook_size} + {shape.n_codebooks} x "
          f"{shape.codebook_size} rows: {v.summary()}")
    assert v.decisions == 40 * (shape.n_codebooks + 1)
    assert not v.outside and not v.ties and not v.invalid, v.flagged
    assert v.ok and float(v.b.max()) <= R.RVQ_B_CAP
    # the oracle's own search on the same latents (f32 throughout): the same picks wherever its two best rows are b apart
    orc = C.CodecOracle.__new__(C.CodecOracle)
    orc.c, orc.w, orc.taps = shape, w, {}
    res = torch.from_numpy(zq).t()[None]
    for q in range(shape.n_codebooks + 1):
        zr, idx = orc._vq(R.vq_prefix(q), res)
        differ = np.flatnonzero(idx[0].numpy() != codes[q])
        assert all(v.gap[q, t] <= v.b[q, t] for t in differ), (q, differ)
        if len(differ):
            break                                              # past a flip the oracle's residual is another one
        res = res - zr


def test_search_check_flags_a_residual_left_as_it_was(search):
    """Up to codebook q + 1 the faulty search has the honest one's picks, so at q + 1 it faces the residual the honest
    one faced: flagged there are exactly the frames whose pick on the stale residual is another row, and nothing before."""
    shape, w, zq, honest = search
    q = 1
    codes = R.rvq_search_emulate(shape, w, zq, {"no_update": q})
    v = R.rvq_search_check(shape, w, zq, codes)
    moved = [(int(t), q + 1) for t in np.flatnonzero(codes[q + 1] != honest[q + 1])]
    assert len(moved) >= 10 and [f for f in v.flagged if f[1] <= q + 1] == moved, (moved, v.flagged[:8])


def test_search_check_flags_rows_read_at_the_semantic_offset_rule(search):
    shape, w, zq, honest = search
    q = 2                                                     # S0 + S0 for S0 + S: the rows of a later codebook
    codes = R.rvq_search_emulate(shape, w, zq, {"offset": q})
    v = R.rvq_search_check(shape, w, zq, codes)
    moved = [(int(t), q) for t in np.flatnonzero(codes[q] != honest[q])]
    assert len(moved) >= 10 and [f for f in v.flagged if f[1] <= q] == moved, (moved, v.flagged[:8])
    # a frame whose pick survived still subtracted the other codebook's table row: caught at the next codebook
    kept = [t for t in range(40) if codes[q, t] == honest[q, t] and codes[q + 1, t] != honest[q + 1, t]]
    assert all((t, q + 1) in v.flagged for t in kept)


def test_search_check_flags_a_dropped_in_projection_bias(search):
    """The bias is small against the projection (0.05 against O(1)), so most picks survive it: the ones that do not are
    flagged at that codebook, and no other decision is (the residual follows the device's pick)."""
    shape, w, zq, honest = search
    q = 1
    codes = R.rvq_search_emulate(shape, w, zq, {"no_bias": q})
    v = R.rvq_search_check(shape, w, zq, codes)
    moved = sorted((int(t), q) for t in np.flatnonzero(codes[q] != honest[q]))
    assert moved and v.flagged == moved, (moved, v.flagged)


def test_search_check_flags_the_highest_index_on_a_planted_tie(search):
    shape, w, zq, _ = search
    w = dict(w)
    for q in range(shape.n_codebooks + 1):
        cb = w[f"{R.vq_prefix(q)}.codebook.weight"].clone()
        cb[cb.shape[0] // 2:] = cb[:cb.shape[0] // 2]
        w[f"{R.vq_prefix(q)}.codebook.weight"] = cb
    good = R.rvq_search_check(shape, w, zq, R.rvq_search_emulate(shape, w, zq))
    assert not good.flagged and good.non_argmax == 0, good.flagged[:8]
    codes = R.rvq_search_emulate(shape, w, zq, {"last_on_ties": 1})
    v = R.rvq_search_check(shape, w, zq, codes)
    assert not v.outside                                       # the score is the best one: only the tie rule is broken
    assert sorted((t, q) for t, q, *_ in v.ties) == [(t, q) for t in range(40) for q in range(shape.n_codebooks + 1)]
    assert all(pick == low + w[f"{R.vq_prefix(q)}.codebook.weight"].shape[0] // 2 for _, q, pick, low in v.ties)


def test_search_check_flags_the_runner_up_at_ten_b(search):
    shape, w, zq, honest = search
    v0 = R.rvq_search_check(shape, w, zq, honest)
    ok = v0.gap >= 10 * v0.b
    q, t = (int(i) for i in np.unravel_index(np.argmin(np.where(ok, v0.gap, np.inf)), v0.gap.shape))    # the narrowest such gap
    assert ok[q, t] and honest[q, t] == v0.argmax[q, t]
    print(f"runner-up planted at frame {t}, codebook {q}: gap {v0.gap[q, t]:.2e}, b {v0.b[q, t]:.2e}")
    v = R.rvq_search_check(shape, w, zq, R.rvq_search_emulate(shape, w, zq, {"force": {(t, q): int(v0.runner[q, t])}}))
    assert v.flagged == [(t, q)] and v.non_argmax == 1, v.flagged
