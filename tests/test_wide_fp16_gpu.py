"""GPU: precision="fp16" lock-step batches of >= 5 rows on the MFMA launches of csrc/wide_kernels.h (five per layer), the
path bf16 batches take.  The set-ups are those of the bf16 wide tests of tests/test_ar_gpu.py; the tolerance is the
project's fp16 convention, the bf16 one / 8 (three more mantissa bits; test_ar_gpu.py: test_greedy_matches_golden):
0.03 x scale -> 0.00375 x scale, scale = max(1, absmax of the oracle's frame-0 logits)."""
import dataclasses
import io
import time
import wave

import numpy as np
import pytest
import torch

from oracle import ar as O
from tests.hip_util import args_from_shape, cached_random_weights, first_divergence
from tests.shapes import make_prompt
from tests.test_ar_gpu import _margin_ok, medium_shape

pytestmark = pytest.mark.gpu

TOL = 0.00375                     # x scale: 0.03 (the wide bf16 tests) / 8
KW = dict(temperature=0.7, top_p=1e-6, repetition_penalty=1.1)
_ORACLES = {}                     # dtype -> AROracle on the shared weights
_RUNS = {}                        # (tag, dtype, utterance) -> (oracle sequence, taps)


def _weights(shape):
    return cached_random_weights(shape, seed=0, std=0.05)


def _engine(shape, B, max_new_tokens=64):
    from fish_tts_amd.ar_engine import ARHipEngine
    eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                      precision="fp16", device=0, max_batch=B, max_new_tokens=max_new_tokens)
    eng.load_state_dict({k: v.to(torch.float16) for k, v in _weights(shape).items()})
    return eng


def _oracle_run(shape, dtype, tag, i, prompt, n_frames):
    """The oracle's sequence and taps of utterance i (same prompt, weights and sampling in every parametrisation: once per run)."""
    if (tag, dtype, i) not in _RUNS:
        if (tag, dtype) not in _ORACLES:
            _ORACLES[(tag, dtype)] = O.AROracle(shape, _weights(shape), dtype)
        orc = _ORACLES[(tag, dtype)]
        taps = []
        orc.reset()
        _RUNS[(tag, dtype, i)] = (orc.generate(prompt.clone(), n_frames, frame_taps=taps, **KW).numpy(), taps)
    return _RUNS[(tag, dtype, i)]


def _judged(B):
    """All rows for B <= 8, else every third utterance and the last row (the judged set of test_wide_batch_vs_oracle)."""
    return [i for i in range(B) if not (i % 3 and B > 8 and i != B - 1)]


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


@pytest.mark.parametrize("B,env", [(5, None), (16, None), (32, None), (40, None), (32, "FT_NO_ATTN_WIDE"), (32, "FT_NO_HEAD_STREAM")])
def test_wide_fp16_batch_vs_oracle(monkeypatch, B, env):
    """test_wide_batch_vs_oracle in fp16: the engine reports and runs the MFMA launches, and every judged utterance follows
    the fp16 ORACLE up to a decision whose top-1/top-2 margin is inside the fp16 evaluation-order tolerance.

    For the plain B = 32 run, three-way logit distance (the rule of test_codec_gpu.py, factor 1.25): for every judged slot
    whose 6 frames equal both the fp16 and the fp32 oracle's, the vocabulary head's output of the last decoded frame must
    sit no farther from the fp32 oracle than 1.25 x the fp16 oracle does.  ft_ar_get_debug returns the head's output as the
    draw left it: the draw writes the repetition penalty in place on the entries named by one earlier frame's column (its
    semantic token and its codes read as vocabulary ids: num_codebooks + 1 entries, sample_block_kernel after
    inference.py:109-111), every other entry is the head's.  The comparison therefore runs over all entries except the
    values of the slot's generated columns (a superset of the rewritten ones, < 70 of 5120); the same figure over the 64
    largest of them is printed."""
    if env:
        monkeypatch.setenv(env, "1")
    shape = medium_shape(n_text=1009)
    eng = _engine(shape, B)
    assert "MFMA launches" in eng.frame_path(), eng.frame_path()
    sp = eng._sampling(0.7, 1e-6, 1.1)
    prompts = [make_prompt(shape, 9 + (3 * i) % 11, seed=300 + i, n_vq=i % 4) for i in range(B)]
    firsts = [eng.prefill(p.numpy(), sp, slot=i) for i, p in enumerate(prompts)]
    frames, n = eng.decode(5, [sp] * B, poll=5)
    checked, followed = 0, []
    for i in _judged(B):
        p = prompts[i]
        want, taps = _oracle_run(shape, torch.float16, "short", i, p, 6)
        got = np.concatenate([p.numpy(), firsts[i][:, None], frames[i, : n[i]].T], axis=1)
        scale = max(1.0, float(taps[0][0].float().abs().max()))
        div = first_divergence(got, want)
        if div is not None:
            col, row = div
            assert _margin_ok(taps, col - p.shape[1], row, TOL * scale), f"utterance {i} diverged at {div}\n{got}\n{want}"
        elif n[i] == 5:
            followed.append(i)
        checked += 1
    assert checked >= min(B, 6)
    print(f"B={B} {env}: judged {checked}, followed the fp16 oracle through all 6 frames: {followed}")
    if B == 32 and env is None:
        three_way = 0
        for i in followed:
            p = prompts[i]
            want16, taps16 = _oracle_run(shape, torch.float16, "short", i, p, 6)
            want32, taps32 = _oracle_run(shape, torch.float32, "short", i, p, 6)
            if not np.array_equal(want16, want32):
                continue
            gpu = eng.debug_state(i)[0].astype(np.float64)
            o16 = taps16[5][0].float().reshape(-1).numpy().astype(np.float64)
            o32 = taps32[5][0].float().reshape(-1).numpy().astype(np.float64)
            keep = np.ones(gpu.shape[0], dtype=bool)
            keep[np.unique(want16[:, p.shape[1]:])] = False          # entries the draw's repetition penalty may have rewritten
            d_g, d_o = _rms((gpu - o32)[keep]), _rms((o16 - o32)[keep])
            top = np.argsort(-np.where(keep, o32, -np.inf))[:64]
            print(f"slot {i}: rms(gpu - o32) {d_g:.3e}, rms(o16 - o32) {d_o:.3e} (x {d_g / d_o:.3f}), rms(o32) {_rms(o32[keep]):.3e}; "
                  f"top-64: {_rms((gpu - o32)[top]):.3e} vs {_rms((o16 - o32)[top]):.3e}")
            assert d_g <= 1.25 * d_o, (i, d_g, d_o)
            three_way += 1
        assert three_way >= 3, three_way
    eng.close()


@pytest.mark.parametrize("B,switch", [(7, "FT_NO_PAIR"), (32, "FT_NO_PAIR"), (19, "FT_NO_QKV0")])
def test_wide_fp16_fused_forms_equal_the_separate_ones(monkeypatch, B, switch):
    """test_wide_batch_paired_codebook_pass_equals_two_passes in fp16: the paired pass of codebook positions 0 and 1 and the
    layer-0 q k v table keep every row's arithmetic, so frames, first frames and counts equal those of the separate
    launches (FT_NO_PAIR / FT_NO_QKV0) bit for bit, sampled rows (top_p = 0.8) included."""
    shape = medium_shape(n_text=1009)
    prompts = [make_prompt(shape, 9 + (3 * i) % 11, seed=300 + i, n_vq=i % 4).numpy() for i in range(B)]
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv(switch, "1")
        eng = _engine(shape, B)
        assert "MFMA launches" in eng.frame_path(), eng.frame_path()
        sps = [eng._sampling(0.7, 0.8 if i % 2 else 1e-6, 1.1, seed=7 + i) for i in range(B)]
        firsts = [eng.prefill(p, sps[i], slot=i) for i, p in enumerate(prompts)]
        frames, n = eng.decode(6, sps, poll=3)
        outs.append((np.stack(firsts), frames.copy(), n.copy()))
        eng.close()
    assert np.array_equal(outs[0][2], outs[1][2])
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


def test_wide_fp16_long_contexts_vs_oracle():
    """test_wide_batch_long_contexts_vs_oracle in fp16 (B = 16, 140-420 positions, the two-pass attn_wide_kernel over several
    chunks of K rows, first frame + 4 decoded).  Judged: utterances 1, 5, 7, 9, 13, 15 (177 to 414 positions), which the
    fp32 oracle - another valid evaluation order - follows through all five frames of the fp16 oracle, so the frames after
    the first are really compared."""
    B = 16
    shape = medium_shape(n_text=1009, max_seq_len=512)
    eng = _engine(shape, B, max_new_tokens=16)
    assert "MFMA launches" in eng.frame_path(), eng.frame_path()
    sp = eng._sampling(0.7, 1e-6, 1.1)
    lens = [140 + (37 * i) % 281 for i in range(B)]
    prompts = [make_prompt(shape, lens[i], seed=700 + i, n_vq=lens[i] - 30) for i in range(B)]
    firsts = [eng.prefill(p.numpy(), sp, slot=i) for i, p in enumerate(prompts)]
    frames, n = eng.decode(4, [sp] * B, poll=4)
    eng.close()
    for i in (1, 5, 7, 9, 13, 15):
        p = prompts[i]
        want, taps = _oracle_run(shape, torch.float16, "long", i, p, 5)
        got = np.concatenate([p.numpy(), firsts[i][:, None], frames[i, : n[i]].T], axis=1)
        scale = max(1.0, float(taps[0][0].float().abs().max()))
        div = first_divergence(got, want)
        print(f"utterance {i} ({lens[i]} positions): first divergence {div}")
        if div is not None:
            col, row = div
            assert _margin_ok(taps, col - p.shape[1], row, TOL * scale), f"utterance {i} ({lens[i]} positions) diverged at {div}"


def _wav_frames(data):
    with wave.open(io.BytesIO(data), "rb") as wf:
        return wf.getnframes()


def test_fp16_server_and_batch_at_s1_widths_step_on_the_mfma_launches():
    """test_server_at_s1_widths_ends_on_the_frame_engine's set-up with precision="fp16" (8 slots, 10 requests): the scheduler
    keys on frame_path(), so with the MFMA launches reported 2..4 active rows ride five wide - steps of width 1 or >= 5
    only.  fp16 has no frame engine (engine_state flags 0).  Then one synthesize_batch call of 8 texts on the same
    instance: 8 WAVs, each as long as the codes of the same lock-step run decode to."""
    import fish_tts_amd as ft
    from fish_tts_amd import serve
    from fish_tts_amd.batch import run_batch
    from fish_tts_amd.tokenizer import NAMED_SPECIAL_TOKENS, ByteTokenizer
    from tests.test_api_gpu import api_codec_shape
    from tests.test_codec_gpu import args_from_shape as codec_args_from_shape
    shape = medium_shape(n_text=1009)
    tok = ByteTokenizer(1009, NAMED_SPECIAL_TOKENS + [f"<|semantic:{i}|>" for i in range(4096)])
    assert tok.semantic_begin_id == shape.semantic_begin_id and tok.get_token_id("<|im_end|>") == shape.im_end_id
    cshape = dataclasses.replace(api_codec_shape(), semantic_codebook_size=4096)
    synth = ft.FishTTS.synthetic(dataclasses.replace(args_from_shape(shape), max_seq_len=2304), tok,
                                 codec_args=codec_args_from_shape(cshape), precision="fp16", max_new_tokens=64, max_batch=8)
    try:
        assert "MFMA launches" in synth._engine.frame_path(), synth._engine.frame_path()
        assert synth._engine.engine_state()[0] == 0
        reqs = []
        with synth.serve(burst=4) as srv:
            for i in range(10):
                utt, n_prefix = synth._serve_prepare(f"request number {i}", None, 0.7, 0.8, 1.1, 48 if i == 3 else 6 + 2 * i, i)
                utt.ban_eos = True
                reqs.append(srv.submit(utt, n_prefix, stream=i % 2 == 1, seamless=i % 4 == 1, chunk_tokens=6,
                                       min_first_chunk=3))
                time.sleep(0.003)
            outs = []
            for r in reqs:
                items = []
                while True:
                    it = r.out.get(timeout=120)
                    if it is serve._END or isinstance(it, bytes) and r.mode == "wav":
                        items.append(it)
                        break
                    assert isinstance(it, bytes), it
                    items.append(it)
                outs.append(items)
            stats = srv.stats()
        assert stats["completed"] == 10 and stats["admitted"] == 10
        sw = stats["steps_by_width"]
        assert sw.get(1, 0) > 0 and max(sw) >= 5, sw
        assert all(w == 1 or w >= 5 for w in sw), sw                 # 2..4 rows ride five wide
        for i, r in enumerate(reqs):
            cols = r.utt.columns()
            assert cols.shape[1] == (48 if i == 3 else 6 + 2 * i)
            assert (cols[0] != shape.im_end_id).all()                 # ban_eos: every request runs its budget
            assert ((cols[1] >= 0) & (cols[1] < 4096)).all() and ((cols[2:] >= 0) & (cols[2:] < 1024)).all()
            assert all(len(p) > 0 for p in outs[i][:-1] if isinstance(p, bytes))
        assert synth._engine.engine_state()[:2] == (0, 0)
        assert not synth._gen_lock.locked()
        # one synthesize_batch call of 8 texts: the lengths of the same lock-step run's codes
        texts = [f"batch text number {i}, " + "la " * (i % 3) for i in range(8)]
        with synth._gen_lock:
            _, utts = synth._batch_utterances(texts, None, 0.7, 0.8, 1.1, 12, 0, None)
            run_batch(synth._engine, utts)
        want = [u.codes().shape[1] for u in utts]
        assert all(1 <= w <= 12 for w in want), want
        wavs = synth.synthesize_batch(texts, max_tokens=12)
        assert len(wavs) == 8
        fl = synth._vocoder.frame_len
        assert [_wav_frames(w) for w in wavs] == [w * fl for w in want]
        assert not synth._gen_lock.locked()
    finally:
        if synth._server is not None:
            synth._server.close(cancel=True)
        synth._engine.close()
        synth._vocoder.close()
