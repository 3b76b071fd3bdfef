"""Batched streamed codec decode (ft_codec_stream_decode_many) at the real codec shape, synthetic weights.

  --part codec: n in {1, 8, 32} streams x 20-frame chunks - n ft_codec_stream_decode calls against ONE batched call per
                round (host clock around the synchronous calls, warm-up first, >= 50 rounds).
  --part e2e:   batch_stream.stream_utterances (the engine of FishTTS.synthesize_batch_stream) at s1-mini shapes, 32
                utterances of 215 frames (ban_eos), one lock-step batch: aggregate frames/s, time to first audio per
                utterance (p50 / p95); beside it the synthesize_batch form (run_batch, then one decode per utterance).
  --part trace: `--calls` batched calls of `--n` streams only (for a rocprofv3 --kernel-trace --stats run of its own).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _codes(rng, R, T):
    c = np.zeros((R, T), dtype=np.int32)
    c[0] = rng.integers(0, 4096, T)
    c[1:] = rng.integers(0, 1024, (R - 1, T))
    return c


def part_codec(rounds, warmup):
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=2056)
    rng = np.random.default_rng(0)
    for n in (1, 8, 32):
        chunks = [_codes(rng, eng.R, 20) for _ in range(n)]
        res = {}
        for mode in ("single", "batched"):
            streams = [eng.stream() for _ in range(n)]
            times = []
            for r in range(warmup + rounds):
                if streams[0].frames + 20 > 2056:
                    for s in streams:
                        s.close()
                    streams = [eng.stream() for _ in range(n)]
                t = time.perf_counter()
                if mode == "single":
                    for s, c in zip(streams, chunks):
                        s.decode(c)
                else:
                    eng.decode_streams(streams, chunks)
                if r >= warmup:
                    times.append(time.perf_counter() - t)
            for s in streams:
                s.close()
            res[mode] = (float(np.median(times)) * 1e3, float(np.mean(times)) * 1e3)
        print(f"codec n={n:2d} x 20 frames: {n} single calls median {res['single'][0]:.2f} ms (mean {res['single'][1]:.2f}); "
              f"one batched call median {res['batched'][0]:.2f} ms (mean {res['batched'][1]:.2f}); "
              f"ratio {res['batched'][0] / res['single'][0]:.3f}; batched {n * 20 / res['batched'][0] * 1e3:.0f} frames/s",
              flush=True)
    eng.close()


def part_trace(n, calls):
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=2056)
    rng = np.random.default_rng(0)
    streams = [eng.stream() for _ in range(n)]
    chunks = [_codes(rng, eng.R, 20) for _ in range(n)]
    for _ in range(calls):
        eng.decode_streams(streams, chunks)
    print(f"trace: {calls} batched calls of {n} streams x 20 frames", flush=True)
    eng.close()


def part_e2e(n_utt, frames, reps):
    from fish_tts_amd.ar_engine import ARHipEngine
    from fish_tts_amd.batch import Utterance, run_batch
    from fish_tts_amd.batch_stream import stream_utterances
    from fish_tts_amd.codec_engine import CodecHipEngine
    from fish_tts_amd.config import s1_mini_args
    from fish_tts_amd.tokenizer import ByteTokenizer
    from fish_tts_amd.weights import random_state_dict
    import torch
    tok = ByteTokenizer()
    im_end = tok.get_token_id("<|im_end|>")
    args = s1_mini_args(max_seq_len=4096)
    eng = ARHipEngine(args, tok.semantic_begin_id, tok.semantic_end_id, im_end, precision="bf16", max_batch=32,
                      max_new_tokens=512)
    eng.load_state_dict(random_state_dict(args, seed=0, dtype=torch.bfloat16))
    codec = CodecHipEngine.synthetic(max_frames=2056)
    rng = np.random.default_rng(1)
    lens = rng.integers(16, 97, n_utt)

    def utts():
        out = []
        for i, L in enumerate(lens):
            p = np.zeros((11, int(L)), dtype=np.int32)
            p[0] = np.random.default_rng(i).integers(0, tok.n_ranks, int(L))
            out.append(Utterance(p, frames + 1, 0.7, 0.8, 1.1, seed=i, ban_eos=True))
        return out
    for rep in range(reps):
        us = utts()
        t0 = time.perf_counter()
        first = {}
        n_frames = 0
        for i, pcm in stream_utterances(lambda f, d: run_batch(eng, us, on_frames=f, on_done=d), n_utt, codec):
            if pcm:
                first.setdefault(i, time.perf_counter() - t0)
                n_frames += len(pcm) // 2 // codec.frame_len
        wall = time.perf_counter() - t0
        ttfa = np.array([first[i] for i in range(n_utt)]) * 1e3
        us = utts()
        t1 = time.perf_counter()
        run_batch(eng, us)
        for u in us:
            codec.decode(u.codes())
        wall_b = time.perf_counter() - t1
        nb = sum(u.codes().shape[1] for u in us)
        print(f"e2e rep {rep}: batch stream {n_utt} x {frames} frames: {n_frames / wall:.0f} frames/s aggregate "
              f"({wall:.2f} s); time to first audio p50 {np.percentile(ttfa, 50):.0f} ms, p95 {np.percentile(ttfa, 95):.0f} ms; "
              f"synthesize_batch form {nb / wall_b:.0f} frames/s ({wall_b:.2f} s, first audio after {wall_b * 1e3:.0f} ms)",
              flush=True)
    eng.close()
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["codec", "e2e", "trace"], required=True)
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if a.part == "codec":
        part_codec(a.rounds, a.warmup)
    elif a.part == "trace":
        part_trace(a.n, a.calls)
    else:
        part_e2e(32, 215, a.reps)


if __name__ == "__main__":
    main()
