"""Continuous batching under arrivals (FishTTS.serve -> BatchServer) at s1-mini shapes, synthetic weights, max_batch=32.

`--n` streaming requests (synthesize_stream, chunks of 20 frames after a first one of 10, seamless=False: the reference's
default) of `--frames` frames each arrive as a Poisson process at each rate of `--rates` (requests/s).  Reported per rate:
aggregate tok/s (generated frames over the time from the first arrival to the last chunk), time to first audio from each
request's arrival (p50 / p95), frame steps by lock-step width and slot moves (BatchServer.stats()); then the same arrivals
through today's serialized FishTTS.synthesize_stream (callers on threads, one utterance at a time under its lock).
The synthetic model draws <|im_end|> with probability ~1/155 776 per frame, so a request runs its `--frames` budget.
`--sample-rate`: every request asks for that output rate (resampled on the device; frames counted from its samples)."""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(synth, texts, arrivals, frames, stream_fn, frame_len, **kw):
    """Callers on threads, each at its arrival time: (tok/s, ttfa ms array, frames generated, wall s).  `frame_len`:
    output samples per frame (fractional at a resampled rate)."""
    t0 = time.perf_counter() + 0.05
    first, got, errs = {}, {}, []

    def call(i):
        time.sleep(max(0.0, t0 + arrivals[i] - time.perf_counter()))
        try:
            n = 0
            for pcm in stream_fn(texts[i], max_tokens=frames, **kw):
                if pcm and i not in first:
                    first[i] = time.perf_counter() - (t0 + arrivals[i])
                n += len(pcm) // 2
            got[i] = int(round(n / frame_len))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=call, args=(i,)) for i in range(len(texts))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    wall = time.perf_counter() - t0
    n_frames = sum(got.values())
    return n_frames / wall, np.array([first[i] for i in range(len(texts))]) * 1e3, n_frames, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--frames", type=int, default=215)
    ap.add_argument("--rates", type=float, nargs="+", default=[5.0, 40.0])
    ap.add_argument("--burst", type=int, default=8)
    ap.add_argument("--no-serial", action="store_true")
    ap.add_argument("--sample-rate", type=int, default=None)
    ap.add_argument("--speed", type=float, default=None)
    a = ap.parse_args()
    import fish_tts_amd as ft
    from fish_tts_amd.config import s1_mini_args
    from fish_tts_amd.tokenizer import ByteTokenizer
    tok = ByteTokenizer()
    synth = ft.FishTTS.synthetic(s1_mini_args(max_seq_len=4096), tok, precision="bf16", max_new_tokens=2048 + 8, max_batch=32)
    fl = synth._vocoder.frame_len
    kw = {} if a.sample_rate is None else {"sample_rate": a.sample_rate}
    if a.sample_rate is not None:
        fl = fl * a.sample_rate / 44100
    if a.speed is not None:
        kw["speed"] = a.speed
        fl = fl / a.speed
    print(f"s1-mini shapes, synthetic weights, max_batch 32; {a.n} streaming requests x {a.frames} frames, Poisson arrivals; "
          f"output rate {a.sample_rate or 44100} Hz, speed {a.speed or 1.0}; frames: {synth._engine.frame_path()}", flush=True)
    rng = np.random.default_rng(0)
    texts = [" ".join(f"word{j}" for j in range(int(k))) for k in rng.integers(4, 24, a.n)]
    list(synth.synthesize_stream(texts[0], max_tokens=16))           # warm-up: graphs, codec
    with synth.serve(burst=a.burst) as srv:                            # warm-up of the batch widths
        ws = [threading.Thread(target=lambda t=t: list(srv.synthesize_stream(t, max_tokens=24))) for t in texts[:32]]
        for w in ws:
            w.start()
        for w in ws:
            w.join()
    for rate in a.rates:
        arrivals = np.cumsum(np.random.default_rng(int(rate * 10)).exponential(1.0 / rate, a.n))
        arrivals -= arrivals[0]
        with synth.serve(burst=a.burst) as srv:
            tps, ttfa, nf, wall = run(synth, texts, arrivals, a.frames, srv.synthesize_stream, fl, **kw)
            st = srv.stats()
        sw = st["steps_by_width"]
        steps = ", ".join(f"{w}:{sw[w]}" for w in sorted(sw))
        print(f"rate {rate:g}/s  serve: {tps:.0f} tok/s aggregate ({nf} frames in {wall:.2f} s, arrivals over "
              f"{arrivals[-1]:.2f} s); first audio p50 {np.percentile(ttfa, 50):.0f} ms, p95 {np.percentile(ttfa, 95):.0f} ms, "
              f"max {ttfa.max():.0f} ms; slot moves {st['slot_moves']}; frame steps by width {{{steps}}}", flush=True)
        if not a.no_serial:
            tps_s, ttfa_s, nf_s, wall_s = run(synth, texts, arrivals, a.frames, synth.synthesize_stream, fl, **kw)
            print(f"rate {rate:g}/s  serialized synthesize_stream: {tps_s:.0f} tok/s ({nf_s} frames in {wall_s:.2f} s); "
                  f"first audio p50 {np.percentile(ttfa_s, 50):.0f} ms, p95 {np.percentile(ttfa_s, 95):.0f} ms, "
                  f"max {ttfa_s.max():.0f} ms; serve / serialized: {tps / tps_s:.2f}x tok/s", flush=True)
    synth._engine.close()
    synth._vocoder.close()


if __name__ == "__main__":
    main()
