"""Cost of the live FLAC stage (ft_codec_flac_stream_push: flacl_stage_kernel, then the FLAC stage's four launches) at the real
codec shape, synthetic weights.  The speech-like signal of tests/flac_cases.py at 44.1 kHz, B = `--blocksize` (default 4096),
mono and stereo (the second channel a scaled copy with a little of another voice).

  --part push:   one push of 20 ms, of 1 s and of 10 s on a fresh stream (opened and closed outside the clock), float32 as
                 segments.join_chunks pushes it and int16 as the pcm16 paths do; beside each, in the same process and
                 alternating, CodecHipEngine.flac of the same samples and the host conversion the push replaces (pcm(): clip,
                 scale, truncate, tobytes); and decode_join of the two five-second segments of random codes that make a 10 s
                 group.  A 20 ms push is below one frame: the staging launch alone.
  --part first:  FishTTS on the tiny synthetic models of the tests: the time from the first next() of synthesize_long_stream
                 to its first chunk, without live_format, with "flac" (4096) and with LiveFlac(256), and the samples of the
                 first PCM chunk.
Host clock around the synchronous calls; median, minimum and 90th percentile of `--rounds` after `--warmup`.
`--out FILE` appends the report to FILE as well.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _pcm(audio) -> bytes:
    return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()


def _push_part(a, report):
    from mix_probe import _ms

    from fish_tts_amd.codec_engine import CodecHipEngine
    from tests.flac_cases import speech
    eng = CodecHipEngine.synthetic(max_frames=1400)
    n = int(10.0 * 44100)
    mono = speech(n, seed=3)
    stereo = np.ascontiguousarray(np.stack([mono, 0.8 * mono + 0.05 * speech(n, seed=4)], 1).astype(np.float32))
    rng = np.random.default_rng(1)
    T = int(round(5.0 * 44100 / eng.frame_len))
    codes = [np.concatenate([rng.integers(0, eng.args.semantic_codebook_size, (1, T)),
                             rng.integers(0, eng.args.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(2)]
    report["decode_join_10s_ms"] = _ms([lambda: eng.decode_join(codes)], max(3, a.rounds // 4), 2)[0]

    def timed_push(x, channels, dtype):
        def run():
            fs = eng.flac_stream(44100, channels, a.blocksize, dtype)
            t0 = time.perf_counter()
            fs.push(x)
            dt = time.perf_counter() - t0
            fs.close()
            return dt
        return run

    for name, whole in (("mono", mono), ("stereo", stereo)):
        for seconds in (0.02, 1.0, 10.0):
            x = np.ascontiguousarray(whole[:int(seconds * 44100)])
            x16 = np.frombuffer(_pcm(x), dtype=np.int16).reshape(x.shape)

            def clocked(fn):
                def run():
                    t0 = time.perf_counter()
                    fn()
                    return time.perf_counter() - t0
                return run
            fns = [timed_push(x, x.ndim, np.float32), timed_push(x16, x.ndim, np.int16),
                   clocked(lambda: eng.flac(x, 44100, a.blocksize)), clocked(lambda: _pcm(x))]
            ts = [[] for _ in fns]
            for r in range(a.warmup + a.rounds):                   # alternating: push f32, push i16, one-shot, host conversion
                for fn, t in zip(fns, ts):
                    dt = fn()
                    if r >= a.warmup:
                        t.append(1e3 * dt)
            stat = [{"median": float(np.median(t)), "min": float(np.min(t)), "p90": float(np.percentile(t, 90))} for t in ts]
            report[f"{name}_{seconds:g}s"] = {"samples": len(x), "frames_completed": len(x) // a.blocksize, "push_f32_ms": stat[0],
                                              "push_i16_ms": stat[1], "flac_ms": stat[2], "host_pcm_ms": stat[3]}
    eng.close()


def _first_part(a, report):
    from fish_tts_amd import LiveFlac
    from tests.test_api_script_gpu import MT, SEED, TEXT
    from tests.test_api_serve_gpu import _tiny_tts
    synth = _tiny_tts()
    kw = dict(seed=SEED, max_tokens=MT, silence_db=None)
    out = {}
    for name, extra in (("pcm", {}), ("flac_4096", dict(live_format="flac")), ("flac_256", dict(live_format=LiveFlac(256)))):
        ts, sizes, counts = [], [], []
        for r in range(a.warmup + a.rounds):
            gen = synth.synthesize_long_stream(TEXT, **kw, **extra)
            t0 = time.perf_counter()
            first = next(gen)
            dt = 1e3 * (time.perf_counter() - t0)
            rest = list(gen)
            if r >= a.warmup:
                ts.append(dt)
                sizes.append(len(first))
                counts.append(1 + len(rest))
        out[name] = {"first_chunk_ms": {"median": float(np.median(ts)), "min": float(np.min(ts)), "p90": float(np.percentile(ts, 90))},
                     "first_chunk_bytes": int(np.median(sizes)), "chunks": int(np.median(counts))}
    report["first_audio"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("push", "first"), default="push")
    ap.add_argument("--blocksize", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    report = {"part": a.part, "blocksize": a.blocksize, "rounds": a.rounds, "warmup": a.warmup}
    (_push_part if a.part == "push" else _first_part)(a, report)
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
