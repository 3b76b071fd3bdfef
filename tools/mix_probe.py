"""Cost of the mix stage at the real codec shape, synthetic weights (ft_codec_mix: the bed's intake, level and resampler
launches, mix_hop_kernel, mix_node_kernel, mix_kernel, mix_scale_kernel).

  --part wall:  CodecHipEngine.mix over `--seconds` of programme (default 60 and 600) at 44.1 kHz - what decode_join returns
                for as many five-second segments of random codes - under a 30 s looped 48 kHz stereo 16-bit bed, and beside
                it decode_join of the same segments, for scale.  Host clock around the synchronous calls, the two
                alternating; median, minimum and 90th percentile of `--rounds` after `--warmup`.
  --part trace: one mix call over the first of `--seconds` after one warm-up call over one second (for a rocprofv3
                --kernel-trace --stats run of its own).
`--out FILE` appends the report to FILE as well.
"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ms(fns, rounds, warmup):
    """The calls in turn, round by round: median / min / p90 each."""
    ts = [[] for _ in fns]
    for r in range(warmup + rounds):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                t.append(1e3 * (time.perf_counter() - t0))
    return [{"median": float(np.median(t)), "min": float(np.min(t)), "p90": float(np.percentile(t, 90))} for t in ts]


def music(seconds, rate, seed=0):
    """16-bit stereo WAV bytes: two detuned chords with a slow swell."""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    ch = []
    for d in (0.0, 1.5):
        v = sum(0.08 * np.sin(2 * np.pi * (f + d) * t) for f in (220.0, 277.2, 329.6)) * (0.7 + 0.3 * np.sin(2 * np.pi * 0.2 * t))
        ch.append(v + 0.003 * rng.standard_normal(n))
    body = np.round(np.clip(np.stack(ch, 1), -1, 1) * 32767).astype("<i2").tobytes()
    head = struct.pack("<HHIIHH", 1, 2, rate, rate * 4, 4, 16)
    chunks = b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--seconds", type=float, nargs="+", default=[60.0, 600.0])
    ap.add_argument("--segment", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from fish_tts_amd.codec_engine import CodecHipEngine
    from fish_tts_amd.mix import Bed, bed_params
    from fish_tts_amd.wavfile import parse_wav
    eng = CodecHipEngine.synthetic(max_frames=1400)
    wav = music(30.0, 48000)
    clip = (wav, parse_wav(wav))
    mp = bed_params(Bed(wav, lead=1.0, tail=2.0), 44100)
    rng = np.random.default_rng(1)
    T = int(round(a.segment * 44100 / eng.frame_len))
    a_ = eng.args
    report = {"part": a.part, "segment_frames": T, "rounds": a.rounds, "warmup": a.warmup, "bed": "30 s 48 kHz stereo s16, looped"}

    def segments(seconds):
        k = max(1, int(round(seconds / a.segment)))
        return [np.concatenate([rng.integers(0, a_.semantic_codebook_size, (1, T)),
                                rng.integers(0, a_.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(k)]

    if a.part == "wall":
        for seconds in a.seconds:
            codes = segments(seconds)
            x, _ = eng.decode_join(codes)
            x = (0.25 * x / max(1e-9, float(np.abs(x).max()))).astype(np.float32)      # a programme well under the ceiling
            y, rep = eng.mix(x, clip, params=mp)
            key = f"{seconds:g}s"
            report[key] = {"samples": len(x), "mixed": rep.n, "bed_len": rep.bed_len, "hops": rep.hops, "active": rep.active,
                           "capped": rep.capped, "bed_lufs": rep.bed.level.lufs}
            report[key]["mix_ms"], report[key]["decode_join_ms"] = _ms(
                [lambda: eng.mix(x, clip, params=mp), lambda: eng.decode_join(codes)], a.rounds, a.warmup)
    else:
        x, _ = eng.decode_join(segments(a.seconds[0]))
        eng.mix(x[:44100], clip, params=mp)
        eng.mix(x, clip, params=mp)
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
