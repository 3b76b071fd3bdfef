"""Cost of pitch= on the one-shot codec path at the real codec shape, synthetic weights (timescale_kernel at its rational
rate, pitch_kernel).

  --part wall:  a 215-frame decode with pitch unset and with pitch=7, host clock around the synchronous calls (warm-up
                first; median, minimum and 90th percentile of `--rounds`).
  --part trace: `--calls` 215-frame decodes at pitch=7 (for a rocprofv3 --kernel-trace --stats run of its own: the two
                kernels' time per launch).
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


def _times_ms(fn, rounds, warmup):
    times = []
    for r in range(warmup + rounds):
        t = time.perf_counter()
        fn()
        if r >= warmup:
            times.append(1e3 * (time.perf_counter() - t))
    return {"median": float(np.median(times)), "min": float(np.min(times)), "p90": float(np.percentile(times, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--frames", type=int, default=215)
    ap.add_argument("--pitch", type=float, default=7.0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=256)
    rng = np.random.default_rng(0)
    codes = np.zeros((eng.R, a.frames), dtype=np.int32)
    codes[0] = rng.integers(0, 4096, a.frames)
    codes[1:] = rng.integers(0, 1024, (eng.R - 1, a.frames))
    report = {"part": a.part, "frames": a.frames, "pitch": a.pitch}
    if a.part == "wall":
        report["decode_ms"] = _times_ms(lambda: eng.decode(codes), a.rounds, a.warmup)
        report["decode_pitch_ms"] = _times_ms(lambda: eng.decode(codes, pitch=a.pitch), a.rounds, a.warmup)
    else:
        for _ in range(a.calls):
            eng.decode(codes, pitch=a.pitch)
        report["calls"] = a.calls
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
