"""Cost of loudness= at the real codec shape, synthetic weights (level_filter_kernel, level_gain_kernel, level_scale_kernel).

  --part wall:  a 215-frame decode (10 s at 44.1 kHz) with loudness unset and at -16 LUFS, and a 32-item decode_join of
                `--join-frames` frames each the same way, host clock around the synchronous calls, the two forms alternating
                (warm-up first; median, minimum and 90th percentile of `--rounds`).
  --part trace: `--calls` levelled 215-frame decodes and as many levelled 32-item joins (for a rocprofv3 --kernel-trace
                --stats run of its own: the three kernels' time per launch).
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


def _pair_ms(fa, fb, rounds, warmup):
    """The two calls in turn: {name: median / min / p90} each."""
    ta, tb = [], []
    for r in range(warmup + rounds):
        for fn, ts in ((fa, ta), (fb, tb)):
            t = time.perf_counter()
            fn()
            if r >= warmup:
                ts.append(1e3 * (time.perf_counter() - t))
    return [{"median": float(np.median(t)), "min": float(np.min(t)), "p90": float(np.percentile(t, 90))} for t in (ta, tb)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--frames", type=int, default=215)
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--join-frames", type=int, default=60)
    ap.add_argument("--loudness", type=float, default=-16.0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=max(256, a.items * a.join_frames))
    rng = np.random.default_rng(0)

    def codes(T):
        c = np.zeros((eng.R, T), dtype=np.int32)
        c[0] = rng.integers(0, 4096, T)
        c[1:] = rng.integers(0, 1024, (eng.R - 1, T))
        return c

    one = codes(a.frames)
    many = [codes(a.join_frames) for _ in range(a.items)]
    jp = (10.0 ** (-45.0 / 20.0), 220, 1323, 220)
    gaps = [8820] * a.items
    report = {"part": a.part, "frames": a.frames, "items": a.items, "join_frames": a.join_frames, "loudness": a.loudness,
              "samples": a.frames * eng.frame_len, "join_samples": a.items * a.join_frames * eng.frame_len}
    if a.part == "wall":
        levels = []
        eng.decode(one, loudness=a.loudness, levels=levels)
        report["info"] = {"lufs": levels[0].lufs, "peak": levels[0].peak, "gain": levels[0].gain, "blocks": levels[0].blocks,
                          "capped": levels[0].capped}
        report["decode_ms"], report["decode_level_ms"] = _pair_ms(
            lambda: eng.decode(one), lambda: eng.decode(one, loudness=a.loudness), a.rounds, a.warmup)
        report["join_ms"], report["join_level_ms"] = _pair_ms(
            lambda: eng.decode_join(many, params=jp, gaps=gaps), lambda: eng.decode_join(many, params=jp, gaps=gaps, loudness=a.loudness),
            max(5, a.rounds // 3), 2)
    else:
        for _ in range(a.calls):
            eng.decode(one, loudness=a.loudness)
            eng.decode_join(many, params=jp, gaps=gaps, loudness=a.loudness)
        report["calls"] = a.calls
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
