"""Cost of sample_rate= on the codec paths at the real codec shape, synthetic weights (resample_kernel).

  --part codec: in one run, host clock around the synchronous calls (warm-up first, median of `--rounds`):
                one 215-frame decode at 44.1 kHz against 16 kHz (ft_codec_decode / ft_codec_decode_at), and one batched
                call of 32 streams x 20 frames all at 44.1 kHz against half of them at 16 kHz
                (ft_codec_stream_decode_many / ft_codec_stream_decode_many_at).
  --part trace: `--calls` batched calls of 32 streams x 20 frames, half at 16 kHz, and `--calls` 215-frame decodes at
                16 kHz (for a rocprofv3 --kernel-trace --stats run of its own: resample_kernel's time per launch).
`--out FILE` appends the report to FILE as well.
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


def _median_ms(fn, rounds, warmup):
    times = []
    for r in range(warmup + rounds):
        t = time.perf_counter()
        fn()
        if r >= warmup:
            times.append(time.perf_counter() - t)
    return 1e3 * float(np.median(times)), 1e3 * float(np.percentile(times, 90))


def _many(eng, rates, chunks):
    """One decode_streams call per round over fresh-enough streams at `rates` (restarted before max_frames)."""
    state = {"streams": [eng.stream(r) for r in rates]}

    def call():
        s = state["streams"]
        if s[0].frames + 20 > eng.max_frames:
            for x in s:
                x.close()
            state["streams"] = s = [eng.stream(r) for r in rates]
        eng.decode_streams(s, chunks)
    return call


def part_codec(rounds, warmup):
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=2056)
    rng = np.random.default_rng(0)
    one = _codes(rng, eng.R, 215)[None]
    lines = ["real codec shape, synthetic weights; host clock around synchronous calls, median (p90) of "
             f"{rounds} after {warmup} warm-up"]
    res = {}
    for rate in (None, 16000):
        res[rate] = _median_ms(lambda: eng.decode(one, sample_rate=rate), rounds, warmup)
    lines.append(f"215-frame decode: 44.1 kHz {res[None][0]:.3f} ms ({res[None][1]:.3f}), 16 kHz {res[16000][0]:.3f} ms "
                 f"({res[16000][1]:.3f}): +{res[16000][0] - res[None][0]:.3f} ms")
    chunks = [_codes(rng, eng.R, 20) for _ in range(32)]
    m = {}
    for name, rates in (("44.1 kHz", [None] * 32), ("half at 16 kHz", [None, 16000] * 16), ("all at 16 kHz", [16000] * 32)):
        m[name] = _median_ms(_many(eng, rates, chunks), rounds, warmup)
    base = m["44.1 kHz"][0]
    lines.append("32 x 20-frame decode_streams: " + "; ".join(
        f"{k} {v[0]:.3f} ms ({v[1]:.3f}, {100 * (v[0] / base - 1):+.1f} %)" for k, v in m.items()))
    eng.close()
    return lines


def part_trace(calls):
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=2056)
    rng = np.random.default_rng(0)
    chunks = [_codes(rng, eng.R, 20) for _ in range(32)]
    call = _many(eng, [None, 16000] * 16, chunks)
    one = _codes(rng, eng.R, 215)[None]
    for _ in range(calls):
        call()
        eng.decode(one, sample_rate=16000)
    eng.close()
    return [f"trace: {calls} x (32 x 20-frame decode_streams, half at 16 kHz) + {calls} x 215-frame decode at 16 kHz"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["codec", "trace"], default="codec")
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = part_codec(a.rounds, a.warmup) if a.part == "codec" else part_trace(a.calls)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
