"""Cost of speed= on the codec paths at the real codec shape, synthetic weights (timescale_kernel), and the paths without
it against another build of the library.

  --part base:    speed unset, host clock around the synchronous calls (warm-up first, median and range of `--rounds`):
                  one 215-frame decode, one 20-frame single-stream call, one 32 x 20-frame decode_streams call.
                  `--lib FILE` loads that build of the library instead of the tree's (entry points it lacks are left out).
  --part compare: `--reps` alternating runs of --part base, each in a process of its own, on the tree's library and on
                  `--parent-lib FILE`; per figure both ranges, and whether the tree's medians stay within the parent's
                  range widened by its own spread.
  --part speed:   a 215-frame decode at speed unset, 0.5, 1.25 and 2.0; 32 x 20-frame decode_streams with no stream and
                  with half the streams at 1.25.
  --part trace:   `--calls` 215-frame decodes at 0.5, 1.25 and 2.0 and `--calls` batched calls with half the streams at
                  1.25 (for a rocprofv3 --kernel-trace --stats run of its own: timescale_kernel's time per launch).
`--out FILE` appends the report to FILE as well.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _use_lib(path):
    """Loads another build of the library; the prototypes of entry points it does not export are dropped."""
    import ctypes
    from fish_tts_amd import _lib as L
    L.LIB_PATH = os.path.abspath(path)
    probe = ctypes.CDLL(L.LIB_PATH)
    for name in list(L.SYMBOLS):
        if not hasattr(probe, name):
            del L.SYMBOLS[name]


def _codes(rng, R, T):
    c = np.zeros((R, T), dtype=np.int32)
    c[0] = rng.integers(0, 4096, T)
    c[1:] = rng.integers(0, 1024, (R - 1, T))
    return c


def _times_ms(fn, rounds, warmup):
    times = []
    for r in range(warmup + rounds):
        t = time.perf_counter()
        fn()
        if r >= warmup:
            times.append(1e3 * (time.perf_counter() - t))
    return {"median": float(np.median(times)), "min": float(np.min(times)), "p90": float(np.percentile(times, 90))}


def _many(eng, kinds, chunks):
    """One decode_streams call per round over streams of `kinds` ((rate, speed) or None), restarted before max_frames."""
    def fresh():
        return [eng.stream() if k is None else eng.stream(k[0], speed=k[1]) for k in kinds]
    state = {"streams": fresh()}

    def call():
        s = state["streams"]
        if s[0].frames + 20 > eng.max_frames:
            for x in s:
                x.close()
            state["streams"] = s = fresh()
        eng.decode_streams(s, chunks)
    return call


def _single(eng, chunk):
    state = {"stream": eng.stream()}

    def call():
        if state["stream"].frames + 20 > eng.max_frames:
            state["stream"].close()
            state["stream"] = eng.stream()
        state["stream"].decode(chunk)
    return call


def _engine():
    from fish_tts_amd.codec_engine import CodecHipEngine
    return CodecHipEngine.synthetic(max_frames=2056)


def part_base(rounds, warmup):
    eng = _engine()
    rng = np.random.default_rng(0)
    one = _codes(rng, eng.R, 215)[None]
    chunks = [_codes(rng, eng.R, 20) for _ in range(32)]
    res = {"decode215": _times_ms(lambda: eng.decode(one), rounds, warmup),
           "stream20": _times_ms(_single(eng, chunks[0]), rounds, warmup),
           "many32x20": _times_ms(_many(eng, [None] * 32, chunks), rounds, warmup)}
    launches = eng.trace(lambda: eng.decode(one))[1]      # the one-shot decode's launches, in order
    res["trace"] = [f"{r['name']} {r['rows']}x{r['cols']} variant {r['variant']}" for r in launches]
    eng.close()
    return res


def _fmt(v):
    return f"{v['median']:.3f} ms (min {v['min']:.3f}, p90 {v['p90']:.3f})"


def part_compare(parent_lib, reps, rounds, warmup):
    runs = {"tree": [], "parent": []}
    for _ in range(reps):
        for who in ("parent", "tree"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", "base", "--json", "--rounds", str(rounds),
                   "--warmup", str(warmup)] + (["--lib", parent_lib] if who == "parent" else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
            runs[who].append(json.loads(out.strip().splitlines()[-1]))
    lines = [f"speed unset, tree against parent build: {reps} alternating runs each, medians of {rounds} calls after "
             f"{warmup} warm-up, one process per run"]
    for key in ("decode215", "stream20", "many32x20"):
        t = [r[key]["median"] for r in runs["tree"]]
        p = [r[key]["median"] for r in runs["parent"]]
        bound = max(p) + (max(p) - min(p))
        lines.append(f"{key}: parent {min(p):.3f} .. {max(p):.3f} ms, tree {min(t):.3f} .. {max(t):.3f} ms; parent's range "
                     f"widened by its spread ends at {bound:.3f} ms: {'within' if max(t) <= bound else 'ABOVE'}")
    tt, pt = runs["tree"][0]["trace"], runs["parent"][0]["trace"]
    lines.append(f"launch trace of the 215-frame decode (name, rows x cols, GEMM variant): {len(tt)} launches in the tree, "
                 f"{len(pt)} in the parent: {'equal line for line' if tt == pt else 'DIFFERENT'}")
    return lines


def part_speed(rounds, warmup):
    eng = _engine()
    rng = np.random.default_rng(0)
    one = _codes(rng, eng.R, 215)[None]
    lines = ["real codec shape, synthetic weights; host clock around synchronous calls, "
             f"{rounds} calls after {warmup} warm-up"]
    base = _times_ms(lambda: eng.decode(one), rounds, warmup)
    lines.append(f"215-frame decode (9.98 s of audio), speed unset: {_fmt(base)}")
    for speed in (0.5, 1.25, 2.0):
        v = _times_ms(lambda: eng.decode(one, speed=speed), rounds, warmup)
        frames = -(-int(215 * eng.frame_len / speed) // 512) + 1
        lines.append(f"215-frame decode at speed {speed}: {_fmt(v)}: +{v['median'] - base['median']:.3f} ms for {frames} "
                     f"frames of the stage, {1e3 * (v['median'] - base['median']) / frames:.2f} us per frame")
    chunks = [_codes(rng, eng.R, 20) for _ in range(32)]
    m = {}
    for name, kinds in (("speed unset", [None] * 32), ("half at 1.25", [None, (None, 1.25)] * 16),
                        ("all at 1.25", [(None, 1.25)] * 32)):
        m[name] = _times_ms(_many(eng, kinds, chunks), rounds, warmup)
    b = m["speed unset"]["median"]
    lines.append("32 x 20-frame decode_streams: " + "; ".join(
        f"{k} {_fmt(v)} ({100 * (v['median'] / b - 1):+.1f} %)" for k, v in m.items()))
    eng.close()
    return lines


def part_trace(calls):
    eng = _engine()
    rng = np.random.default_rng(0)
    chunks = [_codes(rng, eng.R, 20) for _ in range(32)]
    call = _many(eng, [None, (None, 1.25)] * 16, chunks)
    one = _codes(rng, eng.R, 215)[None]
    for _ in range(calls):
        call()
        for speed in (0.5, 1.25, 2.0):
            eng.decode(one, speed=speed)
    eng.close()
    return [f"trace: {calls} x (32 x 20-frame decode_streams, half at 1.25) + {calls} x 215-frame decode at 0.5, 1.25, 2.0"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["base", "compare", "speed", "trace"], default="speed")
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        _use_lib(a.lib)
    if a.part == "base":
        res = part_base(a.rounds, a.warmup)
        lines = [json.dumps(res)] if a.json else [f"{k}: {_fmt(v)}" for k, v in res.items() if k != "trace"] + \
            [f"launch trace of the 215-frame decode: {len(res['trace'])} launches"]
    elif a.part == "compare":
        if not a.parent_lib:
            ap.error("--part compare needs --parent-lib")
        lines = part_compare(a.parent_lib, a.reps, a.rounds, a.warmup)
    elif a.part == "speed":
        lines = part_speed(a.rounds, a.warmup)
    else:
        lines = part_trace(a.calls)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
