"""Cost and gain of FishTTS.synthesize_script at s1-mini shapes, synthetic weights, max_batch 16: a script of `--lines`
lines in three synthetic voices, every line one segment held at exactly `--frames` frames (<|im_end|> banned), in runs of
three lines slow, pitched and at a level of their own (of twelve lines: six slow, three pitched, three levelled).

  (1) synthesize_script: all lines as one lock-step batch, every voice's prefix from the cache, one decode_join with a
      chain per item;
  (2) the path a caller had before: one synthesize_at call per line with that line's voice and values (the join in numpy
      that would follow is not timed).
Host clock around the synchronous calls: warm-up first, then the median, minimum and 90th percentile of `--rounds`.
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
    ap.add_argument("--lines", type=int, default=12)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import fish_tts_amd as ft
    from fish_tts_amd.config import s1_mini_args
    from fish_tts_amd.script import plan_script
    from fish_tts_amd.tokenizer import ByteTokenizer
    synth = ft.FishTTS.synthetic(s1_mini_args(max_seq_len=4096), ByteTokenizer(), precision="bf16",
                                 max_new_tokens=2048 + 8, max_batch=a.max_batch)
    eng = synth._engine
    plain = eng._sampling
    eng._sampling = lambda t, p, r, seed=0, ban_eos=False: plain(t, p, r, seed, True)     # every line runs its full budget
    rng = np.random.default_rng(0)
    voices = {name: [ft.VoiceProfile(codes=np.concatenate([rng.integers(0, 4096, (1, 100)), rng.integers(0, 1024, (9, 100))]),
                                     text=f"a synthetic reference voice of one hundred frames, called {name}")]
              for name in ("anna", "ben", "carl")}
    names = list(voices)
    styles = [dict(speed=0.8), dict(pitch=2.0), dict(loudness=-20.0)]
    lines = [ft.Line(f"This is line number {i + 1} of the probe's script.", voice=names[i % 3], **styles[(i // 3) % 3])
             for i in range(a.lines)]
    assert len(plan_script(lines, voices).texts) == a.lines
    mt = a.frames + 1                     # the last generated column is dropped
    report = {"lines": a.lines, "voices": len(voices), "frames": a.frames, "max_batch": a.max_batch, "frame_path": eng.frame_path()}
    print(f"script_probe: {a.lines} lines x {a.frames} frames, max_batch {a.max_batch}; {eng.frame_path()}", file=sys.stderr, flush=True)

    def one_by_one():
        return [synth.synthesize_at(ln.text, references=voices[ln.voice], max_tokens=mt, speed=ln.speed, pitch=ln.pitch,
                                    loudness=ln.loudness) for ln in lines]

    report["synthesize_script_ms"] = _times_ms(lambda: synth.synthesize_script(lines, voices, max_tokens=mt), a.rounds, a.warmup)
    report["synthesize_at_loop_ms"] = _times_ms(one_by_one, a.rounds, a.warmup)
    report["speedup"] = report["synthesize_at_loop_ms"]["median"] / report["synthesize_script_ms"]["median"]
    report["tok_per_s_script"] = a.lines * a.frames / (1e-3 * report["synthesize_script_ms"]["median"])
    report["tok_per_s_loop"] = a.lines * a.frames / (1e-3 * report["synthesize_at_loop_ms"]["median"])
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
