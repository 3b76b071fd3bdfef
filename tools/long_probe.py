"""Cost and gain of FishTTS.synthesize_long at s1-mini shapes, synthetic weights, max_batch 16: a text of `--segments`
sentences, every segment held at exactly `--frames` frames (<|im_end|> banned), one synthetic reference voice.

  --part wall:  (1) synthesize_long against a loop of synthesize over the same segments (the path a caller had before);
                (2) the codec side of the call alone on the segments' codes: decode_join (decode of every item + the three
                    join launches, one copy to the host), decode_join with the identity parameters, and the join stage
                    alone through its test hook on waveforms already decoded (upload + three launches + copy back);
                (3) the same join in numpy on the host after one decode (and one device-to-host copy) per segment.
                Host clock around the synchronous calls: warm-up first, then the median, minimum and 90th percentile of
                `--rounds`.
  --part trace: `--calls` decode_join calls of the same group (for a rocprofv3 --kernel-trace --stats run of its own: the
                device time of the three join kernels per call against the codec's kernels).
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


def _host_join(rows, jp, gaps):
    """The join stage in numpy (tests/join_ref.py restates it the same way)."""
    thr, hop, keep, fade = jp
    out, started = [], False
    for x, gap in zip(rows, gaps):
        idx = np.flatnonzero(np.abs(x) >= np.float32(thr))
        if not len(idx):
            continue
        a, e = max(0, int(idx[0]) // hop * hop - keep), min(len(x), (int(idx[-1]) // hop + 1) * hop + keep)
        y = x[a:e].copy()
        f = min(fade, (e - a) // 2)
        if f:
            ramp = ((2 * np.arange(f) + 1) / (2.0 * f)).astype(np.float32)
            y[:f] *= ramp
            y[len(y) - f:] *= ramp[::-1]
        if started:
            out.append(np.zeros(gap, dtype=np.float32))
        out.append(y)
        started = True
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--segments", type=int, default=12)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import fish_tts_amd as ft
    from fish_tts_amd.config import s1_mini_args
    from fish_tts_amd.longform import join_params, split_text
    from fish_tts_amd.tokenizer import ByteTokenizer
    synth = ft.FishTTS.synthetic(s1_mini_args(max_seq_len=4096), ByteTokenizer(), precision="bf16",
                                 max_new_tokens=2048 + 8, max_batch=a.max_batch)
    eng, codec = synth._engine, synth._vocoder
    plain = eng._sampling
    eng._sampling = lambda t, p, r, seed=0, ban_eos=False: plain(t, p, r, seed, True)     # every segment runs its full budget
    rng = np.random.default_rng(0)
    voice = [ft.VoiceProfile(codes=np.concatenate([rng.integers(0, 4096, (1, 100)), rng.integers(0, 1024, (9, 100))]),
                             text="a synthetic reference voice of one hundred frames")]
    text = " ".join(f"This is sentence number {i + 1} of the probe's long text." for i in range(a.segments))
    segs = [s.text for s in split_text(text)]
    assert len(segs) == a.segments, segs
    mt = a.frames + 1                     # the last generated column is dropped
    kw = dict(references=voice, max_tokens=mt)
    report = {"part": a.part, "segments": a.segments, "frames": a.frames, "max_batch": a.max_batch,
              "frame_path": eng.frame_path()}
    jp, gap, pgap = join_params(None)
    jp, gaps = tuple(jp), [gap] * a.segments
    # the segments' codes once, for the codec-side parts
    from fish_tts_amd.batch import run_batch
    with synth._gen_lock:
        _, utts = synth._batch_utterances(segs, voice, 0.7, 0.8, 1.1, mt, 0, None)
        run_batch(eng, utts)
    codes = [u.codes() for u in utts]
    print(f"long_probe: {a.segments} segments x {a.frames} frames, max_batch {a.max_batch}; {eng.frame_path()}", file=sys.stderr,
          flush=True)
    assert all(c.shape[1] == a.frames for c in codes), [c.shape for c in codes]
    if a.part == "wall":
        report["synthesize_long_ms"] = _times_ms(lambda: synth.synthesize_long(text, **kw), a.rounds, a.warmup)
        report["synthesize_loop_ms"] = _times_ms(lambda: [synth.synthesize(s, **kw) for s in segs], a.rounds, a.warmup)
        print("long_probe: wall times of the two synthesis paths done", file=sys.stderr, flush=True)
        report["speedup"] = report["synthesize_loop_ms"]["median"] / report["synthesize_long_ms"]["median"]
        report["tok_per_s_long"] = a.segments * a.frames / (1e-3 * report["synthesize_long_ms"]["median"])
        report["tok_per_s_loop"] = a.segments * a.frames / (1e-3 * report["synthesize_loop_ms"]["median"])
        report["decode_join_ms"] = _times_ms(lambda: codec.decode_join(codes, params=jp, gaps=gaps), 10, 2)
        report["decode_join_identity_ms"] = _times_ms(lambda: codec.decode_join(codes, gaps=gaps), 10, 2)
        rows = [codec.decode(c)[0] for c in codes]
        report["join_hook_ms"] = _times_ms(lambda: codec.test_join(rows, jp, gaps), 10, 2)
        report["decode_each_ms"] = _times_ms(lambda: [codec.decode(c)[0] for c in codes], 10, 2)
        report["host_join_ms"] = _times_ms(lambda: _host_join(rows, jp, gaps), 10, 2)
        dev, cuts = codec.decode_join(codes, params=jp, gaps=gaps)
        report["joined_samples"] = int(len(dev))
        report["input_samples"] = int(sum(len(r) for r in rows))
        report["equals_host_join"] = bool(np.array_equal(dev.view(np.uint32), _host_join(rows, jp, gaps).view(np.uint32)))
    else:
        for _ in range(a.calls):
            codec.decode_join(codes, params=jp, gaps=gaps)
        report["calls"] = a.calls
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
