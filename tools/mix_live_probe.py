"""Cost of the live mix stage at the real codec shape, synthetic weights (ft_codec_mix_stream_push: mixl_hop_kernel,
mixl_node_kernel, mixl_sample_kernel, mixl_limit_kernel, mixl_apply_kernel).

  --part push:  one push of a joined group of `--seconds` (default 10 and 60) at 44.1 kHz - what decode_join returns for as
                many five-second segments of random codes - into an open stream under a 30 s looped 48 kHz stereo 16-bit bed,
                and beside it decode_join of the same group, for scale.  The stream stays open over the rounds, so every push
                is a push in the middle of a stream.  Host clock around the synchronous calls, the two alternating; median,
                minimum and 90th percentile of `--rounds` after `--warmup`.  Opening a stream (the bed's preparation) apart.
  --part ttfa:  time from the call to the first chunk of synthesize_long_stream - real model shape, synthetic weights,
                `--segments` sentences of `--frames` frames - without live_bed, with a live bed of lead 0 and with a lead of
                2 s; median, minimum and 90th percentile of `--calls` after one warm-up, the three alternating.  The stage
                holds back (Wa + La + 2) hops at most: 22 hops, 0.44 s of audio, at the default attack.
  --part trace: three pushes of the first of `--seconds` into one stream after a warm-up stream (for a rocprofv3
                --kernel-trace --stats run of its own).
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

from tools.mix_probe import _ms, music  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("push", "ttfa", "trace"), default="push")
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 60.0])
    ap.add_argument("--segment", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--segments", type=int, default=6)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    from fish_tts_amd.mix import Bed, bed_params
    from fish_tts_amd.wavfile import parse_wav
    wav = music(30.0, 48000)
    clip = (wav, parse_wav(wav))
    report = {"part": a.part, "rounds": a.rounds, "warmup": a.warmup, "bed": "30 s 48 kHz stereo s16, looped"}
    if a.part == "ttfa":
        import fish_tts_amd as ft
        from fish_tts_amd.config import s1_mini_args
        from fish_tts_amd.tokenizer import ByteTokenizer
        synth = ft.FishTTS.synthetic(s1_mini_args(max_seq_len=4096), ByteTokenizer(), precision="bf16", max_new_tokens=2048 + 8,
                                     max_batch=2)          # two segments at a time: the first group is ready while the rest generates
        eng = synth._engine
        plain = eng._sampling
        eng._sampling = lambda t, p, r, seed=0, ban_eos=False: plain(t, p, r, seed, True)     # every segment runs its full budget
        rng = np.random.default_rng(0)
        voice = [ft.VoiceProfile(codes=np.concatenate([rng.integers(0, 4096, (1, 100)), rng.integers(0, 1024, (9, 100))]),
                                 text="a synthetic reference voice of one hundred frames")]
        text = " ".join(f"This is sentence number {i + 1} of the probe's long text." for i in range(a.segments))
        kw = dict(references=voice, max_tokens=a.frames + 1, silence_db=None)

        def first(bed):
            def run():
                gen = synth.synthesize_long_stream(text, live_bed=bed, **kw)
                t0 = time.perf_counter()
                chunk = next(gen)
                dt = 1e3 * (time.perf_counter() - t0)
                rest = sum(len(c) for c in gen)
                run.last = (dt, len(chunk) // 2, rest // 2)
            return run
        runs = [first(None), first(Bed(wav, lead=0.0)), first(Bed(wav, lead=2.0))]
        ts = [[] for _ in runs]
        for r in range(1 + a.calls):
            for fn, t in zip(runs, ts):
                fn()
                if r >= 1:
                    t.append(fn.last[0])
        for name, fn, t in zip(("plain", "lead0", "lead2s"), runs, ts):
            report[name] = {"first_chunk_ms": {"median": float(np.median(t)), "min": float(np.min(t)), "p90": float(np.percentile(t, 90))},
                            "first_chunk_samples": fn.last[1], "rest_samples": fn.last[2]}
        report.update(segments=a.segments, frames=a.frames, calls=a.calls, frame_path=eng.frame_path(),
                      hold_back_samples=22 * 882, hold_back_ms=440.0)
    else:
        from fish_tts_amd.codec_engine import CodecHipEngine
        eng = CodecHipEngine.synthetic(max_frames=1400)
        mp = bed_params(Bed(wav), 44100)
        rng = np.random.default_rng(1)
        T = int(round(a.segment * 44100 / eng.frame_len))
        a_ = eng.args

        def segments(seconds):
            k = max(1, int(round(seconds / a.segment)))
            return [np.concatenate([rng.integers(0, a_.semantic_codebook_size, (1, T)),
                                    rng.integers(0, a_.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(k)]
        if a.part == "push":
            report["segment_frames"] = T
            for seconds in a.seconds:
                codes = segments(seconds)
                x, _ = eng.decode_join(codes)
                x = (0.25 * x / max(1e-9, float(np.abs(x).max()))).astype(np.float32)      # a programme well under the ceiling
                y, rep = eng.mix_live(x, clip, params=mp)
                key = f"{seconds:g}s"
                report[key] = {"samples": len(x), "mixed": rep.n, "bed_len": rep.bed_len, "hops": rep.hops, "active": rep.active,
                               "limit_max": rep.limit_max, "peak": rep.peak}
                ms = eng.mix_stream(clip, params=mp)
                ms.push(x)
                report[key]["push_ms"], report[key]["decode_join_ms"] = _ms([lambda: ms.push(x), lambda: eng.decode_join(codes)],
                                                                            a.rounds, a.warmup)
                ms.close()

                def open_close():
                    eng.mix_stream(clip, params=mp).close()
                report[key]["open_close_ms"] = _ms([open_close], a.rounds, a.warmup)[0]
        else:
            x, _ = eng.decode_join(segments(a.seconds[0]))
            with eng.mix_stream(clip, params=mp) as ms:
                ms.push(x[:44100])
            with eng.mix_stream(clip, params=mp) as ms:
                for _ in range(3):
                    ms.push(x)
                ms.push(None, final=True)
        eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
