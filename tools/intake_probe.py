"""Cost of the reference intake at the real codec shape, synthetic weights (intake_kernel and the chain behind it).

  --part wall:  (a) FishTTS.encode_reference_at (nothing trimmed, no level: the same codes) against FishTTS.encode_reference
                on the same 10 s and 30 s 48 kHz mono 16-bit WAV bytes, the two calls alternating; then encode_reference_at
                with its defaults (trim at -45 dB) and with a level.  (b) encode_references of `--clips` ten-second clips
                against as many single encode_reference_at calls.  Host clock around the synchronous calls; median, minimum
                and 90th percentile of `--rounds` after `--warmup`.
  --part trace: one encode_references call of `--clips` ten-second clips after one warm-up call of one clip (for a rocprofv3
                --kernel-trace --stats run of its own).
`--out FILE` appends the report to FILE as well.
"""
import argparse
import io
import json
import os
import sys
import time
import wave

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


def speech_like(seconds, rate, seed):
    """16-bit mono WAV bytes: a modulated tone with noise, half a second of room tone at either end."""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    x = 0.25 * np.sin(2 * np.pi * (140.0 + 10 * seed) * t) * (0.55 + 0.45 * np.sin(2 * np.pi * 2.5 * t)) + 0.02 * rng.standard_normal(n)
    edge = rate // 2
    x[:edge] = 0.001 * rng.standard_normal(edge)
    x[-edge:] = 0.001 * rng.standard_normal(edge)
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(np.round(np.clip(x, -1, 1) * 32767).astype(np.int16).tobytes())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import fish_tts_amd as ft
    from fish_tts_amd.codec_engine import CodecHipEngine
    eng = CodecHipEngine.synthetic(max_frames=1400, with_encoder=True)
    tts = ft.FishTTS.__new__(ft.FishTTS)
    tts._vocoder = eng
    tts._server = None
    report = {"part": a.part, "rate": a.rate, "clips": a.clips, "rounds": a.rounds, "warmup": a.warmup}
    ten = [(speech_like(10.0, a.rate, i), f"clip {i}") for i in range(a.clips)]
    if a.part == "wall":
        for seconds in (10.0, 30.0):
            b = speech_like(seconds, a.rate, 0)
            old = tts.encode_reference(b, "x")
            new = tts.encode_reference_at(b, "x", silence_db=None)
            rep = []
            tts.encode_reference_at(b, "x", loudness=-20.0, report=rep)
            key = f"{seconds:g}s"
            report[key] = {"frames": int(old.codes.shape[1]), "frames_at": int(new.codes.shape[1]), "frames_trimmed": rep[0].frames,
                           "lufs": rep[0].level.lufs, "gain": rep[0].level.gain}
            (report[key]["encode_reference_ms"], report[key]["encode_reference_at_ms"], report[key]["at_trim_ms"],
             report[key]["at_trim_level_ms"]) = _ms(
                [lambda: tts.encode_reference(b, "x"), lambda: tts.encode_reference_at(b, "x", silence_db=None),
                 lambda: tts.encode_reference_at(b, "x"), lambda: tts.encode_reference_at(b, "x", loudness=-20.0)], a.rounds, a.warmup)
        report["many"] = {}
        report["many"]["encode_references_ms"], report["many"]["single_calls_ms"] = _ms(
            [lambda: tts.encode_references(ten), lambda: [tts.encode_reference_at(b, t) for b, t in ten]], a.rounds, a.warmup)
    else:
        tts.encode_references(ten[:1])
        tts.encode_references(ten)
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
