"""Cost of the room stage at the real codec shape, synthetic weights (ft_codec_room: the response's intake, level and
resampler launches, room_ir_kernel, room_gain_kernel, room_send_kernel, room_conv_kernel, mix_scale_kernel).

  --part wall:  CodecHipEngine.room over `--seconds` of programme (default 60) at 44.1 kHz - what decode_join returns for as
                many five-second segments of random codes - under impulse responses of `--responses` seconds (default 1.5
                and 0.3; decaying noise, 44.1 kHz mono float32), and beside them decode_join of the same segments and
                CodecHipEngine.mix of the same programme under mix_probe's bed, for scale.  Host clock around the synchronous
                calls, all alternating; median, minimum and 90th percentile of `--rounds` after `--warmup`.  The report also
                holds the chain's operations, 2 N L, for the rate a kernel trace gives.
  --part trace: one room call per response over `--seconds` after one warm-up call over one second (for a rocprofv3
                --kernel-trace --stats run of its own).
`--out FILE` appends the report to FILE as well.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def response(seconds, rate=44100, seed=0):
    """Float32 mono WAV bytes: noise under an exponential decay of 60 dB over its length."""
    from tests.intake_ref import wav_bytes
    n = int(seconds * rate)
    v = 0.5 * np.random.default_rng(seed).standard_normal(n) * np.power(10.0, -3.0 * np.arange(n) / n)
    return wav_bytes(v.astype(np.float32), "f32", rate)


def main():
    from mix_probe import _ms, music
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--responses", type=float, nargs="+", default=[1.5, 0.3])
    ap.add_argument("--segment", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from fish_tts_amd.codec_engine import CodecHipEngine
    from fish_tts_amd.mix import Bed, bed_params
    from fish_tts_amd.room import Room, room_params
    from fish_tts_amd.wavfile import parse_wav
    eng = CodecHipEngine.synthetic(max_frames=1400)
    rng = np.random.default_rng(1)
    T = int(round(a.segment * 44100 / eng.frame_len))
    a_ = eng.args
    k = max(1, int(round(a.seconds / a.segment)))
    codes = [np.concatenate([rng.integers(0, a_.semantic_codebook_size, (1, T)),
                             rng.integers(0, a_.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(k)]
    x, _ = eng.decode_join(codes)
    x = (0.25 * x / max(1e-9, float(np.abs(x).max()))).astype(np.float32)      # a programme well under the ceiling
    rooms = []
    for s in a.responses:
        wav = response(s)
        rooms.append((s, (wav, parse_wav(wav)), room_params(Room(wav), 44100)))
    report = {"part": a.part, "seconds": a.seconds, "samples": len(x), "rounds": a.rounds, "warmup": a.warmup}
    if a.part == "wall":
        bed = music(30.0, 48000)
        bclip, mp = (bed, parse_wav(bed)), bed_params(Bed(bed, lead=1.0, tail=2.0), 44100)
        fns = [lambda: eng.decode_join(codes), lambda: eng.mix(x, bclip, params=mp)]
        for s, clip, rp in rooms:
            y, rep = eng.room(x, clip, params=rp)
            report[f"room_{s:g}s"] = {"n": rep.n, "taps": rep.taps, "capped": rep.capped, "peak": rep.peak, "chain_flop": 2.0 * rep.n * rep.taps}
            fns.append(lambda clip=clip, rp=rp: eng.room(x, clip, params=rp))
        ms = _ms(fns, a.rounds, a.warmup)
        report["decode_join_ms"], report["mix_ms"] = ms[0], ms[1]
        for (s, _, _), m in zip(rooms, ms[2:]):
            report[f"room_{s:g}s"]["room_ms"] = m
    else:
        eng.room(x[:44100], rooms[0][1], params=rooms[0][2])
        for s, clip, rp in rooms:
            eng.room(x, clip, params=rp)
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
