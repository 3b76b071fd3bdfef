"""Cost of the FLAC stage at the real codec shape, synthetic weights (ft_codec_flac: flac_analyse_kernel, flac_pack_kernel,
flac_scan_kernel, flac_gather_kernel).

  --part wall:  CodecHipEngine.flac over `--seconds` of programme (default 60) at 44.1 kHz, B = `--blocksize` (default 4096),
                mono and stereo - the speech-like signal of tests/flac_cases.py, the second channel a scaled copy with a
                little of another voice - and beside it, in the same process, decode_join of as many five-second segments
                of random codes and the host path the stage replaces: a float32 copy of the programme off the device
                (torch, pinned neither way) plus FishTTS._to_wav_bytes.  Host clock around the synchronous calls, all
                alternating; median, minimum and 90th percentile of `--rounds` after `--warmup`.  The report also holds
                the stream's bytes over the PCM bytes, and the FlacReport.
  --part trace: one mono and one stereo call over `--seconds` after one warm-up call over one second (for a rocprofv3
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


def main():
    from mix_probe import _ms
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--blocksize", type=int, default=4096)
    ap.add_argument("--segment", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from fish_tts_amd.codec_engine import CodecHipEngine
    from fish_tts_amd.synthesizer import FishTTS
    from tests.flac_cases import speech
    eng = CodecHipEngine.synthetic(max_frames=1400)
    n = int(a.seconds * 44100)
    mono = speech(n, seed=3)
    stereo = np.ascontiguousarray(np.stack([mono, 0.8 * mono + 0.05 * speech(n, seed=4)], 1).astype(np.float32))
    report = {"part": a.part, "seconds": a.seconds, "samples": n, "blocksize": a.blocksize, "rounds": a.rounds, "warmup": a.warmup}
    if a.part == "wall":
        rng = np.random.default_rng(1)
        T = int(round(a.segment * 44100 / eng.frame_len))
        k = max(1, int(round(a.seconds / a.segment)))
        codes = [np.concatenate([rng.integers(0, eng.args.semantic_codebook_size, (1, T)),
                                 rng.integers(0, eng.args.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(k)]
        dev = {"mono": torch.from_numpy(mono).cuda(), "stereo": torch.from_numpy(stereo).cuda()}

        def host_path(name):
            x = dev[name].cpu().numpy()                    # the float32 copy-back of today's path ...
            return FishTTS._to_wav_bytes(x, 44100)         # ... and the int16 conversion on the host

        fns = [lambda: eng.decode_join(codes)]
        for name, x in (("mono", mono), ("stereo", stereo)):
            data, rep = eng.flac(x, 44100, a.blocksize)
            report[name] = {"bytes": len(data), "pcm_bytes": 2 * x.size, "ratio": len(data) / (2 * x.size), "frames": rep.frames,
                            "min_frame": rep.min_frame, "max_frame": rep.max_frame, "kinds": rep.kinds, "assignments": rep.assignments,
                            "wav_bytes": len(host_path(name))}
            fns += [lambda x=x: eng.flac(x, 44100, a.blocksize), lambda name=name: host_path(name)]
        ms = _ms(fns, a.rounds, a.warmup)
        report["decode_join_ms"] = ms[0]
        report["mono"]["flac_ms"], report["mono"]["host_path_ms"] = ms[1], ms[2]
        report["stereo"]["flac_ms"], report["stereo"]["host_path_ms"] = ms[3], ms[4]
    else:
        eng.flac(mono[:44100], 44100, a.blocksize)
        eng.flac(mono, 44100, a.blocksize)
        eng.flac(stereo, 44100, a.blocksize)
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
