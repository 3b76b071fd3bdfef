"""Cost of the stereo mix stage at the real codec shape, synthetic weights (ft_codec_mix_stereo: the two sides' intake, the
pair level, the resampler, mix_hop_kernel, mix_node_kernel, mix_stereo_kernel, mix_scale_kernel), beside the mix stage.

  --part wall:  CodecHipEngine.mix_stereo over `--seconds` of programme (default 60) at 44.1 kHz - what decode_join returns
                for as many five-second segments of random codes, one pan region per segment, left and right in turn - under
                tools/mix_probe.py's 30 s looped 48 kHz stereo 16-bit bed, and beside it CodecHipEngine.mix of the same
                programme under the same bed.  Host clock around the synchronous calls, the two alternating; median,
                minimum and 90th percentile of `--rounds` after `--warmup`.
  --part trace: one mix_stereo call and one mix call over `--seconds` after one warm-up call of each over one second (for a
                rocprofv3 --kernel-trace --stats run of its own).
`--out FILE` appends the report to FILE as well.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("wall", "trace"), default="wall")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--segment", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from mix_probe import _ms, music

    from fish_tts_amd.codec_engine import CodecHipEngine
    from fish_tts_amd.mix import Bed, bed_params
    from fish_tts_amd.wavfile import parse_wav
    eng = CodecHipEngine.synthetic(max_frames=1400)
    wav = music(30.0, 48000)
    clip = (wav, parse_wav(wav))
    mp = bed_params(Bed(wav, lead=1.0, tail=2.0), 44100)
    rng = np.random.default_rng(1)
    T = int(round(a.segment * 44100 / eng.frame_len))
    a_ = eng.args
    k = max(1, int(round(a.seconds / a.segment)))
    codes = [np.concatenate([rng.integers(0, a_.semantic_codebook_size, (1, T)),
                             rng.integers(0, a_.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(k)]
    x, cuts = eng.decode_join(codes)
    x = (0.25 * x / max(1e-9, float(np.abs(x).max()))).astype(np.float32)      # a programme well under the ceiling
    edges = np.linspace(0, len(x), k + 1).astype(np.int64)
    regions = [(int(edges[i]), int(edges[i + 1]), -50 if i % 2 == 0 else 50) for i in range(k)]
    report = {"part": a.part, "seconds": a.seconds, "samples": len(x), "regions": len(regions), "rounds": a.rounds,
              "warmup": a.warmup, "bed": "30 s 48 kHz stereo s16, looped"}
    if a.part == "wall":
        y, rep = eng.mix_stereo(x, clip, regions, params=mp)
        m, mrep = eng.mix(x, clip, params=mp)
        report.update(frames=rep.n, bed_len=rep.bed_len, capped=rep.capped, bed_lufs=rep.bed.level.lufs,
                      bed_gain=rep.bed.level.gain, mono_bed_lufs=mrep.bed.level.lufs, bytes_to_host=int(y.nbytes),
                      mono_bytes_to_host=int(m.nbytes))
        report["mix_stereo_ms"], report["mix_ms"] = _ms(
            [lambda: eng.mix_stereo(x, clip, regions, params=mp), lambda: eng.mix(x, clip, params=mp)], a.rounds, a.warmup)
    else:
        eng.mix_stereo(x[:44100], clip, [(0, 44100, -50)], params=mp)
        eng.mix(x[:44100], clip, params=mp)
        eng.mix_stereo(x, clip, regions, params=mp)
        eng.mix(x, clip, params=mp)
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
