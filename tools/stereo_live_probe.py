"""Cost of the live stereo mix stage at the real codec shape, synthetic weights (ft_codec_mix_stream_push_stereo:
mixl_hop_kernel, mixl_node_kernel, mixls_pan_kernel, mixls_sample_kernel, mixl_limit_kernel, mixls_apply_kernel), beside the
mono live mix stage in the same call.

  --part push:  one stereo push of a joined group of `--seconds` (default 10 and 60) at 44.1 kHz - what decode_join returns
                for as many five-second segments of random codes - with one region per segment at alternating places, into an
                open stereo stream under a 30 s looped 48 kHz stereo 16-bit bed, and beside it the mono push of the same group
                into an open mono stream under the same bed.  Both streams stay open over the rounds, so every push is a push
                in the middle of a stream.  Host clock around the synchronous calls, the two alternating; median, minimum and
                90th percentile of `--rounds` after `--warmup`.  Opening a stereo stream beside opening a mono one, apart.
  --part trace: three pushes of the first of `--seconds` into one stereo and into one mono stream after a warm-up stream of each
                (for a rocprofv3 --kernel-trace --stats run of its own).
`--out FILE` appends the report to FILE as well.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mix_probe import _ms, music  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("push", "trace"), default="push")
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 60.0])
    ap.add_argument("--segment", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from fish_tts_amd.codec_engine import CodecHipEngine
    from fish_tts_amd.mix import Bed, bed_params
    from fish_tts_amd.wavfile import parse_wav
    wav = music(30.0, 48000)
    clip = (wav, parse_wav(wav))
    report = {"part": a.part, "rounds": a.rounds, "warmup": a.warmup, "bed": "30 s 48 kHz stereo s16, looped"}
    eng = CodecHipEngine.synthetic(max_frames=1400)
    mp = bed_params(Bed(wav), 44100)
    rng = np.random.default_rng(1)
    T = int(round(a.segment * 44100 / eng.frame_len))
    a_ = eng.args

    def group(seconds):
        k = max(1, int(round(seconds / a.segment)))
        codes = [np.concatenate([rng.integers(0, a_.semantic_codebook_size, (1, T)),
                                 rng.integers(0, a_.codebook_size, (eng.R - 1, T))]).astype(np.int32) for _ in range(k)]
        x, _ = eng.decode_join(codes)
        x = (0.25 * x / max(1e-9, float(np.abs(x).max()))).astype(np.float32)      # a programme well under the ceiling
        edges = np.linspace(0, len(x), k + 1).astype(np.int64)
        return x, [(int(edges[j]), int(edges[j + 1]), -50 if j % 2 == 0 else 50) for j in range(k)]

    if a.part == "push":
        report["segment_frames"] = T
        for seconds in a.seconds:
            x, regions = group(seconds)
            y, rep = eng.mix_live_stereo(x, clip, regions, params=mp)
            key = f"{seconds:g}s"
            report[key] = {"samples": len(x), "regions": len(regions), "mixed": rep.n, "bed_len": rep.bed_len, "hops": rep.hops,
                           "active": rep.active, "limit_max": rep.limit_max, "peak": rep.peak}
            st, mo = eng.mix_stream(clip, params=mp, stereo=True), eng.mix_stream(clip, params=mp)
            st.push(x, regions)
            mo.push(x)
            report[key]["stereo_push_ms"], report[key]["mono_push_ms"] = _ms([lambda: st.push(x, regions), lambda: mo.push(x)],
                                                                             a.rounds, a.warmup)
            st.close()
            mo.close()

            def open_stereo():
                eng.mix_stream(clip, params=mp, stereo=True).close()

            def open_mono():
                eng.mix_stream(clip, params=mp).close()
            report[key]["stereo_open_close_ms"], report[key]["mono_open_close_ms"] = _ms([open_stereo, open_mono], a.rounds, a.warmup)
    else:
        x, regions = group(a.seconds[0])
        for stereo in (True, False):
            extra = (regions,) if stereo else ()
            with eng.mix_stream(clip, params=mp, stereo=stereo) as ms:
                ms.push(x[:44100])
            with eng.mix_stream(clip, params=mp, stereo=stereo) as ms:
                for _ in range(3):
                    ms.push(x, *extra)
                ms.push(None, final=True)
    eng.close()
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
