"""Cost of the live room stage beside the room stage at the real codec shape, synthetic weights.
usage: room_live_probe.py LIB MODE [OUT.json]
LIB: the libfishtts_hip.so to load - this tree's, or one built from another commit, so that two commits are measured by the
     same script in one job, alternating (a library without the live symbols: they are left out of the table).
MODE: whole  ft_codec_room over a 60 s and a 10 s programme at 44.1 kHz under a 1.5 s response (66 150 taps): host clock around
             the call, which ends in a wait
      live   one push of a 10 s, a 1 s and a 20 ms group through a room stream under the 1.5 s and the 0.3 s response, with
             ft_codec_room of the same 10 s and decode_join of a 10 s group of four items beside them
      first  the bare limiter's push of the same 10 s; then, on the tiny synthetic models of the API tests, the time to the first
             chunk of synthesize_long_stream with and without live_room
      prof   a few calls of each, for a rocprofv3 --kernel-trace run of its own
Medians, minima and maxima of the timed calls after two warm-up calls; the report is one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lib, mode = sys.argv[1], sys.argv[2]
out_path = sys.argv[3] if len(sys.argv) > 3 else None

from fish_tts_amd import _lib as L  # noqa: E402

L.LIB_PATH = os.path.abspath(lib)
import ctypes as C  # noqa: E402

probe = C.CDLL(L.LIB_PATH)
has_live = hasattr(probe, "ft_codec_room_stream_begin")
if not has_live:
    for k in ("ft_codec_room_stream_begin", "ft_codec_room_stream_push", "ft_codec_room_stream_info", "ft_codec_room_stream_end",
              "ft_codec_room_live", "ft_codec_mix_stream_begin_bare"):
        L.SYMBOLS.pop(k, None)

from fish_tts_amd.codec_engine import CodecHipEngine  # noqa: E402
from fish_tts_amd.room import Room, room_params  # noqa: E402
from fish_tts_amd.wavfile import parse_wav  # noqa: E402
from tests.intake_ref import wav_bytes  # noqa: E402

RATE = 44100
rng = np.random.default_rng(1)


def ir(seconds):
    n = int(seconds * RATE)
    v = (0.5 * rng.standard_normal(n) * np.exp(-np.arange(n) / (0.25 * n))).astype(np.float32)
    b = wav_bytes(v, "f32", RATE)
    return b, parse_wav(b)


def med(f, reps, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), reps=reps)


eng = CodecHipEngine.synthetic(device=0, max_frames=440)
res = dict(lib=lib, mode=mode, has_live=has_live)
ir15, ir03 = ir(1.5), ir(0.3)
rp = room_params(Room(b"", wet_db=-12.0), RATE)
x60 = (0.1 * rng.standard_normal(60 * RATE)).astype(np.float32)
x10 = x60[:10 * RATE]

if mode == "whole":
    res["room_60s_ir1.5s"] = med(lambda: eng.room(x60, ir15, (), params=rp, ceiling=False), 8)
    res["room_10s_ir1.5s"] = med(lambda: eng.room(x10, ir15, (), params=rp, ceiling=False), 8)
elif mode == "live":
    for name, c in (("ir1.5s", ir15), ("ir0.3s", ir03)):
        rs = eng.room_stream(c, params=rp)
        rs.push(x10)
        res["push_10s_" + name] = med(lambda: rs.push(x10), 10)
        res["push_1s_" + name] = med(lambda: rs.push(x10[:RATE]), 10)
        res["push_20ms_" + name] = med(lambda: rs.push(x10[:882]), 10)
        rs.close()
        res["room_10s_" + name] = med(lambda: eng.room(x10, c, (), params=rp, ceiling=False), 8)
    T = 10 * RATE // eng.frame_len // 4
    a = eng.args
    codes = []
    for _ in range(4):
        c = rng.integers(0, a.codebook_size, (eng.R, T))
        c[0] = rng.integers(0, a.semantic_codebook_size, T)
        codes.append(c)
    res["frames_per_item"] = int(T)
    res["decode_join_10s"] = med(lambda: eng.decode_join(codes, gaps=[0, 100, 100, 100]), 6)
elif mode == "first":
    ms = eng.mix_stream(None, bedless=True)
    ms.push(x10)
    res["bare_push_10s"] = med(lambda: ms.push(x10), 10)
    ms.close()
    from tests.test_api_script_gpu import MT, SEED, TEXT, _voice
    from tests.test_api_serve_gpu import _tiny_tts
    tts = _tiny_tts()
    v = 0.5 * rng.standard_normal(300) * np.exp(-np.arange(300) / 75.0)
    small = Room(wav_bytes(v.astype(np.float32), "f32", RATE), fade=0.001)
    kw = dict(references=_voice(0, "v"), max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)

    def first(**k):
        t0 = time.perf_counter()
        gen = tts.synthesize_long_stream(TEXT, **kw, **k)
        c = next(gen)
        t1 = time.perf_counter()
        rest = list(gen)
        return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, len(c), 1 + len(rest)

    for name, k in (("plain", {}), ("live_room", dict(live_room=small))):
        for _ in range(2):
            first(**k)
        runs = [first(**k) for _ in range(7)]
        res["tiny_first_chunk_" + name] = dict(first_ms_median=float(np.median([r[0] for r in runs])),
                                                whole_ms_median=float(np.median([r[1] for r in runs])),
                                                first_chunk_bytes=runs[0][2], chunks=runs[0][3])
elif mode == "prof":
    for _ in range(4):
        eng.room(x60, ir15, (), params=rp, ceiling=False)
    if has_live:
        for name, c in (("ir1.5s", ir15), ("ir0.3s", ir03)):
            rs = eng.room_stream(c, params=rp)
            for _ in range(5):
                rs.push(x10)
            for _ in range(5):
                rs.push(x10[:882])
            rs.close()
eng.close()
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
