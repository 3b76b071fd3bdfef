"""The codebook loop's resident form (csrc/frame_engine.h: fast_engine_kernel<.., true>): the gathering waves keep W13
pairs of every codebook-loop layer in registers from kernel entry on and compute them beside the compute waves.  Which
wave computes a row does not enter its arithmetic, so the frames must equal, token for token, the all-streaming form
(FT_NO_RESIDENT=1) and the launch path (FT_NO_ENGINE=1).

Shape: the real s1-mini widths with 2 slow layers and all 4 codebook-loop layers (the resident set lives in the loop's
layers).  One utterance of 20 frames: frame 0 draws with no repetition penalty, frames 17.. have left the 16-frame
penalty window's growing phase."""
import dataclasses

import numpy as np
import pytest

from tests.hip_util import make_pair
from tests.shapes import make_prompt
from tests.test_ar_gpu import medium_shape

pytestmark = pytest.mark.gpu

N_FRAMES = 20
SWITCHES = ("FT_NO_ENGINE", "FT_NO_FAST_ENGINE", "FT_NO_RESIDENT")


def _frames(monkeypatch, shape, prompt, kw, switch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    eng, _ = make_pair(shape, "bf16", max_new_tokens=N_FRAMES + 8)
    try:
        flags = eng.engine_state()[0]
        path = eng.frame_path()
        seq = eng.generate(prompt, N_FRAMES, **kw)
        strikes = eng.engine_state()[1]
    finally:
        eng.close()
    return flags, strikes, path, seq


@pytest.mark.parametrize("kw", [dict(temperature=0.7, top_p=1e-6, repetition_penalty=1.1),
                                dict(temperature=0.7, top_p=0.8, repetition_penalty=1.1, seed=7)],
                         ids=["greedy", "top_p_0.8_seeded"])
def test_resident_streaming_and_launch_frames_are_identical(monkeypatch, kw):
    shape = dataclasses.replace(medium_shape(n_fast_layer=4), max_seq_len=1024)
    prompt = make_prompt(shape, 20, seed=31, n_vq=2).numpy()
    fr, sr, pr, res = _frames(monkeypatch, shape, prompt, kw, None)
    fs, ss, ps, stream = _frames(monkeypatch, shape, prompt, kw, "FT_NO_RESIDENT")
    fl, _, _, launch = _frames(monkeypatch, shape, prompt, kw, "FT_NO_ENGINE")
    assert (fr, sr) == (3, 0), (fr, sr, pr)
    assert (fs, ss) == (3, 0), (fs, ss, ps)
    assert fl == 0
    assert "resident in the gathering waves" in pr, pr          # the runs really took the forms they are named after
    assert "FT_NO_RESIDENT" in ps and "resident in" not in ps, ps
    assert res.shape == launch.shape and res.shape[1] >= prompt.shape[1] + N_FRAMES, (res.shape, launch.shape)
    assert np.array_equal(res, stream)
    assert np.array_equal(res, launch)
    assert np.array_equal(stream, launch)
