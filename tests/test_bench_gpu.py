"""bench.py's plain run the way it is called for every change: one JSON line whose ms_per_step is the time of one of the
--steps timed steps, none of --full's blocks, and --dump-outputs writing what the last timed step handed its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "FT_NO_GRAPH")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == "semantic tokens/sec" and out["unit"] == "tokens/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["steps"] == 2 and out["warmup"] == 1
    # value = 215 frames per step over the timed steps' wall clock = 215 / ms_per_step
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 215) < 1, out
    assert out["roofline"] is None and out["configs"] == {} and out["cpu_baseline"] is None

    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    from fish_tts_amd.tokenizer import ByteTokenizer
    tokens, audio = np.load(tmp_path / "tokens.npy"), np.load(tmp_path / "audio.npy")
    assert tokens.dtype == np.float64 and tokens.shape == (11, m.PROMPT_LEN + m.N_FRAMES)
    assert np.array_equal(tokens[:, : m.PROMPT_LEN], m.synth_prompt(ByteTokenizer()))
    assert (tokens == np.round(tokens)).all() and (tokens[1:, m.PROMPT_LEN:] >= 0).all()
    assert audio.dtype == np.float32 and audio.shape == (1, m.N_FRAMES * 2048) and np.isfinite(audio).all()
    assert float(np.abs(audio).max()) > 0
