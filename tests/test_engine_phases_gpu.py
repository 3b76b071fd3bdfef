"""GPU: the persistent frame engine (csrc/frame_engine.h) held to float64 PHASE BY PHASE.  The engine was judged through the
launch path alone - tokens, the vocabulary logits and the slow hidden state after the last frame (tests/test_engine_gpu.py,
test_engine_long_context_gpu.py, test_engine_resident_gpu.py) - which sees the codebook loop through its draws only: a
written but wrong granule (another layer's gain in one wave's rows, a history row one position off, one workgroup's slice
from a stale embedding row) moves a 1024-way logit vector a little and flips a top-p 0.8 draw rarely.

Here every vector a phase hands over is read back after the launch (ft_test_engine_handoffs: the last two codebook steps at
every loop layer, the last two slow layers, the replicas, the epoch) and every planned phase is recomputed in float64 from
its RECORDED input by tests/engine_phase_ref.py under tests/ar_ref.check's bound, unchanged; every unit must carry its
launch's tag, every replica unit under that tag must equal the source, and the plan must account for every (step, layer,
phase) of the last two steps / layers: checked, or listed as not handed off.  The loop's K/V history is a launch-path twin's
(same weights, prompt and sampling under FT_NO_ENGINE, equal tokens asserted); at two codebooks the engine's own records.

Shapes: the s1-mini widths (the smallest the engine is instantiated for), 2 slow layers, a 4 224-row vocabulary, a
20-position prompt, prefill + decode(1): the hook is read after the prompt pass's first frame and after each of 20 frames
(frame 0 draws without a penalty window, frames 17.. are past its growth)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import engine_phase_ref as E
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import make_prompt
from tests.test_ar_gpu import medium_shape

pytestmark = pytest.mark.gpu

N_FRAMES, LP = 20, 20
SWITCHES = ("FT_NO_ENGINE", "FT_NO_FAST_ENGINE", "FT_NO_RESIDENT", "FT_NO_PAIR", "FT_NO_QKV0", "FT_NO_RELAY", "FT_NO_XL")
GREEDY = dict(temperature=0.7, top_p=1e-6, repetition_penalty=1.1, seed=0)
SEEDED = dict(temperature=0.7, top_p=0.8, repetition_penalty=1.1, seed=7)
_W = {}
STATS = E.Report()
CASES = []


def base_shape(max_seq_len=1024, **over):
    kw = dict(n_text=113, n_fast_layer=4)
    kw.update(over)
    return dataclasses.replace(medium_shape(**kw), max_seq_len=max_seq_len)


def weights(shape):
    """The float64 side's weights, once per shape (they do not depend on max_seq_len but for the rope table)."""
    key = tuple(sorted((k, str(v)) for k, v in shape.__dict__.items()))
    if key not in _W:
        _W.clear()
        sd = cached_random_weights(shape, seed=0)
        _W[key] = (E.loop_weights(sd, shape), E.slow_weights(sd, shape))
    return _W[key]


def context(shape, env, max_new):
    from fish_tts_amd.ar_engine import ARHipEngine
    saved = {n: os.environ.get(n) for n in SWITCHES}
    for n in SWITCHES:
        os.environ.pop(n, None)
    os.environ.update({n: "1" for n in env})
    try:
        eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                          precision="bf16", device=0, max_batch=1, max_new_tokens=max_new)
        eng.load_state_dict({k: v.to(torch.bfloat16) for k, v in cached_random_weights(shape, seed=0).items()})
    finally:
        for n, v in saved.items():
            os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
    return eng


def twin_history(shape, prompt, kw, n_frames, env=()):
    """The launch path on the same weights, prompt, sampling and switches (FT_NO_XL changes the launch path's KV split count
    too): per frame its tokens and, per loop layer, the codebook-loop K/V cache fast_attn_kernel left."""
    tw = context(shape, ("FT_NO_ENGINE",) + tuple(env), n_frames + 8)
    try:
        assert tw.engine_state()[0] == 0, tw.frame_path()
        sp = tw._sampling(ban_eos=True, **kw)
        toks, hist = [tw.prefill(prompt, sp)], []
        for f in range(n_frames + 1):
            if f:
                fr, n = tw.decode(1, [sp])
                assert n[0] == 1
                toks.append(fr[0, 0].copy())
            kv = [tw.engine_handoffs(1, vectors=False, kv=(li, 0, shape.num_codebooks)) for li in range(shape.n_fast_layer)]
            hist.append([(d["kv_k"], d["kv_v"]) for d in kv])
    finally:
        tw.close()
    return toks, hist


def collect(shape, env=(), kw=SEEDED, lp=LP, n_frames=N_FRAMES, prompt_seed=31):
    """One engine context driven frame by frame; returns (hook geometry of the loop, loop frames, slow frames, frame path)."""
    prompt = make_prompt(shape, lp, seed=prompt_seed, n_vq=2).numpy()
    ncb, nLs = shape.num_codebooks, shape.n_layer
    twin = twin_history(shape, prompt, kw, n_frames, env) if ncb > 2 else None
    eng = context(shape, env, n_frames + 8)
    try:
        flags, path = eng.engine_state()[0], eng.frame_path()
        assert flags == 3, f"the engine refused this case (flags {flags}): {path}"
        sp = eng._sampling(ban_eos=True, **kw)
        loop, slow, toks = [], [], [eng.prefill(prompt, sp)]
        for f in range(n_frames + 1):
            if f:
                fr, n = eng.decode(1, [sp])
                assert n[0] == 1
                toks.append(fr[0, 0].copy())
            rec = eng.engine_handoffs(1)
            cfg = E.LoopCfg.of(rec)
            tabs = {s: eng.engine_handoffs(1, vectors=False, tab_row=int(toks[f][s]))["tab"] for s in E.loop_steps(cfg) if cfg.qkv0 and s >= 2}
            loop.append(E.LoopFrame(rec, eng.debug_state()[1], toks[f], None if twin is None else twin[1][f], tabs))
            if f:                                   # the first frame's slow pass is the prompt pass: no slow-stack launch
                pos = lp + f - 1
                srec = eng.engine_handoffs(0)
                caches = {}
                for li in E.slow_layers(nLs):
                    d = eng.engine_handoffs(0, vectors=False, kv=(li, 0, pos + 1))
                    caches[li] = (d["kv_k"], d["kv_v"])
                slow.append(E.SlowFrame(srec, pos, toks[f - 1], caches, loop[-1].hid))
        strikes = eng.engine_state()[1]
    finally:
        eng.close()
    assert strikes == 0, "a hand-off timed out"
    if twin is not None:
        assert np.array_equal(np.stack(toks), np.stack(twin[0])), "the engine's frames differ from the launch-path twin's"
    return cfg, loop, slow, path


def not_handed_loop(cfg):
    """What the kernels do not hand off, restated from frame_engine.h without the plan."""
    out = set()
    for s in E.loop_steps(cfg):
        if cfg.qkv0 and s >= 2:
            out.add((s, 0, "qkv"))
        if cfg.pair and s == 0:
            out |= {(0, cfg.n_layer - 1, k) for k in ("attn_wo", "w13", "w2")}
        if s == 0:
            out.add((0, cfg.n_layer, "head"))
    return out


def judge_loop(shape, cfg, frames, what):
    rep = E.check_loop(cfg, weights(shape)[0], frames)
    print(f"{what}: loop {rep.phases} phases, {rep.units} units, {rep.tag_units} tags, {rep.replica_units} replica units under the tag; "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(rep.worst.items())))
    assert set(rep.listed) == E.loop_phase_keys(cfg), set(rep.listed) ^ E.loop_phase_keys(cfg)
    assert {k for k, st in rep.listed.items() if st == E.NOT_HANDED} == not_handed_loop(cfg)
    assert {k for k, st in rep.listed.items() if st == E.CHECKED} <= rep.checked
    assert not rep.flagged, f"{what}: " + "\n".join(rep.flagged[:10])
    assert all(not f.rec["code"].any() for f in frames), "the code lines are written: the plan says every workgroup draws for itself"
    STATS.merge(rep)
    return rep


def judge_slow(shape, frames, what):
    rep = E.check_slow(weights(shape)[1], frames)
    print(f"{what}: slow stack {rep.phases} phases, {rep.units} units, {rep.tag_units} tags, {rep.replica_units} replica units under the tag; "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(rep.worst.items())))
    assert set(rep.listed) == E.slow_phase_keys(shape.n_layer), set(rep.listed) ^ E.slow_phase_keys(shape.n_layer)
    assert {k for k, st in rep.listed.items() if st == E.CHECKED} <= rep.checked
    assert not rep.flagged, f"{what}: " + "\n".join(rep.flagged[:10])
    STATS.merge(rep)
    return rep


@pytest.mark.parametrize("kw", [GREEDY, SEEDED], ids=["greedy", "top_p_0.8_seeded"])
@pytest.mark.parametrize("ncb", range(2, 11))
def test_codebook_counts_resident_form(ncb, kw):
    """2 .. 10 codebooks at four loop layers: the last two steps of these nine contexts are every step index of the real loop
    at every layer (two: the paired pass is the whole loop, no table, no twin; three: one table step)."""
    shape = base_shape(num_codebooks=ncb)
    cfg, loop, slow, path = collect(shape, kw=kw)
    assert "resident in the gathering waves" in path and cfg.resident, path
    assert cfg.pair and cfg.qkv0 == (ncb > 2) and cfg.pk3, cfg
    judge_loop(shape, cfg, loop, f"{ncb} codebooks")
    judge_slow(shape, slow, f"{ncb} codebooks")
    CASES.append(f"ncb {ncb}")


@pytest.mark.parametrize("env", ["FT_NO_RESIDENT", "FT_NO_PAIR", "FT_NO_QKV0", "FT_NO_RELAY", "FT_NO_XL"])
def test_forms_at_ten_codebooks(env):
    shape = base_shape()
    cfg, loop, slow, path = collect(shape, env=(env,))
    assert cfg.resident == (env != "FT_NO_RESIDENT") and cfg.pair == (env != "FT_NO_PAIR") and cfg.qkv0 == (env != "FT_NO_QKV0"), (cfg, path)
    assert loop[0].rec["relay"] == (env != "FT_NO_RELAY") and loop[0].rec["copies"] == (1 if env == "FT_NO_RELAY" else 9)
    assert slow[0].rec["xl"] == (env != "FT_NO_XL") and slow[0].rec["nsplit"] == (8 if env == "FT_NO_XL" else 32), slow[0].rec["nsplit"]
    rep = judge_loop(shape, cfg, loop, env)
    if env == "FT_NO_QKV0":
        assert (9, 0, "qkv") in rep.checked and (8, 0, "qkv") in rep.checked          # layer 0's q k v is a real hand-off again
    judge_slow(shape, slow, env)
    CASES.append(env)


@pytest.mark.parametrize("over", [dict(fast_intermediate_size=4096), dict(intermediate_size=4096), dict(n_local_heads=4), dict(n_fast_layer=1),
                                  dict(n_fast_layer=3), dict(fast_attention_qk_norm=True), dict(n_layer=1)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_shape_classes(over):
    """The other instantiations and depths: plain (non-PK3) SwiGLU granules in the loop / in the slow stack, four kv heads (the
    general split form of the attention), one and three loop layers (the skipped tail sits on the last one), q / k norms
    inside the loop's attention, a one-layer slow stack (one parity of every slow buffer)."""
    shape = base_shape(**over)
    cfg, loop, slow, path = collect(shape)
    assert cfg.pk3 == (shape.fast_intermediate_size == 3072) and bool(slow[0].rec["pk3"]) == (shape.intermediate_size == 3072), path
    assert cfg.resident == (shape.fast_intermediate_size == 3072), path
    judge_loop(shape, cfg, loop, str(over))
    judge_slow(shape, slow, str(over))
    CASES.append(str(over))


@pytest.mark.parametrize("max_seq_len,lp,n_frames,xl", [(1024, 300, 6, 1), (8192, 3064, 10, 1)], ids=["300", "xl-3064"])
def test_slow_stack_long_prompts(max_seq_len, lp, n_frames, xl):
    """QKV, the split partials, gy, Wo, W13 and W2 of both slow layers behind a 300-position prompt and, XCD-local at
    max_seq_len 8192, behind 3064 positions: ten frames, positions 3064 .. 3073, across 3072 where a split outgrows the
    attention's register window and the walk first wraps (`xl-3064` of tests/test_engine_long_context_gpu.py)."""
    shape = base_shape(max_seq_len=max_seq_len)
    cfg, loop, slow, path = collect(shape, lp=lp, n_frames=n_frames)
    assert slow[0].rec["xl"] == xl and slow[0].pos == lp and slow[-1].pos == lp + n_frames - 1, (slow[0].rec["xl"], slow[0].pos)
    judge_slow(shape, slow, f"prompt {lp}")
    judge_loop(shape, cfg, loop, f"prompt {lp}")
    CASES.append(f"prompt {lp}")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    """After the module's cases: what they checked, in one line (shown with -s)."""
    yield
    _W.clear()
    print(f"\n{len(CASES)} cases; {STATS.phases} phases, {STATS.units} units, {STATS.tag_units} tags, {STATS.replica_units} replica units under the "
          "current tag; largest |got - ref| / bound per kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(STATS.worst.items())))
