"""CPU: the frame engine's phase checker (tests/engine_phase_ref.py) pinned without a GPU.  The records of a codebook-loop launch
are built at the real widths from ar_ref's float32 / bf16 emulations (emulate_gemv, emulate_fast_attn: the device's work split
and rounding points).  The honest emulation must pass with no unit flagged; each planted fault - the ones the launch-path
comparison lets through, see tests/test_engine_phases_gpu.py - must be flagged at its own step, layer, phase and units, and
nowhere earlier.  The plan must account for every (step, layer, phase) of every configuration the GPU file runs."""
import itertools

import numpy as np
import pytest
import torch

from tests import engine_phase_ref as E
from tests.hip_util import cached_random_weights
from tests.test_engine_phases_gpu import base_shape, not_handed_loop

NCB, NL, EPOCH = 7, 2, 64 * 5
_S = {}


def setup():
    """One honest pair of launches (7 codebooks, 2 loop layers, every feature on), made once: the second runs on the buffers the
    first left, as a context's launches do."""
    if not _S:
        shape = base_shape(num_codebooks=NCB, n_fast_layer=NL)
        W = E.loop_weights(cached_random_weights(shape, seed=0), shape)
        cfg = E.LoopCfg(NL, NCB, True, True, True, True)
        g = torch.Generator().manual_seed(5)
        hid = [torch.randn(1024, generator=g).to(torch.bfloat16).float().numpy() for _ in range(2)]
        toks = [torch.randint(0, 1024, (NCB + 1,), generator=g).numpy() for _ in range(2)]
        prev, _ = E.emulate_loop(cfg, W, hid[0], toks[0], EPOCH - 2 * E.EPOCH_STEP)
        fr, snaps = E.emulate_loop(cfg, W, hid[1], toks[1], EPOCH, prev=prev)
        _S.update(shape=shape, W=W, cfg=cfg, hid=hid[1], toks=toks[1], prev=prev, fr=fr, snaps=snaps)
    return _S


def test_honest_emulation_passes_with_no_unit_flagged():
    S = setup()
    rep = E.check_loop(S["cfg"], S["W"], [S["fr"]])
    assert not rep.flagged, rep.flagged
    assert set(rep.listed) == E.loop_phase_keys(S["cfg"])
    assert {k for k, st in rep.listed.items() if st == E.CHECKED} <= rep.checked
    assert rep.units > 0 and rep.tag_units > 0 and rep.replica_units == rep.tag_units          # one replica, wholly under the tag
    assert max(rep.worst.values()) <= 1.0, rep.worst
    # the launch before it on the same buffers passes as well (its records were overwritten only where the second wrote)
    assert not E.check_loop(S["cfg"], S["W"], [S["prev"]]).flagged


def test_two_codebooks_take_their_history_from_their_own_records():
    S = setup()
    cfg = E.LoopCfg(NL, 2, True, False, True, True)
    W = E.StackWeights(S["W"].layers, S["W"].H, S["W"].Hkv, S["W"].hd, S["W"].eps, S["W"].rope[:2], S["W"].extra)
    fr, _ = E.emulate_loop(cfg, W, S["hid"], S["toks"][:3], EPOCH)
    assert fr.hist is None
    rep = E.check_loop(cfg, W, [fr])
    assert not rep.flagged, rep.flagged
    assert {k for k, st in rep.listed.items() if st == E.NOT_HANDED} == not_handed_loop(cfg)
    assert (1, NL - 1, "attn_wo") in rep.checked and (0, 0, "attn_wo") in rep.checked


RES_UNIT = int(E.resident_pairs(3072)[8 * 37 + 3])            # a pair the gathering waves of workgroup 37 hold
FAULTS = [
    ("swiglu_unrounded", dict(step=6, layer=1), (6, 1, "w2"), None),
    ("gain_other_layer", dict(step=5, layer=0, unit=RES_UNIT), (5, 0, "w13"), [RES_UNIT]),
    ("pair_swapped", dict(step=6, layer=1, unit=RES_UNIT), (6, 1, "w13"), [RES_UNIT]),
    ("hist_prev", dict(step=5, layer=1), (5, 1, "attn_wo"), None),
    ("stale_code_head", dict(step=6, wg=201), (6, NL, "head"), list(range(804, 808))),
    ("logit_shift", dict(step=5, wg=64), (5, NL, "head"), [256]),
    ("two_ulp", dict(step=6, layer=0, unit=517), (6, 0, "w2"), [517]),
    ("replica_stale", dict(step=6, layer=1, unit=300, name="xb"), (6, 1, "attn_wo", "replica", 0), None),
    ("tag_prev_step", dict(step=5, layer=1, unit=700, name="xb"), (5, 1, "attn_wo", "tag"), [700]),
]


@pytest.mark.parametrize("bug,at,key,units", FAULTS, ids=[f[0] for f in FAULTS])
def test_planted_fault_is_flagged_where_it_sits_and_nowhere_earlier(bug, at, key, units):
    S = setup()
    s = at["step"]
    fr, _ = E.emulate_loop(S["cfg"], S["W"], S["hid"], S["toks"], EPOCH, bug=bug, at=at, resume=(s, S["snaps"][s]), prev=S["prev"])
    rep = E.check_loop(S["cfg"], S["W"], [fr])
    assert rep.flagged, f"{bug}: nothing flagged"
    order = [p.key for p in E.plan_loop(S["cfg"])]
    first = rep.where[0]
    assert first[0] == key, (bug, rep.flagged)
    at_ = lambda k: order.index((k[0], k[1], "attn_wo" if k[2].startswith("twin") else k[2]))       # (the twin's rows are judged with the attention)
    assert all(at_(w[0]) >= at_(key) for w in rep.where), (bug, [w[0] for w in rep.where])
    if units is not None:
        assert first[2] == units, (bug, first[2])
    elif bug == "replica_stale":
        assert first[2] and all(256 <= u < 512 for u in first[2]), first[2]
    elif bug == "hist_prev":
        assert len(first[2]) > 8, (bug, first[2])                 # a wrong history row moves many units of x'
    else:
        assert len(first[2]) >= 1, (bug, first[2])                # a rounding left out shows where a sum sits near a rounding boundary


def cfgs():
    for ncb, nl in itertools.product(range(2, 11), (1, 3, 4)):
        for pair, qkv0, pk3, res in itertools.product((True, False), repeat=4):
            yield E.LoopCfg(nl, ncb, pair, qkv0 and ncb > 2, pk3, res)


def test_the_plan_accounts_for_every_phase_of_every_configuration():
    n = 0
    for cfg in cfgs():
        plan = [p for p in E.plan_loop(cfg) if not p.extra]
        keys = [p.key for p in plan]
        assert len(keys) == len(set(keys)) and set(keys) == E.loop_phase_keys(cfg), cfg
        assert {p.key for p in plan if p.status == E.NOT_HANDED} == not_handed_loop(cfg), cfg
        assert all((p.dst is None) == (p.status == E.NOT_HANDED) and (p.status == E.CHECKED or p.why) for p in plan), cfg
        # no two phases of a launch leave their output in the same buffer; every buffer read was written by an earlier phase
        dsts = [p.dst for p in E.plan_loop(cfg) if p.dst is not None]
        assert len(dsts) == len(set(dsts)), cfg
        written = set()
        for p in E.plan_loop(cfg):
            if p.status == E.CHECKED:
                for src in p.src:
                    assert src[0] in ("hid", "emb", "hist") or src in written, (cfg, p)
            if p.dst is not None:
                written.add(p.dst)
        # SwiGLU granules: plain where the paired pass carries position 0 on, PK3 triples elsewhere in a PK3 class
        for p in plan:
            if p.kind == "w13" and p.dst is not None:
                plain = not cfg.pk3 or (cfg.pair and p.step <= 1 and p.layer < cfg.n_layer - 1)
                assert p.dst[0] == ("g" if plain else "g3"), (cfg, p)
        n += 1
    assert n == 9 * 3 * 16
    for n_layer, ns, pk3 in itertools.product((1, 2, 5), (1, 8, 32), (True, False)):
        plan = E.plan_slow(n_layer, ns, pk3)
        assert {p.key for p in plan} == E.slow_phase_keys(n_layer) and len(plan) == 6 * min(n_layer, 2)
        assert [p.key for p in plan if p.status == E.NOT_HANDED] == ([(-1, li, "merge") for li in E.slow_layers(n_layer)] if ns == 1 else [])


def test_tags_follow_the_kernels_rule():
    assert E.tag16(0) == 0x8000 and E.tag16(0x7FFF + 2) == 0x8001 and E.tag32(5) == 0x80000005
    assert E.resident_pairs(3072).size == 8 * 256 and E.resident_pairs(3072)[:8].tolist() == list(range(4, 12))
