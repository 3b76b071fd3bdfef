"""GPU: ft_ar_slot_move (ARHipEngine.move_slot) - an utterance moved between decode calls goes on exactly as it would have
in its first slot: K/V, frame store (the repetition-penalty window still reaches its prompt region), position, flags.
Refused moves change nothing."""
import numpy as np
import pytest

from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import make_prompt, tiny_shape

pytestmark = pytest.mark.gpu


def _engine(shape, precision, max_batch, max_new_tokens):
    import torch

    from fish_tts_amd.ar_engine import ARHipEngine
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(precision, torch.float32)
    eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                      precision=precision, device=0, max_batch=max_batch, max_new_tokens=max_new_tokens)
    eng.load_state_dict({k: v.to(dtype) for k, v in cached_random_weights(shape, seed=0).items()})
    return eng


def _moved_equals_unmoved(eng, shape, n_before=3, n_after=9, width_after=None, lp=14, bytes_too=False):
    """Utterance A (an lp-column prompt; sampled, repetition_penalty 1.1, ban_eos: fixed length) runs n_before frames in
    slot 3 of a 4-wide batch while slot 0 holds what another utterance left there, moves to slot 0 and finishes: every
    column equals A's unmoved single run with the same seed.  bytes_too: the move itself is first held to tests/slot_ref.py
    byte by byte - the lp + n_before moved K/V rows of every layer and head, the rows behind them, every other slot, the state
    arrays."""
    pa, pb = make_prompt(shape, lp, seed=5, n_vq=2).numpy(), make_prompt(shape, 9, seed=6, n_vq=1).numpy()
    kw = dict(temperature=0.7, top_p=0.8, repetition_penalty=1.1)
    spa = eng._sampling(seed=11, ban_eos=True, **kw)
    spb = eng._sampling(seed=12, **kw)
    idle = eng._sampling(0.7, 0.8, 1.0)
    want = eng.generate(pa, 1 + n_before + n_after, seed=11, ban_eos=True, **kw)[:, pa.shape[1]:]
    assert want.shape[1] == 1 + n_before + n_after
    eng.generate(pb, 6, seed=12, **kw)                            # B in slot 0: its frames, position, flags stay there
    eng.park(1)
    eng.park(2)
    first = eng.prefill_many([pa], [spa], [3])[0]
    frames, n = eng.decode(n_before, [spb, idle, idle, spa], poll=n_before)
    assert n[3] == n_before and n[1] == n[2] == 0
    if bytes_too:
        from tests import slot_ref as S
        before = S.State.from_hook(eng.test_slots())
        assert S.moved_positions(before, 3) == lp + n_before
    eng.move_slot(3, 0)
    if bytes_too:
        after, model = S.State.from_hook(eng.test_slots()), S.move(before, 3, 0)
        assert S.diff(after, model) is None, S.describe(S.diff(after, model), after, model)
        assert np.array_equal(after.kv[:, :, 0, :, :lp + n_before], before.kv[:, :, 3, :, :lp + n_before])
    w = width_after or 4
    sps = [spa] + [idle] * (w - 1)
    after, m = eng.decode(n_after, sps, poll=4)
    assert m[0] == n_after
    if w > 1:
        assert (m[1:] == 0).all()                                 # slot 3 was left parked: it draws nothing, limits nothing
    got = np.concatenate([first[:, None], frames[3, :n_before].T, after[0, :n_after].T], axis=1)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_moved_slot_continues_bit_identically(precision):
    from fish_tts_amd.ar_engine import HipError
    eng = _engine(tiny_shape(), precision, max_batch=4, max_new_tokens=48)
    try:
        _moved_equals_unmoved(eng, tiny_shape())
        # refusals come before any device work: a decode after them equals one without
        p = make_prompt(tiny_shape(), 10, seed=8).numpy()
        sp = eng._sampling(0.7, 0.8, 1.1, seed=3, ban_eos=True)
        eng.prefill_many([p], [sp], [1])
        for a, b in ((1, 1), (-1, 0), (1, 4), (4, 1)):
            with pytest.raises(HipError, match=r"ft_ar_slot_move failed \(1\)"):
                eng.move_slot(a, b)
        eng.park(0)
        frames, n = eng.decode(5, [eng._sampling(0.7, 0.8, 1.0), sp], poll=5)
        want = eng.generate(p, 6, 0.7, 0.8, 1.1, seed=3, ban_eos=True)[:, p.shape[1] + 1:]
        assert n[1] == 5 and np.array_equal(frames[1, :5].T, want)
    finally:
        eng.close()


def test_refused_without_the_ar_model():
    import ctypes as C

    from fish_tts_amd import _lib as L
    from fish_tts_amd.codec_engine import CodecHipEngine
    from tests.test_api_gpu import api_codec_shape
    from tests.test_codec_gpu import args_from_shape as codec_args
    codec = CodecHipEngine(codec_args(api_codec_shape()), device=0, max_frames=16)
    try:
        assert codec.lib.ft_ar_slot_move(codec._h, 0, 1) == L.FT_ERR_STATE
    finally:
        codec.close()
    assert L.load().ft_ar_slot_move(C.c_void_p(), 0, 1) == L.FT_ERR_ARG


def test_moved_slot_at_s1_widths_runs_on_the_frame_engine():
    """medium_shape (s1-mini widths): the frames after the move run at width 1 on the persistent frame engine.  The slot
    holds 150 + 3 positions when it moves: the K/V copy spans three chunks of 64 positions (head_dim 128, bf16); its 153 rows
    and everything the move must leave alone are checked byte by byte in front of the decode."""
    from tests.test_ar_gpu import medium_shape
    shape = medium_shape()
    eng = _engine(shape, "bf16", max_batch=4, max_new_tokens=32)
    try:
        assert eng.engine_state()[0] == 3, eng.frame_path()
        _moved_equals_unmoved(eng, shape, n_before=3, n_after=9, width_after=1, lp=150, bytes_too=True)
        flags, aborted, _ = eng.engine_state()
        assert flags == 3 and aborted == 0
    finally:
        eng.close()
