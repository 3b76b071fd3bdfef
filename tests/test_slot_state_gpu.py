"""GPU: the calls that carry an utterance's state between two launches - ft_ar_slot_move, ft_ar_park, ft_ar_reset,
ft_ar_kv_save / ft_ar_kv_restore and the ft_ar_prefill_at behind a restore - byte by byte.  Every case reads the WHOLE per-slot
state of the context (ft_test_ar_slots: K/V of every layer and slot, frame store, columns, position, flags, sampling rows, the
host's hidden-row note) before and after ONE call and holds it to tests/slot_ref.py's prediction bit for bit: the bytes the
header names are equal, every other byte is untouched, a refused call leaves every byte as it was.  No arithmetic, no bound.

The shapes are the smallest that cross the edges of the move's work split (one workgroup per layer, K | V, kv head and chunk of
1024 16-byte pieces): head_dim 128 gives chunks of 64 positions in bf16 / fp16 and 32 in fp32 inside a 197-row cache (n_slots
200); head_dim 16 and 8 never leave their first chunk; 65 and 130 layers take two and three launches.  The case lists below are
imported by tests/test_slot_ref_host.py, which runs the same geometries through an emulation of the device's work split.

Wall time of the file on an MI355X: 7 s for 43 tests, the slowest 0.4 s (440 calls held to the model, 114 refusals, 5.6e8 bytes
compared; the last test prints the counts and the (n_pos, chunk) pairs reached)."""
import dataclasses

import numpy as np
import pytest

from tests import slot_ref as S
from tests.hip_util import args_from_shape, cached_random_weights
from tests.shapes import make_prompt, tiny_shape, tiny_shape_b

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16", "fp16", "fp32")
ESZ = {"bf16": 2, "fp16": 2, "fp32": 4}
MAX_NEW = 8                                       # cap = 32 columns of frame store per row


def hd128_shape():
    """head_dim 128 at the narrowest width that has it: chunks of 64 / 32 positions, a cache of 200 rows for 197 positions."""
    return dataclasses.replace(tiny_shape(), dim=256, n_head=2, n_local_heads=2, head_dim=128, intermediate_size=128, max_seq_len=197)


def hd8_shape():
    """One 16-byte piece per position in bf16 (row16 = 1)."""
    return dataclasses.replace(tiny_shape(), n_head=8, n_local_heads=2, head_dim=8, max_seq_len=52)


SHAPES = {"tiny": tiny_shape, "tinyb": tiny_shape_b, "hd128": hd128_shape, "hd8": hd8_shape}
DEEP_LAYERS = (65, 130)                           # two and three launches of the move
DEEP_POSITIONS = 20
WIDE_BATCH = 256                                  # one context of 256 slots: 255 -> 0


def n_slots_of(shape):
    return shape.max_seq_len + (-shape.max_seq_len) % 8


def move_positions(shape, precision):
    """The n_pos a move is asked to carry on this shape and type: a parked slot, one row, the edges of the first two chunks
    where the cache reaches them, the longest prompt the API takes, the last cache row (reached by decoding up to it)."""
    c = S.chunk_positions(shape.head_dim, ESZ[precision])
    longest = shape.max_seq_len - 1
    want = [0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1, 7, longest, shape.max_seq_len]
    return sorted({n for n in want if 0 <= n <= shape.max_seq_len})


def snapshot_positions(shape, precision):
    c = S.chunk_positions(shape.head_dim, ESZ[precision])
    ns = n_slots_of(shape)
    return sorted({n for n in (1, c - 1, c, c + 1, 13, ns) if 1 <= n <= ns})


def geometries():
    """(name, n_layer, Hkv, n_slots, head_dim, esz, max_batch, n_pos list) of every context this file builds for a move."""
    out = []
    for name, mk in SHAPES.items():
        sh = mk()
        for pr in PRECISIONS:
            out.append((f"{name}-{pr}", sh.n_layer, sh.n_local_heads, n_slots_of(sh), sh.head_dim, ESZ[pr], 4, move_positions(sh, pr)))
    sh = tiny_shape()
    for nl in DEEP_LAYERS:
        out.append((f"deep{nl}-bf16", nl, sh.n_local_heads, n_slots_of(sh), sh.head_dim, 2, 3, [DEEP_POSITIONS]))
    out.append((f"wide{WIDE_BATCH}-bf16", sh.n_layer, sh.n_local_heads, n_slots_of(sh), sh.head_dim, 2, WIDE_BATCH, [9]))
    return out


def expected_reached():
    """{precision: {(n_pos, chunk)}} the move cases must have reached by the end of the file."""
    exp = {pr: set() for pr in PRECISIONS}
    for name, mk in SHAPES.items():
        for pr in PRECISIONS:
            c = S.chunk_positions(mk().head_dim, ESZ[pr])
            exp[pr] |= {(n, c) for n in move_positions(mk(), pr)}
    c = S.chunk_positions(16, 2)
    exp["bf16"] |= {(DEEP_POSITIONS, c), (9, c)}
    return exp


REACHED = {pr: set() for pr in PRECISIONS}
TALLY = {"calls": 0, "bytes": 0, "refused": 0}
DEEP_SEEN = set()


# ------------------------------------------------------------------------------------------------ the common routine
def make_engine(shape, precision, max_batch=4, seed=0):
    import torch

    from fish_tts_amd.ar_engine import ARHipEngine
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(precision, torch.float32)
    eng = ARHipEngine(args_from_shape(shape), shape.semantic_begin_id, shape.semantic_end_id, shape.im_end_id,
                      precision=precision, device=0, max_batch=max_batch, max_new_tokens=MAX_NEW)
    eng.load_state_dict({k: v.to(dtype) for k, v in cached_random_weights(shape, seed=seed).items()})
    return eng


def read(eng):
    return S.State.from_hook(eng.test_slots())


def held(eng, call, predict, what):
    """Runs ONE call between two reads of the whole state; the second read must equal predict(first) bit for bit.  Returns
    (before, after)."""
    before = read(eng)
    call()
    after = read(eng)
    want = predict(before)
    d = S.diff(after, want)
    assert d is None, f"{what}: {S.describe(d, after, want)}"
    TALLY["calls"] += 1
    TALLY["bytes"] += after.n_bytes()
    return before, after


def refused(eng, call, what, exc=None):
    """A refused call raises and leaves every byte as it was."""
    from fish_tts_amd.ar_engine import HipError
    before = read(eng)
    with pytest.raises(exc or HipError):
        call()
    after = read(eng)
    d = S.diff(after, before)
    assert d is None, f"{what} was refused and still changed the state: {S.describe(d, after, before)}"
    TALLY["refused"] += 1
    TALLY["bytes"] += after.n_bytes()


def do_move(eng, precision, src, dst, what=""):
    before, after = held(eng, lambda: eng.move_slot(src, dst), lambda s: S.move(s, src, dst), f"move {src} -> {dst} {what}")
    n = S.moved_positions(before, src)
    REACHED[precision].add((n, S.chunk_positions(before.geo["head_dim"], before.geo["esz"])))
    return before, after


def do_park(eng, slot):
    return held(eng, lambda: eng.park(slot), lambda s: S.park(s, slot), f"park {slot}")


def sampling(eng, seed, ban_eos=True):
    return eng._sampling(0.7, 0.8, 1.1, seed=seed, ban_eos=ban_eos)


def fill(eng, shape, slot, lp, seed, sp=None):
    """A prompt of lp columns into `slot`: position lp, one frame.  Its first column differs by seed too (make_prompt starts
    every prompt with the same token, and equal tokens at row 0 mean equal K/V there: a move that lost row 0 would not show)."""
    prompt = make_prompt(shape, lp, seed=seed, n_vq=min(2, max(0, lp - 3))).numpy()
    prompt[0, 0] = 1 + (seed * 37) % 241
    eng.prefill(prompt, sp or sampling(eng, seed), slot)


def fill_long(eng, shape, slots):
    """Different stale data in every row of every slot: the longest prompt the API takes, another one per slot."""
    for m in slots:
        fill(eng, shape, m, shape.max_seq_len - 1, seed=100 + m)


def same_utterance(st, a, b, n_pos):
    """Slots a and b hold the same bytes in everything an utterance owns (K/V rows [0, n_pos))."""
    for k in ("seq", "tok", "tokn", "pos", "nf", "done", "ctl"):
        assert np.array_equal(getattr(st, k)[a], getattr(st, k)[b]), (k, a, b)
    assert np.array_equal(st.kv[:, :, a, :, :n_pos], st.kv[:, :, b, :, :n_pos]), ("kv", a, b)


# ------------------------------------------------------------------------------------------------ moves
# (from, to, twin) by turn: from > to and from < to, to = max_batch - 1 and from = 0
ROUTES = ((3, 0, 1), (0, 3, 2), (2, 1, 0), (1, 2, 3))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_moves_carry_what_the_header_names_and_nothing_else(name, precision):
    shape = SHAPES[name]()
    eng = make_engine(shape, precision)
    try:
        geo = eng.test_slots(kv=False)["geo"]
        assert (geo["n_slots"], geo["head_dim"], geo["esz"], geo["Hkv"]) == (n_slots_of(shape), shape.head_dim, ESZ[precision], shape.n_local_heads)
        fill_long(eng, shape, range(4))
        st = read(eng)
        for li in range(shape.n_layer):                                   # the hook reads what ft_test_engine_handoffs reads
            d = eng.engine_handoffs(0, vectors=False, kv=(li, 2, n_slots_of(shape)))
            for k, name_k in enumerate(("kv_k", "kv_v")):
                assert np.array_equal(d[name_k].view(np.uint8).reshape(st.kv[li, k, 2].shape), st.kv[li, k, 2]), (li, name_k)
        assert st.kv[:, :, :, :, :shape.max_seq_len - 1].any(axis=-1).all()
        for i, n_pos in enumerate(move_positions(shape, precision)):
            src, dst, twin = ROUTES[i % 4]
            spare = 6 - src - dst - twin
            sp = sampling(eng, seed=40 + i)
            if n_pos == 0:
                for m in (src, twin):                    # a parked slot (and its twin: the same columns and sampling row)
                    fill(eng, shape, m, 5, seed=60, sp=sp)
                    do_park(eng, m)
            elif n_pos == shape.max_seq_len:
                # the last cache row: the longest prompt, then one frame; the utterance and its twin sit in slots 0 and 1
                src, twin, dst, spare = 0, 1, 3, 2
                for m in (src, twin):
                    fill(eng, shape, m, n_pos - 1, seed=60, sp=sp)
                frames, n = eng.decode(1, [sp, sp])
                assert n.tolist() == [1, 1] and np.array_equal(frames[0], frames[1])
            else:
                for m in (src, twin):
                    fill(eng, shape, m, n_pos, seed=60 + i, sp=sp)
            if i % 2:
                do_park(eng, dst)                        # into a parked slot; otherwise into one holding a longer utterance
            else:
                fill(eng, shape, dst, shape.max_seq_len - 1, seed=200 + i)
            st = read(eng)
            assert S.moved_positions(st, src) == n_pos, (st.pos, n_pos)
            same_utterance(st, src, twin, n_pos)
            # the rows to carry differ from what `to` holds: row 0 at every layer, every row behind the first layer
            ne = (st.kv[:, :, src, :, :n_pos] != st.kv[:, :, dst, :, :n_pos]).any(axis=-1)
            assert ne[:, :, :, :1].all() and ne[1:].all(), (n_pos, np.argwhere(~ne)[:4].tolist())
            before, after = do_move(eng, precision, src, dst, f"({n_pos} positions)")
            assert np.array_equal(after.kv[:, :, dst, :, n_pos:], before.kv[:, :, dst, :, n_pos:])          # (diff() said so already)
            # `from` is as ft_ar_park leaves the twin that held the same utterance
            _, parked = do_park(eng, twin)
            same_utterance(parked, src, twin, n_pos)
            assert parked.done[src] == 1 and parked.nf[src] == 1 and parked.seq[src, 0, 0] == shape.im_end_id
            fill(eng, shape, spare, shape.max_seq_len - 1, seed=300 + i)         # fresh stale rows for the next turn
            fill(eng, shape, src, shape.max_seq_len - 1, seed=400 + i)
    finally:
        eng.close()


@pytest.mark.parametrize("precision", ("bf16", "fp32"))
def test_finished_slot_chain_and_swap(precision):
    shape = tiny_shape()
    eng = make_engine(shape, precision)
    try:
        fill_long(eng, shape, range(4))
        # a finished slot: <|im_end|> forced by the noise of frame index 1, as the draw tests force it
        V, fastV = shape.vocab_size, min(1024, shape.codebook_size)
        q = np.ones((4, V + (shape.num_codebooks - 1) * fastV), dtype=np.float32)
        q[1, :V] = 2.0 ** 60
        q[1, shape.im_end_id] = 2.0 ** -60
        eng.set_noise(q)
        plain = eng._sampling(1.0, 1.0, 1.0, seed=0)
        do_park(eng, 0)
        eng.prefill(make_prompt(shape, 11, seed=7, n_vq=2).numpy(), plain, 1)
        frames, n = eng.decode(2, [plain, plain])
        assert n.tolist() == [0, 1] and frames[1, 0, 0] == shape.im_end_id
        eng.set_noise(None)
        st = read(eng)
        assert st.done[1] == 1 and st.nf[1] == 2
        _, after = do_move(eng, precision, 1, 3, "(a finished slot)")
        assert after.done[3] == 1 and after.nf[3] == 2
        # a chain a -> b -> c
        fill(eng, shape, 0, 17, seed=8)
        do_move(eng, precision, 0, 1, "(chain)")
        _, after = do_move(eng, precision, 1, 2, "(chain)")
        assert after.pos.tolist()[:3] == [0, 0, 17]
        # a swap through a third slot: 2 and 3 change places through 0
        want2 = read(eng)
        do_move(eng, precision, 2, 0, "(swap)")
        do_move(eng, precision, 3, 2, "(swap)")
        _, after = do_move(eng, precision, 0, 3, "(swap)")
        for k in ("seq", "tok", "tokn", "pos", "nf", "done", "ctl"):
            assert np.array_equal(getattr(after, k)[3], getattr(want2, k)[2]) and np.array_equal(getattr(after, k)[2], getattr(want2, k)[3]), k
        assert np.array_equal(after.kv[:, :, 3, :, :17], want2.kv[:, :, 2, :, :17])
        assert np.array_equal(after.kv[:, :, 2, :, :11 + 1], want2.kv[:, :, 3, :, :11 + 1])
    finally:
        eng.close()


def test_moves_between_the_ends_of_256_slots():
    shape = tiny_shape()
    eng = make_engine(shape, "bf16", max_batch=WIDE_BATCH)
    try:
        for m, lp in ((0, 30), (1, 25), (254, 21), (255, 9)):
            fill(eng, shape, m, lp, seed=m)
        do_move(eng, "bf16", 255, 0, "(256 slots)")
        _, after = do_move(eng, "bf16", 1, 255, "(256 slots)")
        assert after.pos[[0, 1, 254, 255]].tolist() == [9, 0, 21, 25]
    finally:
        eng.close()


@pytest.mark.parametrize("n_layer", DEEP_LAYERS)
def test_deep_models_move_in_several_launches(n_layer):
    shape = dataclasses.replace(tiny_shape(), n_layer=n_layer)
    eng = make_engine(shape, "bf16", max_batch=3)
    try:
        fill(eng, shape, 0, 31, seed=1)
        fill(eng, shape, 1, 26, seed=2)
        fill(eng, shape, 2, DEEP_POSITIONS, seed=3)
        before, after = do_move(eng, "bf16", 2, 0, f"({n_layer} layers)")
        assert before.geo["n_layer"] == n_layer and after.pos.tolist() == [DEEP_POSITIONS, 26, 0]
        DEEP_SEEN.add(n_layer)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ park and reset alone
@pytest.mark.parametrize("precision", PRECISIONS)
def test_park_and_reset_alone(precision):
    from fish_tts_amd import _lib as L
    shape = tiny_shape_b()
    eng = make_engine(shape, precision)
    try:
        fill_long(eng, shape, range(4))
        eng.decode(2, [sampling(eng, m) for m in range(4)])              # tokn and the sampling rows hold something
        before, after = do_park(eng, 2)
        assert before.tokn[2].any() and before.ctl[2].any() and np.array_equal(after.tokn, before.tokn) and np.array_equal(after.ctl, before.ctl)
        assert np.array_equal(after.kv, before.kv)
        do_park(eng, 2)                                                   # twice: nothing more
        do_park(eng, 3)
        held(eng, lambda: eng._check(eng.lib.ft_ar_reset(eng._h, 1), "ft_ar_reset"), lambda s: S.reset(s, 1), "reset 1")
        held(eng, lambda: eng._check(eng.lib.ft_ar_reset(eng._h, 0), "ft_ar_reset"), lambda s: S.reset(s, 0), "reset 0")
        for slot in (-1, 4):
            refused(eng, lambda: eng.park(slot), f"park {slot}")
            refused(eng, lambda: eng._check(eng.lib.ft_ar_reset(eng._h, slot), "ft_ar_reset"), f"reset {slot}")
        for a, b in ((1, 1), (-1, 0), (1, 4), (4, 1)):
            refused(eng, lambda: eng.move_slot(a, b), f"move {a} -> {b}")
        assert L.FT_ERR_ARG == 1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ snapshots
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ("tiny", "tinyb", "hd128"))
def test_snapshots_hold_and_put_back_exactly_their_rows(name, precision):
    shape = SHAPES[name]()
    eng = make_engine(shape, precision)
    unchanged = lambda s: s
    try:
        fill_long(eng, shape, range(4))
        ns = n_slots_of(shape)
        for i, n_pos in enumerate(snapshot_positions(shape, precision)):
            src = (1, 3, 2)[i % 3]                                           # saved from a slot other than 0
            other = (src + 1) % 4
            if i == 1:
                # saved from a slot that has decoded past n_pos since its prompt
                sp = sampling(eng, 500)
                fill(eng, shape, src, n_pos, seed=500, sp=sp)
                _, n = eng.decode(1, [sp] * (src + 1))
                assert n[src] == 1 and read(eng).pos[src] == n_pos + 1
            box = {}
            before, _ = held(eng, lambda: box.update(pf=eng.kv_save(n_pos, src)), unchanged, f"save {n_pos} rows of slot {src}")
            snap = S.save(before, src, n_pos)
            pf = box["pf"]
            assert pf.n_pos == n_pos
            fill(eng, shape, src, shape.max_seq_len - 1, seed=520 + i)        # other, longer content in the source itself
            _, after = held(eng, lambda: eng.kv_restore(pf, other), lambda s: S.restore(s, snap, other), f"restore {n_pos} rows into slot {other}")
            assert np.array_equal(after.kv[:, :, other, :, :n_pos], before.kv[:, :, src, :, :n_pos])
            held(eng, lambda: eng.kv_restore(pf, src), lambda s: S.restore(s, snap, src), f"restore {n_pos} rows into their slot {src}")
            held(eng, lambda: eng.kv_restore(pf, src), lambda s: S.restore(s, snap, src), "the same snapshot again")
            pf.free()
            refused(eng, lambda: eng.kv_restore(pf, other), "restore of a freed snapshot", exc=ValueError)
            fill(eng, shape, other, shape.max_seq_len - 1, seed=530 + i)
        # two snapshots alive, restored in both orders
        b0 = read(eng)
        pa, pb = eng.kv_save(5, 1), eng.kv_save(ns - 1, 2)
        sa, sb = S.save(b0, 1, 5), S.save(b0, 2, ns - 1)
        held(eng, lambda: eng.kv_restore(pa, 0), lambda s: S.restore(s, sa, 0), "first of two snapshots")
        held(eng, lambda: eng.kv_restore(pb, 0), lambda s: S.restore(s, sb, 0), "second of two over the first")
        _, after = held(eng, lambda: eng.kv_restore(pa, 0), lambda s: S.restore(s, sa, 0), "first over the second")
        assert np.array_equal(after.kv[:, :, 0, :, :5], b0.kv[:, :, 1, :, :5]) and np.array_equal(after.kv[:, :, 0, :, 5:ns - 1], b0.kv[:, :, 2, :, 5:ns - 1])
        # refusals
        for slot in (-1, 4):
            refused(eng, lambda: eng.kv_save(3, slot), f"save from slot {slot}")
            refused(eng, lambda: eng.kv_restore(pa, slot), f"restore into slot {slot}")
        for n_pos in (0, ns + 1):
            refused(eng, lambda: eng.kv_save(n_pos, 1), f"save of {n_pos} rows")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ continuation
N_AFTER = 4


def compare_continuations(a, slot_a, b, slot_b, what):
    """Two contexts, the utterance in slot_a of one and slot_b of the other: K/V rows [0, pos) of every layer, the vocabulary
    logits, the hidden row (defined again: a frame has run since the move) and the state arrays, bit for bit."""
    sa, sb = read(a), read(b)
    n = int(sa.pos[slot_a])
    assert n == int(sb.pos[slot_b]) and n > 0
    for k in ("seq", "tok", "tokn", "pos", "nf", "done", "ctl", "hid_in_xo"):
        assert np.array_equal(getattr(sa, k)[slot_a], getattr(sb, k)[slot_b]), (what, k)
    ne = (sa.kv[:, :, slot_a, :, :n] != sb.kv[:, :, slot_b, :, :n]).any(axis=-1)
    assert not ne.any(), (what, "K/V differs first at (layer, K|V, head, row)", np.argwhere(ne)[0].tolist())
    (la, ha), (lb, hb) = a.debug_state(slot_a), b.debug_state(slot_b)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (what, "logits")
    assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32)), (what, "hidden")
    TALLY["bytes"] += 2 * sa.kv[:, :, slot_a, :, :n].nbytes + la.nbytes + ha.nbytes


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ("tiny", "tinyb", "hd128"))
def test_a_moved_utterance_goes_on_bit_for_bit(name, precision):
    shape = SHAPES[name]()
    c = S.chunk_positions(shape.head_dim, ESZ[precision])
    lp = min(c + 1, shape.max_seq_len - 12)                               # two chunks where the cache has them
    a, b = make_engine(shape, precision), make_engine(shape, precision)
    try:
        prompt = make_prompt(shape, lp, seed=5, n_vq=2).numpy()
        sp, idle = sampling(a, 11), a._sampling(0.7, 0.8, 1.0)
        # unmoved: slot 0 of its own context, width 1 throughout
        first_b = b.prefill(prompt, sp, 0)
        fb, nb = b.decode(2 + N_AFTER, [sp], poll=2)
        # moved: two frames in slot 2 of a 3-wide batch over what other utterances left, then slot 0 at width 1
        fill_long(a, shape, range(4))
        do_park(a, 0)
        do_park(a, 1)
        first_a = a.prefill(prompt, sp, 2)
        fa, na = a.decode(2, [idle, idle, sp], poll=2)
        hid0 = read(a).hid_in_xo.copy()
        _, after = do_move(a, precision, 2, 0, "(before a continuation)")
        assert np.array_equal(after.hid_in_xo, hid0)                       # the move does not carry the host's note
        fa2, na2 = a.decode(N_AFTER, [sp], poll=2)
        assert na[2] == 2 and na2[0] == N_AFTER and nb[0] == 2 + N_AFTER
        assert np.array_equal(first_a, first_b) and np.array_equal(np.concatenate([fa[2, :2], fa2[0, :N_AFTER]]), fb[0, :2 + N_AFTER])
        compare_continuations(a, 0, b, 0, f"moved {name} {precision}")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name,precision", (("tiny", "fp32"), ("tiny", "bf16"), ("tinyb", "fp32")))
def test_a_restored_prefix_goes_on_bit_for_bit(name, precision):
    """Where test_prefix_kv_reuse_equals_full_prefill demands equal tokens (tiny_shape in fp32 and bf16: every prompt product
    is row-independent; fp32 runs its prompts position by position at every shape) the tail rows [n_pos, n_pos + Lp) and
    everything behind them equal the whole-prompt twin's bit for bit.  Elsewhere only rows [0, n_pos) are held, to the
    snapshot's source (test_snapshots_hold_and_put_back_exactly_their_rows)."""
    shape = SHAPES[name]()
    a, b = make_engine(shape, precision), make_engine(shape, precision)
    try:
        prompt = make_prompt(shape, 40, seed=5, n_vq=4).numpy()
        sp = sampling(a, 21)
        n_pos = 29
        first_b = b.prefill(prompt, sp, 0)
        fb, nb = b.decode(N_AFTER, [sp], poll=2)
        fill_long(a, shape, range(4))
        pf = a.build_prefix(prompt[:, :n_pos], slot=3)                    # built in another slot than the one that speaks
        fill(a, shape, 3, shape.max_seq_len - 1, seed=77)
        before = read(a)
        a.kv_restore(pf, 0)
        first_a = a.prefill(prompt[:, n_pos:], sp, 0, pos0=n_pos)
        mid = read(a)
        # the prefill behind the restore: rows [0, n_pos) stay the snapshot's, rows >= 40 and every other slot stay
        assert np.array_equal(mid.kv[:, :, 0, :, 40:], before.kv[:, :, 0, :, 40:]) and np.array_equal(mid.kv[:, :, 1:], before.kv[:, :, 1:])
        fa, na = a.decode(N_AFTER, [sp], poll=2)
        assert na[0] == nb[0] == N_AFTER and np.array_equal(first_a, first_b) and np.array_equal(fa[0], fb[0])
        compare_continuations(a, 0, b, 0, f"restored {name} {precision}")
    finally:
        a.close()
        b.close()


def test_a_move_does_not_carry_the_hidden_row():
    """The one piece of per-slot state the host keeps - hid_in_xo, where ft_ar_get_debug(hidden) finds the slot's residual
    stream - stays with the slot index: after a frame on the MFMA launches it is 1 for the rows of that frame, a move leaves
    it as it is on both slots, and the hidden row of `to` is the utterance's again once its next frame has run (it equals an
    unmoved twin's, row for row of the same lock-step frame)."""
    from tests.test_ar_gpu import medium_shape
    shape = dataclasses.replace(medium_shape(n_text=1009, num_codebooks=4), max_seq_len=64)
    eng = make_engine(shape, "bf16", max_batch=8)
    try:
        assert "MFMA launches" in eng.frame_path(), eng.frame_path()
        sps = [sampling(eng, 30 + min(m, 4)) for m in range(7)]
        for m in range(6):
            fill(eng, shape, m, 9 + min(m, 4), seed=30 + min(m, 4), sp=sps[m])     # slots 4 and 5: the same utterance
        do_park(eng, 6)
        _, n = eng.decode(1, sps[:6])
        assert n.tolist() == [1] * 6
        st = read(eng)
        assert st.hid_in_xo.tolist() == [1] * 6 + [0, 0]
        same_utterance(st, 4, 5, 14)
        assert np.array_equal(eng.debug_state(4)[1].view(np.uint32), eng.debug_state(5)[1].view(np.uint32))
        _, after = do_move(eng, "bf16", 5, 6, "(after an MFMA frame)")
        assert after.hid_in_xo.tolist() == [1] * 6 + [0, 0]                # not carried: slot 6 still says "no MFMA frame yet"
        _, n = eng.decode(1, sps[:4] + [sps[4], sps[4], sps[4]])
        assert n.tolist() == [1, 1, 1, 1, 1, 0, 1]
        st = read(eng)
        assert st.hid_in_xo.tolist() == [1] * 7 + [0]
        (l4, h4), (l6, h6) = eng.debug_state(4), eng.debug_state(6)
        assert np.array_equal(h4.view(np.uint32), h6.view(np.uint32)) and np.array_equal(l4.view(np.uint32), l6.view(np.uint32))
        for k in ("seq", "tok", "tokn", "pos", "nf", "done", "ctl"):
            assert np.array_equal(getattr(st, k)[4], getattr(st, k)[6]), k
        assert np.array_equal(st.kv[:, :, 4, :, :15], st.kv[:, :, 6, :, :15])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ what the file reached
def test_every_position_and_chunk_pair_was_reached():
    """Last in the file: the (n_pos, chunk) pairs the moves above carried, per type, are the ones the case lists promise."""
    exp = expected_reached()
    for pr in PRECISIONS:
        assert exp[pr] <= REACHED[pr], (pr, "not reached", sorted(exp[pr] - REACHED[pr]))
        chunks = sorted({c for _, c in REACHED[pr]})
        print(f"{pr}: " + "; ".join(f"chunk {c}: n_pos " + " ".join(str(n) for n, cc in sorted(REACHED[pr]) if cc == c) for c in chunks))
    assert DEEP_SEEN == set(DEEP_LAYERS), DEEP_SEEN
    print(f"{TALLY['calls']} calls held to the model, {TALLY['refused']} refusals, {TALLY['bytes']} bytes compared")
