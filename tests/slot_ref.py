"""The state an utterance owns between two launches of the dual-AR path, and the calls that carry it, as a model in numpy
integers and bytes (no floats: nothing here is arithmetic).  The transitions restate the WORDING of include/fishtts_hip.h,
not the kernel of csrc/engine.hip:

  move(from, to)     "Carried: the slow stack's K/V rows [0, pos) of every layer, the slot's row of the frame store, position,
                     input column, frame count, done flag and sampling row; `from` is left parked (as ft_ar_park leaves it),
                     `to`'s former content is overwritten."  (The column under construction, tokn, travels with the input
                     column.)  pos is held inside the cache: [0, n_slots].
  park(slot)         the slot counts as finished: its frame store holds one frame = <|im_end|>, nf = 1, done = 1, a harmless
                     input column (zeros) at position 0.  K/V, tokn and the sampling row are not its business.
  reset(slot)        frame store, position, frame count and done flag cleared.
  save(slot, n_pos)  a snapshot of K/V rows [0, n_pos) of every layer and kv head; the context is not changed.
  restore(snap, s)   those rows into slot s; rows >= n_pos, every other slot, every state array stay.

Everything a transition does not name must come back bit-unchanged: diff(got, want) compares WHOLE states and names the first
differing buffer, layer, K | V, slot, head and row (or the word, for the state arrays) - frame_ref's rule "rows outside a
launch must stay bit-unchanged", applied to slots.  hid_in_xo (the host's note of where ft_ar_get_debug(hidden) finds a slot's
residual stream) belongs to no transition: a move does not carry it, which is why the hidden row of `to` is defined only after
its next frame."""
import numpy as np

STATE_ARRAYS = ("seq", "tok", "tokn", "pos", "nf", "done", "ctl", "hid_in_xo")      # the order diff() walks them in, behind kv


class State:
    """kv (n_layer, 2, MB, Hkv, n_slots, head_dim x esz) uint8; seq (MB, R, cap), tok, tokn (MB, R), pos, nf, done (MB,) int32;
    ctl (MB, words) uint32; hid_in_xo (MB,) uint8; geo: the geometry words of ft_test_ar_slots by name."""

    def __init__(self, geo, kv, **arrays):
        self.geo, self.kv = dict(geo), kv
        for k in STATE_ARRAYS:
            setattr(self, k, arrays[k])

    @classmethod
    def from_hook(cls, d):
        return cls(d["geo"], d["kv"], **{k: d[k] for k in STATE_ARRAYS})

    def copy(self):
        return State(self.geo, self.kv.copy(), **{k: getattr(self, k).copy() for k in STATE_ARRAYS})

    @property
    def n_slots(self):
        return self.geo["n_slots"]

    def n_bytes(self):
        return self.kv.nbytes + sum(getattr(self, k).nbytes for k in STATE_ARRAYS)

    def _slot(self, slot):
        assert 0 <= slot < self.geo["max_batch"], slot


def chunk_positions(head_dim, esz):
    """Positions one workgroup of the move copies: 1024 16-byte pieces (the number the GPU cases are laid around; the model
    itself has no chunks)."""
    return max(1, 1024 // (head_dim * esz // 16))


def _park_in_place(s, slot):
    s.seq[slot] = 0
    s.seq[slot, 0, 0] = s.geo["im_end_id"]
    s.nf[slot], s.done[slot], s.pos[slot] = 1, 1, 0
    s.tok[slot] = 0


def park(s, slot):
    s._slot(slot)
    o = s.copy()
    _park_in_place(o, slot)
    return o


def reset(s, slot):
    s._slot(slot)
    o = s.copy()
    o.seq[slot] = 0
    o.pos[slot] = o.nf[slot] = o.done[slot] = 0
    return o


def moved_positions(s, slot):
    return int(max(0, min(int(s.pos[slot]), s.n_slots)))


def move(s, src, dst):
    s._slot(src), s._slot(dst)
    assert src != dst
    o = s.copy()
    n = moved_positions(s, src)
    o.kv[:, :, dst, :, :n] = s.kv[:, :, src, :, :n]
    for k in ("seq", "tok", "tokn", "pos", "nf", "done", "ctl"):
        getattr(o, k)[dst] = getattr(s, k)[src]
    _park_in_place(o, src)
    return o


def save(s, slot, n_pos):
    """The snapshot: (n_layer, 2, Hkv, n_pos, head_dim x esz) bytes."""
    s._slot(slot)
    assert 1 <= n_pos <= s.n_slots, n_pos
    return s.kv[:, :, slot, :, :n_pos].copy()


def restore(s, snap, slot):
    s._slot(slot)
    o = s.copy()
    o.kv[:, :, slot, :, :snap.shape[3]] = snap
    return o


def diff(got, want):
    """None, or where the two states first differ: ("kv", layer, "K" | "V", slot, head, row) or (array, slot, word), walking
    kv first and then STATE_ARRAYS, each in memory order."""
    assert got.geo == want.geo, (got.geo, want.geo)
    assert got.kv.shape == want.kv.shape
    if not np.array_equal(got.kv, want.kv):
        rows = (got.kv != want.kv).any(axis=-1)
        l, k, m, h, r = (int(v) for v in np.argwhere(rows)[0])
        return ("kv", l, "KV"[k], m, h, r)
    for name in STATE_ARRAYS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if not np.array_equal(a, b):
            ne = (a != b).reshape(a.shape[0], -1)
            m, w = (int(v) for v in np.argwhere(ne)[0])
            return (name, m, w)
    return None


def describe(d, got=None, want=None):
    if d is None:
        return "no difference"
    if d[0] == "kv":
        text = "K/V differs first at layer %d, %s, slot %d, kv head %d, row %d" % d[1:]
        if got is not None:
            i = (d[1], "KV".index(d[2]), d[3], d[4], d[5])
            text += ": got %s.., want %s.." % (got.kv[i][:8].tobytes().hex(), want.kv[i][:8].tobytes().hex())
        return text
    text = "%s differs first at slot %d, word %d" % d
    if got is not None:
        g, w = getattr(got, d[0]).reshape(got.geo["max_batch"], -1)[d[1], d[2]], getattr(want, d[0]).reshape(got.geo["max_batch"], -1)[d[1], d[2]]
        text += ": got %d, want %d" % (int(g), int(w))
    return text
