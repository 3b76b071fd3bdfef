"""Host only: tests/slot_ref.py pinned on a numpy emulation of the device's work split - ft_ar_slot_move as one workgroup per
(layer, K | V, kv head, chunk of max(1, 1024 / row16) positions) copying 16-byte pieces between flat caches, one launch per
64 layers with the state block in the last, and kv_copy's 2-D strided copy (row n_pos x hd, pitch n_slots x hd).  The honest
emulation must show no difference on every geometry of tests/test_slot_state_gpu.py (its case lists are imported, not
copied); every planted fault must be flagged at its buffer, layer, head and row."""
import numpy as np
import pytest

from tests import slot_ref as S
from tests import test_slot_state_gpu as G

MAX_LAYERS = 64
IM_END = 260


def random_state(n_layer, hkv, n_slots, hd, esz, mb, seed=0, R=5, cap=12, words=6):
    """Every byte of K/V random; every state word random, nonzero and no <|im_end|>; positions set by the caller."""
    g = np.random.default_rng(seed)
    geo = dict(max_batch=mb, R=R, cap=cap, ctl_words=words, n_layer=n_layer, Hkv=hkv, n_slots=n_slots, head_dim=hd, esz=esz, im_end_id=IM_END)
    i32 = lambda *shape: g.integers(1000, 2 ** 31 - 1, size=shape, dtype=np.int64).astype(np.int32)
    return S.State(geo, g.integers(0, 256, size=(n_layer, 2, mb, hkv, n_slots, hd * esz), dtype=np.uint8),
                   seq=i32(mb, R, cap), tok=i32(mb, R), tokn=i32(mb, R), pos=i32(mb), nf=g.integers(2, cap, size=mb, dtype=np.int32),
                   done=np.zeros(mb, dtype=np.int32), ctl=i32(mb, words).view(np.uint32), hid_in_xo=g.integers(0, 2, size=mb, dtype=np.uint8))


def cp(buf, dst, src, n, src_buf=None):
    """n bytes inside flat buffers, as a workgroup's threads would copy them; what lies past a buffer's end is dropped (the
    emulation of a faulty split must not fault itself) and read as 0xEE."""
    src_buf = buf if src_buf is None else src_buf
    data = np.full(n, 0xEE, dtype=np.uint8)
    have = max(0, min(n, src_buf.size - src))
    data[:have] = src_buf[src:src + have]
    room = max(0, min(n, buf.size - dst))
    buf[dst:dst + room] = data[:room]


def emu_move(s, src, dst, fault=None):
    """ft_ar_slot_move as the device splits it.  fault: one of the planted ones below."""
    o = s.copy()
    g = s.geo
    L, hkv, n_slots, mb = g["n_layer"], g["Hkv"], g["n_slots"], g["max_batch"]
    row_bytes = g["head_dim"] * g["esz"]
    flat = [[o.kv[l, k].reshape(-1) for k in range(2)] for l in range(L)]           # views: one flat cache per layer and K | V
    assert all(f.base is not None for fl in flat for f in fl)
    n_pos = max(0, min(int(s.pos[src]), n_slots))
    if fault == "n_pos-1":
        n_pos -= 1
    row16 = row_bytes // 16
    assert row16 >= 1 and row_bytes % 16 == 0
    chunk = max(1, 1024 // row16)
    nchunk = max(1, (n_pos + chunk - 1) // chunk)
    head_bytes = (n_pos if fault == "head-stride" else n_slots) * row_bytes
    slot_bytes = hkv * n_slots * row_bytes
    if fault == "slot-stride":
        slot_bytes = n_slots * row_bytes                                              # the stride of a layer with one kv head
    for l0 in range(0, L, MAX_LAYERS):
        nl = min(MAX_LAYERS, L - l0)
        base_l = 0 if (fault == "layer-base" and l0 > 0) else l0
        kv = [flat[base_l + i // 2][i % 2] for i in range(2 * nl)]
        if fault == "v-from-k":
            kv_src = [flat[base_l + i // 2][0] for i in range(2 * nl)]
        else:
            kv_src = kv
        nkv = 2 * nl * hkv * nchunk if n_pos > 0 else 0
        state = l0 + nl == L or fault == "state-every-launch"
        if fault == "state-first-launch":
            state = l0 == 0
        for b in range(nkv):
            ci, rest = b % nchunk, b // nchunk
            head, lk = rest % hkv, rest // hkv
            p0 = ci * chunk
            np_ = min(chunk, n_pos - p0)
            if fault == "drop-last-chunk" and ci == nchunk - 1:
                continue
            if fault == "tail-copies-chunk":
                np_ = chunk
            base = head * head_bytes + p0 * row16 * 16
            cp(kv[lk], base + dst * slot_bytes, base + src * slot_bytes, np_ * row16 * 16, kv_src[lk])
        if not state:
            continue
        R, cap = g["R"], g["cap"]
        seq_words = R * int(s.nf[src]) if fault == "seq-R-x-nf" else R * cap
        sf, st = o.seq[src].reshape(-1), o.seq[dst].reshape(-1)
        for i in range(R * cap):
            v = sf[i]
            if i < seq_words:
                st[i] = v
            if fault != "from-seq0" or i != 0:
                sf[i] = g["im_end_id"] if i == 0 else 0
        for i in range(R):
            a, c = o.tok[src, i], o.tokn[src, i]
            o.tok[dst, i] = a
            if fault != "tokn-stays":
                o.tokn[dst, i] = c
            if fault != "from-tok":
                o.tok[src, i] = 0
            if fault == "from-tokn-cleared":
                o.tokn[src, i] = 0
        if fault != "ctl-stays":
            o.ctl[dst] = o.ctl[src]
        if fault == "from-ctl-cleared":
            o.ctl[src] = 0
        ps, nf, dn = o.pos[src], o.nf[src], o.done[src]
        o.pos[dst], o.nf[dst], o.done[dst] = ps, nf, dn
        if fault != "from-pos":
            o.pos[src] = 0
        if fault != "from-nf":
            o.nf[src] = 1
        if fault != "from-done":
            o.done[src] = 1
    return o


def copy2d(dst, dpitch, src, spitch, width, height):
    for h in range(height):
        cp(dst, h * dpitch, h * spitch, width, src)


def emu_kv_copy(s, snap, n_pos, slot, save, fault=None):
    """kv_copy: per layer and K | V one 2-D copy of Hkv rows of n_pos x hd elements at a pitch of n_slots x hd.  snap: flat
    bytes [layer][K | V][Hkv][n_pos][hd]."""
    g = s.geo
    row_bytes = g["head_dim"] * g["esz"]
    row, pitch = n_pos * row_bytes, g["n_slots"] * row_bytes
    slot_bytes = g["Hkv"] * pitch
    for l in range(g["n_layer"]):
        for k in range(2):
            cache = s.kv[l, k].reshape(-1)[slot * slot_bytes:]
            packed = snap[(l * 2 + k) * g["Hkv"] * row:]
            if save:
                copy2d(packed, row, cache, pitch, row, g["Hkv"])
            elif fault == "row-pitch-swapped":
                copy2d(cache, row, packed, pitch, row, g["Hkv"])
            elif fault == "writes-n_slots-rows":
                copy2d(cache, pitch, packed, row, pitch, g["Hkv"])
            else:
                copy2d(cache, pitch, packed, row, row, g["Hkv"])


def emu_save(s, slot, n_pos, fault=None):
    g = s.geo
    snap = np.zeros(g["n_layer"] * 2 * g["Hkv"] * n_pos * g["head_dim"] * g["esz"], dtype=np.uint8)
    emu_kv_copy(s, snap, n_pos, slot + 1 if fault == "wrong-slot" else slot, True)
    return snap


def emu_restore(s, snap, n_pos, slot, fault=None):
    o = s.copy()
    emu_kv_copy(o, snap, n_pos, slot, False, fault)
    return o


# ------------------------------------------------------------------------------------------------ the honest emulation
@pytest.mark.parametrize("geo", G.geometries(), ids=lambda g: g[0])
def test_honest_emulation_shows_no_difference(geo):
    name, n_layer, hkv, n_slots, hd, esz, mb, positions = geo
    if mb > 8:
        routes = ((mb - 1, 0), (1, mb - 1))
    else:
        routes = tuple((a, b) for a, b, _ in G.ROUTES if a < mb and b < mb) or ((mb - 1, 0),)
    s = random_state(n_layer, hkv, n_slots, hd, esz, mb, seed=len(name))
    for i, n_pos in enumerate(positions):
        src, dst = routes[i % len(routes)]
        s.pos[:] = np.random.default_rng(i).integers(0, n_slots + 1, size=mb)
        s.pos[src] = n_pos
        got, want = emu_move(s, src, dst), S.move(s, src, dst)
        assert S.diff(got, want) is None, (n_pos, S.describe(S.diff(got, want), got, want))
        assert np.array_equal(got.kv[:, :, dst, :, :n_pos], s.kv[:, :, src, :, :n_pos])
        s = got
    # positions outside the cache are held inside it
    for p, n in ((-3, 0), (n_slots + 5, n_slots)):
        s.pos[0] = p
        assert S.moved_positions(s, 0) == n and S.diff(emu_move(s, 0, 1), S.move(s, 0, 1)) is None


@pytest.mark.parametrize("geo", [g for g in G.geometries() if g[6] == 4], ids=lambda g: g[0])
def test_honest_snapshots_show_no_difference(geo):
    name, n_layer, hkv, n_slots, hd, esz, mb, _ = geo
    shape_name, pr = name.split("-")
    s = random_state(n_layer, hkv, n_slots, hd, esz, mb, seed=7)
    for n_pos in G.snapshot_positions(G.SHAPES[shape_name](), pr):
        snap = emu_save(s, 2, n_pos)
        assert np.array_equal(snap, S.save(s, 2, n_pos).reshape(-1))
        for slot in (2, 0, 3):
            got, want = emu_restore(s, snap, n_pos, slot), S.restore(s, S.save(s, 2, n_pos), slot)
            assert S.diff(got, want) is None, S.describe(S.diff(got, want), got, want)
            assert np.array_equal(got.kv[:, :, slot, :, n_pos:], s.kv[:, :, slot, :, n_pos:])


def test_park_and_reset_touch_what_they_name():
    s = random_state(2, 2, 16, 16, 2, 3)
    p = S.park(s, 1)
    assert p.seq[1, 0, 0] == IM_END and not p.seq[1].reshape(-1)[1:].any() and (p.nf[1], p.done[1], p.pos[1]) == (1, 1, 0) and not p.tok[1].any()
    assert np.array_equal(p.tokn, s.tokn) and np.array_equal(p.ctl, s.ctl) and np.array_equal(p.kv, s.kv)
    assert S.diff(p, s) == ("seq", 1, 0)
    r = S.reset(s, 2)
    assert not r.seq[2].any() and (r.pos[2], r.nf[2], r.done[2]) == (0, 0, 0) and np.array_equal(r.tok, s.tok)
    assert S.diff(S.park(p, 1), p) is None and S.diff(r, s) == ("seq", 2, 0)
    # diff names the first place in walking order, and describe says it in words
    t = s.copy()
    t.kv[1, 1, 2, 1, 5, 3] ^= 1
    t.kv[1, 1, 2, 1, 9, 0] ^= 1
    t.pos[0] += 1
    assert S.diff(t, s) == ("kv", 1, "V", 2, 1, 5) and "layer 1, V, slot 2, kv head 1, row 5" in S.describe(S.diff(t, s), t, s)
    u = s.copy()
    u.hid_in_xo[2] ^= 1
    assert S.diff(u, s) == ("hid_in_xo", 2, 0)


# ------------------------------------------------------------------------------------------------ planted faults
# head_dim 128 in bf16: chunks of 64 positions; 4 slots, 2 kv heads, a 200-row cache; 150 = 64 + 64 + 22 positions from 3 to 1
def fault_state(n_layer=2):
    s = random_state(n_layer, 2, 200, 128, 2, 4, seed=3)
    s.pos[:] = (190, 170, 33, 150)
    s.nf[3] = 4
    return s


KV_FAULTS = [("drop-last-chunk", 2, ("kv", 0, "K", 1, 0, 128)),
             ("tail-copies-chunk", 2, ("kv", 0, "K", 1, 0, 150)),          # the overrun: rows 150 .. 191 of `to`
             ("n_pos-1", 2, ("kv", 0, "K", 1, 0, 149)),
             ("head-stride", 2, ("kv", 0, "K", 1, 0, 150)),                # head 1 lands behind head 0's 150 rows
             ("v-from-k", 2, ("kv", 0, "V", 1, 0, 0)),
             ("layer-base", 65, ("kv", 64, "K", 1, 0, 0)),                 # the second launch copies layer 0 again
             ("slot-stride", 2, ("kv", 0, "K", 0, 1, 0))]                  # 1 x head stride: slot 0's head 1 is written
STATE_FAULTS = [("state-every-launch", 65, ("seq", 1, 0)),                  # the second block moves a parked `from` over `to`
                ("tokn-stays", 2, ("tokn", 1, 0)),
                ("ctl-stays", 2, ("ctl", 1, 0)),
                ("seq-R-x-nf", 2, ("seq", 1, 5 * 4)),
                ("from-seq0", 2, ("seq", 3, 0)),
                ("from-tok", 2, ("tok", 3, 0)),
                ("from-pos", 2, ("pos", 3, 0)),
                ("from-nf", 2, ("nf", 3, 0)),
                ("from-done", 2, ("done", 3, 0)),
                ("from-tokn-cleared", 2, ("tokn", 3, 0)),
                ("from-ctl-cleared", 2, ("ctl", 3, 0))]


@pytest.mark.parametrize("fault,n_layer,where", KV_FAULTS + STATE_FAULTS, ids=lambda v: v if isinstance(v, str) else None)
def test_planted_move_faults_are_flagged_where_they_sit(fault, n_layer, where):
    s = fault_state(n_layer)
    want = S.move(s, 3, 1)
    assert S.diff(emu_move(s, 3, 1), want) is None
    got = emu_move(s, 3, 1, fault)
    assert S.diff(got, want) == where, (fault, S.describe(S.diff(got, want), got, want))


def test_a_state_block_in_the_first_launch_alone_leaves_the_same_bytes():
    """Which of the 64-layer launches carries the state block cannot show in the bytes - the launches are stream-ordered and
    n_pos is read before the first - so the planted fault above is the block running in EVERY launch."""
    s = fault_state(65)
    assert S.diff(emu_move(s, 3, 1, "state-first-launch"), S.move(s, 3, 1)) is None


SNAP_FAULTS = [("row-pitch-swapped", ("kv", 0, "K", 0, 0, 70)),            # head 1's rows land behind head 0's 70
               ("writes-n_slots-rows", ("kv", 0, "K", 0, 0, 70)),
               ("wrong-slot", ("kv", 0, "K", 0, 0, 0))]


@pytest.mark.parametrize("fault,where", SNAP_FAULTS, ids=lambda v: v if isinstance(v, str) else None)
def test_planted_snapshot_faults_are_flagged_where_they_sit(fault, where):
    s = fault_state()
    snap = emu_save(s, 2, 70, fault)
    want = S.restore(s, S.save(s, 2, 70), 0)
    got = emu_restore(s, snap, 70, 0, fault)
    assert S.diff(got, want) == where, (fault, S.describe(S.diff(got, want), got, want))
    assert S.diff(emu_restore(s, emu_save(s, 2, 70), 70, 0), want) is None


def test_the_case_lists_keep_their_edges():
    """A later edit of the GPU file's lists cannot silently drop an edge."""
    sh = G.hd128_shape()
    assert G.n_slots_of(sh) == 200 and sh.max_seq_len % 8
    for pr, c in (("bf16", 64), ("fp16", 64), ("fp32", 32)):
        assert S.chunk_positions(128, G.ESZ[pr]) == c
        assert {0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1, 196, 197} <= set(G.move_positions(sh, pr))
        assert {1, c - 1, c, c + 1, 200} <= set(G.snapshot_positions(sh, pr))
        assert {(n, c) for n in (0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1, 196, 197)} <= G.expected_reached()[pr]
    assert S.chunk_positions(8, 2) == 1024 and S.chunk_positions(16, 4) == 256
    assert G.DEEP_LAYERS == (65, 130) and G.WIDE_BATCH == 256
    assert {(a > b) for a, b, _ in G.ROUTES} == {True, False} and any(b == 3 for _, b, _ in G.ROUTES) and any(a == 0 for a, _, _ in G.ROUTES)
