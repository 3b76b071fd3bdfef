"""GPU: the reference intake on the device (include/fishtts_hip.h: "Reference intake"; CodecHipEngine.intake and
encode_items) against its float64 restatement (tests/intake_ref.py) on the tiny encoder shape of tests/test_codec_gpu.py.

Bounds.  Conversion, downmix, counters, lengths, cuts, the multiply of the level stage and the ramps of the trim are stated to
the bit and compared bit for bit.  The polyphase sum is float32 over K taps in a fixed order: against the float64 sum of the
same float32 products' exact values each partial sum rounds once, so |y - ref| <= (K + 2) 2^-24 sum_t |w[p][t] m[.]| +
2^-24 |ref| (K - 1 additions and K products of relative error 2^-24 each, first-order, one spare; the last term is the
rounding of the reference's own conversion) - derived, not measured.  A 1 kHz tone comes out within 1e-3 of the tone at
44.1 kHz away from the edges (the figure tests/test_resample_gpu.py holds for the same design: 0.01 dB of ripple is 1.2e-3
relative on an amplitude of 0.5, plus the stop band's -70 dB).  The loudness agrees with tests/level_ref.py within 1e-6 LU
(tests/test_level_gpu.py's bound) on inputs whose gate margin is at least 1e-3 LU.

The stop-band case.  A 26 460 Hz tone (0.6 x 44 100: what folds back to 17 640 Hz if it is let through) must be down by
70 dB at every input rate above 44 100 Hz that can hold it: 64 000 Hz and up.  A file at 48 000 Hz cannot contain 26 460 Hz
(its Nyquist frequency is 24 000 Hz; sampled there the tone IS a 21 540 Hz tone, inside the transition band), so at 48 000 Hz
the case uses 23 000 Hz, which lies in the stop band (from 22 050 Hz) and folds back to 21 100 Hz."""
import ctypes as C

import numpy as np
import pytest

from tests import intake_ref as R
from tests import join_ref, level_ref
from tests.test_codec_gpu import encode_shape, make_codec, make_codec_with_encoder

pytestmark = pytest.mark.gpu
FO = 44100
MAX_FRAMES = 4200            # the level stage's longest item then exceeds 573 300 samples (13 s at 8 kHz -> 44.1 kHz)
NOTHING = (0.0, 1, 0, 0)
TRIM = (10.0 ** (-45.0 / 20.0), 220, 1323, 220)      # longform.join_params(44100, 0, 0, -45.0)


@pytest.fixture(scope="module")
def eng():
    e, _ = make_codec_with_encoder(encode_shape(), max_frames=MAX_FRAMES)
    yield e
    e.close()


def clip(v, fmt, rate, **kw):
    from fish_tts_amd.wavfile import parse_wav
    b = R.wav_bytes(v, fmt, rate, **kw)
    return b, parse_wav(b)


def raw_of(c):
    b, info = c
    return b[info.data_offset:info.data_offset + info.n_frames * info.channels * R.WIDTH[info.fmt]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pcm16(n, seed=0, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = amp * np.sin(2 * np.pi * 220.0 * t / FO) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t / FO)) + 0.02 * rng.standard_normal(n)
    return np.clip(np.round(x * 32768), -32767, 32767).astype(np.int64)


def test_anchor_16_bit_mono_native_rate(eng):
    k = pcm16(30 * 64 + 17)
    want = k.astype(np.int16).astype(np.float32) / 32768.0
    pieces, reps = eng.intake([clip(k, "s16", FO)])
    assert np.array_equal(bits(pieces[0]), bits(want))
    assert (reps[0].n44, reps[0].cut, reps[0].frames, reps[0].status) == (len(k), (0, len(k)), 31, 0)
    codes, reps2 = eng.encode_items([clip(k, "s16", FO)])
    assert reps2 == reps
    assert codes[0].dtype == np.int64 and np.array_equal(codes[0], eng.encode(want))


def test_formats_give_the_same_bits_and_exact_counters(eng):
    k = pcm16(30000, seed=1)
    k[[5, 900, 29999]] = (32767, -32768, 32767)          # extreme codes: counted
    f = (k / 32768.0).astype(np.float32)
    f2 = np.stack([f, f], 1)
    same = [clip(k, "s16", FO), clip(k << 8, "s24", FO), clip(k << 16, "s32", FO), clip(f, "f32", FO),
            clip(np.stack([k, k], 1), "s16", FO), clip(np.stack([k << 8] * 8, 1), "s24", FO, extensible=True), clip(f2, "f32", FO)]
    pieces, reps = eng.intake(same)
    codes, reps2 = eng.encode_items(same)
    assert reps == reps2
    want = k.astype(np.float32) / 32768.0
    for c, p, r, cd in zip(same, pieces, reps, codes):
        m, clipped, bad = R.mono(raw_of(c), c[1].fmt, c[1].channels)
        assert np.array_equal(bits(m), bits(want))
        assert np.array_equal(bits(p), bits(want)), c[1]
        assert (r.clipped, r.nonfinite) == (clipped, bad), (c[1], r)
        assert np.array_equal(cd, codes[0])
    assert [r.clipped for r in reps] == [3, 1, 1, 1, 6, 8, 2]     # -32768 alone is extreme after a shift; |f| >= 1 for it alone
    # u8, every code
    u = np.random.default_rng(2).integers(0, 256, 5000)
    u[:256] = np.arange(256)
    pieces, reps = eng.intake([clip(u, "u8", FO)])
    assert np.array_equal(bits(pieces[0]), bits(((u - 128) / 128.0).astype(np.float32)))
    assert reps[0].clipped == int(np.sum((u == 0) | (u == 255)))
    # L = x, R = -x: the mean is silence; channel 0 alone is the mono file
    k = np.clip(k, -32767, 32767)                       # (-32768 has no negative in 16 bits)
    want = k.astype(np.float32) / 32768.0
    st = clip(np.stack([k, -k], 1), "s16", FO)
    pieces, reps = eng.intake([st], TRIM)
    assert reps[0].status == 1 and reps[0].cut == (0, 0) and len(pieces[0]) == 0 and reps[0].level.peak == 0.0
    pieces, reps = eng.intake([st])
    assert np.array_equal(bits(pieces[0]), np.zeros(len(k), dtype=np.uint32))          # +0.0 throughout
    pieces, reps = eng.intake([st], channel=0)
    assert np.array_equal(bits(pieces[0]), bits(want)) and reps[0].clipped == 2
    pieces, reps = eng.intake([st], channel=1)
    assert np.array_equal(bits(pieces[0]), bits((-k).astype(np.float32) / 32768.0)) and reps[0].clipped == 1     # (a zero stays +0.0)
    # float samples that are not finite count as 0, in a 3-channel mean
    g = np.random.default_rng(3).uniform(-1.2, 1.2, (4000, 3)).astype(np.float32)
    g[7, 0], g[8, 1], g[4000 - 1, 2], g[100, 1] = np.inf, np.nan, -np.inf, 1.0
    c = clip(g, "f32", FO)
    m, clipped, bad = R.mono(raw_of(c), "f32", 3)
    pieces, reps = eng.intake([c])
    assert np.array_equal(bits(pieces[0]), bits(m)) and (reps[0].clipped, reps[0].nonfinite) == (clipped, bad) and bad == 3
    m1, c1, b1 = R.mono(raw_of(c), "f32", 3, channel=1)
    pieces, reps = eng.intake([c], channel=1)
    assert np.array_equal(bits(pieces[0]), bits(m1)) and (reps[0].clipped, reps[0].nonfinite) == (c1, b1) and b1 == 1


def check_sum(y, m, rate, tab):
    """The float32 accumulation bound of the module docstring, per output."""
    ref, mag = R.resample(m, rate, tab, with_bound=True)
    K = tab[2]
    assert len(y) == len(ref) == -(-len(m) * tab[0] // tab[1])
    bound = (K + 2) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(ref)
    err = np.abs(y.astype(np.float64) - ref)
    worst = int(np.argmax(err - bound))
    print(f"rate {rate}: K {K}, n_out {len(y)}, max err {err.max():.3e}, worst err / bound {err[worst] / max(bound[worst], 1e-300):.3f}")
    assert np.all(err <= bound), (rate, worst, err[worst], bound[worst])


@pytest.mark.parametrize("rate", R.RATES)
def test_resampler_at_every_input_rate(eng, rate):
    tab = L, M, K, w = R.filter_table(rate)
    n = rate // 2
    t = np.arange(n) / rate
    tone = (0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    noise = np.random.default_rng(rate).uniform(-0.9, 0.9, n).astype(np.float32)
    clips = [clip(tone, "f32", rate), clip(noise, "f32", rate)]
    stop_hz = None
    if rate > FO:
        stop_hz = 26460.0 if rate >= 64000 else 23000.0          # (module docstring)
        clips.append(clip((0.5 * np.sin(2 * np.pi * stop_hz * t)).astype(np.float32), "f32", rate))
    pieces, reps = eng.intake(clips)
    n_out = -(-n * L // M)
    assert [len(p) for p in pieces] == [n_out] * len(clips) and all(r.n44 == n_out and r.cut == (0, n_out) for r in reps)
    edge = (K // 2) * L // M + 2            # outputs whose taps reach past either end of the clip
    to = np.arange(n_out) / FO
    err = np.abs(pieces[0] - 0.5 * np.sin(2 * np.pi * 1000.0 * to))[edge:n_out - edge]
    print(f"rate {rate}: tone err {err.max():.2e}")
    assert err.max() <= 1e-3
    check_sum(pieces[1], noise, rate, tab)
    if stop_hz:
        left = np.max(np.abs(pieces[2][edge:n_out - edge]))
        print(f"rate {rate}: {stop_hz:g} Hz down by {-20 * np.log10(left / 0.5):.1f} dB")
        assert left <= 0.5 * 10.0 ** (-70.0 / 20.0)


def test_more_outputs_than_one_pass_of_the_grid(eng):
    """13 s at 8 kHz: 573 300 outputs, more than the 2048 workgroups x 256 of one pass."""
    rate, n = 8000, 13 * 8000
    k = np.random.default_rng(5).integers(-30000, 30000, n)
    c = clip(k, "s16", rate)
    pieces, reps = eng.intake([c])
    assert reps[0].n44 == len(pieces[0]) == 573300 > 2048 * 256
    m, clipped, _ = R.mono(raw_of(c), "s16", 1)
    check_sum(pieces[0], m, rate, R.filter_table(rate))
    assert reps[0].clipped == clipped == 0


def mixed_clips():
    rng = np.random.default_rng(11)
    f8 = rng.uniform(-0.8, 0.8, (96000, 8)).astype(np.float32)                    # 0.5 s at 192 kHz, 8 channels: the widest window
    s24 = rng.integers(-(1 << 22), 1 << 22, 24001)                                # an odd number of 3-byte frames ...
    f16 = rng.uniform(-0.8, 0.8, 8000).astype(np.float32)                         # ... in front of a float clip
    return [clip(pcm16(1, 2) + 900, "s16", FO), clip(f8, "f32", 192000, extensible=True), clip(s24, "s24", 48000), clip(f16, "f32", 16000),
            clip(pcm16(255, 3), "s16", FO), clip(rng.integers(0, 256, (256, 2)), "u8", FO), clip(pcm16(257, 4) << 16, "s32", FO)]


def test_one_launch_many_clips_equals_each_clip_alone(eng):
    clips = mixed_clips()
    pieces, reps = eng.intake(clips)
    codes, reps2 = eng.encode_items(clips)
    assert reps == reps2 and [r.status for r in reps] == [0] * 7
    assert [r.n44 for r in reps] == [1, 22050, 22051, 22050, 255, 256, 257]
    for i, c in enumerate(clips):
        p1, r1 = eng.intake([c])
        c1, _ = eng.encode_items([c])
        assert r1[0] == reps[i], i
        assert np.array_equal(bits(p1[0]), bits(pieces[i])), i
        assert np.array_equal(c1[0], codes[i]) and codes[i].shape == (eng.R, reps[i].frames), i
        assert np.array_equal(codes[i], eng.encode(pieces[i])), i
    again, reps3 = eng.intake(clips)
    assert reps3 == reps and all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, pieces))
    # the restatement, for the clips of the call that no other test covers: 8 channels at 192 kHz, 24 bits at 48 kHz
    for i in (1, 2):
        info = clips[i][1]
        m, clipped, bad = R.mono(raw_of(clips[i]), info.fmt, info.channels)
        check_sum(pieces[i], m, info.rate, R.filter_table(info.rate))
        assert (reps[i].clipped, reps[i].nonfinite) == (clipped, bad)


def padded_clip(rate=FO, fmt="s16"):
    """0.4 s of digital silence, 1 s of signal, 0.4 s of digital silence."""
    q, n = int(0.4 * rate), rate
    t = np.arange(n) / rate
    x = 0.2 * np.sin(2 * np.pi * 330.0 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 2.0 * t) ** 2) + 0.01 * np.random.default_rng(8).standard_normal(n)
    k = np.concatenate([np.zeros(q), np.round(x * 32768), np.zeros(q)]).astype(np.int64)
    return clip(k, fmt, rate)


@pytest.mark.parametrize("rate", [FO, 48000])
def test_level_and_trim(eng, rate):
    c = padded_clip(rate)
    plain, reps = eng.intake([c])
    x = plain[0]
    ref = level_ref.measure(x, FO, -2300)
    assert ref.margin >= 1e-3, ref.margin
    print(f"rate {rate}: L {reps[0].level.lufs:.6f} ref {ref.L:.6f} margin {ref.margin:.3e}")
    assert abs(reps[0].level.lufs - ref.L) <= 1e-6 and reps[0].level.gain == 1.0
    assert np.array_equal(bits(np.float32(reps[0].level.peak)), bits(ref.p))
    # a target: one float32 multiply by the reported gain
    lev, lreps = eng.intake([c], loudness=-23.0)
    g = np.float32(lreps[0].level.gain)
    assert abs(float(g) - float(ref.g)) <= 4e-7 * float(ref.g) and lreps[0].level.lufs == reps[0].level.lufs
    assert np.array_equal(bits(lev[0]), bits(x * g))
    # the trim: the join stage's result over the untrimmed one, with and without the level
    for untrimmed, loud in ((x, None), (lev[0], -23.0)):
        cut, creps = eng.intake([c], TRIM, loudness=loud)
        a, e = join_ref.edges(untrimmed, np.float32(TRIM[0]), TRIM[1], TRIM[2])
        assert creps[0].cut == (a, e) and 0 < a < e < len(x)
        assert np.array_equal(bits(cut[0]), bits(join_ref.piece(untrimmed, a, e, TRIM[3])))
        assert abs(a - (0.4 * FO - TRIM[2])) <= 2 * TRIM[1] + 80 and abs(e - (1.4 * FO + TRIM[2])) <= 2 * TRIM[1] + 80
        codes, ereps = eng.encode_items([c], TRIM, loudness=loud)
        assert ereps == creps and creps[0].frames == -(-(e - a) // eng.enc_frame_len) == codes[0].shape[1]
        assert np.array_equal(codes[0], eng.encode(cut[0]))
    full, _ = eng.encode_items([c])
    assert full[0].shape[1] == -(-len(x) // eng.enc_frame_len) > creps[0].frames
    # the chain's restatement gives the same piece from the same 44.1 kHz samples
    piece, (a2, e2), _ = R.chain(x, -2300, TRIM)
    if np.array_equal(bits(np.float32(ref.g)), bits(g)):
        assert (a2, e2) == (a, e) and np.array_equal(bits(piece), bits(cut[0]))


def test_statuses(eng):
    quiet = clip(np.random.default_rng(1).integers(-40, 41, 20000), "s16", FO)           # below -45 dBFS (184 codes) throughout
    long_ = clip(pcm16(eng.max_enc_frames * eng.enc_frame_len + 3000, 6), "s16", FO)
    good = clip(pcm16(9000, 7), "s16", 22050)
    codes, reps = eng.encode_items([quiet, good, long_, good], TRIM)
    assert [r.status for r in reps] == [1, 0, 2, 0] and [r.frames > 0 for r in reps] == [False, True, False, True]
    assert codes[0] is None and codes[2] is None and reps[2].kept > eng.max_enc_frames * eng.enc_frame_len
    alone, areps = eng.encode_items([good], TRIM)
    assert areps[0] == reps[1] == reps[3] and np.array_equal(alone[0], codes[1]) and np.array_equal(alone[0], codes[3])
    pieces, preps = eng.intake([quiet, good, long_, good], TRIM)
    assert preps == reps and [len(p) for p in pieces] == [r.kept for r in reps] and len(pieces[0]) == 0


def _item(L, buf, n_frames, rate=FO, channels=1, fmt=1, channel=-1):
    return L.ft_intake_item(buf.ctypes.data if buf is not None else None, n_frames, rate, channels, fmt, channel)


def test_refusals_change_nothing(eng):
    from fish_tts_amd import _lib as L
    lib = eng.lib
    k = pcm16(30 * 64 + 17)
    anchor = clip(k, "s16", FO)
    want_codes, _ = eng.encode_items([anchor])
    buf = np.zeros(1 << 16, dtype=np.uint8)
    jp = L.ft_join_params(0.0, 1, 0, 0)
    audio = np.zeros(1 << 16, dtype=np.float32)
    codes = np.zeros(eng.R * 2048, dtype=np.int32)
    lens = np.zeros(64, dtype=np.int64)
    infos = (L.ft_intake_info * 64)()
    P = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def both(status, items, B=None, jp_=jp, loudness=0, cap=1 << 16, cap_frames=2048, infos_=infos, what=""):
        B = len(items) if B is None else B
        arr = (L.ft_intake_item * max(len(items), 1))(*items)
        assert lib.ft_codec_intake(eng._h, B, arr, C.byref(jp_) if jp_ else None, loudness, P(audio), cap, P(lens), infos_) == status, what
        assert lib.ft_codec_encode_items(eng._h, B, arr, C.byref(jp_) if jp_ else None, loudness, P(codes), cap_frames, infos_) == status, what

    ok = _item(L, buf, 1000)
    ARG, LONG = L.FT_ERR_ARG, L.FT_ERR_TOO_LONG
    both(ARG, [ok], B=0, what="B = 0")
    both(ARG, [ok] * 65, what="B = 65")
    both(ARG, [ok], jp_=None, what="null jp")
    both(ARG, [ok], infos_=None, what="null infos")
    both(ARG, [_item(L, None, 1000)], what="null data")
    both(ARG, [_item(L, buf, 0)], what="0 frames")
    both(ARG, [ok, _item(L, buf, 1000, fmt=5)], what="fmt 5")
    both(ARG, [_item(L, buf, 1000, fmt=-1)], what="fmt -1")
    both(ARG, [_item(L, buf, 1000, channels=0)], what="0 channels")
    both(ARG, [_item(L, buf, 1000, channels=9)], what="9 channels")
    both(ARG, [_item(L, buf, 1000, channels=2, channel=2)], what="channel 2 of 2")
    both(ARG, [_item(L, buf, 1000, channel=-2)], what="channel -2")
    for rate in (7999, 192001, 44099, 47999):
        both(ARG, [ok, _item(L, buf, 1000, rate=rate)], what=f"rate {rate}")
    for loud in (-1, -5001, -499, 100):
        both(ARG, [ok], loudness=loud, what=f"loudness {loud}")
    for bad in (L.ft_join_params(-1.0, 1, 0, 0), L.ft_join_params(float("nan"), 1, 0, 0), L.ft_join_params(0.0, 0, 0, 0),
                L.ft_join_params(0.0, 1, -1, 0), L.ft_join_params(0.0, 1, 0, -1)):
        both(ARG, [ok], jp_=bad, what="join parameters")
    both(ARG, [ok, ok], cap=1999, cap_frames=2 * 16 - 1, what="capacity")          # 1000 samples: 16 frames of 64 each
    assert lib.ft_codec_intake(eng._h, 1, (L.ft_intake_item * 1)(ok), C.byref(jp), 0, None, 1 << 16, P(lens), infos) == ARG
    assert lib.ft_codec_intake(eng._h, 1, (L.ft_intake_item * 1)(ok), C.byref(jp), 0, P(audio), 1 << 16, None, infos) == ARG
    assert lib.ft_codec_encode_items(eng._h, 1, (L.ft_intake_item * 1)(ok), C.byref(jp), 0, None, 2048, infos) == ARG
    assert lib.ft_codec_intake(eng._h, 1, None, C.byref(jp), 0, P(audio), 1 << 16, P(lens), infos) == ARG
    # too long: beyond the level stage's longest item; beyond 2^30 raw bytes (judged before a byte is read)
    most = -(-2 * MAX_FRAMES * eng.frame_len * 48000 // FO)
    both(LONG, [_item(L, buf, most + 1, fmt=0)], cap=1 << 40, cap_frames=1 << 40, what="n44")
    both(LONG, [_item(L, buf, (1 << 30) + 16, fmt=0)], cap=1 << 40, cap_frames=1 << 40, what="2^30 bytes in one clip")
    both(LONG, [ok, _item(L, buf, 1 << 28, rate=192000, fmt=3)], cap=1 << 40, cap_frames=1 << 40, what="2^30 bytes over two clips")
    # no encoder: the pieces still come, the codes are refused
    dec, _ = make_codec(encode_shape(), max_frames=64)
    try:
        arr = (L.ft_intake_item * 1)(_item(L, buf, 1000))
        assert lib.ft_codec_encode_items(dec._h, 1, arr, C.byref(jp), 0, P(codes), 2048, infos) == L.FT_ERR_STATE
        assert lib.ft_codec_intake(dec._h, 1, arr, C.byref(jp), 0, P(audio), 1 << 16, P(lens), infos) == L.FT_OK
        assert lens[0] == 1000 and infos[0].frames == 0 and infos[0].status == 0 and not audio[:1000].any()
        with pytest.raises(RuntimeError, match="encoder not built"):
            dec.encode_items([anchor])
    finally:
        dec.close()
    # the Python layer refuses before the native call
    for bad_kw in (dict(channel=1), dict(channel=-1), dict(channel=True), dict(loudness=-4.0), dict(loudness="x"),
                   dict(params=(0.0, 0, 0, 0)), dict(params=(-1.0, 1, 0, 0))):
        with pytest.raises(ValueError):
            eng.intake([anchor], **bad_kw)
    with pytest.raises(ValueError, match="1 to 64"):
        eng.intake([])
    with pytest.raises(ValueError, match="1 to 64"):
        eng.encode_items([anchor] * 65)
    with pytest.raises(ValueError, match="sample rate"):
        eng.intake([clip(k, "s16", 44099)])
    # nothing changed: the anchor's bits
    got, _ = eng.encode_items([anchor])
    assert np.array_equal(got[0], want_codes[0])
    pieces, _ = eng.intake([anchor])
    assert np.array_equal(bits(pieces[0]), bits(k.astype(np.float32) / 32768.0))
