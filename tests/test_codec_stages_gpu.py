"""Every launch of a one-shot codec decode / encode, element by element, against the float64 stage reference.

The engine's launch trace (include/fishtts_hip_test.h, ft_test_codec_trace_*) hands out, per launch, what that launch
wrote; tests/codec_stage_ref.py recomputes it in float64 from the RECORDED inputs (teacher forcing) and the weights as
the device holds them.  Every checked element must satisfy
    |got - ref| <= half a ulp of the stored format (bf16 / f32) at max(|got|, |ref|) + err,
with err the bound derived in codec_stage_ref's docstring from the arithmetic (the contraction's from the reference's
own float32 re-evaluation in three orders; nothing is calibrated on the device's output), and the allowed number of
failing or excluded elements is zero.  Checked rows: all of them below 4096 rows, else the subset select_rows states
(first halo + 8 rows, the last two row tiles of the instantiation picked, tile boundaries, 1024 seeded rows).
tests/test_codec_stage_ref_host.py shows on the CPU that this checker passes an honest float32 emulation and flags
each of a list of subtle emulated kernel bugs.

Cases: decode at the real widths at lengths on both sides of every row threshold of gemm() (skinny <= 1024, 8-wave
>= 4096, full-width >= 30000 rows) for the stages that cross it below 320 frames, plus 1 and 215 frames; decode at
tiny_codec_shape(); a narrow shape (96-wide latent) that reaches the BK = 32 tiles with 128-wide N; encode at
encode_shape(); two decodes in a row, the second shorter (stale rows in front of the work buffers).

Encode at the real widths: ENC_REAL_LENGTHS (both sides of every gemm() threshold an encode stage crosses, and of BOTH
attention windows: the encoder transformer's 512 at 4 rows per frame and the pre-module's 128 at 1 row per frame first
drop a key at frame 129), the sample counts that leave no zero fill / one sample in the last frame / one sample in all,
and a 17-frame encode after a 257-frame one.  From 127 frames on a case is one of three launch ranges of the plan
(blocks 0-2; block 3 with its transformer; enc.out, the down stages and the pre-module), each a test of its own: every
launch of every length is checked in one of them, on the same rows as a whole trace would be.  Every traced encode also
has every decision of its quantiser search judged by codec_stage_ref.rvq_search_check on the recorded zq, and
test_search_keeps_the_lowest_index_on_planted_ties runs the search on codebooks in which every decision is an exact tie.
Not run: encodes above 264 frames at the real widths (max_reference_seconds allows 1292): the float64 side of one costs
minutes; every row threshold and both windows are crossed below 264.
test_every_gemm_instantiation_is_covered asserts the coverage over exactly these cases."""
import time

import numpy as np
import pytest
import torch

from oracle import codec as C
from tests import codec_stage_ref as R
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_gpu import _test_audio, args_from_shape, encode_shape, make_codec_with_encoder

pytestmark = pytest.mark.gpu
WINDOW_BYTES = 1.2e9          # host copies held per traced call (a 257-frame trace held whole is ~4 GB)

# decode lengths at the real widths.  Rows per frame: 1 (transformer, up.0.ct), 2 (up.0, up.1.ct), 4 (up.1, dec.in,
# dec.0.ct), 32 (block 0, dec.1.ct), 256 (block 1, dec.2.ct), 1024 (block 2, dec.3.ct), 2048 (block 3).
#   1024 rows: 4 T crosses at 256 | 257.     4096 rows: 2048 T at 1 | 2, 1024 T at 3 | 4, 256 T at 15 | 16, 32 T at 127 | 128.
#   30000 rows: 2048 T at 14 | 15, 1024 T at 29 | 30, 256 T at 117 | 118.      1 and 215: the issue's fixed lengths.
REAL_LENGTHS = (1, 2, 3, 4, 14, 15, 16, 29, 30, 117, 118, 127, 128, 215, 256, 257)
MAX_FRAMES = 320
THRESHOLDS = (("skinny", 1024, lambda rows: rows <= 1024), ("8-wave", 4096, lambda rows: rows >= 4096),
              ("full-width", 30000, lambda rows: rows >= 30000))
# encode lengths at the real widths.  Rows per frame: 2048 (enc.in, block 0), 1024 (enc.0.sc, block 1), 256 (enc.1.sc,
# block 2), 32 (enc.2.sc, block 3), 4 (enc.3.sc, enc.3.tf, enc.out), 2 (down.0), 1 (down.1, pre.).
#   4096 rows (8-wave tiles; N % 128 == 0 or N % 96 == 0 only, so block 0's N = 64 stays at 1 | 2): 1024 T at 3 | 4,
#   256 T at 15 | 16, 32 T at 127 | 128.     1024 rows (skinny: one tap, N <= 2048): 4 T at 256 | 257 (wo, w2 of enc.3.tf).
#   30000 rows: the full-width tiles need N % 192 == 0 or N = 96; the encode has one only at 4 rows per frame (qkv: 7500 frames).
#   attention: 128 is the last length at which every query sees every earlier key; 129 limits one pre. query and four
#   enc.3.tf queries, 130 two and eight.     1: one frame.  215: a 10 s reference.  6, 121: the earlier cases.
ENC_REAL_LENGTHS = (1, 3, 4, 6, 15, 16, 121, 127, 128, 129, 130, 215, 256, 257)
ENC_MAX_FRAMES = 264
ENC_STEPS = ((3, 4), (15, 16), (127, 128), (256, 257))      # each must change the instantiation of some encode stage
ENC_SPLIT_FROM = 127                                         # from here on a case is one launch range of three
ENC_PARTS = ("blocks0-2", "block3", "out-down-pre")
# instantiation ids no supported shape reaches, with the reason (reported as dead code, not skipped silently)
UNREACHABLE = {
    13: "tapgemm<128,128,2,2>: taken only when K % 32 != 0 or a halo exceeds 56 rows; codec_create refuses channel counts "
        "that are not multiples of 32 and the largest halo is 54 (k = 7, dilation 9)",
    14: "tapgemm<128,64,4,1>: as id 13, for N < 128",
}


def narrow_shape():
    """A 96-wide latent: K = 96 (K % 64 = 32) with N = 384 in the ConvNeXt pwconv1 - the BK = 32 tiles with 128-wide N,
    which no other shape of this file reaches (the real widths have K % 64 = 32 only at N = 96)."""
    return C.CodecShape(n_codebooks=3, codebook_size=64, semantic_codebook_size=128, codebook_dim=8, latent_dim=96,
                        n_tf_layer=1, tf_n_head=2, tf_head_dim=48, tf_ffn=96, tf_window=16, tf_block_size=2048,
                        upsample=[2, 2], decoder_dim=64, rates=[2])


def rand_codes(shape, T, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.zeros(shape.n_codebooks + 1, T, dtype=torch.long)
    codes[0] = torch.randint(0, shape.semantic_codebook_size, (T,), generator=g)
    codes[1:] = torch.randint(0, shape.codebook_size, (shape.n_codebooks, T), generator=g)
    return codes.numpy()


def make_decoder(shape, max_frames):
    from fish_tts_amd.codec_engine import CodecHipEngine
    w = C.random_weights(shape, seed=0)
    eng = CodecHipEngine(args_from_shape(shape), device=0, max_frames=max_frames)
    eng.load_state_dict(w)
    return eng, w


def encoder_weights(shape):
    w = C.random_weights(shape, seed=0)
    w.update(C.random_encoder_weights(shape, seed=1))
    return w


class Stats:
    """Per stage kind: the largest |got - ref| / bound, r_stage and (f32-stored contractions) |got - ref| / S."""

    def __init__(self):
        self.kinds, self.variants, self.checked, self.launches = {}, {}, 0, 0

    def add(self, v, rec):
        k = self.kinds.setdefault(v.kind, {"worst": 0.0, "r_stage": 0.0, "over_S": 0.0, "at": ""})
        if v.worst > k["worst"]:
            k["worst"], k["at"] = v.worst, v.name
        k["r_stage"] = max(k["r_stage"], v.r_stage or 0.0)
        k["over_S"] = max(k["over_S"], v.over_S or 0.0)
        self.checked += v.checked
        self.launches += 1

    def report(self, title, variants):
        print(f"\n{title}: {self.launches} launches, {self.checked} elements checked, 0 excluded")
        for kind, k in sorted(self.kinds.items()):
            print(f"  {kind:13s} max |got-ref|/bound {k['worst']:.3f} (at {k['at']})  r_stage {k['r_stage']:.2e}  "
                  f"device |got-ref|/S (f32 stores) {k['over_S']:.2e}")
        print("  instantiations: " + ", ".join(f"{i}:{variants[i]['name']} x{n}" for i, n in sorted(self.variants.items())))


def traced_check(eng, call, plan, weights, stats, same, seed=0, span=None):
    """Run `call` untraced once, then traced in windows of launches; check every launch of `plan` (span = (first, last):
    the names and shapes of all of them, the values of launches [first, last) only).  `same(a, b)`: the traced result
    equals the untraced one bit for bit."""
    variants = eng.trace_variants()
    base = call()
    res, meta = eng.trace(call, 0, 0)
    assert same(res, base), "a traced call (nothing held) differs from the untraced one"
    assert [m["name"] for m in meta] == [st.name for st in plan], \
        [(m["name"], st.name) for m, st in zip(meta, plan) if m["name"] != st.name][:5]
    for m, st in zip(meta, plan):
        assert (m["rows"], m["cols"], sorted(m["kinds"])) == (st.rows, st.cols, sorted(st.dst)), (m, st.name, st.rows, st.cols)
        assert m["halo"] == st.halo, (m, st.halo)
        if st.kind == "gemm":
            assert 0 <= m["variant"] < len(variants) and (m["ntap"], m["K"]) == (len(st.p["offs"]), st.p["K"]), m
            stats.variants[m["variant"]] = stats.variants.get(m["variant"], 0) + 1
        else:
            assert m["variant"] == -1, m
    prod = R.producers(plan)
    size = [st.rows * st.cols * sum(4 if k == "f32" else 2 for k in st.dst) for st in plan]
    W = R.Weights(weights, dev=True)
    bad = []
    c0, last = span or (0, len(plan))
    assert 0 <= c0 < last <= len(plan), (span, len(plan))
    while c0 < last:
        c1, a = c0 + 1, min(prod[c0] + [c0])
        while c1 < last:
            a2 = min(prod[c1] + [a])
            if sum(size[a2:c1 + 1]) > WINDOW_BYTES:
                break
            a, c1 = a2, c1 + 1
        res, launches = eng.trace(call, a, c1 - a)
        assert same(res, base), f"the traced call holding launches [{a}, {c1}) differs from the untraced one"
        env = {}
        for i in range(a, c1):
            st, rec = plan[i], launches[i]
            assert set(rec["out"]) == set(st.dst), (st.name, sorted(rec["out"]))
            if i >= c0:
                bm = variants[rec["variant"]]["bm"] if st.kind == "gemm" else 256
                rows = R.select_rows(st.rows, st.halo, bm, seed)
                assert st.kind != "attn" or len(rows) == st.rows          # every query of every attention launch, windows included
                v = R.check_stage(st, env, W, rec["out"], rows)
                stats.add(v, rec)
                if v.flagged:
                    bad.append((v.name, variants[rec["variant"]]["name"] if st.kind == "gemm" else st.kind, v.flagged,
                                v.checked, round(v.worst, 3), v.rows[:12]))
            for k, b in st.dst.items():
                env[b] = rec["out"][k]
        c0 = c1
    return meta, bad


def same_audio(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_codes(a, b):
    return np.array_equal(a, b)


@pytest.fixture(scope="module")
def real_decoder():
    shape = C.CodecShape()
    eng, w = make_decoder(shape, MAX_FRAMES)
    yield shape, eng, w
    eng.close()


def check_decode(shape, eng, w, T, seed, title):
    codes = rand_codes(shape, T, seed)
    plan = R.plan_decode(shape, codes)
    stats = Stats()
    t0 = time.time()
    meta, bad = traced_check(eng, lambda: eng.decode(codes[None]), plan, w, stats, same_audio, seed)
    stats.report(f"{title}, {T} frames ({time.time() - t0:.1f} s)", eng.trace_variants())
    assert not bad, bad
    return meta


@pytest.mark.parametrize("T", REAL_LENGTHS)
def test_decode_at_the_real_widths(real_decoder, T):
    """Measured on an MI355X: see DESIGN.md ("Codec, per launch") for the recorded ratios per stage kind."""
    shape, eng, w = real_decoder
    check_decode(shape, eng, w, T, seed=100 + T, title="decode, real widths")


@pytest.mark.parametrize("T", (1, 17, 40))
def test_decode_at_the_tiny_shape(T):
    shape = tiny_codec_shape()
    eng, w = make_decoder(shape, 64)
    try:
        check_decode(shape, eng, w, T, seed=T, title="decode, tiny shape")
    finally:
        eng.close()


def test_a_recorded_element_two_ulp_off_is_flagged():
    """The harness end to end on a real trace: the tiny decode held whole passes; the same trace with ONE recorded
    element of one launch moved by two bf16 ulp (or, in the f32 residual stream, by 1e-5 relative) is flagged at that
    launch and row only (the launches after it read the altered value, as they would have on the device, so they are
    judged on what they were given: only the altered launch itself can be off)."""
    shape = tiny_codec_shape()
    eng, w = make_decoder(shape, 64)
    try:
        codes = rand_codes(shape, 40, 2)
        plan = R.plan_decode(shape, codes)
        _, launches = eng.trace(lambda: eng.decode(codes[None]), 0, len(plan))
        trace = [rec["out"] for rec in launches]
        assert not [v.name for v in R.check_trace(plan, trace, w) if v.flagged]
        for name, kind in (("dec.0.u1.c7", "act"), ("up.1.pw2", "bf"), ("dec.1.ct", "bf"), ("post.1.w2", "f32")):
            i = next(j for j, st in enumerate(plan) if st.name == name)
            st = plan[i]
            r, c = st.rows // 2, st.cols // 3
            bad = trace[i][kind].copy()
            if kind == "f32":
                bad[r, c] *= np.float32(1.00001)
            else:
                assert (int(bad[r, c]) & 0x7F) < 0x7D
                bad[r, c] += 2
            env = {}
            for j in range(i):
                for k, b in plan[j].dst.items():
                    env[b] = trace[j][k]
            v = R.check_stage(st, env, R.Weights(w, dev=True), {**trace[i], kind: bad})
            assert v.flagged == 1 and v.rows == [r], (name, v.flagged, v.rows)
    finally:
        eng.close()


@pytest.mark.parametrize("T", (40, 1100))
def test_decode_at_the_narrow_shape(T):
    shape = narrow_shape()
    eng, w = make_decoder(shape, 1104)
    try:
        check_decode(shape, eng, w, T, seed=T, title="decode, narrow shape")
    finally:
        eng.close()


def test_second_shorter_decode_still_sees_zero_padding(real_decoder):
    """Two decodes in a row on one context with different codes, the second shorter: the rows in front of every work
    buffer hold the first decode's values by then, and the second decode's first rows must read zeros there."""
    shape, eng, w = real_decoder
    eng.decode(rand_codes(shape, 64, seed=7)[None])
    check_decode(shape, eng, w, 17, seed=8, title="decode after a longer decode, real widths")


def encode_parts(shape, plan):
    """The three launch ranges of ENC_PARTS: up to the last encoder block; that block; everything after it."""
    i1 = next(i for i, st in enumerate(plan) if st.name.startswith(f"enc.{len(shape.encoder_rates) - 1}."))
    i2 = next(i for i, st in enumerate(plan) if st.name == "enc.out")
    return (0, i1), (i1, i2), (i2, len(plan))


def check_search(shape, eng, w, call, plan, title):
    """Every decision of the traced call's quantiser search, on the zq its last launch recorded."""
    assert plan[-1].name == "pre.norm" and plan[-1].dst == {"f32": "zq"}
    codes, launches = eng.trace(call, len(plan) - 1, 1)
    v = R.rvq_search_check(shape, w, launches[-1]["out"]["f32"], codes)
    print(f"  search, {title}: {v.summary()}")
    assert not v.flagged, (v.outside[:8], v.ties[:8], v.invalid[:8])
    assert v.non_argmax <= R.RVQ_NON_ARGMAX_CAP * v.decisions, (v.non_argmax, v.decisions)
    return v


def check_encode(shape, eng, w, n, seed, title, part=None):
    audio = _test_audio(n, seed=seed)
    plan = R.plan_encode(shape, audio)
    span = None if part is None else encode_parts(shape, plan)[part]
    stats = Stats()
    t0 = time.time()

    def call():
        return eng.encode(audio)
    meta, bad = traced_check(eng, call, plan, w, stats, same_codes, seed, span)
    where = "" if part is None else f", launches [{span[0]}, {span[1]}) of {len(plan)} ({ENC_PARTS[part]})"
    stats.report(f"{title}, {n} samples{where} ({time.time() - t0:.1f} s)", eng.trace_variants())
    assert not bad, bad
    if span is None or span[1] == len(plan):
        check_search(shape, eng, w, call, plan, f"{n} samples")
    print(f"  case time {time.time() - t0:.1f} s")
    return meta


@pytest.mark.parametrize("frames,cut", ((37, 11), (61, 5)))
def test_encode_at_the_encode_shape(frames, cut):
    shape = encode_shape()
    eng, _ = make_codec_with_encoder(shape)
    try:
        check_encode(shape, eng, encoder_weights(shape), frames * shape.enc_frame_len - cut, seed=frames, title="encode, encode_shape")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def real_encoder():
    shape = C.CodecShape()
    eng, _ = make_codec_with_encoder(shape, max_frames=ENC_MAX_FRAMES)
    yield shape, eng, encoder_weights(shape)
    eng.close()


@pytest.mark.parametrize("frames", [T for T in ENC_REAL_LENGTHS if T < ENC_SPLIT_FROM])
def test_encode_at_the_real_widths(real_encoder, frames):
    """Measured on an MI355X: see DESIGN.md ("Codec, per launch") for the recorded ratios per stage kind."""
    shape, eng, w = real_encoder
    check_encode(shape, eng, w, frames * shape.enc_frame_len - 9, seed=frames, title="encode, real widths")


# 129 frames exactly (no zero fill) and 128 frames and one sample (the last frame holds one sample)
ENC_LONG_CASES = [(T, T * 2048 - 9) for T in ENC_REAL_LENGTHS if T >= ENC_SPLIT_FROM] + [(129, 129 * 2048), (129, 128 * 2048 + 1)]


@pytest.mark.parametrize("part", range(3), ids=ENC_PARTS)
@pytest.mark.parametrize("frames,n", ENC_LONG_CASES, ids=[f"{T}f-{n}" for T, n in ENC_LONG_CASES])
def test_encode_at_the_real_widths_by_launch_range(real_encoder, frames, n, part):
    """The lengths at which a window binds (129 on: rows >= 512 of enc.3.tf.*.attn, rows >= 128 of pre.*.attn) and wo / w2
    of enc.3.tf leave the skinny kernel (257), one launch range per test."""
    shape, eng, w = real_encoder
    assert -(-n // shape.enc_frame_len) == frames
    check_encode(shape, eng, w, n, seed=frames, title="encode, real widths", part=part)


def test_encode_of_one_sample(real_encoder):
    shape, eng, w = real_encoder
    check_encode(shape, eng, w, 1, seed=1, title="encode of one sample, real widths")


def test_second_shorter_encode_still_sees_zero_padding_and_fill(real_encoder):
    """The encode's twin of test_second_shorter_decode_still_sees_zero_padding: after a 257-frame encode the rows in front
    of every work buffer and the tail of the audio buffer hold that call's values; the 17-frame encode must read zeros
    in front of its first rows and a zero fill behind its last sample."""
    shape, eng, w = real_encoder
    eng.encode(_test_audio(257 * shape.enc_frame_len - 9, seed=7))
    check_encode(shape, eng, w, 17 * shape.enc_frame_len - 9, seed=8, title="encode after a longer encode, real widths")


# ----------------------------------------------------------------------------------------------- the search on ties
def tie_layout(cb, layout):
    """Codebook rows planted so that every row has a bit-identical twin: "halves": rows [N/2, N) = rows [0, N/2) (at the
    real sizes a multiple of 256 apart: the same thread's stride; at 128 rows 64 apart: another wave); "pairs": row
    2k + 1 = row 2k (adjacent lanes); "blocks": row i + 64 = row i within every block of 128 (another wave of the same
    pass; a 64-row codebook has no such block and takes i + 32 within its 64: another lane of one wave)."""
    cb, N = cb.clone(), cb.shape[0]
    i = torch.arange(N)
    if layout == "halves":
        src = i % (N // 2)
    elif layout == "pairs":
        src = i - i % 2
    else:
        blk = min(128, N)
        src = i - i % blk + i % (blk // 2)
    assert N % 2 == 0 and int((src != i).sum()) == N // 2
    return cb[src]


@pytest.fixture(scope="module")
def search_weights():
    return {"real": (C.CodecShape(), encoder_weights(C.CodecShape())), "encode_shape": (encode_shape(), encoder_weights(encode_shape()))}


@pytest.mark.parametrize("layout", ("halves", "pairs", "blocks"))
@pytest.mark.parametrize("which", ("real", "encode_shape"))
def test_search_keeps_the_lowest_index_on_planted_ties(search_weights, which, layout):
    """ft_codec_rvq_encode on 40 seeded latents with EVERY codebook planted (before the load, so the normalised rows, their
    norms and the tables of twins are equal too): every decision of every frame is an exact tie; every pick must be the
    lower index of its twins and its float64 score the best one - no tolerance."""
    from fish_tts_amd.codec_engine import CodecHipEngine
    shape, base = search_weights[which]
    w = dict(base)
    for q in range(shape.n_codebooks + 1):
        k = f"{R.vq_prefix(q)}.codebook.weight"
        w[k] = tie_layout(base[k], layout)
        assert int((R.first_identical(w[k]) != torch.arange(w[k].shape[0])).sum()) == w[k].shape[0] // 2
    a = args_from_shape(shape)
    a.encoder_dim, a.encoder_rates = shape.encoder_dim, list(shape.encoder_rates)
    a.encoder_transformer_layers, a.encoder_tf_window = list(shape.encoder_tf_layers), shape.enc_tf_window
    eng = CodecHipEngine(a, device=0, max_frames=64, with_encoder=True)
    try:
        eng.load_state_dict(w)
        z = torch.randn(40, shape.latent_dim, generator=torch.Generator().manual_seed(23)).numpy()
        got = eng.rvq_encode(z)
        v = R.rvq_search_check(shape, w, z, got)
        print(f"search on ties, {which}, {layout}: {v.summary()}")
        assert not v.invalid and not v.ties, (v.invalid[:8], v.ties[:8])
        assert v.non_argmax == 0 and not v.outside, (v.non_argmax, v.outside[:8])
    finally:
        eng.close()


def test_every_gemm_instantiation_is_covered(real_decoder, real_encoder):
    """Over exactly the cases above (traced again without holding data: a decode costs milliseconds): (a) every GEMM
    stage of the real-width decode whose row count crosses a threshold of gemm() below MAX_FRAMES frames was run on both
    sides of it, and each threshold changes the instantiation of some stage; the same for the real-width encode below
    ENC_MAX_FRAMES, where each frame step of ENC_STEPS must change the instantiation of some encode stage; (b) every
    instantiation id was picked somewhere, except those listed in UNREACHABLE with the reason."""
    shape, eng, _ = real_decoder
    enc_eng = real_encoder[1]
    variants = eng.trace_variants()
    seen = {}                                         # id -> set of "case:stage"
    per_stage = {}                                    # real-width decode: stage -> {rows: id}

    def collect(tag, e, call):
        _, meta = e.trace(call, 0, 0)
        for m in meta:
            if m["variant"] >= 0:
                seen.setdefault(m["variant"], set()).add(f"{tag}:{m['name']}")
        return meta
    for T in REAL_LENGTHS:
        codes = rand_codes(shape, T, 1)
        for m in collect(f"real{T}", eng, lambda: eng.decode(codes[None])):
            if m["variant"] >= 0:
                per_stage.setdefault(m["name"], {})[m["rows"]] = m["variant"]
    for mk, frames, tag in ((tiny_codec_shape, (1, 17, 40), "tiny"), (narrow_shape, (40, 1100), "narrow")):
        s = mk()
        e, _ = make_decoder(s, max(frames) + 4)
        for T in frames:
            codes = rand_codes(s, T, 1)
            collect(f"{tag}{T}", e, lambda: e.decode(codes[None]))
        e.close()
    e, _ = make_codec_with_encoder(encode_shape(), max_frames=64)
    for n in (37 * 64 - 11, 61 * 64 - 5):
        audio = _test_audio(n)
        collect(f"enc{n}", e, lambda: e.encode(audio))
    e.close()
    enc_stage, enc_case = {}, {}                      # real-width encode: stage -> {frames: id}; frames -> ids
    for T in ENC_REAL_LENGTHS:
        audio = _test_audio(T * 2048 - 9)
        for m in collect(f"encreal{T}", enc_eng, lambda: enc_eng.encode(audio)):
            if m["variant"] >= 0:
                assert m["rows"] % T == 0, m
                enc_stage.setdefault(m["name"], {})[T] = (m["rows"], m["variant"])
                enc_case.setdefault(T, set()).add(m["variant"])
    # (a)
    for label, thr, above in THRESHOLDS:
        changed = []
        for name, by_rows in per_stage.items():
            per_frame = min(by_rows) // min(REAL_LENGTHS)
            if above(per_frame * 1) == above(per_frame * MAX_FRAMES):
                continue                               # this stage cannot cross the threshold within MAX_FRAMES frames
            lo = [r for r in by_rows if not above(r)]
            hi = [r for r in by_rows if above(r)]
            assert lo and hi, (label, name, sorted(by_rows))
            near = (max(lo), min(hi)) if above(max(by_rows)) else (min(lo), max(hi))     # the two lengths nearest the threshold
            if by_rows[near[0]] != by_rows[near[1]]:
                changed.append(f"{name} ({near[0]} rows: {variants[by_rows[near[0]]]['name']}, "
                               f"{near[1]} rows: {variants[by_rows[near[1]]]['name']})")
        print(f"threshold {label} ({thr} rows): the instantiation changes across it for {len(changed)} stages, e.g. {changed[:3]}")
        assert changed, label
    # (a), encode
    for label, thr, above in THRESHOLDS:
        for name, by_T in enc_stage.items():
            per_frame = by_T[1][0]
            if above(per_frame * 1) == above(per_frame * ENC_MAX_FRAMES):
                continue
            assert [T for T, (r, _) in by_T.items() if not above(r)] and [T for T, (r, _) in by_T.items() if above(r)], (label, name)
    for lo, hi in ENC_STEPS:
        changed = [f"{name} ({by_T[lo][0]} rows: {variants[by_T[lo][1]]['name']}, {by_T[hi][0]} rows: {variants[by_T[hi][1]]['name']})"
                   for name, by_T in enc_stage.items() if by_T[lo][1] != by_T[hi][1]]
        print(f"encode, {lo} | {hi} frames: the instantiation changes for {len(changed)} stages, e.g. {changed[:3]}")
        assert changed, (lo, hi)
    print("instantiations seen per encode case: " + "; ".join(f"{T} {sorted(ids)}" for T, ids in sorted(enc_case.items())))
    # (b)
    print("instantiations seen:")
    for i, v in enumerate(variants):
        where = sorted(seen.get(i, ()))
        print(f"  {i:2d} {v['name']:28s} {len(where):4d} launches" + (f", e.g. {where[0]}" if where else "  -- NOT REACHED: " + UNREACHABLE.get(i, "?")))
    missing = [i for i in range(len(variants)) if i not in seen]
    assert sorted(missing) == sorted(UNREACHABLE), (missing, sorted(UNREACHABLE))
