"""Every launch of a STREAMED codec decode (ft_codec_stream_decode, ft_codec_stream_decode_many), element by element,
against the float64 stage reference, and every carrying launch bit for bit.

The launch trace (include/fishtts_hip_test.h) also arms the streamed entry points: per launch what it wrote, the rows of a
batched call dense (gap rows left out), and per carrying launch (tail_roll_kernel, kv_carry_in_kernel,
kv_carry_out_kernel) and chunk the rows placed in front of the chunk and the whole carry left.  tests/codec_stage_ref.py
(`plan_stream`) restates one chunk: the arithmetic launches in their carried-context form (rows before 0 from the
recorded front rows, rope at t0, nh carried keys in front) under the bounds of the one-shot check, unchanged,
    |got - ref| <= half a ulp of the stored format at max(|got|, |ref|) + err,
and the carrying launches as copies of recorded bit patterns, accepted bit for bit, the unwritten head of a K/V carry
included.  The allowed number of flagged or excluded elements is zero.  Across chunks the test keeps the state: the rows
a chunk's roll / kv-in puts in front must be the carry the previous traced chunk was recorded to leave (zeros before
the first chunk); a chunk traced behind untraced chunks is judged on its own recorded front rows, and
test_a_chunk_traced_behind_untraced_chunks_records_what_the_fully_traced_stream_records closes that link.  Every traced
call runs beside an untraced twin stream: the samples are equal bit for bit, also after a traced chunk.

A case is a script of calls on one context (SCRIPTS): untraced chunks advance the streams, short traced chunks are
checked.  Every GEMM of a traced streamed call must report the instantiation the same stage takes in a traced one-shot
decode of 215 frames on the same context, and test_instantiations_by_row_count asserts which (instantiation, M < BM /
M % BM != 0 / M > nominal rows) combinations the scripts reach."""
import time

import numpy as np
import pytest

from oracle import codec as C
from tests import codec_stage_ref as R
from tests.golden.make_golden_codec import tiny_codec_shape
from tests.test_codec_stages_gpu import Stats, make_decoder, narrow_shape, rand_codes, same_audio

pytestmark = pytest.mark.gpu
ALL = 1 << 30
NOMINAL = 215                  # frames the streamed decode picks its GEMM instantiations for (STREAM_NOMINAL_FRAMES)
COMPACT = (".wo", ".w13", ".w2")   # GEMMs that run once over the compact rows of ALL chunks of a batched call

# A script: (streams, [(mode, traced, [(stream, frames), ...]), ...]); mode "one": CodecStream.decode, "many": decode_streams
# in the order given.
ONE, MANY = "one", "many"
REAL_MAX, TINY_MAX, NARROW_MAX = 320, 1536, 256      # max_frames of the three contexts


def single(*steps):
    """One stream: ("u", T) an untraced chunk, ("t", T) a traced one."""
    return 1, [(ONE, k == "t", [(0, T)]) for k, T in steps]


def batched(t0s, order, lens, cap):
    """Streams advanced untraced to t0s (batched calls of at most `cap` frames), then ONE traced batched call over streams
    `order` with chunk lengths `lens`."""
    pre = []
    for sid, t in enumerate(t0s):
        if t > 0 and pre and sum(T for _, T in pre[-1][2]) + t <= cap:
            pre[-1][2].append((sid, t))
        elif t > 0:
            pre.append((MANY, False, [(sid, t)]))
    return len(t0s), pre + [(MANY, True, list(zip(order, lens)))]


SCRIPTS = {
    # real widths (window 128; halos 6 at 2 and 4 rows per frame, up to 54 at 32 rows per frame and above)
    "real-t0=0": ("real", single(("t", 1), ("t", 1), ("t", 2), ("t", 5))),
    "real-t0=126,127,128": ("real", single(("u", 126), ("t", 1), ("t", 1), ("t", 2))),
    "real-t0=214": ("real", single(("u", 214), ("t", 1), ("t", 3))),
    "real-last-rope-row": ("real", single(("u", REAL_MAX - 4), ("t", 4))),
    "real-17": ("real", single(("u", 40), ("t", 17))),
    "real-many-3": ("real", batched([0, 127, 300], [1, 2, 0], [1, 3, 2], REAL_MAX)),
    "real-many-1": ("real", batched([10], [0], [3], REAL_MAX)),
    "real-many-5": ("real", batched([0, 5, 130, 0, 64], [0, 1, 2, 3, 4], [1, 2, 9, 1, 4], REAL_MAX)),
    # tiny shape (window 8)
    "tiny-chunks": ("tiny", single(*[("t", T) for T in (1, 1, 1, 3, 7, 1, 20, 9)])),
    "tiny-260": ("tiny", single(("u", 3), ("t", 260))),
    "tiny-many-64": ("tiny", batched([(7 * j) % 41 for j in range(64)], list(range(64)), [9 if j == 37 else 1 for j in range(64)], TINY_MAX)),
    # 96-wide latent: the BK = 32 tiles
    "narrow-chunks": ("narrow", single(("t", 1), ("t", 5), ("t", 40))),
}
SHAPES = {"real": (C.CodecShape, REAL_MAX), "tiny": (tiny_codec_shape, TINY_MAX), "narrow": (narrow_shape, NARROW_MAX)}
TOTAL = Stats()
TIMES = {}


@pytest.fixture(scope="module")
def decoders():
    """One context per shape, made on first use."""
    made = {}

    def get(key):
        if key not in made:
            mk, mf = SHAPES[key]
            shape = mk()
            eng, w = make_decoder(shape, mf)
            made[key] = (shape, eng, w)
        return made[key]
    yield get
    for _, eng, _ in made.values():
        eng.close()


def nominal_variants(eng, shape):
    """stage -> instantiation id of a traced one-shot decode of NOMINAL frames on this context (nothing held)."""
    if not hasattr(eng, "_nominal_variants"):
        codes = rand_codes(shape, NOMINAL, 1)
        _, meta = eng.trace(lambda: eng.decode(codes[None]), 0, 0)
        eng._nominal_variants = {m["name"]: m["variant"] for m in meta if m["variant"] >= 0}
    return eng._nominal_variants


def split_chunks(launches, table):
    """The records of a traced streamed call, per chunk: an arithmetic launch's dense rows cut at the chunk borders, a
    carrying record to its chunk.  "M": the rows the launch itself ran over (all chunks' for the compact GEMMs)."""
    frames = sum(c["L"] for c in table)
    per = [[] for _ in table]
    for rec in launches:
        if "chunk" in rec:
            per[rec["chunk"]].append(rec)
            continue
        assert rec["rows"] % frames == 0, (rec["name"], rec["rows"], frames)
        m = rec["rows"] // frames
        for z, c in enumerate(table):
            lo, hi = c["P"] * m, (c["P"] + c["L"]) * m
            per[z].append(dict(rec, rows=hi - lo, M=rec["rows"] if rec["name"].endswith(COMPACT) else hi - lo,
                               out={k: a[lo:hi] for k, a in rec["out"].items()}))
    return per


def note_variant(rec, st, L, eng, shape, reach):
    """The instantiation is the nominal utterance's; which row-count classes this launch puts it in."""
    want = nominal_variants(eng, shape)[st.name]
    assert rec["variant"] == want, (st.name, rec["variant"], want)
    assert (rec["ntap"], rec["K"]) == (len(st.p["offs"]), st.p["K"]), rec
    bm, M, m = eng.trace_variants()[want]["bm"], rec["M"], st.rows // L
    for cls, hit in (("M < BM", M < bm), ("M % BM != 0", M % bm != 0), ("M > nominal rows", M > NOMINAL * m)):
        if hit:
            reach.add((want, cls))


def check_chunk(recs, plan, L, W, before, eng, shape, stats, reach, seed):
    """One chunk of a traced call against its plan; `before`: the carries recorded for the chunk before it (None: not
    traced).  Returns (the carries it was recorded to leave, flagged launches)."""
    assert [r["name"] for r in recs] == [st.name for st in plan], \
        [(r["name"], st.name) for r, st in zip(recs, plan) if r["name"] != st.name][:5]
    env = R.seed_unlinked(plan, [r["out"] for r in recs]) if before is None else dict(before)
    variants, bad = eng.trace_variants(), []
    for st, rec in zip(plan, recs):
        assert (rec["rows"], rec["cols"], sorted(rec["kinds"]), rec["halo"]) == (st.rows, st.cols, sorted(st.dst), st.halo), (rec["name"], rec["rows"], rec["cols"])
        assert set(rec["out"]) == set(st.dst), (st.name, sorted(rec["out"]))
        if st.kind == "gemm":
            note_variant(rec, st, L, eng, shape, reach)
        else:
            assert rec["variant"] == -1, rec["name"]
        bm = variants[rec["variant"]]["bm"] if st.kind == "gemm" else 256
        v = R.check_stage(st, env, W, rec["out"], R.select_rows(st.rows, st.halo, bm, seed))
        for s_ in (stats, TOTAL):
            s_.add(v, rec)
            if st.kind == "gemm":
                s_.variants[rec["variant"]] = s_.variants.get(rec["variant"], 0) + 1
        if v.flagged:
            bad.append((v.name, variants[rec["variant"]]["name"] if st.kind == "gemm" else st.kind, v.flagged, v.checked,
                        round(v.worst, 3), v.rows[:12]))
        for k, b in st.dst.items():
            env[b] = rec["out"][k]
    return R.carries(env), bad


def run_script(eng, shape, w, script, seed, check=True, stats=None, reach=None, only=None):
    """The calls of a script on fresh streams.  check: every traced call holds what it wrote and is checked, beside an
    untraced twin of every stream; else the traced calls hold nothing (names, instantiations and row classes only).
    only = (step, chunk or None): the script up to that step, and only that traced call (that chunk of it) is checked;
    the traced calls before it are held for the carries they were recorded to leave."""
    n, steps = script
    if only is not None:
        steps = steps[:only[0] + 1]
    W1 = shape.tf_window - 1
    total = [sum(T for _, _, parts in steps for sid, T in parts if sid == j) for j in range(n)]
    codes = [rand_codes(shape, total[j], seed + j) for j in range(n)]
    traced = [eng.stream() for _ in range(n)]
    plain = [eng.stream() for _ in range(n)] if check else None
    W = R.Weights(w, dev=True)
    pos, car, bad = [0] * n, [{} for _ in range(n)], []
    reach = set() if reach is None else reach
    try:
        for mode, tr, parts in steps:
            chunks = [codes[sid][:, pos[sid]:pos[sid] + T] for sid, T in parts]

            def call(ss):
                if mode == ONE:
                    return [ss[parts[0][0]].decode(chunks[0])]
                return eng.decode_streams([ss[sid] for sid, _ in parts], chunks)
            base = call(plain) if check else None
            if not tr:
                got = call(traced)
                for sid, _ in parts:
                    car[sid] = None
            else:
                got, launches = eng.trace(lambda: call(traced), 0, ALL if check else 0)
                table = eng.trace_chunks()
                P = np.cumsum([0] + [T for _, T in parts]).tolist()
                assert table == [dict(P=P[z], L=T, t0=pos[sid], nh=min(pos[sid], W1)) for z, (sid, T) in enumerate(parts)], table
                for z, ((sid, T), recs) in enumerate(zip(parts, split_chunks(launches, table))):
                    plan = R.plan_stream(shape, chunks[z], pos[sid], min(pos[sid], W1))
                    if check and only is not None and (steps[only[0]][2] is not parts or only[1] not in (None, z)):
                        assert [r["name"] for r in recs] == [st.name for st in plan]
                        car[sid] = {st.dst["carry"]: rec["out"]["carry"] for st, rec in zip(plan, recs) if "carry" in st.dst}
                    elif check:
                        car[sid], b = check_chunk(recs, plan, T, W, car[sid], eng, shape, stats, reach, seed + z)
                        bad += [(f"chunk {z} (stream {sid}, t0 {pos[sid]}, {T} frames)",) + x for x in b]
                    else:
                        assert [r["name"] for r in recs] == [st.name for st in plan]
                        for st, rec in zip(plan, recs):
                            if st.kind == "gemm":
                                note_variant(rec, st, T, eng, shape, reach)
            if check:
                assert len(got) == len(base) and all(same_audio(a, b) for a, b in zip(got, base)), \
                    f"the samples of {'a traced' if tr else 'an untraced'} call differ from the untraced twin's ({mode} {parts})"
            for sid, T in parts:
                pos[sid] += T
    finally:
        for st in traced + (plain or []):
            st.close()
    return bad, reach


def cases():
    """The small shapes: a script is one case.  The real widths, where the float64 reference of one chunk costs a second
    or more: one case per traced call, and per chunk of a batched call (the script runs again up to that call)."""
    out = []
    for name in sorted(SCRIPTS):
        key, (_, steps) = SCRIPTS[name]
        if key != "real":
            out.append(pytest.param(name, None, id=name))
            continue
        for si, (mode, tr, parts) in enumerate(steps):
            for z in (range(len(parts)) if len(parts) > 1 else (None,)) if tr else ():
                out.append(pytest.param(name, (si, z), id=f"{name}-call{si}" + ("" if z is None else f"-chunk{z}")))
    return out


@pytest.mark.parametrize("case,only", cases())
def test_streamed_launches(decoders, case, only):
    """Measured on an MI355X ("Codec, per streamed launch"): 0 flagged, 0 excluded, every carrying record
    bit-exact; largest |got - ref| / bound 1.000 (GEMMs, RMSNorm, RoPE: values on a rounding boundary), attention 0.996."""
    key, script = SCRIPTS[case]
    shape, eng, w = decoders(key)
    stats = Stats()
    t0 = time.time()
    bad, reach = run_script(eng, shape, w, script, seed=1000 + sorted(SCRIPTS).index(case), stats=stats, only=only)
    label = case if only is None else f"{case} call {only[0]}" + ("" if only[1] is None else f" chunk {only[1]}")
    TIMES[label] = time.time() - t0
    stats.report(f"streamed decode, {label} ({TIMES[label]:.1f} s)", eng.trace_variants())
    assert stats.launches and not bad, bad


def test_a_chunk_traced_behind_untraced_chunks_records_what_the_fully_traced_stream_records(decoders):
    """The link the per-chunk check cannot see when untraced chunks lie between two traced ones: the last chunk of a
    stream records the same bytes, carrying launches included, whether the chunks before it were traced or not."""
    for key, chunks in (("tiny", (1, 1, 1, 3, 7, 1, 20, 9)), ("real", (5, 1, 3))):
        shape, eng, _ = decoders(key)
        codes = rand_codes(shape, sum(chunks), 77)
        last = []
        for traced_before in (True, False):
            st, t = eng.stream(), 0
            try:
                for i, T in enumerate(chunks):
                    c = codes[:, t:t + T]
                    if traced_before or i + 1 == len(chunks):
                        audio, launches = eng.trace(lambda: st.decode(c), 0, ALL)
                    else:
                        audio = st.decode(c)
                    t += T
            finally:
                st.close()
            last.append((audio, launches))
        (a0, l0), (a1, l1) = last
        assert same_audio(a0, a1) and [r["name"] for r in l0] == [r["name"] for r in l1]
        assert any(r["name"].endswith(".kvin") for r in l0) and any(r["name"].endswith(".roll") for r in l0)
        for r0, r1 in zip(l0, l1):
            assert sorted(r0["out"]) == sorted(r1["out"]) and all(np.array_equal(r0["out"][k], r1["out"][k]) for k in r0["out"]), \
                (key, r0["name"])


def test_an_armed_trace_is_dropped_by_the_resampled_stream_entry_point(decoders):
    """ft_codec_stream_decode_many_at stays untraced and disarms: the streamed decode after it records nothing new."""
    shape, eng, _ = decoders("tiny")
    codes = rand_codes(shape, 6, 5)
    a, b = eng.stream(sample_rate=24000), eng.stream()
    try:
        _, launches = eng.trace(lambda: a.decode(codes[:, :3]), 0, 0)
        assert launches == []
        b.decode(codes[:, :3])
        assert eng.lib.ft_test_codec_trace_count(eng._h) == 0
    finally:
        a.close()
        b.close()


# Classes of a launch of M rows on an instantiation of row tile BM at a stage of m rows per frame: M < BM, M % BM != 0,
# M > NOMINAL m.  The instantiations a nominal utterance picks over the three shapes are ids 0 .. 9; the scripts reach every
# (id, class) but these, each with the reason:
CLASSES = ("M < BM", "M % BM != 0", "M > nominal rows")
_WIDE = ("picked at the real widths only, from 30000 nominal rows on, that is at the stages of 256, 1024 and 2048 rows per frame: "
         "every chunk is a whole number of its row tiles there")
_LONG = "would take a traced chunk of more than 215 frames at the {}: the float64 reference of one costs minutes"
UNREACHED = {
    (2, "M > nominal rows"): "tapgemm64<64,64,32> is picked at the narrow shape only, whose script traces at most 40 frames",
    (4, "M > nominal rows"): "tapgemm64<64,96,32>: as id 2",
    (7, "M < BM"): "tapgemm64<128,192,32,2,4>: " + _WIDE,
    (7, "M % BM != 0"): "as (7, M < BM)",
    (7, "M > nominal rows"): _LONG.format("real widths"),
    (8, "M < BM"): "tapgemm64<256,96,32,4,2>: " + _WIDE + " (2048 rows per frame)",
    (8, "M % BM != 0"): "as (8, M < BM)",
    (8, "M > nominal rows"): _LONG.format("real widths"),
    (9, "M > nominal rows"): "tapgemm64<128,128,64,2,4>: " + _LONG.format("real widths, the only shape that picks it"),
}
REACHED = {(i, c) for i in range(10) for c in CLASSES} - set(UNREACHED)


def test_instantiations_by_row_count(decoders):
    """Over exactly the scripts above, traced again without holding data: every GEMM of every traced streamed call runs
    the instantiation of the nominal utterance (asserted per launch), at row counts in these classes."""
    reach = set()
    for case in sorted(SCRIPTS):
        key, script = SCRIPTS[case]
        shape, eng, w = decoders(key)
        run_script(eng, shape, w, script, seed=1, check=False, reach=reach)
    names = {v["id"]: v["name"] for v in decoders("real")[1].trace_variants()}
    nominal = sorted({i for key in SHAPES for i in nominal_variants(decoders(key)[1], decoders(key)[0]).values()})
    classes = CLASSES
    print("instantiation x row-count class reached by the streamed scripts:")
    for i in nominal:
        print(f"  {i:2d} {names[i]:28s} " + "  ".join(f"{c}: {'yes' if (i, c) in reach else 'NO '}" for c in classes))
    if TOTAL.launches:
        TOTAL.report("all streamed cases of this run", decoders("real")[1].trace_variants())
        print("  seconds per case: " + ", ".join(f"{k} {v:.1f}" for k, v in sorted(TIMES.items(), key=lambda kv: -kv[1])))
    missing = {(i, c) for i in nominal for c in classes} - reach
    for k in sorted(missing):
        print(f"  not reached: {k}: {UNREACHED.get(k, '?')}")
    assert nominal == list(range(10)), nominal
    assert reach == REACHED, (sorted(reach - REACHED), sorted(REACHED - reach))
    assert missing == set(UNREACHED), (sorted(missing), sorted(UNREACHED))
