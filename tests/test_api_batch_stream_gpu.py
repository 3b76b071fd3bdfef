"""GPU, public API: FishTTS.synthesize_batch_stream with tiny synthetic models - each utterance's PCM is one stateful
streamed decode of the codes synthesize_batch's helper and run_batch give for the same seeds; chunk lengths; the object
serves synthesize_batch as before after an early break."""
import dataclasses

import numpy as np
import pytest

from tests.hip_util import args_from_shape
from tests.shapes import tiny_shape
from tests.test_api_gpu import api_codec_shape
from tests.test_codec_gpu import args_from_shape as codec_args_from_shape

pytestmark = pytest.mark.gpu


def _expected(synth, texts, kw, seeds, references=None):
    from fish_tts_amd.batch import run_batch, run_batch_streams
    with synth._gen_lock:
        engines, utts = synth._batch_utterances(texts, references, kw["temperature"], kw["top_p"], kw["repetition_penalty"],
                                                kw["max_tokens"], 0, seeds)
        if len(engines) > 1:
            run_batch_streams(engines, utts)
        else:
            run_batch(synth._engine, utts)
    out = []
    for u in utts:
        codes = u.codes()
        if codes.shape[1] == 0:
            out.append(b"")
            continue
        st = synth._vocoder.stream()
        out.append((st.decode(codes) * 32767).astype(np.int16).tobytes())
        st.close()
    return out, [u.codes().shape[1] for u in utts]


def _check(synth, texts, kw, seeds, references=None, chunk_tokens=6, min_first_chunk=3):
    want, n = _expected(synth, texts, kw, seeds, references)
    got = {i: [] for i in range(len(texts))}
    for i, pcm in synth.synthesize_batch_stream(texts, references=references, chunk_tokens=chunk_tokens,
                                                min_first_chunk=min_first_chunk, seeds=seeds, **kw):
        got[i].append(pcm)
    fl = synth._vocoder.frame_len
    for i in range(len(texts)):
        assert got[i][-1] == b"" and got[i].count(b"") == 1
        lens = [len(p) // 2 // fl for p in got[i][:-1]]
        cuts = [min_first_chunk] if n[i] >= min_first_chunk else []
        while n[i] - sum(cuts) >= chunk_tokens:
            cuts.append(chunk_tokens)
        if n[i] - sum(cuts):
            cuts.append(n[i] - sum(cuts))
        assert lens == cuts, (i, lens, n[i])
        assert b"".join(got[i][:-1]) == want[i], i
    assert sum(n) > 0


def test_batch_stream_equals_streamed_decodes_and_leaves_the_object_usable():
    import fish_tts_amd as ft
    from fish_tts_amd.tokenizer import NAMED_SPECIAL_TOKENS, ByteTokenizer
    shape = dataclasses.replace(tiny_shape(), max_seq_len=2304)
    tok = ByteTokenizer(256, NAMED_SPECIAL_TOKENS + [f"<|semantic:{i}|>" for i in range(2048)])
    kw = dict(temperature=0.7, top_p=0.8, repetition_penalty=1.1, max_tokens=24)
    texts = ["Hi there", "Yo", "A third, longer sentence.", "Four", "Five is here too", "Six."]
    seeds = [3, 1, 4, 1, 5, 9]
    # one lock-step batch of 4 slots
    synth = ft.FishTTS.synthetic(args_from_shape(shape), tok, codec_args=codec_args_from_shape(api_codec_shape()),
                                 precision="bf16", max_new_tokens=96, max_batch=4)
    _check(synth, texts, kw, seeds)
    # an early break: the generation stops, the lock is released, synthesize_batch equals synthesize
    gen = synth.synthesize_batch_stream(texts, seeds=seeds, chunk_tokens=2, min_first_chunk=1, **kw)
    next(gen)
    gen.close()
    assert not synth._gen_lock.locked()
    short = dict(kw, max_tokens=10, top_p=1e-6)
    assert synth.synthesize_batch(texts[:3], seeds=[0] * 3, **short) == [synth.synthesize(t, **short) for t in texts[:3]]
    synth._engine.close()
    synth._vocoder.close()
    # two lock-step batches of 2 side by side, with a cloned voice
    synth = ft.FishTTS.synthetic(args_from_shape(shape), tok, codec_args=codec_args_from_shape(api_codec_shape()),
                                 precision="bf16", max_new_tokens=96, max_batch=2, batch_streams=2)
    rng = np.random.default_rng(0)
    ref = np.concatenate([rng.integers(0, 2048, (1, 40)), rng.integers(0, 1024, (9, 40))]).astype(np.int32)
    prof = ft.VoiceProfile(codes=ref, text="the reference text", name="v")
    _check(synth, texts[:5], kw, seeds[:5], references=[prof], chunk_tokens=5, min_first_chunk=2)
    assert len(synth._more_engines) == 1
    for e in synth._more_engines:
        e.close()
    synth._engine.close()
    synth._vocoder.close()
