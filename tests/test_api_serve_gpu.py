"""GPU, public API: FishTTS.serve() - concurrent callers on threads join one continuous lock-step batch.  Tiny shapes, 4
slots: every result is bit-identical to the serialized calls (draws depend on seed, frame, codebook and index only; an
engine of <= 4 slots gives every row the bits of a single run).  At s1-mini widths with 8 slots (MFMA launches) the bits
depend on the schedule: the structure is checked, and the last survivor ends alone on slot 0 (the frame engine)."""
import dataclasses
import threading
import time

import numpy as np
import pytest

from tests.hip_util import args_from_shape
from tests.shapes import tiny_shape
from tests.test_api_gpu import api_codec_shape
from tests.test_codec_gpu import args_from_shape as codec_args_from_shape

pytestmark = pytest.mark.gpu


def _tiny_tts():
    import fish_tts_amd as ft
    from fish_tts_amd.tokenizer import NAMED_SPECIAL_TOKENS, ByteTokenizer
    shape = dataclasses.replace(tiny_shape(), max_seq_len=2304)
    tok = ByteTokenizer(256, NAMED_SPECIAL_TOKENS + [f"<|semantic:{i}|>" for i in range(2048)])
    return ft.FishTTS.synthetic(args_from_shape(shape), tok, codec_args=codec_args_from_shape(api_codec_shape()),
                                precision="bf16", max_new_tokens=96, max_batch=4)


def _codes(synth, text, seed, max_tokens, references, ban_eos=False):
    """Utterance.codes() of a single run (run_batch on the instance's engine), as synthesize_batch decodes them."""
    from fish_tts_amd.batch import run_batch
    with synth._gen_lock:
        _, utts = synth._batch_utterances([text], references, 0.7, 0.8, 1.1, max_tokens, 0, [seed])
        utts[0].ban_eos = ban_eos
        run_batch(synth._engine, utts)
    return utts[0].codes()


def _stream_pcm(synth, codes):
    st = synth._vocoder.stream()
    try:
        return (st.decode(codes) * 32767).astype(np.int16).tobytes()
    finally:
        st.close()


def test_concurrent_callers_get_the_serialized_results():
    import fish_tts_amd as ft
    synth = _tiny_tts()
    try:
        rng = np.random.default_rng(0)
        ref = np.concatenate([rng.integers(0, 2048, (1, 40)), rng.integers(0, 1024, (9, 40))]).astype(np.int32)
        voice = [ft.VoiceProfile(codes=ref, text="the reference text", name="v")]
        # (kind, text, seed, max_tokens, references)
        plan = [("wav", "Hi there", 3, 24, None), ("seam", "Yo", 1, 30, None), ("plain", "A third, longer sentence.", 0, 28, None),
                ("wav", "Four", 5, 12, voice), ("seam", "Five is here too", 9, 40, voice), ("wav", "Six.", 0, 20, None),
                ("drop", "Seven", 2, 90, None), ("plain", "Eight and more", 0, 16, voice), ("wav", "Nine", 4, 33, None)]
        want = {}
        for i, (kind, text, seed, mt, refs) in enumerate(plan):
            if kind == "wav":
                w = synth.synthesize_batch([text], references=refs, seeds=[seed], max_tokens=mt)[0]
                if seed == 0:
                    assert w == synth.synthesize(text, references=refs, max_tokens=mt)
                want[i] = w
            elif kind == "seam":
                want[i] = _stream_pcm(synth, _codes(synth, text, seed, mt, refs))
            elif kind == "plain":
                want[i] = list(synth.synthesize_stream(text, references=refs, chunk_tokens=5, min_first_chunk=3, max_tokens=mt))
        # a request that is sure to outlive a shorter one admitted before it (fixed lengths): the first hole, a move
        short_codes = _codes(synth, "short one", 7, 12, None, ban_eos=True)
        long_codes = _codes(synth, "the long one", 8, 48, None, ban_eos=True)
        got, errors = {}, []
        with synth.serve(burst=4) as srv:
            with pytest.raises(RuntimeError, match="BatchServer is open"):
                synth.synthesize_batch(["x"])
            u_short, n_short = synth._serve_prepare("short one", None, 0.7, 0.8, 1.1, 12, 7)
            u_long, n_long = synth._serve_prepare("the long one", None, 0.7, 0.8, 1.1, 48, 8)
            u_short.ban_eos = u_long.ban_eos = True
            r_short = srv.submit(u_short, n_short)
            r_long = srv.submit(u_long, n_long, stream=True, seamless=True, chunk_tokens=8, min_first_chunk=4)
            # a stream whose consumer goes away after its first chunk (fixed length: it cannot end before)
            u_drop, n_drop = synth._serve_prepare("dropped", None, 0.7, 0.8, 1.1, 90, 6)
            u_drop.ban_eos = True
            gen = srv._chunks(srv.submit(u_drop, n_drop, stream=True, chunk_tokens=2, min_first_chunk=2))
            assert next(gen)
            gen.close()
            assert r_short.out.get(timeout=60) == synth._decode_to_wav(short_codes)
            long_chunks, long_done = [], threading.Event()

            def drain():
                while True:
                    it = r_long.out.get(timeout=60)
                    if it is srv_end():
                        break
                    long_chunks.append(it)
                long_done.set()
            threading.Thread(target=drain, daemon=True).start()

            def call(i, kind, text, seed, mt, refs):
                time.sleep(0.03 + 0.004 * i)          # after the short request has left its slot
                try:
                    if kind == "wav":
                        got[i] = srv.synthesize(text, references=refs, max_tokens=mt, seed=seed) if seed else \
                            synth.synthesize(text, references=refs, max_tokens=mt)        # routed through the server
                    elif kind == "drop":
                        gen = srv.synthesize_stream(text, chunk_tokens=2, min_first_chunk=2, max_tokens=mt, seed=seed)
                        next(gen)
                        gen.close()
                    else:
                        got[i] = list(srv.synthesize_stream(text, references=refs, chunk_tokens=5, min_first_chunk=3,
                                                            seamless=kind == "seam", max_tokens=mt, seed=seed))
                except BaseException as e:  # noqa: BLE001
                    errors.append(e)
            threads = [threading.Thread(target=call, args=(i,) + p) for i, p in enumerate(plan)]
            for t in threads:
                t.start()
            for t in threads:
                t.join(120)
                assert not t.is_alive()
            assert long_done.wait(120)
            stats = srv.stats()
        assert not errors, errors
        assert synth._server is None and not synth._gen_lock.locked()
        assert stats["slot_moves"] >= 1 and stats["cancelled"] >= 1, stats
        assert stats["admitted"] == len(plan) + 3
        assert b"".join(long_chunks) == _stream_pcm(synth, long_codes)
        assert short_codes.shape[1] == 11
        for i, (kind, text, seed, mt, refs) in enumerate(plan):
            if kind == "seam":
                assert b"".join(got[i]) == want[i], i
            elif kind in ("wav", "plain"):
                assert got[i] == want[i], i
        # the instance serves its calls itself again
        assert synth.synthesize_batch(["Hi there"], seeds=[3], max_tokens=24)[0] == want[0]
        assert list(synth.synthesize_stream("A third, longer sentence.", chunk_tokens=5, min_first_chunk=3, max_tokens=28)) == want[2]
    finally:
        if synth._server is not None:
            synth._server.close(cancel=True)
        synth._engine.close()
        synth._vocoder.close()


def srv_end():
    from fish_tts_amd import serve
    return serve._END


def test_server_at_s1_widths_ends_on_the_frame_engine():
    """medium_shape(n_text=1009), 8 slots, bf16: lock-step steps on the MFMA launches beside the codec worker; every request
    completes with valid codes and the longest one ends alone on slot 0 (steps of width 1: the frame engine), with no
    hand-off time-out."""
    import fish_tts_amd as ft
    from fish_tts_amd.tokenizer import NAMED_SPECIAL_TOKENS, ByteTokenizer
    from tests.test_ar_gpu import medium_shape
    shape = medium_shape(n_text=1009)
    tok = ByteTokenizer(1009, NAMED_SPECIAL_TOKENS + [f"<|semantic:{i}|>" for i in range(4096)])
    assert tok.semantic_begin_id == shape.semantic_begin_id and tok.get_token_id("<|im_end|>") == shape.im_end_id
    cshape = dataclasses.replace(api_codec_shape(), semantic_codebook_size=4096)
    synth = ft.FishTTS.synthetic(dataclasses.replace(args_from_shape(shape), max_seq_len=2304), tok,
                                 codec_args=codec_args_from_shape(cshape), precision="bf16", max_new_tokens=64, max_batch=8)
    try:
        assert "MFMA launches" in synth._engine.frame_path() and synth._engine.engine_state()[0] == 3
        reqs = []
        with synth.serve(burst=4) as srv:
            for i in range(10):
                utt, n_prefix = synth._serve_prepare(f"request number {i}", None, 0.7, 0.8, 1.1, 48 if i == 3 else 6 + 2 * i, i)
                utt.ban_eos = True
                reqs.append(srv.submit(utt, n_prefix, stream=i % 2 == 1, seamless=i % 4 == 1, chunk_tokens=6,
                                       min_first_chunk=3))
                time.sleep(0.003)
            outs = []
            for r in reqs:
                items = []
                while True:
                    it = r.out.get(timeout=120)
                    if it is srv_end() or isinstance(it, bytes) and r.mode == "wav":
                        items.append(it)
                        break
                    assert isinstance(it, bytes), it
                    items.append(it)
                outs.append(items)
            stats = srv.stats()
        assert stats["completed"] == 10 and stats["admitted"] == 10
        sw = stats["steps_by_width"]
        assert sw.get(1, 0) > 0 and max(sw) >= 5, sw
        assert all(w == 1 or w >= 5 for w in sw), sw                 # 2..4 rows ride five wide
        for i, r in enumerate(reqs):
            cols = r.utt.columns()
            assert cols.shape[1] == (48 if i == 3 else 6 + 2 * i)
            assert (cols[0] != shape.im_end_id).all()                 # ban_eos: every request runs its budget
            assert ((cols[1] >= 0) & (cols[1] < 4096)).all() and ((cols[2:] >= 0) & (cols[2:] < 1024)).all()
            assert all(len(p) > 0 for p in outs[i][:-1] if isinstance(p, bytes))
        flags, aborted, _ = synth._engine.engine_state()
        assert flags == 3 and aborted == 0
        assert not synth._gen_lock.locked()
    finally:
        if synth._server is not None:
            synth._server.close(cancel=True)
        synth._engine.close()
        synth._vocoder.close()
