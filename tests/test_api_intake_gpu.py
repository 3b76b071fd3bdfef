"""GPU, public API: FishTTS.encode_reference_at / encode_references / prepare_reference - any WAV to a voice profile, prepared
on the GPU (include/fishtts_hip.h: "Reference intake").  The anchor: a 16-bit mono 44.1 kHz file with nothing trimmed and no
level is encode_reference, bit for bit."""
import dataclasses
import io
import threading
import wave

import numpy as np
import pytest

from tests import intake_ref as R
from tests.hip_util import args_from_shape
from tests.shapes import tiny_shape
from tests.test_codec_gpu import args_from_shape as codec_args_from_shape
from tests.test_codec_gpu import encode_shape, make_codec_with_encoder
from tests.test_intake_gpu import FO, bits, pcm16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth():
    """The API over the tiny encoder alone (as tests/test_codec_gpu.py::test_encode_reference_api builds it)."""
    import fish_tts_amd as ft
    eng, _ = make_codec_with_encoder(encode_shape(), max_frames=1024)
    s = ft.FishTTS.__new__(ft.FishTTS)
    s._vocoder = eng
    s._server = None
    yield s
    eng.close()


def wav16(rate, pcm):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(rate)
        wf.writeframes(np.asarray(pcm, dtype=np.int16).tobytes())
    return buf.getvalue()


def test_anchor_is_encode_reference(synth):
    import fish_tts_amd as ft
    from fish_tts_amd.codec_engine import IntakeReport
    pcm = pcm16(30 * 64 + 5).astype(np.int16)
    b = wav16(FO, pcm)
    old = synth.encode_reference(b, "hello")
    rep = []
    new = synth.encode_reference_at(b, "hello", silence_db=None, loudness=None, report=rep)
    assert isinstance(new, ft.VoiceProfile) and new.text == "hello" and new.codes.dtype == np.int64
    assert new.codes.shape == old.codes.shape == (4, 31) and np.array_equal(new.codes, old.codes)
    assert isinstance(rep[0], IntakeReport) and rep[0].status == 0 and rep[0].cut == (0, len(pcm)) and rep[0].level.gain == 1.0
    audio, r = synth.prepare_reference(b, silence_db=None)
    assert audio.dtype == np.float32 and np.array_equal(bits(audio), bits(pcm.astype(np.float32) / 32768.0)) and r == rep[0]
    # the defaults trim: a clip with silence around it gives fewer frames, and what was kept is what is encoded
    padded = np.concatenate([np.zeros(9000, np.int16), pcm, np.zeros(9000, np.int16)])
    kept, r2 = synth.prepare_reference(wav16(FO, padded))
    prof = synth.encode_reference_at(wav16(FO, padded), "hello")
    assert 0 < r2.cut[0] < r2.cut[1] < len(padded) and prof.codes.shape[1] == r2.frames == -(-len(kept) // 64) < -(-len(padded) // 64)
    assert np.array_equal(prof.codes, synth._vocoder.encode(kept))
    # a level: the kept piece sits at the target
    lev, r3 = synth.prepare_reference(wav16(FO, padded), loudness=-30.0)
    after, _ = synth._vocoder.loudness(np.concatenate([np.zeros(r3.cut[0], np.float32), lev, np.zeros(len(padded) - r3.cut[1], np.float32)]))
    assert r3.level.gain < 1.0 and abs(after.lufs - (-30.0)) <= 0.05


def test_refusals_before_and_after_the_call(synth):
    pcm = pcm16(4000).astype(np.int16)
    good = wav16(FO, pcm)
    for bad, match in ((b"RIFX" + good[4:], "clip 0: not a RIFF/WAVE"), (wav16(44099, pcm), "clip 0: unsupported input sample rate 44099"),
                       (good[:40], "clip 0")):
        with pytest.raises(ValueError, match=match):
            synth.encode_reference_at(bad, "x")
        with pytest.raises(ValueError, match=match):
            synth.prepare_reference(bad)
    with pytest.raises(ValueError, match="clip 1: unsupported input sample rate 7999"):
        synth.encode_references([(good, "a"), (wav16(7999, pcm), "b")])
    for kw in (dict(silence_db=1.0), dict(silence_db=-91.0), dict(silence_db="x"), dict(loudness=-4.0), dict(loudness=-51.0),
               dict(channel=1), dict(channel=-1), dict(channel=1.0)):
        with pytest.raises(ValueError):
            synth.encode_reference_at(good, "x", **kw)
    # after the call: a clip with nothing above silence_db, and one longer than the encoder takes - by index
    quiet = wav16(FO, np.random.default_rng(0).integers(-30, 31, 5000))
    long_ = wav16(22050, pcm16(33000, 3))                      # 66 000 samples at 44.1 kHz; the encoder takes 1024 x 64
    reps = []
    with pytest.raises(ValueError, match="clip 1: nothing in it is louder"):
        synth.encode_references([(good, "a"), (quiet, "b")], reports=reps)
    assert [r.status for r in reps] == [0, 1]
    with pytest.raises(ValueError, match=r"clip 2: 1\.50 s are kept, the encoder takes 1\.49 s \(max_reference_seconds = 60\)"):
        synth.encode_references([(good, "a"), (good, "b"), (long_, "c")], silence_db=None)
    audio, r = synth.prepare_reference(long_)                  # nothing is refused here: the report tells
    assert r.status == 2 and r.frames == 0 and len(audio) == r.kept
    assert synth.encode_references([]) == []
    synth2 = type(synth).__new__(type(synth))
    synth2._vocoder = None
    with pytest.raises(RuntimeError, match="Vocoder not loaded"):
        synth2.encode_reference_at(good, "x")


def test_seventy_clips_equal_seventy_single_calls(synth):
    rng = np.random.default_rng(4)
    clips = []
    for i in range(70):
        fmt = R.FORMATS[i % 5]
        rate = (FO, 16000, 48000, 22050, 96000, 8000, 32000)[i % 7]
        ch = (1, 2, 1, 3)[i % 4]
        n = int(rate * (0.10 + 0.002 * i)) + i
        t = np.arange(n)[:, None] / rate
        x = 0.3 * np.sin(2 * np.pi * (150.0 + 7 * i) * t + np.arange(ch)[None, :]) + 0.02 * rng.standard_normal((n, ch))
        if fmt == "f32":
            v = x.astype(np.float32)
        elif fmt == "u8":
            v = np.round(x * 127) + 128
        else:
            v = np.round(x * (1 << (8 * R.WIDTH[fmt] - 1)) * 0.99).astype(np.int64)
        clips.append((R.wav_bytes(v, fmt, rate, extensible=i % 3 == 0), f"text {i}"))
    reps = []
    profs = synth.encode_references(clips, loudness=-20.0, reports=reps)
    assert len(profs) == len(reps) == 70 and [p.text for p in profs] == [t for _, t in clips]
    for i, (b, t) in enumerate(clips):
        r1 = []
        one = synth.encode_reference_at(b, t, loudness=-20.0, report=r1)
        assert r1[0] == reps[i] and np.array_equal(one.codes, profs[i].codes) and one.codes.shape[1] == reps[i].frames > 0, i


def _tts_with_encoder():
    """A whole synthetic FishTTS whose codec has the encoder and the AR model's code layout (9 + 1 codebooks)."""
    import fish_tts_amd as ft
    from fish_tts_amd.tokenizer import NAMED_SPECIAL_TOKENS, ByteTokenizer
    shape = dataclasses.replace(tiny_shape(), max_seq_len=2304 + 512)
    tok = ByteTokenizer(256, NAMED_SPECIAL_TOKENS + [f"<|semantic:{i}|>" for i in range(2048)])
    cshape = dataclasses.replace(encode_shape(), n_codebooks=9, codebook_size=1024, semantic_codebook_size=2048)
    a = codec_args_from_shape(cshape)
    a.encoder_dim, a.encoder_rates = cshape.encoder_dim, list(cshape.encoder_rates)
    a.encoder_transformer_layers, a.encoder_tf_window = list(cshape.encoder_tf_layers), cshape.enc_tf_window
    return ft.FishTTS(None, "cuda", "bf16", False, max_batch=4,
                      _synthetic=dict(args=args_from_shape(shape), tokenizer=tok, codec_args=a, max_new_tokens=256, with_encoder=True))


def test_profiles_drive_synthesis_and_the_calls_work_under_a_server():
    tts = _tts_with_encoder()
    try:
        pcm = pcm16(100 * 64).astype(np.int16)
        b = wav16(FO, pcm)
        old = tts.encode_reference(b, "the reference text")
        new = tts.encode_reference_at(b, "the reference text", silence_db=None)
        assert new.codes.shape == (10, 100) and np.array_equal(new.codes, old.codes)
        w_old = tts.synthesize("Hi there", references=[old], max_tokens=12)
        w_new = tts.synthesize("Hi there", references=[new], max_tokens=12)
        assert w_old == w_new and len(w_new) > 44
        stereo24 = R.wav_bytes(np.stack([pcm.astype(np.int64) << 8] * 2, 1), "s24", FO, extensible=True)
        assert np.array_equal(tts.encode_reference_at(stereo24, "t", silence_db=None).codes, old.codes)
        trimmed = tts.encode_reference_at(b, "the reference text")
        got, errors = {}, []
        with tts.serve(burst=4):
            def speak():
                try:
                    got["wav"] = tts.synthesize("Hi there", references=[old], max_tokens=12)
                except BaseException as e:  # noqa: BLE001
                    errors.append(e)
            th = threading.Thread(target=speak)
            th.start()
            under = tts.encode_reference_at(b, "the reference text", silence_db=None)
            many = tts.encode_references([(b, "a"), (stereo24, "b")])
            audio, rep = tts.prepare_reference(b)
            th.join()
        assert not errors and got["wav"] == w_old
        assert np.array_equal(under.codes, old.codes)
        assert np.array_equal(many[0].codes, trimmed.codes) and np.array_equal(many[1].codes, trimmed.codes)
        assert rep.frames == trimmed.codes.shape[1] and len(audio) == rep.kept
    finally:
        tts._vocoder.close()
        tts._engine.close()
