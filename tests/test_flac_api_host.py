"""`format=` without a GPU: which calls take it and which refuse it, what reaches the codec engine (the float32 samples
_to_wav_bytes would have quantised, at the call's rate; a WAV's own int16 samples from to_flac), the BatchServer handing the
format to its decoder only when it is not "wav", CodecHipEngine.flac's own argument checks, and flacfile.stream_info."""
import io
import wave

import numpy as np
import pytest

from fish_tts_amd.flacfile import FlacInfo, stream_info
from fish_tts_amd.script import Line
from tests import flac_cases as FC
from tests import flac_ref as R
from tests.intake_ref import wav_bytes
from tests.test_serve_host import MovingEngine, _frames, _plain, _prepare
from tests.test_batch_stream_host import FakeCodec

T = "Some text is here."


class FlacCodec:
    """A codec engine that packs with the reference and records what it was asked."""
    def __init__(self):
        self.calls = []

    def flac(self, audio, sample_rate=None, blocksize=4096):
        self.calls.append((np.array(audio), sample_rate, blocksize))
        return R.encode(R.quantise(audio), sample_rate, blocksize), None

    def decode(self, codes, fx=None):
        return np.linspace(-1.2, 1.2, 500, dtype=np.float32)[None]


def _tts(vocoder=None):
    from fish_tts_amd.synthesizer import FishTTS
    tts = FishTTS.__new__(FishTTS)                           # the checks come before anything else of the instance is used
    tts._vocoder = vocoder
    return tts


def test_whole_calls_refuse_an_unknown_format():
    tts = _tts()
    for bad in ("ogg", "FLAC", "", None, 1, b"flac"):
        for call in (lambda: tts.synthesize_at(T, format=bad), lambda: tts.synthesize_batch([T], format=bad),
                     lambda: tts.synthesize_long(T, format=bad), lambda: tts.synthesize_script([Line(T)], format=bad),
                     lambda: tts.mix(b"", None, format=bad), lambda: tts.reverb(b"", None, format=bad)):
            with pytest.raises(ValueError, match="format must be one of"):
                call()


def test_the_streams_refuse_a_format():
    from fish_tts_amd.serve import BatchServer
    from fish_tts_amd.synthesizer import _no_streamed_format
    tts = _tts()
    for fmt in ("flac", "wav", "ogg"):
        with pytest.raises(ValueError, match="format needs the whole piece: synthesize_batch_stream"):
            tts.synthesize_batch_stream([T], format=fmt)
        with pytest.raises(ValueError, match="format needs the whole piece: synthesize_long_stream"):
            tts.synthesize_long_stream(T, format=fmt)
        with pytest.raises(ValueError, match="format needs the whole piece: synthesize_script_stream"):
            tts.synthesize_script_stream([Line(T)], format=fmt)
        with pytest.raises(ValueError, match="format needs the whole piece: synthesize_stream"):
            next(tts.synthesize_stream(T, format=fmt))                     # a generator: at the first next(), before any work
        with pytest.raises(ValueError, match="format needs the whole piece: BatchServer.synthesize_stream"):
            BatchServer.__new__(BatchServer).synthesize_stream(T, format=fmt)
    _no_streamed_format(None, "synthesize_stream")
    with pytest.raises(ValueError, match="format must be one of"):
        BatchServer.__new__(BatchServer).synthesize(T, format="ogg")


def test_a_finished_waveform_reaches_the_stage_as_it_would_reach_the_wav():
    codec = FlacCodec()
    tts = _tts(codec)
    mono = np.linspace(-1.5, 1.5, 3000, dtype=np.float32)
    stereo = np.stack([mono, -0.5 * mono], 1)
    for audio, rate in ((mono, 44100), (stereo, 24000)):
        wav = tts._to_file_bytes(audio, rate, "wav")
        assert wav == tts._to_wav_bytes(audio, rate) and not codec.calls
        flac = tts._to_file_bytes(audio, rate, "flac")
        got, at, blocksize = codec.calls.pop()
        assert got.dtype == np.float32 and np.array_equal(got, audio) and (at, blocksize) == (rate, 4096)
        d = R.decode(flac)
        with wave.open(io.BytesIO(wav), "rb") as wf:
            pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).reshape(audio.shape)
            assert (d.rate, d.channels) == (wf.getframerate(), wf.getnchannels())
        assert np.array_equal(d.pcm, pcm)                                   # the FLAC's samples are the WAV's
    # the calls that decode codes: the same rule through _decode_to_wav
    codes = np.zeros((3, 7), dtype=np.int32)
    assert tts._decode_to_wav(codes) == tts._to_wav_bytes(codec.decode(codes)[0], 44100) and not codec.calls
    d = R.decode(tts._decode_to_wav(codes, None, format="flac"))
    assert d.rate == 44100 and np.array_equal(d.pcm, R.quantise(codec.decode(codes)[0]))
    with pytest.raises(RuntimeError, match="Vocoder not loaded"):
        _tts()._to_file_bytes(mono, 44100, "flac")


def test_to_flac_takes_a_wavs_own_samples():
    codec = FlacCodec()
    tts = _tts(codec)
    rng = np.random.default_rng(1)
    for channels, rate in ((1, 16000), (2, 48000)):
        pcm = rng.integers(-32768, 32768, (700, channels)).astype(np.int16)
        wav = wav_bytes(pcm, "s16", rate)
        with wave.open(io.BytesIO(wav), "rb") as wf:                        # (what the file really holds)
            held = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).reshape(-1, channels)
        flac = tts.to_flac(wav, blocksize=512)
        got, at, blocksize = codec.calls.pop()
        assert got.dtype == np.int16 and got.shape == ((700,) if channels == 1 else (700, 2)) and (at, blocksize) == (rate, 512)
        assert np.array_equal(got.reshape(held.shape), held)
        assert np.array_equal(R.decode(flac).pcm.reshape(held.shape), held)
    for fmt, channels, word in (("f32", 1, "16-bit PCM"), ("u8", 1, "16-bit PCM"), ("s24", 2, "16-bit PCM"), ("s16", 3, "mono or stereo")):
        with pytest.raises(ValueError, match=word):
            tts.to_flac(wav_bytes(np.zeros((50, channels), dtype=np.float32 if fmt == "f32" else np.int32), fmt, 44100))
    with pytest.raises(ValueError, match="RIFF"):
        tts.to_flac(b"fLaC....")
    with pytest.raises(ValueError, match="sample_rate"):
        tts.to_flac(wav_bytes(np.zeros(50, dtype=np.int16), "s16", 7000))
    assert not codec.calls


def test_server_hands_the_format_to_its_decoder():
    from fish_tts_amd.serve import BatchServer
    seen = []

    def wav(codes, fx=None, **kw):
        seen.append(kw)
        return b"W" + np.ascontiguousarray(codes[0], dtype=np.int32).tobytes()

    srv = BatchServer(MovingEngine(), FakeCodec(), 4, prepare=_prepare, decode_wav=wav, decode_pcm=_plain)
    try:
        assert srv.synthesize("1", max_tokens=5).startswith(b"W" + _frames(1, 1).tobytes())
        assert srv.synthesize("2", max_tokens=5, format="wav").startswith(b"W" + _frames(2, 1).tobytes())
        assert srv.synthesize("3", max_tokens=5, format="flac").startswith(b"W" + _frames(3, 1).tobytes())
        with pytest.raises(ValueError, match="format must be one of"):     # refused on the caller's thread: the server lives on
            srv.submit(*_prepare("4", None, 0.7, 0.8, 1.1, 5, 0), format="ogg")
        assert srv.synthesize("5", max_tokens=5).startswith(b"W" + _frames(5, 1).tobytes())
    finally:
        srv.close()
    assert seen[:3] == [{}, {}, {"format": "flac"}]          # a decoder that knows no format is called as it always was


def test_stream_info():
    data, census, pcm = FC.reference("st_speech_pair")
    assert stream_info(data) == FlacInfo(32000, 2, 16, 5000, 2048, 2048, census.min_frame, census.max_frame, bytes(16), 42)
    assert stream_info(memoryview(data)).samples == 5000
    anchor = bytes.fromhex("664c6143" "80000022" "10001000" "00000f00000f" "0ac442f000000001" "3e84b41807dc690307586a3dad1a2e0f")
    got = stream_info(anchor)
    assert got[:8] == (44100, 2, 16, 1, 4096, 4096, 15, 15) and got.md5.hex().startswith("3e84b418") and got.data_offset == 42
    # a padding block behind STREAMINFO is skipped
    padded = anchor[:4] + b"\x00" + anchor[5:] + bytes([0x81, 0, 0, 3, 0, 0, 0]) + b"\xff\xf8"
    assert stream_info(padded).data_offset == 49
    for bad, word in ((b"RIFF....", "fLaC"), (b"fLa", "fLaC"), (anchor[:20], "past the end"), (anchor[:4] + b"\x81" + anchor[5:], "STREAMINFO"),
                      (anchor[:4] + b"\x00" + anchor[5:], "past the end"), (anchor[:4] + b"\x00" + anchor[5:] + anchor[4:], "second STREAMINFO"),
                      (anchor[:18] + bytes(3) + anchor[21:], "rate of 0"), (anchor[:8] + bytes(4) + anchor[12:], "blocksizes")):
        with pytest.raises(ValueError, match=word):
            stream_info(bad)
