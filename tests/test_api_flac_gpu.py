"""GPU, public API: `format="flac"` on the tiny synthetic models of tests/test_api_script_gpu.py.  A call with format="flac"
returns a FLAC file whose decoded samples (tests/flac_ref.decode, which also checks every CRC and STREAMINFO) are, bit for
bit, the int16 samples of the same call's WAV - mono and stereo, at the codec's rate and resampled, from the one-shot, batch,
long, script, served, mix and reverb calls; to_flac is lossless on a WAV's own samples; the streams refuse a format; any
other format raises ValueError before any work.  The stream's own bytes are tests/test_flac_gpu.py's."""
import numpy as np
import pytest

from tests import flac_ref as R
from tests import intake_ref as IR
from tests.test_api_mix_gpu import _bed
from tests.test_api_room_gpu import _room
from tests.test_api_script_gpu import MT, SEED, TEXT, _script, _voice
from tests.test_api_serve_gpu import _tiny_tts
from tests.test_api_stereo_gpu import _wav2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth():
    s = _tiny_tts()
    yield s
    if s._server is not None:
        s._server.close(cancel=True)


@pytest.fixture(scope="module")
def voices():
    return {"anna": _voice(1, "anna"), "ben": _voice(2, "ben")}


def _same(flac: bytes, wav: bytes, channels: int = 1):
    """The FLAC decodes to the WAV: rate, channels, 16 bits, every sample."""
    from fish_tts_amd import stream_info
    rate, ch, pcm = _wav2(wav)
    d = R.decode(flac)
    assert ch == channels and (d.rate, d.channels, d.bits, d.n) == (rate, ch, 16, len(pcm))
    assert np.array_equal(d.pcm.reshape(pcm.shape), pcm)
    info = stream_info(flac)
    assert (info.rate, info.channels, info.bits, info.samples, info.min_blocksize, info.max_blocksize) == (rate, ch, 16, len(pcm), 4096, 4096)
    assert info.md5 == bytes(16) and flac[info.data_offset:info.data_offset + 2] == b"\xff\xf8"
    return d


@pytest.mark.parametrize("rate", [None, 24000])
def test_synthesize_at(synth, rate):
    kw = dict(max_tokens=MT, sample_rate=rate)
    wav = synth.synthesize_at("A short sentence.", **kw)
    assert wav == synth.synthesize_at("A short sentence.", format="wav", **kw)
    d = _same(synth.synthesize_at("A short sentence.", format="flac", **kw), wav)
    assert d.rate == (rate or 44100)
    if rate is None:
        assert wav == synth.synthesize("A short sentence.", max_tokens=MT)          # the default is byte for byte what it was


def test_synthesize_batch_and_long(synth):
    texts, seeds = ["One", "the second text"], [3, 4]
    wavs = synth.synthesize_batch(texts, seeds=seeds, max_tokens=MT, sample_rate=16000)
    flacs = synth.synthesize_batch(texts, seeds=seeds, max_tokens=MT, sample_rate=16000, format="flac")
    assert len(flacs) == 2
    for f, w in zip(flacs, wavs):
        _same(f, w)
    kw = dict(seed=SEED, max_tokens=MT, silence_db=None)
    _same(synth.synthesize_long(TEXT, format="flac", **kw), synth.synthesize_long(TEXT, **kw))


def test_synthesize_script_mono_and_stereo(synth, voices):
    kw = dict(voices=voices, references=_voice(0, "v"), seed=SEED, max_tokens=MT, silence_db=None)
    _same(synth.synthesize_script(_script(), format="flac", **kw), synth.synthesize_script(_script(), **kw))
    st = dict(kw, stereo=True, pans={"anna": -0.6, "ben": 0.7}, sample_rate=32000)
    wav = synth.synthesize_script(_script(), **st)
    d = _same(synth.synthesize_script(_script(), format="flac", **st), wav, channels=2)
    assert d.rate == 32000 and not np.array_equal(d.pcm[:, 0], d.pcm[:, 1])
    assert {f["assignment"] for f in d.frames} <= {1, 8, 9, 10}


def test_mix_reverb_and_to_flac(synth):
    wav = synth.synthesize_at("A sentence to be mixed.", max_tokens=MT)
    bed = _bed()
    _same(synth.mix(wav, bed, format="flac"), synth.mix(wav, bed))
    _same(synth.mix(wav, bed, stereo=True, format="flac"), synth.mix(wav, bed, stereo=True), channels=2)
    room = _room()
    _same(synth.reverb(wav, room, format="flac"), synth.reverb(wav, room))
    # to_flac: the file's own samples, mono and stereo, at every blocksize
    _same(synth.to_flac(wav), wav)
    two = synth.mix(wav, bed, stereo=True)
    for B in (256, 1024):
        flac = synth.to_flac(two, blocksize=B)
        rate, ch, pcm = _wav2(two)
        d = R.decode(flac)
        assert (d.rate, d.channels, d.min_block) == (rate, 2, B) and np.array_equal(d.pcm, pcm)
    full = IR.wav_bytes(np.array([[-32768, 32767], [32767, -32768]] * 40, dtype=np.int16), "s16", 8000)
    _, _, pcm = _wav2(full)
    assert pcm.min() == -32768 and np.array_equal(R.decode(synth.to_flac(full)).pcm, pcm)    # -32768 survives: nothing is re-quantised
    for bad, word in ((IR.wav_bytes(np.zeros(50, dtype=np.float32), "f32", 44100), "16-bit PCM"),
                      (IR.wav_bytes(np.zeros((50, 3), dtype=np.int16), "s16", 44100), "mono or stereo")):
        with pytest.raises(ValueError, match=word):
            synth.to_flac(bad)
    with pytest.raises(ValueError, match="blocksize"):
        synth.to_flac(wav, blocksize=300)


def test_served(synth):
    wav = synth.synthesize_at("Served text.", max_tokens=MT, sample_rate=22050)
    with synth.serve() as srv:
        assert srv.synthesize("Served text.", max_tokens=MT, sample_rate=22050) == wav
        _same(srv.synthesize("Served text.", max_tokens=MT, sample_rate=22050, format="flac"), wav)
        _same(synth.synthesize_at("Served text.", max_tokens=MT, sample_rate=22050, format="flac"), wav)   # joins the server's batch
        _same(synth.to_flac(wav), wav)                                                # under the server's codec lock
        with pytest.raises(ValueError, match="format"):
            srv.synthesize_stream("Served text.", format="flac")
        with pytest.raises(ValueError, match="format"):
            srv.synthesize("Served text.", format="ogg")


def test_streams_and_unknown_formats_raise(synth, voices):
    with pytest.raises(ValueError, match="format"):
        next(synth.synthesize_stream("Some text.", format="flac"))
    with pytest.raises(ValueError, match="format"):
        synth.synthesize_batch_stream(["Some text."], format="flac")
    with pytest.raises(ValueError, match="format"):
        synth.synthesize_long_stream(TEXT, format="flac")
    with pytest.raises(ValueError, match="format"):
        synth.synthesize_script_stream(_script(), voices=voices, format="flac")
    wav = synth.synthesize_at("A sentence.", max_tokens=MT)
    for call in (lambda: synth.synthesize_at("A sentence.", format="ogg"), lambda: synth.synthesize_batch(["A"], format="ogg"),
                 lambda: synth.synthesize_long(TEXT, format="ogg"), lambda: synth.synthesize_script(_script(), voices=voices, format="ogg"),
                 lambda: synth.mix(wav, _bed(), format="ogg"), lambda: synth.reverb(wav, _room(), format="ogg")):
        with pytest.raises(ValueError, match="format must be one of"):
            call()
