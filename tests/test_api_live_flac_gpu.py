"""GPU, public API: `live_format=` on the five streaming calls, on the tiny synthetic models of tests/test_api_script_gpu.py.
Each call runs once with live_format and once without, with the same arguments: the chunks with it concatenate to one FLAC
stream whose decoded samples (tests/flac_ref.decode, which also checks every CRC and every frame number) are, bit for bit, the
int16 PCM chunks of the call without it - mono, stereo, behind live_bed, live_room and live_loudness, at another blocksize,
through a BatchServer; a file of the chunks, patched with flac_report's head, is to_flac() of the PCM's WAV byte for byte; the
batch stream gives one valid stream per utterance.  The stage's own bytes are tests/test_flac_stream_gpu.py's."""
import numpy as np
import pytest

from fish_tts_amd import LiveFlac, stream_info
from tests import flac_ref as R
from tests import intake_ref as IR
from tests.test_api_mix_gpu import _bed
from tests.test_api_room_gpu import _room
from tests.test_api_script_gpu import MT, SEED, TEXT, _script, _voice
from tests.test_api_serve_gpu import _tiny_tts

pytestmark = pytest.mark.gpu
PANS = {"anna": -0.5, "ben": 0.5}


@pytest.fixture(scope="module")
def synth():
    s = _tiny_tts()
    yield s
    if s._server is not None:
        s._server.close(cancel=True)


@pytest.fixture(scope="module")
def voices():
    return {"anna": _voice(1, "anna"), "ben": _voice(2, "ben")}


def _same(chunks, pcm_chunks, rate=44100, channels=1, blocksize=4096, report=None):
    """The FLAC chunks decode to the PCM chunks: no empty chunk, the unknown-values head in front, every sample."""
    chunks = list(chunks)
    assert chunks and all(chunks)
    data = b"".join(chunks)
    assert data[:42] == R.streaminfo(blocksize, 0, 0, rate, channels, 0)
    pcm = np.frombuffer(b"".join(pcm_chunks), dtype=np.int16)
    pcm = pcm if channels == 1 else pcm.reshape(-1, 2)
    assert len(pcm)
    d = R.decode(data)
    assert (d.rate, d.channels, d.bits, d.min_block, d.max_block) == (rate, channels, 16, blocksize, blocksize)
    assert np.array_equal(d.pcm.reshape(pcm.shape), pcm)
    assert [f["number"] for f in d.frames] == list(range(-(-len(pcm) // blocksize)))
    info = stream_info(data)
    assert (info.rate, info.channels, info.samples, info.min_frame, info.max_frame) == (rate, channels, 0, 0, 0)
    if report is not None:
        (rep, head), = report
        assert rep.frames == len(d.frames) and rep.bytes == len(data) and len(head) == 42
        assert stream_info(head + data[42:]).samples == len(pcm)
    return data, pcm


def test_synthesize_stream_both_ways(synth):
    for seamless, extra in ((False, {}), (True, {}), (True, dict(live_loudness=-20.0, sample_rate=24000))):
        kw = dict(chunk_tokens=6, min_first_chunk=3, max_tokens=30, seamless=seamless, **extra)
        plain = list(synth.synthesize_stream(TEXT, **kw))
        report = []
        got = list(synth.synthesize_stream(TEXT, live_format=LiveFlac(256), flac_report=report, **kw))
        _same(got, plain, rate=extra.get("sample_rate", 44100), blocksize=256, report=report)


def test_the_patched_file_is_to_flac_of_the_pcms_wav(synth):
    kw = dict(chunk_tokens=6, min_first_chunk=3, max_tokens=30, seamless=True, sample_rate=22050)
    plain = b"".join(synth.synthesize_stream(TEXT, **kw))
    report = []
    data = b"".join(synth.synthesize_stream(TEXT, live_format="flac", flac_report=report, **kw))
    (rep, head), = report
    wav = IR.wav_bytes(np.frombuffer(plain, dtype=np.int16), "s16", 22050)
    assert head + data[42:] == synth.to_flac(wav)
    assert rep.bytes == len(data) and rep.frames == -(-len(plain) // 2 // 4096)


def test_long_stream_with_a_bed_and_a_room(synth):
    base = dict(seed=SEED, max_tokens=MT, silence_db=None)
    for extra in (dict(), dict(live_bed=_bed()), dict(live_room=_room(), sample_rate=32000)):
        kw = dict(base, **extra)
        plain = list(synth.synthesize_long_stream(TEXT, **kw))
        report = []
        got = synth.synthesize_long_stream(TEXT, live_format="flac", flac_report=report, **kw)
        _same(got, plain, rate=extra.get("sample_rate", 44100), report=report)


def test_script_stream_mono_and_stereo(synth, voices):
    kw = dict(voices=voices, references=_voice(0, "v"), seed=SEED, max_tokens=MT, silence_db=None)
    marks, want_marks = [], []
    plain = list(synth.synthesize_script_stream(_script(), marks=want_marks, **kw))
    _same(synth.synthesize_script_stream(_script(), marks=marks, live_format="flac", **kw), plain)
    assert marks == want_marks
    st = dict(kw, live_stereo=True, live_pans=PANS, sample_rate=16000)
    plain = list(synth.synthesize_script_stream(_script(), **st))
    report = []
    data, pcm = _same(synth.synthesize_script_stream(_script(), live_format=LiveFlac(1024), flac_report=report, **st), plain,
                      rate=16000, channels=2, blocksize=1024, report=report)
    assert pcm.shape[1] == 2 and not np.array_equal(pcm[:, 0], pcm[:, 1])
    assert {f["assignment"] for f in R.decode(data).frames} <= {1, 8, 9, 10}


def test_batch_stream_gives_one_stream_per_utterance(synth):
    texts, seeds = ["batch one", "and batch two is longer"], [7, 8]
    kw = dict(seeds=seeds, max_tokens=40, chunk_tokens=6, min_first_chunk=3)
    plain = {0: [], 1: []}
    for i, pcm in synth.synthesize_batch_stream(texts, **kw):
        plain[i].append(pcm)
    got, report = {0: [], 1: []}, []
    for i, b in synth.synthesize_batch_stream(texts, live_format=LiveFlac(512), flac_report=report, **kw):
        got[i].append(b)
    assert sorted(r[0] for r in report) == [0, 1]
    for i in (0, 1):
        assert got[i][-1] == b"" and got[i].count(b"") == 1 and plain[i][-1] == b""
        _same(got[i][:-1], plain[i], blocksize=512, report=[r[1:] for r in report if r[0] == i])


def test_served(synth):
    kw = dict(seamless=True, max_tokens=30, chunk_tokens=5, min_first_chunk=2, seed=3)
    with synth.serve(burst=4) as srv:
        plain = list(srv.synthesize_stream(TEXT, **kw))
        report = []
        _same(srv.synthesize_stream(TEXT, live_format=LiveFlac(256), flac_report=report, **kw), plain, blocksize=256, report=report)
        # the instance's own call joins the server's batch; its stream is pushed under the server's codec lock
        _same(synth.synthesize_stream(TEXT, live_format=LiveFlac(256), **kw), plain, blocksize=256)
        with pytest.raises(ValueError, match="format"):
            srv.synthesize_stream(TEXT, format="flac")
        with pytest.raises(ValueError, match="live_format must be"):
            srv.synthesize_stream(TEXT, live_format="wav")


def test_bad_values_raise_before_any_work(synth, voices):
    for call in (lambda: next(synth.synthesize_stream("Some text.", live_format="ogg")),
                 lambda: synth.synthesize_batch_stream(["Some text."], live_format="ogg"),
                 lambda: synth.synthesize_long_stream(TEXT, live_format=4096),
                 lambda: synth.synthesize_script_stream(_script(), voices=voices, live_format="wav")):
        with pytest.raises(ValueError, match="live_format must be"):
            call()
    with pytest.raises(ValueError, match="blocksize"):
        LiveFlac(300)
