"""GPU, public API: `bed=` of FishTTS.synthesize_long / synthesize_script and FishTTS.mix on the tiny synthetic models of
tests/test_api_script_gpu.py.  bed=None is the call as it was, byte for byte; with a Bed the mix stage is given the joined
piece itself (a spy on CodecHipEngine.mix: its programme, packed, is the un-bedded call's PCM) and the WAV is the packing of
what it returns, `lead` + `tail` longer, the marks moved by `lead`; a bed of digital silence returns the un-bedded PCM between
lead and tail; an open BatchServer gives the same bytes; the streams refuse a bed; every bad Bed raises ValueError before
any device work.  All comparisons are equalities (the stage's own arithmetic is tests/test_mix_gpu.py's)."""
import numpy as np
import pytest

from tests import intake_ref as IR
from tests.test_api_script_gpu import MT, SEED, TEXT, _pcm, _script, _voice, _wav
from tests.test_api_serve_gpu import _tiny_tts

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


@pytest.fixture(scope="module")
def default():
    return _voice(0, "v")


def _music(n=4000, rate=44100, seed=3):
    t = np.arange(n)
    v = 0.2 * np.sin(2 * np.pi * 440.0 * t / rate) + 0.02 * np.random.default_rng(seed).standard_normal(n)
    return IR.wav_bytes(v.astype(np.float32), "f32", rate)


def _bed(**kw):
    from fish_tts_amd import Bed
    kw.setdefault("wav", _music())
    kw.setdefault("fade_out", 0.05)
    return Bed(**kw)


@pytest.fixture
def spy(synth, monkeypatch):
    """Every CodecHipEngine.mix call of a test: (programme, rate, params) -> (y, report)."""
    calls = []
    real = synth._vocoder.mix

    def mix(x, bed, sample_rate=None, params=None, nodes=False):
        out = real(x, bed, sample_rate=sample_rate, params=params, nodes=nodes)
        calls.append((np.array(x, dtype=np.float32), sample_rate, params, out))
        return out
    monkeypatch.setattr(synth._vocoder, "mix", mix)
    return calls


def test_bed_none_is_the_call_as_it_was(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED)
    assert synth.synthesize_long(TEXT, bed=None, **kw) == synth.synthesize_long(TEXT, **kw)
    m1, m2 = [], []
    assert synth.synthesize_script(_script(), voices, bed=None, marks=m1, **kw) == synth.synthesize_script(_script(), voices, marks=m2, **kw)
    assert m1 == m2 and not spy


@pytest.mark.parametrize("kw", [dict(), dict(sample_rate=16000, loudness=-23.0, silence_db=-30.0)], ids=["native", "16k-levelled"])
def test_the_mix_runs_over_the_joined_piece(synth, voices, default, spy, kw):
    kw = dict(kw, references=default, max_tokens=MT, seed=SEED)
    rate = kw.get("sample_rate", 44100)
    bed = _bed(lead=0.013, tail=0.021, duck_db=9.0, attack=0.04, release=0.06)
    lead, tail = int(round(0.013 * rate)), int(round(0.021 * rate))
    plain_marks, marks = [], []
    plain = synth.synthesize_script(_script(), voices, marks=plain_marks, **kw)
    got = synth.synthesize_script(_script(), voices, marks=marks, bed=bed, **kw)
    assert len(spy) == 1
    x, r, mp, (y, rep) = spy[0]
    assert r == rate and (mp.lead, mp.tail, mp.depth, mp.attack, mp.release, mp.bed_loudness) == (lead, tail, 900, 2, 3, -3000)
    assert mp.threshold == 10.0 ** (kw.get("silence_db", -45.0) / 20.0)        # the call's silence_db
    assert _pcm(x) == _wav(plain)[1]                                            # the programme is the un-bedded piece
    assert _wav(got) == (rate, _pcm(y))                                         # the WAV is the packing of the stage's output
    assert len(y) == lead + len(x) + tail and rep.n == len(y) and rep.active > 0
    assert marks == [(a + lead, b + lead) for a, b in plain_marks]
    # the same through synthesize_long
    del spy[:]
    plain = synth.synthesize_long(TEXT, **kw)
    got = synth.synthesize_long(TEXT, bed=bed, **kw)
    x, r, mp, (y, rep) = spy[0]
    assert len(spy) == 1 and _pcm(x) == _wav(plain)[1] and _wav(got) == (rate, _pcm(y)) and len(y) == lead + len(x) + tail


def test_a_silent_bed_returns_the_piece(synth, voices, default):
    # (levelled: the piece then peaks far below the -1 dBFS ceiling, which would otherwise turn the whole piece down)
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)
    silence = IR.wav_bytes(np.zeros((3000, 2), dtype=np.int64), "s16", 48000)
    plain = _wav(synth.synthesize_script(_script(), voices, **kw))[1]
    got = _wav(synth.synthesize_script(_script(), voices, bed=_bed(wav=silence, lead=0.01, tail=0.02, level=None), **kw))[1]
    assert got == b"\0\0" * 160 + plain + b"\0\0" * 320
    # a silent bed cannot be levelled either: the level stage leaves digital silence as it is
    assert _wav(synth.synthesize_script(_script(), voices, bed=_bed(wav=silence, lead=0.01, tail=0.02), **kw))[1] == got


def test_through_an_open_server_and_on_a_finished_wav(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, silence_db=-30.0)
    bed = _bed(lead=0.01, tail=0.01, threshold_db=-20.0, loop=False, offset=0.002)
    m0, m1 = [], []
    want = synth.synthesize_script(_script(), voices, marks=m0, bed=bed, **kw)
    want_long = synth.synthesize_long(TEXT, bed=bed, **kw)
    plain = synth.synthesize_long(TEXT, **kw)
    report = []
    mixed = synth.mix(plain, bed, silence_db=-30.0, report=report)
    assert spy[-1][2].threshold == 10.0 ** (-20.0 / 20.0) and spy[-1][2].loop == 0
    # the finished WAV's samples are the programme of that call: v / 32768, as the reference intake reads 16-bit audio
    assert (spy[-1][0] * 32768).astype(np.int16).tobytes() == _wav(plain)[1]
    assert _wav(mixed)[0] == 44100 and report[0].n == len(_wav(mixed)[1]) // 2
    with synth.serve(burst=4):
        assert synth.synthesize_script(_script(), voices, marks=m1, bed=bed, **kw) == want and m1 == m0
        assert synth.synthesize_long(TEXT, bed=bed, **kw) == want_long
        assert synth.mix(plain, bed, silence_db=-30.0) == mixed


def test_the_streams_refuse_a_bed(synth, voices, default):
    with pytest.raises(ValueError, match="whole piece"):
        synth.synthesize_long_stream(TEXT, references=default, bed=_bed())
    with pytest.raises(ValueError, match="whole piece"):
        synth.synthesize_script_stream(_script(), voices, references=default, bed=_bed())
    chunks = list(synth.synthesize_long_stream(TEXT, references=default, max_tokens=MT, seed=SEED, bed=None))
    assert b"".join(chunks) == _wav(synth.synthesize_long(TEXT, references=default, max_tokens=MT, seed=SEED))[1]


def test_bad_beds_raise_before_any_work(synth, voices, default, monkeypatch, spy):
    from fish_tts_amd import Bed, Line

    def no_work(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    ok = _music()
    nan = float("nan")
    bad = [dict(level=-4.0), dict(level=-51), dict(level="x"), dict(level=nan), dict(duck_db=-0.1), dict(duck_db=60.5), dict(duck_db=None),
           dict(threshold_db=0.5), dict(threshold_db=-91), dict(attack=0.0), dict(attack=0.009), dict(attack=10.1), dict(attack=True),
           dict(release=0), dict(release=11), dict(release=nan), dict(lead=-0.1), dict(lead=601), dict(tail=-1), dict(tail="1"),
           dict(fade_in=-1), dict(fade_in=nan), dict(fade_out=-0.5), dict(fade_out=None), dict(offset=-1), dict(offset=1e9),
           dict(loop=1), dict(loop=None), dict(channel=-1), dict(channel=1), dict(channel=1.0), dict(channel=True),
           dict(wav=b"not a wav"), dict(wav=ok[:40]), dict(wav=None), dict(wav=3),
           dict(wav=IR.wav_bytes(np.zeros(100, dtype=np.float32), "f32", 7000)),           # a rate the intake refuses
           dict(wav=IR.wav_bytes(np.zeros(100, dtype=np.float32), "f32", 44100)[:46])]     # no whole frame is there
    plain = synth.synthesize_long("Some text is here.", references=default, max_tokens=MT, seed=SEED)
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth._vocoder, "decode_join", no_work)
    monkeypatch.setattr(synth._vocoder.lib, "ft_codec_mix", no_work, raising=False)
    monkeypatch.setattr(synth._vocoder.lib, "ft_codec_intake", no_work, raising=False)
    for kw in bad:
        kw.setdefault("wav", ok)
        b = Bed(**kw)
        for call in (lambda: synth.synthesize_long(TEXT, references=default, bed=b),
                     lambda: synth.synthesize_script([Line("Some text is here.")], voices, references=default, bed=b),
                     lambda: synth.mix(plain, b)):
            with pytest.raises(ValueError):
                call()
    for notbed in (ok, (ok,), {"wav": ok}, "bed.wav"):
        with pytest.raises(ValueError, match="Bed"):
            synth.synthesize_long(TEXT, references=default, bed=notbed)
        with pytest.raises(ValueError, match="Bed"):
            synth.mix(plain, notbed)
    with pytest.raises(ValueError):
        synth.mix(plain, None)
    stereo = IR.wav_bytes(np.zeros((50, 2), dtype=np.int64), "s16", 44100)
    for wav in (stereo, IR.wav_bytes(np.zeros(50, dtype=np.int64), "s16", 12345), IR.wav_bytes(np.zeros(0, dtype=np.int64), "s16", 44100)):
        with pytest.raises(ValueError):
            synth.mix(wav, Bed(ok))
    assert not spy
