"""GPU, public API: `stereo=` of FishTTS.synthesize_script / synthesize_long / mix on the tiny synthetic models of
tests/test_api_script_gpu.py.  The stereo mix stage is given the joined mono piece itself and the lines' marks as regions (a
spy on CodecHipEngine.mix_stereo), and the WAV is the two-channel packing of what it returns; on the float path a line's
frames are the mono piece's times the pan table's gains, bit for bit; with every pan 0 and a mono bed both channels are the
mono call's samples; the ValueErrors come before any device work; the streams stay mono and refuse a pan.  All comparisons
are equalities (the stage's own arithmetic is tests/test_stereo_mix_gpu.py's)."""
import io
import wave

import numpy as np
import pytest

from tests import intake_ref as IR
from tests import stereo_ref as SR
from tests.test_api_mix_gpu import _bed, _music
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


def _stereo_music(n=4000, rate=48000):
    t = np.arange(n)
    v = np.stack([0.2 * np.sin(2 * np.pi * 440.0 * t / rate), 0.1 * np.sin(2 * np.pi * 660.0 * t / rate)], 1)
    return IR.wav_bytes(v.astype(np.float32), "f32", rate)


def _wav2(data):
    """(rate, channels, int16 frames [N, channels]) of a WAV."""
    with wave.open(io.BytesIO(data), "rb") as wf:
        assert wf.getsampwidth() == 2
        ch = wf.getnchannels()
        return wf.getframerate(), ch, np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).reshape(-1, ch)


def _pack(y):
    return (np.clip(y, -1.0, 1.0) * 32767).astype(np.int16)


@pytest.fixture
def spy(synth, monkeypatch):
    """Every CodecHipEngine.mix_stereo call of a test: (programme, bed, regions, rate, params, (y, report))."""
    calls = []
    real = synth._vocoder.mix_stereo

    def mix_stereo(x, bed, regions=(), sample_rate=None, params=None, nodes=False):
        out = real(x, bed, regions, sample_rate=sample_rate, params=params, nodes=nodes)
        calls.append((np.array(x, dtype=np.float32), bed, list(regions), sample_rate, params, out))
        return out
    monkeypatch.setattr(synth._vocoder, "mix_stereo", mix_stereo)
    return calls


def test_a_script_with_two_voices_left_and_right_over_a_stereo_bed(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)
    bed = _bed(wav=_stereo_music(), lead=0.013, tail=0.021)
    lead = int(round(0.013 * 16000))
    plain_marks, marks = [], []
    plain = synth.synthesize_script(_script(), voices, marks=plain_marks, **kw)
    got = synth.synthesize_script(_script(), voices, marks=marks, bed=bed, stereo=True, pans={"anna": -0.5, "ben": 0.5}, **kw)
    assert len(spy) == 1
    x, clip, regions, rate, mp, (y, rep) = spy[0]
    assert rate == 16000 and mp.lead == lead and _pcm(x) == _wav(plain)[1]       # the programme is the mono piece
    (a0, e0), (a1, e1), _, (a3, e3) = plain_marks                                 # anna, ben, the narrator, anna
    assert regions == [(a0, e0, -50), (a1, e1, 50), (a3, e3, -50)]
    assert marks == [(a + lead, b + lead) for a, b in plain_marks]                # frames, moved by the bed's lead
    r, ch, frames = _wav2(got)
    assert (r, ch) == (16000, 2) and y.shape == (rep.n, 2) and np.array_equal(frames, _pack(y))
    assert not np.array_equal(frames[:lead, 0], frames[:lead, 1])                 # the bed's own left and right
    # the float path without a bed: every line's frames are the mono piece's times the table's gains
    z, zrep = synth._vocoder.mix_stereo(x, None, regions, sample_rate=16000)
    sg = np.float32(zrep.gain)
    for (a, e), pan in zip(plain_marks, (-50, 50, 0, -50)):
        for c, gain in enumerate(SR.gains_of(pan)):
            want = (x[a:e] * gain).astype(np.float32)
            want = (want * sg).astype(np.float32) if zrep.capped else want
            assert np.array_equal(z[a:e, c].view(np.uint32), want.view(np.uint32)), (a, e, pan, c)
    assert SR.gains_of(-50)[0] == 1.0 and SR.gains_of(-50)[1] == SR.pan_gains()[50] < 1.0
    # Line.pan wins over the voice's place; a pan of the call's own voice
    from fish_tts_amd import Line
    del spy[:]
    lines = _script()
    lines[1] = lines[1]._replace(pan=-1.0)
    lines[2] = lines[2]._replace(pan=0.25)
    synth.synthesize_script(lines, voices, stereo=True, pans={"anna": -0.5, "ben": 0.5}, **kw)
    assert [r[2] for r in spy[0][2]] == [-50, -100, 25, -50] and spy[0][1] is None


def test_every_pan_zero_over_a_mono_bed_is_the_mono_call_twice(synth, voices, default):
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, silence_db=-30.0)
    bed = _bed(lead=0.01, tail=0.02)
    mono = _wav2(synth.synthesize_script(_script(), voices, bed=bed, **kw))
    for extra in (dict(), dict(pans={"anna": 0.0, "ben": 0})):
        r, ch, frames = _wav2(synth.synthesize_script(_script(), voices, bed=bed, stereo=True, **kw, **extra))
        assert (r, ch, mono[1]) == (16000, 2, 1)
        assert np.array_equal(frames[:, 0], mono[2][:, 0]) and np.array_equal(frames[:, 1], mono[2][:, 0])
    # without a bed: two channels of the plain call, unless the ceiling turns the piece down
    plain = _wav2(synth.synthesize_script(_script(), voices, loudness=-23.0, **kw))
    r, ch, frames = _wav2(synth.synthesize_script(_script(), voices, loudness=-23.0, stereo=True, **kw))
    assert ch == 2 and np.array_equal(frames[:, 0], plain[2][:, 0]) and np.array_equal(frames[:, 1], plain[2][:, 0])


def test_mix_and_synthesize_long_in_stereo(synth, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, silence_db=-30.0, loudness=-23.0)
    plain = synth.synthesize_long(TEXT, **kw)
    got = synth.synthesize_long(TEXT, stereo=True, pan=-1.0, **kw)
    x, clip, regions, rate, mp, (y, rep) = spy[0]
    assert clip is None and _pcm(x) == _wav(plain)[1] and len(regions) == 1 and regions[0][2] == -100
    assert regions[0][0] == 0 and regions[0][1] == len(x)                        # one region over the piece
    r, ch, frames = _wav2(got)
    assert (r, ch) == (44100, 2) and not frames[:, 1].any() and frames[:, 0].tobytes() == _wav(plain)[1]
    bed = _bed(wav=_stereo_music(), lead=0.01)
    got = synth.synthesize_long(TEXT, stereo=True, pan=0.3, bed=bed, **kw)
    assert spy[1][2] == [(0, len(x), 30)] and spy[1][1] is not None and _wav2(got)[1] == 2
    report = []
    mixed = synth.mix(plain, bed, silence_db=-30.0, stereo=True, report=report)
    r, ch, frames = _wav2(mixed)
    assert (r, ch) == (44100, 2) and report[0].n == len(frames) == 441 + len(x) and spy[2][2] == []
    assert not np.array_equal(frames[:, 0], frames[:, 1]) and np.array_equal(frames, _pack(spy[2][5][0]))
    assert _wav2(synth.mix(plain, bed, silence_db=-30.0))[1] == 1                 # mono callers are as they were
    with synth.serve(burst=4):                                                    # ... and through an open server
        assert synth.synthesize_long(TEXT, stereo=True, pan=0.3, bed=bed, **kw) == got
        assert synth.mix(plain, bed, silence_db=-30.0, stereo=True) == mixed


def test_bad_pans_raise_before_any_work(synth, voices, default, monkeypatch, spy):
    from fish_tts_amd import Line

    def no_work(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    t = "Some text is here."
    plain = synth.synthesize_long(t, references=default, max_tokens=MT, seed=SEED)
    monkeypatch.setattr(synth, "_batch_utterances", no_work)
    monkeypatch.setattr(synth._vocoder, "decode_join", no_work)
    monkeypatch.setattr(synth._vocoder.lib, "ft_codec_mix_stereo", no_work, raising=False)
    nan = float("nan")
    script = lambda *a, **k: synth.synthesize_script(*a, references=default, **k)      # noqa: E731
    bad = [lambda: script([Line(t, pan=0.5)], voices),                                  # a pan without stereo
           lambda: script([Line(t, pan=0.0)], voices),
           lambda: script([Line(t)], voices, pans={"anna": 0.5}),
           lambda: script([Line(t)], voices, pans={}),
           lambda: script([Line(t)], voices, stereo=1),
           lambda: script([Line(t)], voices, stereo=True, pans={"carl": 0.5}),          # no voice of the call
           lambda: script([Line(t)], None, stereo=True, pans={"anna": 0.5}),
           lambda: script([Line(t)], voices, stereo=True, pans=[("anna", 0.5)]),
           lambda: synth.synthesize_long(t, references=default, pan=0.5),
           lambda: synth.synthesize_long(t, references=default, stereo="yes"),
           lambda: synth.mix(plain, _bed(), stereo=1)]
    for v in (1.01, -1.5, nan, True, "0.5", None):
        if v is not None:
            bad.append(lambda v=v: script([Line(t, pan=v)], voices, stereo=True))
        bad.append(lambda v=v: script([Line(t)], voices, stereo=True, pans={"anna": v}))
        bad.append(lambda v=v: synth.synthesize_long(t, references=default, stereo=True, pan=v))
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    crowd = [Line(t, pan=(0.5 if i % 2 else -0.5)) for i in range(4097)]                # 4097 regions after merging
    with pytest.raises(ValueError, match="4096"):
        script(crowd, voices, stereo=True)
    assert not spy


def test_the_streams_stay_mono_and_refuse_a_pan(synth, voices, default):
    from fish_tts_amd import Line
    t = "Some text is here."
    with pytest.raises(ValueError, match="stereo"):
        synth.synthesize_script_stream([Line(t, pan=0.5)], voices, references=default)
    with pytest.raises(ValueError, match="stereo"):
        synth.synthesize_script_stream([Line(t, pan=0.5)], voices, references=default, live_bed=_bed(wav=_music()))
    with pytest.raises(TypeError):
        synth.synthesize_script_stream([Line(t)], voices, references=default, stereo=True)
    with pytest.raises(TypeError):
        synth.synthesize_long_stream(t, references=default, stereo=True)
    with pytest.raises(TypeError):
        synth.synthesize_long_stream(t, references=default, pan=0.5)
    chunks = list(synth.synthesize_script_stream(_script(), voices, references=default, max_tokens=MT, seed=SEED))
    assert b"".join(chunks) == _wav(synth.synthesize_script(_script(), voices, references=default, max_tokens=MT, seed=SEED))[1]
