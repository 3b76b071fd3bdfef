"""GPU, public API: `live_stereo=` of FishTTS.synthesize_script_stream / synthesize_long_stream on the tiny synthetic models and
the two-voice script of tests/test_api_stereo_gpu.py.  Where neither ceiling binds - asserted through the reports: the
one-shot call's MixReport not capped, the live stage's limit_max 0 - the chunks concatenate to the PCM of the one-shot
`stereo=` call byte for byte, with and without a quiet bed; with every pan 0 and a mono bed both channels are the mono
`live_bed=` stream; a loud hard-left voice over a loud bed stays under -1 dBFS on both channels; `marks` are the one-shot
call's; an abandoned generator closes its stream.  A spy on CodecHipEngine.mix_stream records every push, so each stream is
also held against CodecHipEngine.mix_live_stereo over its whole programme (the stage's own arithmetic is
tests/test_stereo_live_gpu.py's)."""
import numpy as np
import pytest

from tests.test_api_mix_gpu import _bed
from tests.test_api_script_gpu import MT, SEED, TEXT, _script, _voice
from tests.test_api_serve_gpu import _tiny_tts
from tests.test_api_stereo_gpu import _pack, _stereo_music, _wav2

pytestmark = pytest.mark.gpu
CEILING = int(10.0 ** (-1.0 / 20.0) * 32767) + 1          # -1 dBFS in int16, one step for the rounding of the factor
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


@pytest.fixture(scope="module")
def default():
    return _voice(0, "v")


@pytest.fixture
def spy(synth, monkeypatch):
    """Every mix stream a test opens: dict(bed, rate, params, stereo, stream, pushes=[(x, regions, final)]), and every
    CodecHipEngine.mix_stereo call's report in `one_shot`."""
    opened, one_shot = [], []
    real_stream, real_stereo = synth._vocoder.mix_stream, synth._vocoder.mix_stereo

    def mix_stream(bed, sample_rate=None, params=None, stereo=False):
        ms = real_stream(bed, sample_rate=sample_rate, params=params, stereo=stereo)
        rec = dict(bed=bed, rate=sample_rate, params=params, stereo=stereo, stream=ms, pushes=[])
        push = ms.push

        def spied(x=None, *a, **k):
            regions = list(a[0] if a else k.get("regions", ())) if stereo else []
            rec["pushes"].append((np.zeros(0, dtype=np.float32) if x is None else np.array(x, dtype=np.float32), regions,
                                  bool(k.get("final", False))))
            return push(x, *a, **k)
        ms.push = spied
        opened.append(rec)
        return ms

    def mix_stereo(x, bed, regions=(), sample_rate=None, params=None, nodes=False):
        out = real_stereo(x, bed, regions, sample_rate=sample_rate, params=params, nodes=nodes)
        one_shot.append((np.array(x, dtype=np.float32), list(regions), out[1]))
        return out
    monkeypatch.setattr(synth._vocoder, "mix_stream", mix_stream)
    monkeypatch.setattr(synth._vocoder, "mix_stereo", mix_stereo)
    return opened, one_shot


def _whole(rec):
    """(programme, regions over it) of a recorded stream: its pushes laid end to end, the regions shifted back."""
    x = np.concatenate([p[0] for p in rec["pushes"]])
    regions, at = [], 0
    for xk, rk, _ in rec["pushes"]:
        for a, e, q in rk:
            if regions and regions[-1][1] == a + at and regions[-1][2] == q:
                regions[-1] = (regions[-1][0], e + at, q)
            else:
                regions.append((a + at, e + at, q))
        at += len(xk)
    return x, regions


def _live(synth, rec):
    x, regions = _whole(rec)
    return synth._vocoder.mix_live_stereo(x, rec["bed"], regions, sample_rate=rec["rate"], params=rec["params"])


@pytest.mark.parametrize("with_bed", [False, True], ids=["no-bed", "quiet-bed"])
def test_a_script_stream_concatenates_to_the_one_shot_stereo_call(synth, voices, default, spy, with_bed):
    opened, one_shot = spy
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, loudness=-23.0, silence_db=-30.0)
    bed = _bed(wav=_stereo_music(), level=-40.0, lead=0.013, tail=0.021, fade_out=0.01) if with_bed else None
    want_marks, marks = [], []
    want = synth.synthesize_script(_script(), voices, marks=want_marks, bed=bed, stereo=True, pans=PANS, **kw)
    chunks = list(synth.synthesize_script_stream(_script(), voices, marks=marks, live_bed=bed, live_stereo=True, live_pans=PANS, **kw))
    (rec,), ((x1, regions1, rep1),) = opened, one_shot
    y, rep = _live(synth, rec)
    print("one-shot", rep1, "live", rep)
    assert not rep1.capped and rep.limit_max == 0.0                              # neither ceiling bound: identity (b) applies
    x, regions = _whole(rec)
    assert np.array_equal(x, x1) and regions == regions1 and rec["stereo"] and rec["stream"]._h is None
    assert rep.n >= 2 * max(rec["params"].fade_in, rec["params"].fade_out) if with_bed else True
    r, ch, frames = _wav2(want)
    assert (r, ch) == (16000, 2) and all(chunks) and b"".join(chunks) == frames.tobytes() == _pack(y).tobytes()
    assert marks == want_marks and len(marks) == 4
    assert [q for _, _, q in regions] == [-50, 50, -50]                          # anna, ben, (the narrator: centre), anna
    assert rec["pushes"][0][0].size == 0 and rec["pushes"][-1][2] and (rec["bed"] is None) == (not with_bed)


def test_every_pan_zero_over_a_mono_bed_is_the_mono_live_bed_stream(synth, voices, default, spy):
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, silence_db=-30.0)
    bed = _bed(lead=0.01, tail=0.02)
    mono = b"".join(synth.synthesize_script_stream(_script(), voices, live_bed=bed, **kw))
    m = np.frombuffer(mono, dtype=np.int16)
    for extra in (dict(), dict(live_pans={"anna": 0.0, "ben": 0})):
        got = np.frombuffer(b"".join(synth.synthesize_script_stream(_script(), voices, live_bed=bed, live_stereo=True, **kw, **extra)),
                            dtype=np.int16).reshape(-1, 2)
        assert np.array_equal(got[:, 0], m) and np.array_equal(got[:, 1], m)
    assert [o["stereo"] for o in spy[0]] == [False, True, True] and all(not r for o in spy[0][1:] for _, r, _ in o["pushes"])


def test_a_loud_hard_left_voice_stays_under_the_ceiling_on_both_channels(synth, voices, default, spy):
    from fish_tts_amd import Line
    opened, _ = spy
    lines = [ln._replace(pan=-1.0, loudness=-8.0) for ln in _script()]
    bed = _bed(wav=_stereo_music(), level=-10.0, duck_db=0.0, lead=0.01, tail=0.01, fade_out=0.0)
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, silence_db=-30.0)
    chunks = list(synth.synthesize_script_stream(lines, voices, live_bed=bed, live_stereo=True, **kw))
    frames = np.frombuffer(b"".join(chunks), dtype=np.int16).reshape(-1, 2)
    y, rep = _live(synth, opened[0])
    print("live", rep, "largest", np.abs(frames).max(axis=0), "ceiling", CEILING)
    assert rep.limit_max > 0.0 and rep.peak > 10.0 ** (-1.0 / 20.0)              # the limiter had work to do
    assert np.abs(frames.astype(np.int32)).max() <= CEILING and frames.tobytes() == _pack(y).tobytes()
    assert isinstance(lines[0], Line) and all(q == -100 for _, r, _ in opened[0]["pushes"] for _, _, q in r)


def test_a_long_stream_at_a_place(synth, default, spy):
    opened, one_shot = spy
    kw = dict(references=default, max_tokens=MT, seed=SEED, silence_db=-30.0, loudness=-23.0)
    want = synth.synthesize_long(TEXT, stereo=True, pan=-0.5, **kw)
    chunks = list(synth.synthesize_long_stream(TEXT, live_stereo=True, live_pan=-0.5, **kw))
    y, rep = _live(synth, opened[0])
    assert not one_shot[0][2].capped and rep.limit_max == 0.0
    r, ch, frames = _wav2(want)
    assert (r, ch) == (44100, 2) and all(chunks) and b"".join(chunks) == frames.tobytes()
    x, regions = _whole(opened[0])
    assert regions == [(0, len(x), -50)] == one_shot[0][1]                       # one line over the piece, gaps included
    bed = _bed(wav=_stereo_music(), level=-40.0, lead=0.01, fade_out=0.01)
    want = synth.synthesize_long(TEXT, stereo=True, pan=0.3, bed=bed, **kw)
    got = b"".join(synth.synthesize_long_stream(TEXT, live_stereo=True, live_pan=0.3, live_bed=bed, **kw))
    assert not one_shot[1][2].capped and _live(synth, opened[1])[1].limit_max == 0.0
    assert got == _wav2(want)[2].tobytes()
    centre = b"".join(synth.synthesize_long_stream(TEXT, live_stereo=True, **kw))        # live_pan 0: the plain stream twice
    plain = np.frombuffer(b"".join(synth.synthesize_long_stream(TEXT, **kw)), dtype=np.int16)
    both = np.frombuffer(centre, dtype=np.int16).reshape(-1, 2)
    assert _live(synth, opened[2])[1].limit_max == 0.0 and np.array_equal(both[:, 0], plain) and np.array_equal(both[:, 1], plain)


def test_an_abandoned_generator_closes_its_stream(synth, voices, default, spy):
    opened, _ = spy
    kw = dict(references=default, max_tokens=MT, seed=SEED, sample_rate=16000, silence_db=-30.0)
    gen = synth.synthesize_script_stream(_script(), voices, live_stereo=True, live_pans=PANS, **kw)
    assert not opened                                     # opened at the first next()
    assert next(gen)
    assert opened[0]["stream"]._h is not None
    gen.close()
    assert opened[0]["stream"]._h is None and not any(final for _, _, final in opened[0]["pushes"])


def test_refusals_with_the_models_loaded(synth, voices, default):
    from fish_tts_amd import Line
    t = "Some text is here."
    with pytest.raises(ValueError, match="live_pans needs live_stereo"):
        synth.synthesize_script_stream([Line(t)], voices, references=default, live_pans={"anna": 0.5})
    with pytest.raises(ValueError, match="live_pan"):
        synth.synthesize_long_stream(t, references=default, live_pan=0.5)
    with pytest.raises(ValueError, match="stereo"):
        synth.synthesize_script_stream([Line(t, pan=0.5)], voices, references=default)
    with pytest.raises(ValueError, match="live_bed"):
        synth.synthesize_script_stream([Line(t)], voices, references=default, bed=_bed(), live_stereo=True)
