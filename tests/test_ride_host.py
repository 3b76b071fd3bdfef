"""CPU: the host side of live_loudness= - OutputFx with the new field, the refusal of both keywords together, no_level
untouched, batch_stream.checked_fx, and synthesize_stream(seamless=False, live_loudness=...) raising before any work."""
import inspect

import numpy as np
import pytest


def test_output_fx_live_loudness():
    from fish_tts_amd.codec_engine import OutputFx
    fx = OutputFx.of(live_loudness=-16)
    assert fx.live == -1600 and fx.level is None and fx.rate is None and fx.pct is None and fx.cents is None
    assert bool(fx) and fx.native == (44100, 100, 0) and fx.native_live == -1600 and fx.native_level == 0 and fx.kw == {"fx": fx}
    assert not fx.emits_empty and OutputFx.of(sample_rate=16000).emits_empty and OutputFx.of().emits_empty
    assert OutputFx.of(live_loudness=-23.456).live == -2346
    assert OutputFx.of(live_loudness=-50).live == -5000 and OutputFx.of(live_loudness=-5.0).live == -500
    assert OutputFx.of(live_loudness=np.float32(-20)).live == -2000
    plain = OutputFx.of()
    assert plain.live is None and not plain and plain.native_live == 0 and plain == OutputFx.of(live_loudness=None)
    assert OutputFx.of(16000, 1.25, 3, live_loudness=-20) == OutputFx(16000, 125, 300, None, -2000)
    assert OutputFx.of(16000, 1.25, 3).native == OutputFx.of(16000, 1.25, 3, live_loudness=-20).native
    # the positional meaning of the four older fields stays
    old = OutputFx(16000, 125, 300, -2000)
    assert old.level == -2000 and old.live is None and old.native == (16000, 125, 300) and old.native_level == -2000
    assert list(inspect.signature(OutputFx.of).parameters)[-1] == "live_loudness"
    assert [f for f in OutputFx.__dataclass_fields__][-1] == "live"
    for bad in (-50.01, -4.99, 0, 16, float("nan"), float("inf"), True, "loud", [-16]):
        with pytest.raises(ValueError):
            OutputFx.of(live_loudness=bad)


def test_both_keywords_together_are_refused():
    from fish_tts_amd.codec_engine import OutputFx
    with pytest.raises(ValueError, match="not both"):
        OutputFx.of(loudness=-16, live_loudness=-16)
    with pytest.raises(ValueError, match="not both"):
        OutputFx.of(16000, 1.25, 3, -20, -23)


def test_no_level_is_untouched_and_no_live_refuses():
    from fish_tts_amd.codec_engine import OutputFx
    live = OutputFx.of(live_loudness=-16)
    assert live.no_level("a stream") is live
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        OutputFx.of(loudness=-16).no_level("a stream")
    with pytest.raises(ValueError, match="rides a stream"):
        live.no_live()
    level = OutputFx.of(loudness=-16)
    assert level.no_live() is level


def test_checked_fx_takes_the_keyword():
    from fish_tts_amd.batch_stream import checked_fx
    from fish_tts_amd.codec_engine import OutputFx
    assert checked_fx(None, 16000, 1.25, 3, live_loudness=-20) == OutputFx(16000, 125, 300, None, -2000)
    assert checked_fx(None, 16000, 1.25, 3, -20) == OutputFx(16000, 125, 300, -2000)
    fx = OutputFx.of(live_loudness=-20)
    assert checked_fx(fx, live_loudness=-30) is fx
    with pytest.raises(ValueError):
        checked_fx(None, live_loudness=-4)
    with pytest.raises(ValueError, match="not both"):
        checked_fx(None, loudness=-20, live_loudness=-20)
    assert list(inspect.signature(checked_fx).parameters) == ["fx", "sample_rate", "speed", "pitch", "loudness", "live_loudness"]


def test_stream_utterances_checks_before_it_starts_a_thread():
    from fish_tts_amd.batch_stream import stream_utterances

    def run(on_frames, on_done):
        raise AssertionError("work was started")
    with pytest.raises(ValueError):
        next(stream_utterances(run, 1, None, live_loudness=-4))
    assert "live_loudness" in inspect.signature(stream_utterances).parameters


def test_unseamless_stream_with_a_live_loudness_raises_before_any_work():
    from fish_tts_amd.synthesizer import FishTTS
    synth = object.__new__(FishTTS)           # no engines: the check comes before the first use of any

    def no_work(*a, **k):
        raise AssertionError("work was started")
    synth._get_prompt_data = no_work
    synth._server = None
    for kw in (dict(), dict(seamless=False)):
        gen = synth.synthesize_stream("x", live_loudness=-16, **kw)          # a generator: nothing has run yet
        with pytest.raises(ValueError, match="seamless=True"):
            next(gen)
    with pytest.raises(ValueError, match="not both"):
        next(synth.synthesize_stream("x", seamless=True, loudness=-16, live_loudness=-16))
    with pytest.raises(ValueError):
        next(synth.synthesize_stream("x", seamless=True, live_loudness=-4))
    with pytest.raises(ValueError, match="loudness needs the whole utterance"):
        next(synth.synthesize_stream("x", seamless=True, loudness=-16))
