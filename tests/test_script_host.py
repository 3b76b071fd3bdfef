"""Host: the planning of a script (fish_tts_amd/script.py) - plan_script's segments, inheritance, gaps as exact sample
counts, the volume arithmetic and every refusal; parse_ssml's elements, nesting, breaks and refusals, and the round trip
from a hand-written list of Lines to its SSML and back; line_marks against the join's layout rule; the built library
exports the native call the feature stands on.  No GPU."""
import numpy as np
import pytest

from fish_tts_amd.script import Line, line_marks, parse_ssml, plan_script

TWO = "The first sentence is right here. And the second one follows it."
PARA = TWO + "\n\nA new paragraph begins with this."
VOICES = {"anna": [], "ben": []}


def _fx(plan):
    return [(f.rate, f.pct, f.cents, f.level, f.live) for f in plan.fx]


def test_segments_keep_their_order_and_their_lines_attributes():
    lines = [Line(TWO, voice="anna", speed=0.8), Line("Just one short sentence here."), Line(PARA, voice="ben", pitch=-2, loudness=-23)]
    p = plan_script(lines, VOICES, speed=1.25, pitch=1, loudness=-16)
    assert p.texts == ["The first sentence is right here.", "And the second one follows it.", "Just one short sentence here.",
                       "The first sentence is right here.", "And the second one follows it.", "A new paragraph begins with this."]
    assert p.line_of == [0, 0, 1, 2, 2, 2] and p.n_lines == 3
    assert p.voices == ["anna", "anna", None, "ben", "ben", "ben"]
    a, b, c = (None, 80, 100, -1600, None), (None, 125, 100, -1600, None), (None, 125, -200, -2300, None)
    assert _fx(p) == [a, a, b, c, c, c]
    assert p.rate == 44100 and len(p.gaps) == 6
    # a speed of 1.0 on the line undoes the call's, as OutputFx.of reads it
    assert _fx(plan_script([Line("Some text is here.", speed=1.0, pitch=0)], speed=1.5, pitch=3)) == [(None, None, None, None, None)]
    # a tuple of lines is a list of lines; an SSML string is parsed
    assert plan_script(tuple(lines), VOICES).texts == p.texts
    assert plan_script("<speak>Some text is here.</speak>").texts == ["Some text is here."]


@pytest.mark.parametrize("rate", [44100, 16000])
def test_gaps_are_exact_sample_counts(rate):
    def ms(x):
        return (x * rate + 500) // 1000
    lines = [Line(PARA, pause=1.0), Line(PARA), Line(TWO, pause=0.0135), Line("The last line of them all.", pause=0)]
    p = plan_script(lines, pause=0.2, paragraph_pause=0.5, line_pause=0.4, sample_rate=rate)
    assert p.rate == rate
    assert p.gaps == [ms(1000), ms(200), ms(500), ms(400), ms(200), ms(500), ms(14), ms(200), 0]
    if rate == 44100:
        assert p.gaps[:4] == [44100, 8820, 22050, 17640] and p.gaps[6] == 617
    else:
        assert p.gaps[:4] == [16000, 3200, 8000, 6400] and p.gaps[6] == 224
    p = plan_script(lines, pause=0.013, paragraph_pause=0, line_pause=5, sample_rate=rate)
    assert p.gaps == [ms(1000), ms(13), 0, ms(5000), ms(13), 0, ms(14), ms(13), 0]
    # the join parameters are synthesize_long's
    from fish_tts_amd.longform import join_params
    assert p.jp == join_params(None if rate == 44100 else rate, 0.013, 0, -45.0)[0]
    assert plan_script(lines, silence_db=None, sample_rate=rate).jp == join_params(None if rate == 44100 else rate, 0.2, 0.5, None)[0]


def test_volume_moves_the_effective_target():
    t = "Some text is here."
    assert _fx(plan_script([Line(t, loudness=-23, volume=3)]))[0][3] == -2000
    assert _fx(plan_script([Line(t, volume=-6.5)], loudness=-16))[0][3] == -2250
    assert _fx(plan_script([Line(t, loudness=-30, volume=-6.5)], loudness=-16))[0][3] == -3650      # the line's target wins
    assert _fx(plan_script([Line(t, volume=0)]))[0][3] is None and _fx(plan_script([Line(t, volume=0.0)], loudness=-16))[0][3] == -1600
    assert _fx(plan_script([Line(t, loudness=-10, volume=5)]))[0][3] == -500
    assert _fx(plan_script([Line(t, loudness=-45, volume=-5)]))[0][3] == -5000
    for bad in (Line(t, volume=3), Line(t, loudness=-10, volume=5.5), Line(t, loudness=-45, volume=-5.5), Line(t, volume="3"),
                Line(t, loudness=-20, volume=float("nan")), Line(t, loudness=-20, volume=float("inf")), Line(t, loudness=-20, volume=True)):
        with pytest.raises(ValueError, match="line 0"):
            plan_script([bad])
    with pytest.raises(ValueError, match="line 1"):
        plan_script([Line(t), Line(t, volume=12)], loudness=-16)


BAD_CALL = [dict(pause=-0.1), dict(pause=5.1), dict(paragraph_pause=None), dict(line_pause=-0.1), dict(line_pause=5.01),
            dict(line_pause=float("nan")), dict(line_pause="1"), dict(line_pause=None), dict(line_pause=True), dict(silence_db=0.5),
            dict(max_chars=15), dict(min_chars=-1), dict(sample_rate=12345), dict(speed=2.5), dict(pitch=12.5),
            dict(pitch=-1, speed=2.0), dict(loudness=-4), dict(voices=["anna"])]
BAD_LINE = [Line("x", voice="carl"), Line("x", speed=0.4), Line("x", speed="fast"), Line("x", pitch=13), Line("x", pitch=-1, speed=2.0),
            Line("x", loudness=-51), Line("x", loudness=0), Line("x", pause=-1), Line("x", pause=5.5), Line("x", pause="1"),
            Line(""), Line(" \n "), Line(7), "x", ("x",), None]


def test_every_refusal_is_a_value_error():
    t = "Some text is here."
    for bad in BAD_CALL:
        with pytest.raises(ValueError):
            plan_script([Line(t)], **bad)
    for bad in BAD_LINE:
        with pytest.raises(ValueError, match="line 1"):
            plan_script([Line(t), bad], VOICES)
    with pytest.raises(ValueError, match="unknown voice 'anna'"):
        plan_script([Line(t, voice="anna")])
    for empty in ([], (), "<speak> </speak>"):
        with pytest.raises(ValueError, match="empty script"):
            plan_script(empty)
    for not_a_script in (None, 7, Line(t), {"a": 1}):
        with pytest.raises(ValueError):
            plan_script(not_a_script)
    # a line's own good values are not disturbed by the call's being absent, and the other way round
    assert _fx(plan_script([Line(t, speed=2.0, pitch=1)])) == [(None, 200, 100, None, None)]
    with pytest.raises(ValueError, match="line 0"):
        plan_script([Line(t, speed=2.0)], pitch=-1)          # the pair is judged per line, the call's pitch inherited


def test_line_marks_follow_the_layout_rule():
    line_of, gaps = [0, 0, 1, 2, 2, 3], [7, 5, 11, 13, 3, 2]
    cuts = np.array([[0, 10], [2, 6], [0, 0], [0, 0], [1, 9], [0, 4]])
    marks = [None] * 4
    assert line_marks(line_of, gaps, cuts, marks) == (10 + 5 + 4 + 3 + 8 + 2 + 4, True)
    assert marks == [(0, 19), (19, 19), (22, 30), (32, 36)]
    # audio went out before: the first piece gets its gap; and group by group the result is the same
    marks = [None] * 4
    assert line_marks(line_of, gaps, cuts, marks, at=100, started=True) == (143, True)
    assert marks == [(107, 126), (126, 126), (129, 137), (139, 143)]
    marks, at, started = [None] * 4, 0, False
    for a, e in ((0, 1), (1, 4), (4, 6)):
        at, started = line_marks(line_of[a:e], gaps[a:e], cuts[a:e], marks, at, started)
    assert marks == [(0, 19), (19, 19), (22, 30), (32, 36)] and at == 36
    # a line that begins with empty pieces starts at its first audio; nothing at all: every line at zero
    marks = [None] * 2
    line_marks([0, 0, 1], [1, 1, 1], [[0, 0], [0, 5], [0, 0]], marks)
    assert marks == [(0, 5), (5, 5)]
    marks = [None] * 2
    assert line_marks([0, 1], [9, 9], [[0, 0], [3, 3]], marks) == (0, False) and marks == [(0, 0), (0, 0)]


def test_ssml_elements_and_attribute_forms():
    assert parse_ssml("<speak>Hello  there.\n How are you?</speak>") == [Line("Hello there. How are you?")]
    assert parse_ssml('<speak version="1.1" xml:lang="en-US" xmlns="http://www.w3.org/2001/10/synthesis"><s>One.</s><s>Two.</s></speak>') \
        == [Line("One. Two.")]
    assert parse_ssml("<speak><p>One para.</p><p>Another  one.</p>tail</speak>") == [Line("One para.\n\nAnother one.\n\ntail")]
    assert parse_ssml('<speak>a<voice name="anna">b</voice>c</speak>') == [Line("a"), Line("b", voice="anna"), Line("c")]
    for value, seconds in (("500ms", 0.5), ("2s", 2.0), ("1.5s", 1.5), ("0ms", 0.0), ("13.5ms", 0.0135)):
        assert parse_ssml(f'<speak>a<break time="{value}"/>b</speak>') == [Line("a"), Line("b", pause=seconds)]
    for value, seconds in (("none", 0.0), ("x-weak", 0.1), ("weak", 0.2), ("medium", 0.35), ("strong", 0.6), ("x-strong", 1.0)):
        assert parse_ssml(f'<speak>a<break strength="{value}"/>b</speak>') == [Line("a"), Line("b", pause=seconds)]
    assert parse_ssml("<speak>a<break/>b</speak>") == [Line("a"), Line("b", pause=0.35)]
    for value, speed in (("80%", 0.8), ("125%", 1.25), ("100%", 1.0), ("x-slow", 0.6), ("slow", 0.8), ("medium", 1.0), ("fast", 1.25),
                         ("x-fast", 1.6)):
        assert parse_ssml(f'<speak><prosody rate="{value}">a</prosody></speak>') == [Line("a", speed=speed)]
    for value, st in (("+2st", 2.0), ("-3.5st", -3.5), ("2st", 2.0), ("+1 st", 1.0), ("x-low", -4.0), ("low", -2.0), ("medium", 0.0),
                      ("high", 2.0), ("x-high", 4.0)):
        assert parse_ssml(f'<speak><prosody pitch="{value}">a</prosody></speak>') == [Line("a", pitch=st)]
    for value, db in (("+6dB", 6.0), ("-3.5dB", -3.5), ("0dB", 0.0), ("-2 dB", -2.0)):
        assert parse_ssml(f'<speak><prosody volume="{value}">a</prosody></speak>') == [Line("a", volume=db)]


def test_ssml_nesting_and_breaks():
    got = parse_ssml('<speak><prosody rate="slow" pitch="high">a <prosody pitch="low" volume="-3dB">b</prosody> c</prosody> d</speak>')
    assert got == [Line("a", speed=0.8, pitch=2.0), Line("b", speed=0.8, pitch=-2.0, volume=-3.0), Line("c", speed=0.8, pitch=2.0),
                   Line("d")]
    got = parse_ssml('<speak><voice name="anna">a<prosody rate="fast">b<voice name="ben">c</voice></prosody></voice></speak>')
    assert got == [Line("a", voice="anna"), Line("b", voice="anna", speed=1.25), Line("c", voice="ben", speed=1.25)]
    # a break sets the NEXT line's pause, also across an element's end and in front of the first line; breaks in a row add up
    got = parse_ssml('<speak><break time="1s"/>a<voice name="anna">b<break time="250ms"/></voice>'
                     '<break strength="weak"/>c<break time="3s"/></speak>')
    assert got == [Line("a", pause=1.0), Line("b", voice="anna"), Line("c", pause=0.45)]
    # a stretch without text gives no line, and a paragraph inside a voice stays inside its line
    got = parse_ssml('<speak> <voice name="anna"> </voice><voice name="ben"><p>x</p><p>y</p></voice></speak>')
    assert got == [Line("x\n\ny", voice="ben")]


SSML_BAD = [
    ('<!DOCTYPE speak [<!ENTITY a "b">]><speak>&a;</speak>', "DOCTYPE"),
    ("<speak>unclosed", "malformed"),
    ("<talk>x</talk>", "<talk>"),
    ("<speak><emphasis>x</emphasis></speak>", "<emphasis>"),
    ("<speak><audio src='x'/></speak>", "<audio>"),
    ('<speak rate="fast">x</speak>', "'rate'"),
    ('<speak><voice>x</voice></speak>', "name"),
    ('<speak><voice name="a" gender="f">x</voice></speak>', "'gender'"),
    ('<speak><p align="left">x</p></speak>', "'align'"),
    ('<speak><break time="1m"/></speak>', "'1m'"),
    ('<speak><break time="-1s"/></speak>', "'-1s'"),
    ('<speak><break strength="huge"/></speak>', "'huge'"),
    ('<speak><break time="1s">x</break></speak>', "empty"),
    ('<speak><break duration="1s"/></speak>', "'duration'"),
    ('<speak><prosody rate="quick">x</prosody></speak>', "'quick'"),
    ('<speak><prosody rate="-10%">x</prosody></speak>', "'-10%'"),
    ('<speak><prosody pitch="+10Hz">x</prosody></speak>', "'+10Hz'"),
    ('<speak><prosody pitch="tall">x</prosody></speak>', "'tall'"),
    ('<speak><prosody volume="loud">x</prosody></speak>', "'loud'"),
    ('<speak><prosody volume="6">x</prosody></speak>', "'6'"),
    ('<speak><prosody contour="(0%,+20Hz)">x</prosody></speak>', "'contour'"),
]


@pytest.mark.parametrize("text,offender", SSML_BAD, ids=[o for _, o in SSML_BAD])
def test_ssml_refusals_name_the_offender(text, offender):
    with pytest.raises(ValueError, match=offender.replace("+", r"\+").replace("(", r"\(")):
        parse_ssml(text)
    with pytest.raises(ValueError):
        plan_script(text)
    with pytest.raises(ValueError):
        parse_ssml(text.encode())


def test_a_hand_written_script_and_its_ssml_give_the_same_lines():
    lines = [Line("Once upon a time, there was a narrator."),
             Line("Hello! I am Anna.\n\nI speak two paragraphs.", voice="anna"),
             Line("And I am slow and low.", voice="ben", speed=0.8, pitch=-2.0, pause=0.5),
             Line("An aside, quietly.", speed=0.8, volume=-6.0),
             Line("The end.", pause=2.0)]
    ssml = ('<speak>Once upon a time,\n   there was a narrator.'
            '<voice name="anna"><p>Hello! I am Anna.</p><p>I speak two paragraphs.</p></voice>'
            '<break time="500ms"/><voice name="ben"><prosody rate="slow" pitch="low">And I am slow and low.</prosody></voice>'
            '<prosody rate="80%"><prosody volume="-6dB">An aside, quietly.</prosody></prosody>'
            '<break time="2s"/>The end.</speak>')
    assert parse_ssml(ssml) == lines
    kw = dict(voices=VOICES, loudness=-20, sample_rate=16000, line_pause=0.3)
    assert plan_script(ssml, **kw) == plan_script(lines, **kw)


def test_the_library_exports_the_per_item_join():
    import ctypes
    from fish_tts_amd import _lib as L
    assert "ft_codec_decode_join_items" in L.SYMBOLS
    lib = ctypes.CDLL(L.LIB_PATH)
    assert lib.ft_codec_decode_join_items is not None
    assert ctypes.sizeof(L.ft_item_fx) == 12
