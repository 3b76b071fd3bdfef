"""Scripts, host side: a dialogue or a narrated piece as a list of Lines - each with its own voice, pace, pitch, level and
pause - for FishTTS.synthesize_script.  plan_script cuts every line into segments (longform.split_text), hands each its
line's attributes, its gap and its checked output stages; parse_ssml reads the same list from an SSML subset; line_marks
turns what the join reports into line timestamps.  Plain Python: neither torch nor the native library is imported here
(the output stages are judged by codec_engine.OutputFx.of, imported when plan_script runs, as the synthesizer does).

The reference speaks one text in one voice (fish_tts/synthesizer.py:431-481) and has nothing of the kind."""
from __future__ import annotations

import math
import re
from numbers import Real
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

from .longform import JoinParams, _seconds, join_params, split_text


class Line(NamedTuple):
    text: str
    voice: Optional[str] = None        # a key of `voices`; None: the call's references / set_references
    speed: Optional[float] = None      # None: the call's
    pitch: Optional[float] = None      # semitones; None: the call's
    loudness: Optional[float] = None   # LUFS target of this line; None: the call's
    volume: float = 0.0                # dB, added to the effective target
    pause: Optional[float] = None      # s of silence before the line; None: line_pause
    pan: Optional[float] = None        # [-1, 1], -1 hard left (stereo=True alone); None: the voice's in `pans`, else the centre


class ScriptPlan(NamedTuple):
    texts: List[str]                   # the segments of all lines, in order
    line_of: List[int]                 # the line every segment came from
    voices: List[Optional[str]]        # every segment's voice (its line's)
    fx: list                           # every segment's checked output stages (codec_engine.OutputFx), one rate throughout
    gaps: List[int]                    # samples of silence before every segment, at the output rate
    jp: JoinParams
    rate: int                          # the output rate (Hz)
    n_lines: int
    pans: Optional[List[int]] = None   # stereo: every line's pan in hundredths, -100 hard left (the stereo mix stage's)
    sends: Optional[List[int]] = None  # room: every line's send in hundredths of a dB of attenuation, -1 muted (the room stage's)


MAX_PAN_REGIONS = 4096                 # ft_codec_mix_stereo


def native_pan(name: str, v) -> int:
    """round(100 pan) of a pan in [-1, 1]; ValueError for anything else (a bool, a NaN)."""
    if isinstance(v, bool) or not isinstance(v, Real) or not -1.0 <= float(v) <= 1.0:       # (a nan fails)
        raise ValueError(f"{name} must be a number in [-1, 1] (-1 hard left), got {v!r}")
    return int(round(100.0 * float(v)))


def pan_regions(pans: Sequence[int], marks: Sequence) -> List[Tuple[int, int, int]]:
    """The stereo mix stage's regions (a, e, pan) from every line's pan and its mark (line_marks, before a bed's lead is
    added): one per line that has audio and a pan other than 0; a line's region is merged into that of the line before it where
    both have the same pan (the silence between them goes along, and a line without audio separates nothing)."""
    out: List[Tuple[int, int, int]] = []
    before = 0                          # the pan of the last line that had audio
    for pan, m in zip(pans, marks):
        if m is None or m[1] <= m[0]:
            continue
        if pan != 0:
            if out and before == pan:
                out[-1] = (out[-1][0], int(m[1]), pan)
            else:
                out.append((int(m[0]), int(m[1]), pan))
        before = pan
    return out


def push_regions(pans: Sequence[int], line_of: Sequence[int], gaps: Sequence[int], cuts, at: int = 0, started: bool = False,
                 before: int = 0):
    """The live stereo mix stage's regions for ONE joined group of a stream - segments of lines `line_of` behind `gaps`, kept
    as `cuts` says, beginning at sample `at` of the programme with `started` saying whether audio went out before it and
    `before` the pan of the last line that had audio by then.  The group's marks (line_marks) go through pan_regions; they
    are then relative to the push: shifted by `at` and clipped to the group.  Where the group's first line with audio sits
    where `before` did - the line continues from the group before, or follows a line of equal pan - its region begins with
    the group, so the silence in front of it goes along as pan_regions has it for the whole piece.  The regions of all groups,
    shifted back and touching ones of equal pan joined, are pan_regions of the final marks.
    Returns (regions, at, started, before) after the group."""
    found: list = [None] * len(pans)
    end, started_after = line_marks(line_of, gaps, cuts, found, at, started)
    spoken = [j for j in sorted(set(line_of)) if found[j] is not None and found[j][1] > found[j][0]]
    regions = pan_regions(pans, found)
    if spoken and regions and pans[spoken[0]] == before != 0:
        regions[0] = (at, regions[0][1], before)
    out = [(max(a, at) - at, min(e, end) - at, q) for a, e, q in regions if max(a, at) < min(e, end)]
    return out, end, started_after, (pans[spoken[-1]] if spoken else before)


def _samples(ms: int, rate: int) -> int:
    return (ms * rate + 500) // 1000


def plan_script(lines, voices: Optional[Dict[str, list]] = None, pause=0.2, paragraph_pause=0.5,
                line_pause=0.4, silence_db: Optional[float] = -45.0, max_chars: int = 200, min_chars: int = 24,
                sample_rate: Optional[int] = None, speed=None, pitch=None, loudness=None, stereo: bool = False,
                pans: Optional[Dict[str, float]] = None, room: bool = False,
                sends: Optional[Dict[str, float]] = None) -> ScriptPlan:
    """Every check of a script - `lines` a list of Line, or an SSML string (parse_ssml) - and its segments.  Each line is
    split on its own (split_text) and its segments inherit its voice and its output stages: `speed`, `pitch` and `loudness` are the line's, or the call's where the line has None; the
    line's `volume` (dB) is added to that loudness target, which must then exist and stay in [-50, -5].  Every value is
    judged by OutputFx.of, the code that judges it for every other call.  Gaps: inside a line `pause`, or `paragraph_pause`
    after a paragraph break, as join_params gives them; the first segment of a line takes the line's `pause`, or
    `line_pause` (the same range and rounding: [0, 5] s, whole milliseconds) - the join drops the gap before the script's
    first audio, as ever.  `stereo`: every line gets a place - its `pan`, else its voice's in `pans` (voice name -> pan),
    else the centre - as ScriptPlan.pans; without it a `pan` or `pans` is refused.  ValueError: no line, a line that is no Line
    or has nothing to speak, a voice that `voices` does not hold, a bad value anywhere, a `pans` key that is no voice of the
    call, more than 4096 runs of lines at one place other than the centre.  `room`: the call has a room - every line gets a send
    into it from `sends`, a dict whose keys are voice names or line indices (-> dB in [-60, 0], -inf muted): the line's own
    entry (its index), else its voice's, else 0 dB, as ScriptPlan.sends; without a room `sends` is refused; a key that is
    neither a voice of the call nor the index of a line is refused, and the limit of `pans` holds for the runs of sends."""
    from .codec_engine import OutputFx
    from .room import MAX_SEND_REGIONS, native_send
    if isinstance(lines, str):
        lines = parse_ssml(lines)
    call_fx = OutputFx.of(sample_rate, speed, pitch, loudness)          # the call's own values first
    jp, gap, pgap = join_params(call_fx.rate, pause, paragraph_pause, silence_db)
    rate = call_fx.wav_rate
    lgap = _samples(_seconds("line_pause", line_pause), rate)
    if isinstance(lines, Line) or not isinstance(lines, (list, tuple)):
        raise ValueError(f"a script is a list of Line or an SSML string, got {type(lines).__name__}")
    if not lines:
        raise ValueError("an empty script: no line to speak")
    if voices is not None and not isinstance(voices, dict):
        raise ValueError("voices must be a dict of name -> list of VoiceProfile")
    if not isinstance(stereo, bool):
        raise ValueError(f"stereo must be True or False, got {stereo!r}")
    if pans is not None:
        if not stereo:
            raise ValueError("pans needs stereo=True: a mono piece has no left and right")
        if not isinstance(pans, dict):
            raise ValueError("pans must be a dict of voice name -> pan")
        for name in pans:
            if voices is None or name not in voices:
                raise ValueError(f"pans: {name!r} is no voice of this call")
        pans = {name: native_pan(f"pans[{name!r}]", v) for name, v in pans.items()}
    if not isinstance(room, bool):
        raise ValueError(f"room must be True or False, got {room!r}")
    if sends is not None:
        if not room:
            raise ValueError("sends needs room=: without a room there is nothing to send to")
        if not isinstance(sends, dict):
            raise ValueError("sends must be a dict of voice name -> send in dB")
        for name in sends:
            if isinstance(name, int) and not isinstance(name, bool):
                if not 0 <= name < len(lines):
                    raise ValueError(f"sends: {name} is no line of this script (it has {len(lines)})")
            elif voices is None or name not in voices:
                raise ValueError(f"sends: {name!r} is neither a voice of this call nor a line index")
        sends = {name: native_send(f"sends[{name!r}]", v) for name, v in sends.items()}
    plan = ScriptPlan([], [], [], [], [], jp, rate, len(lines), [] if stereo else None, [] if room else None)
    for j, ln in enumerate(lines):
        if not isinstance(ln, Line):
            raise ValueError(f"line {j}: expected a Line, got {type(ln).__name__}")
        if ln.voice is not None and (voices is None or ln.voice not in voices):
            raise ValueError(f"line {j}: unknown voice {ln.voice!r}" +
                             (f" (voices: {sorted(map(str, voices))})" if voices else " (no voices were given)"))
        if ln.pan is not None and not stereo:
            raise ValueError(f"line {j}: pan={ln.pan!r} needs stereo=True (the streams are mono)")
        if stereo:
            plan.pans.append(native_pan(f"line {j}: pan", ln.pan) if ln.pan is not None else (pans or {}).get(ln.voice, 0))
        if room:
            plan.sends.append((sends or {}).get(j, (sends or {}).get(ln.voice, 0) if ln.voice is not None else 0))
        target = loudness if ln.loudness is None else ln.loudness
        if isinstance(ln.volume, bool) or not isinstance(ln.volume, Real) or not math.isfinite(float(ln.volume)):
            raise ValueError(f"line {j}: volume must be a number of dB, got {ln.volume!r}")
        if float(ln.volume) != 0.0:
            if target is None:
                raise ValueError(f"line {j}: volume={ln.volume!r} needs a loudness target to move, the line's or the call's")
            if isinstance(target, bool) or not isinstance(target, Real):
                raise ValueError(f"line {j}: loudness must be a number of LUFS, got {target!r}")
            target = float(target) + float(ln.volume)
        try:
            fx = OutputFx.of(sample_rate, speed if ln.speed is None else ln.speed, pitch if ln.pitch is None else ln.pitch, target)
            first = lgap if ln.pause is None else _samples(_seconds("pause", ln.pause), rate)
            segs = split_text(ln.text, max_chars, min_chars)
        except ValueError as e:
            raise ValueError(f"line {j}: {e}") from None
        for k, seg in enumerate(segs):
            plan.texts.append(seg.text)
            plan.line_of.append(j)
            plan.voices.append(ln.voice)
            plan.fx.append(fx)
            plan.gaps.append(first if k == 0 else pgap if seg.paragraph else gap)
    if stereo:
        runs = sum(1 for j, q in enumerate(plan.pans) if q != 0 and (j == 0 or plan.pans[j - 1] != q))
        if runs > MAX_PAN_REGIONS:
            raise ValueError(f"{runs} pan regions after merging: the stereo mix stage takes {MAX_PAN_REGIONS} (split the script)")
    if room:
        runs = sum(1 for j, q in enumerate(plan.sends) if q != 0 and (j == 0 or plan.sends[j - 1] != q))
        if runs > MAX_SEND_REGIONS:
            raise ValueError(f"{runs} send regions after merging: the room stage takes {MAX_SEND_REGIONS} (split the script)")
    return plan


def line_marks(line_of: Sequence[int], gaps: Sequence[int], cuts, marks: Optional[list] = None, at: int = 0,
               started: bool = False) -> Tuple[int, bool]:
    """Line timestamps from what the join reports, by its stated layout rule off_b = sum_{c<b} (G_c + m_c): segment b kept
    m_b = e_b - a_b samples behind G_b = gaps[b] samples of silence (none for an empty piece, none before the first audio).
    `marks` (one entry per line, None where a line has not begun) receives (start_sample, end_sample) of every line that has a
    segment here - the span from its first non-empty piece to the end of its last, (at, at) for a line whose pieces are
    all empty; `at`, `started`: where this group of segments begins in the output, and whether audio went out before it.
    Returns (at, started) after the group."""
    for b, (j, g) in enumerate(zip(line_of, gaps)):
        m = int(cuts[b][1]) - int(cuts[b][0])
        if m > 0:
            if started:
                at += int(g)
            start, at, started = at, at + m, True
            if marks is not None:
                marks[j] = (start, at) if marks[j] is None or marks[j][0] == marks[j][1] else (marks[j][0], at)
        elif marks is not None and marks[j] is None:
            marks[j] = (at, at)
    return at, started


# ---- SSML subset
BREAK_STRENGTH = {"none": 0.0, "x-weak": 0.1, "weak": 0.2, "medium": 0.35, "strong": 0.6, "x-strong": 1.0}
PROSODY_RATE = {"x-slow": 0.6, "slow": 0.8, "medium": 1.0, "fast": 1.25, "x-fast": 1.6}
PROSODY_PITCH = {"x-low": -4.0, "low": -2.0, "medium": 0.0, "high": 2.0, "x-high": 4.0}
_NUM = r"(\d+(?:\.\d*)?|\.\d+)"
_TIME = re.compile(rf"^{_NUM}(ms|s)$")
_PCT = re.compile(rf"^\+?{_NUM}%$")
_ST = re.compile(rf"^([+-]?){_NUM}\s*st$")
_DB = re.compile(rf"^([+-]?){_NUM}\s*dB$")
_SPEAK_ATTRS = ("version", "{http://www.w3.org/XML/1998/namespace}lang")


def _signed(m) -> float:
    return -float(m.group(2)) if m.group(1) == "-" else float(m.group(2))


def _attrs(el, tag: str, allowed: Sequence[str]) -> dict:
    for a in el.attrib:
        if a not in allowed:
            raise ValueError(f"SSML: unsupported attribute {a!r} on <{tag}>")
    return el.attrib


def _break_seconds(el) -> float:
    a = _attrs(el, "break", ("time", "strength"))
    if (el.text or "").strip() or len(el):
        raise ValueError("SSML: <break> must be empty")
    if "time" in a:
        m = _TIME.match(a["time"].strip())
        if not m:
            raise ValueError(f"SSML: unsupported <break time={a['time']!r}>: a number followed by ms or s")
        if "strength" in a and a["strength"] not in BREAK_STRENGTH:
            raise ValueError(f"SSML: unsupported <break strength={a['strength']!r}>: one of {', '.join(BREAK_STRENGTH)}")
        return float(m.group(1)) / 1000.0 if m.group(2) == "ms" else float(m.group(1))
    s = a.get("strength", "medium")
    if s not in BREAK_STRENGTH:
        raise ValueError(f"SSML: unsupported <break strength={s!r}>: one of {', '.join(BREAK_STRENGTH)}")
    return BREAK_STRENGTH[s]


def _prosody(el, state: dict) -> dict:
    a = _attrs(el, "prosody", ("rate", "pitch", "volume"))
    new = dict(state)
    if "rate" in a:
        v = a["rate"].strip()
        m = _PCT.match(v)
        if not m and v not in PROSODY_RATE:
            raise ValueError(f"SSML: unsupported <prosody rate={v!r}>: N% or one of {', '.join(PROSODY_RATE)}")
        new["speed"] = float(m.group(1)) / 100.0 if m else PROSODY_RATE[v]
    if "pitch" in a:
        v = a["pitch"].strip()
        m = _ST.match(v)
        if not m and v not in PROSODY_PITCH:
            raise ValueError(f"SSML: unsupported <prosody pitch={v!r}>: +Nst / -Nst or one of {', '.join(PROSODY_PITCH)}")
        new["pitch"] = _signed(m) if m else PROSODY_PITCH[v]
    if "volume" in a:
        v = a["volume"].strip()
        m = _DB.match(v)
        if not m:
            raise ValueError(f"SSML: unsupported <prosody volume={v!r}>: +NdB / -NdB")
        new["volume"] = _signed(m)
    return new


def parse_ssml(text: str) -> List[Line]:
    """The Lines of an SSML document, as a user would write them by hand.  The subset: <speak> (the root; `version` and
    `xml:lang` are accepted and ignored), <p> (a paragraph break inside a line), <s>, <voice name>, <break time="Nms|Ns">
    or <break strength> (BREAK_STRENGTH; a bare <break/> is medium), <prosody rate> (N% or PROSODY_RATE), <prosody pitch>
    (+Nst / -Nst or PROSODY_PITCH), <prosody volume> (+NdB / -NdB).  A change of voice or prosody - entering or leaving
    such an element - or a break starts a new Line; a break sets the next line's `pause` (breaks in a row add up); nested
    <prosody> compose, the innermost winning per attribute; a stretch without text gives no line.  A line's text is its
    paragraphs, whitespace collapsed, separated by a blank line.  ValueError naming the offender: a DOCTYPE, malformed
    XML, another root, any other element, attribute or attribute value, a <voice> without a name."""
    import xml.etree.ElementTree as ET
    if not isinstance(text, str):
        raise ValueError(f"SSML: expected a string, got {type(text).__name__}")
    if "<!doctype" in text.lower() or "<!entity" in text.lower():
        raise ValueError("SSML: a DOCTYPE is not accepted")
    try:
        root = ET.fromstring(text)
    except ET.ParseError as e:
        raise ValueError(f"SSML: malformed XML: {e}") from None

    def local(el) -> str:
        return el.tag.rsplit("}", 1)[-1] if isinstance(el.tag, str) else repr(el.tag)

    if local(root) != "speak":
        raise ValueError(f"SSML: the root must be <speak>, got <{local(root)}>")
    _attrs(root, "speak", _SPEAK_ATTRS)
    lines: List[Line] = []
    paragraphs: List[List[str]] = [[]]
    pending: List[Optional[float]] = [None]

    def flush(state: dict) -> None:
        body = "\n\n".join(p for p in (" ".join(" ".join(q).split()) for q in paragraphs) if p)
        paragraphs[:] = [[]]
        if body:
            lines.append(Line(body, state["voice"], state["speed"], state["pitch"], None, state["volume"], pending[0]))
            pending[0] = None

    def walk(el, state: dict) -> None:
        if el.text:
            paragraphs[-1].append(el.text)
        for child in el:
            tag = local(child)
            if tag == "break":
                flush(state)
                pending[0] = (pending[0] or 0.0) + _break_seconds(child)
            elif tag in ("p", "s"):
                _attrs(child, tag, ())
                for _ in range(2):           # a paragraph break, or a sentence's white space, on either side
                    if tag == "p":
                        paragraphs.append([])
                    else:
                        paragraphs[-1].append(" ")
                    if _ == 0:
                        walk(child, state)
            elif tag == "voice":
                a = _attrs(child, "voice", ("name",))
                if not a.get("name"):
                    raise ValueError("SSML: <voice> needs a name")
                flush(state)
                inner = dict(state, voice=a["name"])
                walk(child, inner)
                flush(inner)
            elif tag == "prosody":
                inner = _prosody(child, state)
                flush(state)
                walk(child, inner)
                flush(inner)
            else:
                raise ValueError(f"SSML: unsupported element <{tag}>")
            if child.tail:
                paragraphs[-1].append(child.tail)

    top = dict(voice=None, speed=None, pitch=None, volume=0.0)
    walk(root, top)
    flush(top)
    return lines
