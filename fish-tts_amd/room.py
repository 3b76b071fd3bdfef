"""Convolution reverb, host side: a Room - the impulse response of a space, as a WAV - for `room=` of
FishTTS.synthesize_long / synthesize_script and for FishTTS.reverb.  room_params is the one place where a Room's seconds and
dB become the integers of ft_room_params (include/fishtts_hip.h: "Room"), each checked; send_regions turns a script's
per-line sends into the stage's regions; CodecHipEngine.room takes both as they are.  Plain Python: neither torch nor the
native library is imported here.

The reference has nothing of the kind."""
from __future__ import annotations

import math
from numbers import Real
from typing import List, NamedTuple, Optional, Sequence, Tuple

MAX_SECONDS = 600.0             # length, fade, offset, tail
MAX_DB = 60.0                   # wet, dry and the sends: attenuations in [0, 60] dB, hundredths of a dB natively
MAX_SEND_REGIONS = 4096         # ft_codec_room
MAX_TAPS = 131072               # the impulse response at the output rate, after `offset` and `length`
MUTED = -1                      # the native send of a muted line, the native dry of a call without a dry signal


class Room(NamedTuple):
    wav: object                            # WAV bytes, or a path to a WAV file (any format the reference intake reads)
    wet_db: float = -12.0                  # the level of the reverberated signal, dB in [-60, 0]
    dry_db: Optional[float] = 0.0          # the level of the programme itself, dB in [-60, 0]; None: no dry signal
    predelay: float = 0.0                  # s before the room answers, [0, 1]
    length: Optional[float] = None         # s of the response used; None: all of it (131072 taps at most: choose a length)
    fade: float = 0.05                     # s over which the used response fades out at its end
    offset: float = 0.0                    # s into the response at which it starts (the direct sound's delay cut away)
    tail: Optional[float] = None           # s the piece rings on after the programme; None: all of it
    normalize: bool = True                 # scale the response to unit energy, so that wet_db means the same for every room
    channel: Optional[int] = None          # that channel alone; None: the mean of all


class RoomParams(NamedTuple):
    """A Room's values as ft_room_params takes them, at one output rate (ceiling is the call's: CodecHipEngine.room)."""
    channel: int           # -1: the mean of all channels
    normalize: int
    wet: int               # hundredths of a dB of attenuation
    dry: int               # ... or -1: no dry signal
    send: int              # outside every region: 0 (a script's lines bring their own)
    offset: int            # samples, as length (0: all), fade, predelay, tail (-1: all)
    length: int
    fade: int
    predelay: int
    tail: int


def _real(name: str, v, lo: float, hi: float, unit: str) -> float:
    if isinstance(v, bool) or not isinstance(v, Real) or not lo <= float(v) <= hi:       # (a nan fails)
        raise ValueError(f"room: {name} must be a number of {unit} in [{lo:g}, {hi:g}], got {v!r}")
    return float(v)


def _samples(name: str, v, rate: int, hi: float = MAX_SECONDS) -> int:
    return int(round(_real(name, v, 0.0, hi, "seconds") * rate))


def native_send(name: str, v) -> int:
    """round(-100 dB) of a send in [-60, 0] dB, -1 (muted) for -inf; ValueError for anything else (a bool, a NaN)."""
    if not isinstance(v, bool) and isinstance(v, Real) and float(v) == -math.inf:
        return MUTED
    if isinstance(v, bool) or not isinstance(v, Real) or not -MAX_DB <= float(v) <= 0.0:
        raise ValueError(f"{name} must be a number of dB in [-60, 0], or -inf for muted, got {v!r}")
    return int(round(-100.0 * float(v)))


def room_params(room: Room, rate: int) -> RoomParams:
    """Every check of a Room's values and their native form at output rate `rate`: wet_db and dry_db -> round(-100 dB) in
    [0, 6000] (dry_db None: -1), predelay -> round(s rate) in [0, rate], length (None: 0, all of it; else at least one
    sample), fade, offset -> round(s rate) samples ([0, 600] s), tail -> samples, None: -1.  ValueError for anything else: a
    value that is no Room, a wav that is neither bytes nor a path, a normalize that is no bool, a channel that is neither None
    nor an index."""
    if not isinstance(room, Room):
        raise ValueError(f"room must be a Room, got {type(room).__name__}")
    if not isinstance(room.wav, (bytes, bytearray, memoryview, str)) and not hasattr(room.wav, "__fspath__"):
        raise ValueError(f"room: wav must be WAV bytes or a path, got {type(room.wav).__name__}")
    wet = int(round(-100.0 * _real("wet_db", room.wet_db, -MAX_DB, 0.0, "dB")))
    dry = MUTED if room.dry_db is None else int(round(-100.0 * _real("dry_db", room.dry_db, -MAX_DB, 0.0, "dB")))
    predelay = _samples("predelay", room.predelay, rate, 1.0)
    length = 0
    if room.length is not None:
        length = _samples("length", room.length, rate)
        if length < 1:
            raise ValueError(f"room: length must be at least one sample, got {room.length!r}")
    fade, offset = _samples("fade", room.fade, rate), _samples("offset", room.offset, rate)
    tail = -1 if room.tail is None else _samples("tail", room.tail, rate)
    if not isinstance(room.normalize, bool):
        raise ValueError(f"room: normalize must be True or False, got {room.normalize!r}")
    if room.channel is not None and (isinstance(room.channel, bool) or not isinstance(room.channel, int) or room.channel < 0):
        raise ValueError(f"room: channel must be None or a channel index, got {room.channel!r}")
    return RoomParams(-1 if room.channel is None else int(room.channel), 1 if room.normalize else 0, wet, dry, 0, offset, length,
                      fade, predelay, tail)


def room_bytes(room: Room) -> bytes:
    """The WAV bytes of a Room: its `wav` itself, or the file it names."""
    if isinstance(room.wav, (bytes, bytearray, memoryview)):
        return bytes(room.wav)
    with open(room.wav, "rb") as f:
        return f.read()


def send_regions(sends: Sequence[int], marks: Sequence) -> List[Tuple[int, int, int]]:
    """The room stage's regions (a, e, send) from every line's native send and its mark (script.line_marks): one per line
    that has audio and a send other than 0; a line's region is merged into that of the line before it where both have the same
    send (the silence between them goes along, and a line without audio separates nothing) - script.pan_regions' rule."""
    out: List[Tuple[int, int, int]] = []
    before = 0                          # the send of the last line that had audio
    for send, m in zip(sends, marks):
        if m is None or m[1] <= m[0]:
            continue
        if send != 0:
            if out and before == send:
                out[-1] = (out[-1][0], int(m[1]), send)
            else:
                out.append((int(m[0]), int(m[1]), send))
        before = send
    return out


def push_send_regions(sends: Sequence[int], line_of: Sequence[int], gaps: Sequence[int], cuts, at: int = 0, started: bool = False,
                      before: int = 0):
    """The live room stage's regions for ONE joined group of a stream (script.push_regions' counterpart) - segments of lines
    `line_of` behind `gaps`, kept as `cuts` says, beginning at sample `at` of the programme with `started` saying whether audio
    went out before it and `before` the send of the last line that had audio by then.  The group's marks (script.line_marks)
    go through send_regions; they are then relative to the push: shifted by `at` and clipped to the group.  Where the group's
    first line with audio has the send `before` had - the line continues from the group before, or follows a line of equal
    send - its region begins with the group, so the silence in front of it goes along as send_regions has it for the whole
    piece.  The regions of all groups, moved back to the timeline and touching ones of equal send joined, are send_regions of
    the final marks.  Returns (regions, at, started, before) after the group."""
    from .script import line_marks
    found: list = [None] * len(sends)
    end, started_after = line_marks(line_of, gaps, cuts, found, at, started)
    spoken = [j for j in sorted(set(line_of)) if found[j] is not None and found[j][1] > found[j][0]]
    regions = send_regions(sends, found)
    if spoken and regions and sends[spoken[0]] == before != 0:
        regions[0] = (at, regions[0][1], before)
    out = [(max(a, at) - at, min(e, end) - at, s) for a, e, s in regions if max(a, at) < min(e, end)]
    return out, end, started_after, (sends[spoken[-1]] if spoken else before)
