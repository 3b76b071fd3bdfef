"""Music bed, host side: a Bed - a WAV put under a narrated piece and pulled down while someone speaks - for `bed=` of
FishTTS.synthesize_long / synthesize_script and for FishTTS.mix.  bed_params is the one place where a Bed's seconds and
dB become the integers of ft_mix_params (include/fishtts_hip.h: "Mix"), each checked; CodecHipEngine.mix takes them as they
are.  Plain Python: neither torch nor the native library is imported here.

The reference has nothing of the kind."""
from __future__ import annotations

import math
from numbers import Real
from typing import NamedTuple, Optional

HOP_MS = 20                     # the mix stage's hop: floor(rate / 50) samples
MAX_SECONDS = 600.0             # attack, release (10 s at most: 500 hops), lead, tail, fades, offset
MAX_WINDOW_HOPS = 500
DEFAULT_THRESHOLD_DB = -45.0


class Bed(NamedTuple):
    wav: object                            # WAV bytes, or a path to a WAV file (any format the reference intake reads)
    level: Optional[float] = -30.0         # LUFS the bed is brought to; None: the file's own level
    duck_db: float = 12.0                  # how far the bed is lowered under speech, dB in [0, 60]
    threshold_db: Optional[float] = None   # the programme is "speaking" above this; None: the call's silence_db, or -45
    attack: float = 0.3                    # s over which the bed falls before speech, (0, 10]
    release: float = 0.8                   # s over which it rises after speech, (0, 10]
    lead: float = 0.0                      # s of bed alone before the programme
    tail: float = 0.0                      # s of bed alone after it
    fade_in: float = 0.0                   # s
    fade_out: float = 1.0                  # s
    offset: float = 0.0                    # s into the bed at which it starts
    loop: bool = True                      # repeat the bed to the programme's length; False: silence past its end
    channel: Optional[int] = None          # that channel alone; None: the mean of all


class MixParams(NamedTuple):
    """A Bed's values as ft_mix_params takes them, at one output rate."""
    bed_loudness: int      # hundredths of a LUFS, 0: the file's own level
    channel: int           # -1: the mean of all channels
    depth: int             # hundredths of a dB
    threshold: float       # linear
    attack: int            # hops
    release: int           # hops
    lead: int              # samples, as tail, fade_in, fade_out, offset
    tail: int
    fade_in: int
    fade_out: int
    offset: int
    loop: int


def _real(name: str, v, lo: float, hi: float, unit: str) -> float:
    if isinstance(v, bool) or not isinstance(v, Real) or not lo <= float(v) <= hi:       # (a nan fails)
        raise ValueError(f"bed: {name} must be a number of {unit} in [{lo:g}, {hi:g}], got {v!r}")
    return float(v)


def _samples(name: str, v, rate: int) -> int:
    return int(round(_real(name, v, 0.0, MAX_SECONDS, "seconds") * rate))


def _hops(name: str, v) -> int:
    h = int(round(_real(name, v, 0.0, MAX_WINDOW_HOPS * HOP_MS / 1000.0, "seconds") * 1000.0 / HOP_MS))
    if h < 1:
        raise ValueError(f"bed: {name} must be at least one hop of {HOP_MS} ms, got {v!r}")
    return h


def bed_params(bed: Bed, rate: int, silence_db: Optional[float] = None) -> MixParams:
    """Every check of a Bed's values and their native form at output rate `rate`: level -> round(100 level) (a target in
    [-50, -5] LUFS), duck_db -> round(100 duck_db) in [0, 6000], threshold_db (None: `silence_db`, or -45 where that is None;
    [-90, 0]) -> 10^(dB / 20), attack and release -> round(s / 0.02) hops in [1, 500], lead, tail, the fades and offset ->
    round(s rate) samples ([0, 600] s).  ValueError for anything else: a value that is no Bed, a wav that is neither bytes nor a
    path, a loop that is no bool, a channel that is neither None nor an index."""
    if not isinstance(bed, Bed):
        raise ValueError(f"bed must be a Bed, got {type(bed).__name__}")
    if not isinstance(bed.wav, (bytes, bytearray, memoryview, str)) and not hasattr(bed.wav, "__fspath__"):
        raise ValueError(f"bed: wav must be WAV bytes or a path, got {type(bed.wav).__name__}")
    level = 0 if bed.level is None else int(round(100.0 * _real("level", bed.level, -50.0, -5.0, "LUFS")))
    depth = int(round(100.0 * _real("duck_db", bed.duck_db, 0.0, 60.0, "dB")))
    thr_db = bed.threshold_db
    if thr_db is None:
        thr_db = DEFAULT_THRESHOLD_DB if silence_db is None else silence_db
    threshold = math.pow(10.0, _real("threshold_db", thr_db, -90.0, 0.0, "dB") / 20.0)
    attack, release = _hops("attack", bed.attack), _hops("release", bed.release)
    lead, tail = _samples("lead", bed.lead, rate), _samples("tail", bed.tail, rate)
    fade_in, fade_out = _samples("fade_in", bed.fade_in, rate), _samples("fade_out", bed.fade_out, rate)
    offset = _samples("offset", bed.offset, rate)
    if not isinstance(bed.loop, bool):
        raise ValueError(f"bed: loop must be True or False, got {bed.loop!r}")
    if bed.channel is not None and (isinstance(bed.channel, bool) or not isinstance(bed.channel, int) or bed.channel < 0):
        raise ValueError(f"bed: channel must be None or a channel index, got {bed.channel!r}")
    return MixParams(level, -1 if bed.channel is None else int(bed.channel), depth, threshold, attack, release, lead, tail,
                     fade_in, fade_out, offset, 1 if bed.loop else 0)


def bare_params() -> MixParams:
    """The values of a live mix stream without a bed (CodecHipEngine.mix_stream(None, bedless=True)): the limiter alone.  No
    duck, no lead, no tail, no fades, nothing loops, and the shortest attack - with no bed to lower, the duck's window would
    only be held back: the stream then holds back (1 + 5 + 2) hops, 160 ms, the limiter's own look-ahead."""
    return MixParams(0, -1, 0, math.pow(10.0, DEFAULT_THRESHOLD_DB / 20.0), 1, 1, 0, 0, 0, 0, 0, 0)


def bed_bytes(bed: Bed) -> bytes:
    """The WAV bytes of a Bed: its `wav` itself, or the file it names."""
    if isinstance(bed.wav, (bytes, bytearray, memoryview)):
        return bytes(bed.wav)
    with open(bed.wav, "rb") as f:
        return f.read()
