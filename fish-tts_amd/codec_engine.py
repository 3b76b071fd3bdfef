"""Host driver of the HIP DAC decode path: the S3 seam of SURVEY.md §8b, `vocoder.decode(indices,
feature_lengths)` (fish_tts/models/vocoder.py:906-912), on top of the C ABI."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .ar_engine import HipError, _rope_table
from .config import CodecArgs


CODEC_RATE = 44100     # the codec's own sample rate (Fi of the resampler)


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}, got {v!r}")
    return float(v)


@dataclass(frozen=True)
class LevelInfo:
    """What the level stage found in one item (ft_level_info): `lufs` the integrated loudness before the gain (-inf when
    nothing was measured), `peak` the sample peak before the gain, `gain` the factor applied, `blocks` / `gated` the
    400 ms blocks and those that passed both gates, `capped` whether the -1 dBFS ceiling bound the gain."""
    lufs: float
    peak: float
    gain: float
    blocks: int
    gated: int
    capped: bool

    @classmethod
    def of(cls, i: "L.ft_level_info") -> "LevelInfo":
        return cls(float(i.lufs), float(np.float32(i.peak)), float(np.float32(i.gain)), int(i.blocks), int(i.gated), bool(i.capped))


@dataclass(frozen=True)
class IntakeReport:
    """What the reference intake did with one clip (ft_intake_info): `n44` its samples at 44.1 kHz, `cut` the samples [a, e)
    of those that were kept, `frames` the code frames of the kept piece (0 unless status is 0), `status` 0 ok, 1 no loud
    window (nothing kept), 2 the kept piece is longer than the encoder takes (not encoded), `clipped` / `nonfinite` the
    channel samples at an extreme code of their format (float: |v| >= 1) and the float samples that were not finite (they
    count as 0), `level` the level stage's result (the loudness and peak before the gain)."""
    n44: int
    cut: Tuple[int, int]
    frames: int
    status: int
    clipped: int
    nonfinite: int
    level: LevelInfo

    @property
    def kept(self) -> int:
        return self.cut[1] - self.cut[0]

    @classmethod
    def of(cls, i: "L.ft_intake_info") -> "IntakeReport":
        return cls(int(i.n44), (int(i.a), int(i.e)), int(i.frames), int(i.status), int(i.clipped), int(i.nonfinite),
                   LevelInfo.of(i.level))


@dataclass(frozen=True)
class MixReport:
    """What the mix stage did (ft_mix_info): `n` the samples of the mixed piece (lead + programme + tail), `bed_len` the bed's
    samples at the output rate, `hops` the 20 ms hops of the timeline and `active` those in which the programme reached the
    threshold, `duck_max` the deepest duck (dB), `peak` the sample peak before the ceiling, `gain` the one gain the ceiling
    applied (1 when `capped` is False), `bed` the intake's report of the bed."""
    n: int
    bed_len: int
    hops: int
    active: int
    duck_max: float
    peak: float
    gain: float
    capped: bool
    bed: IntakeReport

    @classmethod
    def of(cls, i: "L.ft_mix_info") -> "MixReport":
        return cls(int(i.N), int(i.nb), int(i.Nh), int(i.active), i.dmax / 100.0, float(np.float32(i.pk)), float(np.float32(i.sg)),
                   bool(i.capped), IntakeReport.of(i.bed))


@dataclass(frozen=True)
class RoomReport:
    """What the room stage did (ft_room_info): `n` the samples of the piece (programme + tail), `ir_len` the impulse
    response's samples at the output rate and `taps` those used, `energy` the used response's energy E and `norm` the gain gn
    that normalised it (1 without normalize), `peak` the sample peak before the ceiling, `gain` the one gain the ceiling
    applied (1 when `capped` is False; never with ceiling=False), `ir` the intake's report of the response."""
    n: int
    ir_len: int
    taps: int
    energy: float
    norm: float
    peak: float
    gain: float
    capped: bool
    ir: IntakeReport

    @classmethod
    def of(cls, i: "L.ft_room_info") -> "RoomReport":
        return cls(int(i.N), int(i.nh), int(i.L), float(i.E), float(np.float32(i.gn)), float(np.float32(i.pk)),
                   float(np.float32(i.sg)), bool(i.capped), IntakeReport.of(i.ir))


@dataclass(frozen=True)
class FlacReport:
    """What the FLAC stage wrote (ft_flac_info): `frames`, the stream's `bytes`, the smallest and the largest frame, `kinds` -
    a count per subframe kind, CONSTANT, VERBATIM, FIXED 0..4 - and `assignments` - a count per channel assignment, 0000 (mono),
    0001 (L, R), 1000 (L, S), 1001 (S, R), 1010 (M, S)."""
    frames: int
    bytes: int
    min_frame: int
    max_frame: int
    kinds: Tuple[int, ...]
    assignments: Tuple[int, ...]

    @classmethod
    def of(cls, i: "L.ft_flac_info") -> "FlacReport":
        return cls(int(i.frames), int(i.bytes), int(i.min_frame), int(i.max_frame), tuple(int(v) for v in i.kinds),
                   tuple(int(v) for v in i.assignments))


FLAC_BLOCKSIZES = (256, 512, 1024, 2048, 4096)
MAX_SEND_REGIONS = 4096           # per call of ft_codec_room


def send_region_table(what: str, regions, n: int):
    """(ft_send_region array, R) of `regions` - (a, e, send) each, integers, sorted and disjoint inside [0, n), send in
    [0, 6000] hundredths of a dB or -1 (muted) - checked as the stage checks them, before any device work."""
    regions = [tuple(r) for r in regions]
    if len(regions) > MAX_SEND_REGIONS:
        raise ValueError(f"{what}: {len(regions)} send regions, a call takes {MAX_SEND_REGIONS}")
    at = 0
    for r in regions:
        if len(r) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r):
            raise ValueError(f"{what}: a region is three integers (a, e, send), got {r!r}")
        a, e, send = r
        if not at <= a < e <= n or not -1 <= send <= 6000:
            raise ValueError(f"{what}: region {r!r} out of order, outside [0, {n}) or its send outside [-1, 6000]")
        at = e
    reg = (L.ft_send_region * max(len(regions), 1))(*[L.ft_send_region(int(a), int(e), int(s), 0) for a, e, s in regions])
    return reg, len(regions)


class RoomStream:
    """An open stream of the live room stage (ft_codec_room_stream_*; CodecHipEngine.room_stream makes one): push(x, regions)
    takes the next programme samples with the send regions of that push - (a, e, send) each, relative to the push - and
    returns the roomed samples for exactly those inputs; push(x, regions, final=True) ends the programme and returns its
    samples and the room's tail behind them.  Nothing is held back, and the pushes concatenate to room(..., ceiling=False) of
    the whole programme, bit for bit, however they are cut.  report(): a RoomReport of the stream so far (`n` the samples
    emitted, `peak` over the pushes so far).  close() frees the stream's device state (a closed stream refuses pushes)."""

    def __init__(self, engine, handle, tail: int):
        self._eng, self._h, self._tail = engine, handle, tail

    def push(self, x=None, regions=(), final: bool = False) -> np.ndarray:
        if self._h is None:
            raise RuntimeError("room stream: closed")
        x = np.zeros(0, dtype=np.float32) if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        table = send_region_table("room stream push", regions, len(x))
        eng = self._eng
        cap = len(x) + (self._tail if final else 0)
        y = np.empty(max(cap, 1), dtype=np.float32)
        n = C.c_int64(0)
        eng._check(eng.lib.ft_codec_room_stream_push(self._h, x.ctypes.data_as(C.c_void_p), len(x), *table, 1 if final else 0,
                                                     y.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "ft_codec_room_stream_push")
        return y[:n.value]

    def report(self) -> RoomReport:
        if self._h is None:
            raise RuntimeError("room stream: closed")
        info = L.ft_room_info()
        self._eng._check(self._eng.lib.ft_codec_room_stream_info(self._h, C.byref(info)), "ft_codec_room_stream_info")
        return RoomReport.of(info)

    def close(self) -> None:
        if self._h is not None:
            self._eng.lib.ft_codec_room_stream_end(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _flac_samples(what: str, audio, dtype=None, channels: Optional[int] = None, empty: bool = False) -> np.ndarray:
    """`audio` as the FLAC stage takes it: float32 or int16, (N,) mono or (N, 2), contiguous - flac()'s checks; with `dtype` /
    `channels` a stream's too (the dtype and channel count it was made for); `empty`: no sample is fine (a stream's push)."""
    x = np.asarray(audio)
    if x.dtype != np.int16:
        if x.dtype.kind not in "fiu":
            raise ValueError(f"{what}: audio must be float32 or int16, got {x.dtype}")
        if x.dtype.kind in "iu":
            raise ValueError(f"{what}: integer audio must be int16, got {x.dtype}")
        x = x.astype(np.float32)
    if dtype is not None and x.dtype != dtype:
        raise ValueError(f"{what}: the stream takes {np.dtype(dtype).name}, got {x.dtype}")
    if x.ndim not in (1, 2) or (x.ndim == 2 and x.shape[1] != 2):
        raise ValueError(f"{what}: a waveform is (N,) or (N, 2), got {x.shape}")
    if channels is not None and x.ndim != channels:
        raise ValueError(f"{what}: the stream has {channels} channel(s), got {x.shape}")
    if x.shape[0] < 1 and not empty:
        raise ValueError(f"{what}: an empty waveform")
    return np.ascontiguousarray(x)


class FlacStream:
    """An open stream of the live FLAC stage (ft_codec_flac_stream_*; CodecHipEngine.flac_stream makes one): push(x) takes the
    next samples - the dtype and channels the stream was made for, checked as flac() checks them - and returns the bytes of
    the frames they complete (b"" where they complete none); push(x, final=True) ends the stream and flushes the short last
    frame.  head(): the 42 leading bytes from what is known - before the final push with the sizes and the sample count
    "unknown" (zero), after it the ones flac() would have written.  head() + the pushes' bytes is one FLAC stream, and the
    pushes' bytes are flac(whole)[42:] byte for byte, however they are cut.  report(): a FlacReport of the stream so far.
    close() frees the stream's device state (a closed stream refuses pushes)."""

    def __init__(self, engine, handle, dtype, channels: int, blocksize: int):
        self._eng, self._h, self._dtype, self._channels, self._B = engine, handle, np.dtype(dtype), channels, blocksize
        self._nin = 0

    def push(self, x=None, final: bool = False) -> bytes:
        if self._h is None:
            raise RuntimeError("flac stream: closed")
        x = np.zeros(0, dtype=self._dtype) if x is None else x
        x = _flac_samples("flac stream push", x, self._dtype, None if np.asarray(x).size == 0 else self._channels, empty=True)
        n = x.shape[0] if x.size else 0
        eng = self._eng
        cap = C.c_int64(0)
        eng._check(eng.lib.ft_flac_stream_plan(self._B, self._channels, self._nin, n, 1 if final else 0, None, C.byref(cap)),
                   "ft_flac_stream_plan")
        out = np.empty(max(cap.value, 1), dtype=np.uint8)
        got = C.c_int64(0)
        eng._check(eng.lib.ft_codec_flac_stream_push(self._h, x.ctypes.data_as(C.c_void_p) if n else None, n, 1 if final else 0,
                                                     out.ctypes.data_as(C.c_void_p), cap.value, C.byref(got)),
                   "ft_codec_flac_stream_push")
        self._nin += n
        return out[:got.value].tobytes()

    def head(self) -> bytes:
        if self._h is None:
            raise RuntimeError("flac stream: closed")
        out = (C.c_uint8 * 42)()
        self._eng._check(self._eng.lib.ft_codec_flac_stream_head(self._h, out), "ft_codec_flac_stream_head")
        return bytes(out)

    def report(self) -> FlacReport:
        if self._h is None:
            raise RuntimeError("flac stream: closed")
        info = L.ft_flac_info()
        self._eng._check(self._eng.lib.ft_codec_flac_stream_info(self._h, C.byref(info)), "ft_codec_flac_stream_info")
        return FlacReport.of(info)

    def close(self) -> None:
        if self._h is not None:
            self._eng.lib.ft_codec_flac_stream_end(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass(frozen=True)
class MixLiveReport:
    """What the live mix stage did (ft_mix_live_info): `n`, `bed_len`, `hops`, `active`, `duck_max` and `bed` as MixReport's;
    `limit_max` the deepest the limiter went (dB), `peak` the largest hop peak before the limiter."""
    n: int
    bed_len: int
    hops: int
    active: int
    duck_max: float
    limit_max: float
    peak: float
    bed: IntakeReport

    @classmethod
    def of(cls, i: "L.ft_mix_live_info") -> "MixLiveReport":
        return cls(int(i.N), int(i.nb), int(i.Nh), int(i.active), i.dmax / 100.0, i.lmax / 100.0, float(np.float32(i.qmax)),
                   IntakeReport.of(i.bed))


class MixStream:
    """An open stream of the live mix stage (ft_codec_mix_stream_*; CodecHipEngine.mix_stream makes one): push(x) takes the
    next programme samples and returns the mixed samples that became final, push(x, final=True) ends the programme and returns
    all that is left; close() frees the stream's device state (a closed stream refuses pushes)."""

    def __init__(self, engine, handle, mp, rate: int):
        self._eng, self._h, self._mp, self._rate = engine, handle, mp, rate
        self._nin, self._out = 0, 0

    def push(self, x=None, final: bool = False) -> np.ndarray:
        return self._push(x, None, final)

    def _push(self, x, regions, final: bool) -> np.ndarray:
        """One push; `regions`: a stereo stream's (None: a mono stream, which has no region table and emits one float per frame)."""
        if self._h is None:
            raise RuntimeError("mix stream: closed")
        x = np.zeros(0, dtype=np.float32) if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        stereo = regions is not None
        table = pan_region_table("mix stream push", regions, len(x)) if stereo else ()
        eng = self._eng
        done = C.c_int64(0)
        eng._check(eng.lib.ft_mix_live_plan(self._rate, C.byref(self._mp), self._nin + len(x), 1 if final else 0, C.byref(done),
                                            None), "ft_mix_live_plan")
        cap = max(done.value - self._out, 0)
        y = np.empty((max(cap, 1), 2) if stereo else max(cap, 1), dtype=np.float32)
        n = C.c_int64(0)
        what = "ft_codec_mix_stream_push_stereo" if stereo else "ft_codec_mix_stream_push"
        eng._check(getattr(eng.lib, what)(self._h, x.ctypes.data_as(C.c_void_p), len(x), *table, 1 if final else 0,
                                          y.ctypes.data_as(C.c_void_p), cap, C.byref(n)), what)
        self._nin += len(x)
        self._out += n.value
        return y[:n.value]

    def close(self) -> None:
        if self._h is not None:
            self._eng.lib.ft_codec_mix_stream_end(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


MAX_PAN_REGIONS = 4096            # per call of ft_codec_mix_stereo, per push of a stereo mix stream


def pan_region_table(what: str, regions, n: int):
    """(ft_pan_region array, R) of `regions` - (a, e, pan) each, integers, sorted and disjoint inside [0, n), pan in
    [-100, 100] - checked as the stage checks them, before any device work."""
    regions = [tuple(r) for r in regions]
    if len(regions) > MAX_PAN_REGIONS:
        raise ValueError(f"{what}: {len(regions)} pan regions, a call takes {MAX_PAN_REGIONS}")
    at = 0
    for r in regions:
        if len(r) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r):
            raise ValueError(f"{what}: a region is three integers (a, e, pan), got {r!r}")
        a, e, pan = r
        if not at <= a < e <= n or not -100 <= pan <= 100:
            raise ValueError(f"{what}: region {r!r} out of order, outside [0, {n}) or its pan outside [-100, 100]")
        at = e
    reg = (L.ft_pan_region * max(len(regions), 1))(*[L.ft_pan_region(int(a), int(e), int(pan), 0) for a, e, pan in regions])
    return reg, len(regions)


class StereoMixStream(MixStream):
    """An open stream of the live stereo mix stage (ft_codec_mix_stream_*_stereo; CodecHipEngine.mix_stream(stereo=True) makes
    one): push(x, regions) takes the next mono programme samples with the pan regions of that push - (a, e, pan) each,
    relative to the push - and returns the frames that became final, (frames, 2) float32, left then right."""

    def push(self, x=None, regions=(), final: bool = False) -> np.ndarray:
        return self._push(x, list(regions), final)


@dataclass(frozen=True)
class OutputFx:
    """The output stages of a call, checked: `rate` (Hz), `pct` (speed, percent), `cents` (pitch), `level` (loudness
    target, hundredths of a LUFS) and `live` (a stream's live loudness target, the same unit), each None where the stage is
    absent - the codec's own rate (None or 44100), the model's own pace (a speed that rounds to 100 percent), pitch (one
    that rounds to 0 cents), level (no loudness given) and ride stage (no live loudness given).  Built once per call by
    of() and handed down to the native call as it is."""
    rate: Optional[int] = None
    pct: Optional[int] = None
    cents: Optional[int] = None
    level: Optional[int] = None
    live: Optional[int] = None

    @classmethod
    def of(cls, sample_rate=None, speed=None, pitch=None, loudness=None, live_loudness=None) -> "OutputFx":
        """A caller's `sample_rate=` (an integer in [8000, 48000] whose reduced L = rate / gcd(rate, 44100) is at most 640:
        ft_resample_filter), `speed=` (a factor in [0.5, 2.0], kept as round(speed * 100): ft_timescaled_len) and `pitch=`
        (semitones in [-12, 12], kept as round(100 * pitch) cents: ft_pitch_filter; a plain shift, formants move with the
        pitch), then the two together (ft_pitch_ok: the time-scale stage under a pitch shift runs at speed / 2^(pitch / 12),
        which has to lie in [0.5, 2]), then `loudness=` (a target in LUFS in [-50, -5], kept as round(100 * loudness):
        ft_codec_loudness; every item is brought to that integrated loudness, its sample peak held at -1 dBFS), or
        `live_loudness=` (the same range and unit: a stream is ridden toward that loudness by a look-ahead gain rider,
        ft_codec_stream_begin_live; not both).  Anything else raises ValueError, before any device work."""
        rate = pct = cents = level = live = None
        if sample_rate is not None:
            if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)):
                raise ValueError(f"sample_rate must be an integer, got {sample_rate!r}")
            rate = int(sample_rate)
            if rate == CODEC_RATE:
                rate = None
            elif not -(1 << 31) <= rate < (1 << 31) or L.load().ft_resample_filter(rate, None, None, None, None) != L.FT_OK:
                raise ValueError(f"unsupported sample_rate {rate}: integers in [8000, 48000] whose ratio to 44100 reduces to "
                                 "L / M with L <= 640 (8000, 11025, 12000, 16000, 22050, 24000, 32000, 48000, ...)")
        if speed is not None:
            if not 0.5 <= _number(speed, "speed must be a number") <= 2.0:      # (a nan fails both comparisons)
                raise ValueError(f"unsupported speed {speed!r}: a factor in [0.5, 2.0]")
            pct = int(round(float(speed) * 100))
            pct = None if pct == 100 else pct
        if pitch is not None:
            if not -12.0 <= _number(pitch, "pitch must be a number of semitones") <= 12.0:
                raise ValueError(f"unsupported pitch {pitch!r}: semitones in [-12, 12]")
            cents = int(round(float(pitch) * 100)) or None
        if cents is not None and L.load().ft_pitch_ok(100 if pct is None else pct, cents) != L.FT_OK:
            raise ValueError(f"unsupported combination speed={speed!r}, pitch={pitch!r}: speed / 2^(pitch / 12) must lie in "
                             "[0.5, 2.0]")
        if loudness is not None:
            if not -50.0 <= _number(loudness, "loudness must be a number of LUFS") <= -5.0:
                raise ValueError(f"unsupported loudness {loudness!r}: a target in LUFS in [-50, -5]")
            level = int(round(float(loudness) * 100))
        if live_loudness is not None:
            if not -50.0 <= _number(live_loudness, "live_loudness must be a number of LUFS") <= -5.0:
                raise ValueError(f"unsupported live_loudness {live_loudness!r}: a target in LUFS in [-50, -5]")
            if loudness is not None:
                raise ValueError("loudness and live_loudness together: one gain over the whole utterance, or a gain ridden "
                                 "over a stream, not both")
            live = int(round(float(live_loudness) * 100))
        return cls(rate, pct, cents, level, live)

    def __bool__(self) -> bool:
        """Any stage at all: the call goes through the chain's native entry points, a stream holds back a tail."""
        return (self.rate is not None or self.pct is not None or self.cents is not None or self.level is not None
                or self.live is not None)

    def no_level(self, what: str) -> "OutputFx":
        """self, for a call that hands out audio before the utterance has ended: ValueError with a level."""
        if self.level is not None:
            raise ValueError(f"loudness needs the whole utterance: {what} hands out audio before its end, and the integrated "
                             "loudness is known only there")
        return self

    def no_live(self) -> "OutputFx":
        """self, for a call that decodes whole items: ValueError with a ride stage (such a call has `loudness`)."""
        if self.live is not None:
            raise ValueError("live_loudness rides a stream: a call that decodes whole utterances takes loudness instead")
        return self

    @property
    def emits_empty(self) -> bool:
        """A stream's empty chunk is handed out: no stage, or a resampler only.  Behind a time-scale, pitch or ride stage a
        chunk that completes nothing gives no samples yet, and nothing is handed out for it."""
        return self.pct is None and self.cents is None and self.live is None

    @property
    def kw(self) -> dict:
        """The value as the keyword of a call that takes it defaulted: {"fx": self}, and nothing without a stage - a decoder
        or codec handed in by a caller, which may know of no stage, is then called as it always was."""
        return {"fx": self} if self else {}

    @property
    def native(self):
        """(sample_rate, speed_pct, pitch_cents) as the native entry points take them."""
        return self.rate or CODEC_RATE, self.pct or 100, self.cents or 0

    @property
    def native_level(self) -> int:
        """The level as the native entry points take it: hundredths of a LUFS, 0 without the stage."""
        return self.level or 0

    @property
    def native_live(self) -> int:
        """The ride stage's target as the native entry points take it: hundredths of a LUFS, 0 without the stage."""
        return self.live or 0

    @property
    def wav_rate(self) -> int:
        return self.rate or CODEC_RATE

    def out_len(self, n: int) -> int:
        """Samples that n codec samples give: ceil(100 n / pct) after the time-scale stage (the pitch stage keeps that
        length), then ceil(n L / M) after the resampler."""
        n = int(n) if self.pct is None else int(L.load().ft_timescaled_len(self.pct, int(n)))
        return n if self.rate is None else int(L.load().ft_resampled_len(self.rate, n))


def output_rate(sample_rate: Optional[int]) -> Optional[int]:
    """OutputFx.of's rate: None for the codec's own rate."""
    return OutputFx.of(sample_rate=sample_rate).rate


def resampled_len(sample_rate: Optional[int], n: int) -> int:
    """Samples that n codec samples give at sample_rate: ceil(n L / M)."""
    return OutputFx.of(sample_rate=sample_rate).out_len(n)


def output_speed(speed) -> Optional[int]:
    """OutputFx.of's speed in percent: None for the model's own pace."""
    return OutputFx.of(speed=speed).pct


def timescaled_len(speed, n: int) -> int:
    """Samples that n codec samples give at `speed`: ceil(100 n / pct)."""
    return OutputFx.of(speed=speed).out_len(n)


def output_pitch(pitch) -> Optional[int]:
    """OutputFx.of's pitch in cents: None for the model's own pitch."""
    return OutputFx.of(pitch=pitch).cents


def output_fx(speed, pitch):
    """(pct, cents) of a caller's `speed=` and `pitch=`, checked together."""
    fx = OutputFx.of(speed=speed, pitch=pitch)
    return fx.pct, fx.cents


def fold_weight_norm(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """codec.pth stores weight-normed convs as parametrizations.weight.original0 (g) / original1 (v)
    (vocoder.py:423-429,457-463: torch weight_norm, dim=0).  Fold them to plain `.weight` tensors and
    drop the "generator." prefix the reference strips in synthesizer.py:276-282."""
    if "state_dict" in sd:
        sd = sd["state_dict"]
    if any("generator." in k for k in sd):
        sd = {k.replace("generator.", ""): v for k, v in sd.items() if "generator." in k}
    out = {}
    for k, v in sd.items():
        if k.endswith("parametrizations.weight.original0"):
            base = k[: -len("parametrizations.weight.original0")]
            g, w = v.float(), sd[base + "parametrizations.weight.original1"].float()
            norm = w.flatten(1).norm(dim=1).view(-1, *([1] * (w.dim() - 1)))
            out[base + "weight"] = g * w / norm
        elif k.endswith("parametrizations.weight.original1"):
            continue
        else:
            out[k] = v
    return out


class CodecHipEngine:
    def __init__(self, args: Optional[CodecArgs] = None, device: int = 0, max_frames: int = 2048, max_batch: int = 1,
                 with_encoder: bool = False):
        """`with_encoder`: also build the encode side (encode_reference); its tensors are then required at load."""
        self.args = args or CodecArgs()
        a = self.args
        self.with_encoder = bool(with_encoder and a.encoder_dim > 0)
        self.lib = L.load()
        self._streams = set()          # open CodecStreams (ended before the native context goes)
        c = L.ft_codec_config()
        c.dtype = L.FT_BF16
        c.n_codebooks, c.codebook_size, c.semantic_codebook_size = a.n_codebooks, a.codebook_size, a.semantic_codebook_size
        c.codebook_dim, c.latent_dim = a.codebook_dim, a.latent_dim
        c.n_tf_layer, c.tf_n_head, c.tf_head_dim, c.tf_ffn, c.tf_window = a.n_tf_layer, a.tf_n_head, a.tf_head_dim, a.tf_ffn, a.tf_window
        c.tf_rope_base, c.tf_norm_eps = float(a.tf_rope_base), float(a.tf_norm_eps)
        if any(f != 2 for f in a.downsample_factor):
            raise NotImplementedError("upsample stages other than x2 are not implemented")
        c.n_upsample = len(a.downsample_factor)
        c.decoder_dim, c.n_rates = a.decoder_dim, len(a.decoder_rates)
        for i, r in enumerate(a.decoder_rates):
            c.rates[i] = r
        c.max_frames, c.max_batch = int(max_frames), int(max_batch)
        self.max_enc_frames = 0
        if self.with_encoder:
            c.encoder_dim, c.n_enc_rates, c.enc_tf_window = a.encoder_dim, len(a.encoder_rates), a.encoder_tf_window
            for i, (r, nt) in enumerate(zip(a.encoder_rates, a.encoder_transformer_layers)):
                c.enc_rates[i], c.enc_tf_layers[i] = r, nt
            want = int(a.max_reference_seconds * a.sample_rate) // a.encode_frame_length + 1
            self.max_enc_frames = c.max_enc_frames = max(1, min(int(max_frames), want))
        self.cfg = c
        self.max_frames = max_frames
        self.R = a.n_codebooks + 1
        self._h = C.c_void_p()
        st = self.lib.ft_create(None, C.byref(c), device, C.byref(self._h))
        if st != L.FT_OK:
            raise HipError(f"ft_create(codec) failed ({st}): {self.lib.ft_last_error(None).decode()}")
        self.frame_len = self.lib.ft_codec_frame_len(self._h)
        self.enc_frame_len = self.lib.ft_codec_enc_frame_len(self._h)

    def close(self):
        for st in list(getattr(self, "_streams", ())):
            st.close()
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.ft_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, what):
        if st != L.FT_OK:
            msg = self.lib.ft_last_error(self._h).decode()
            if st == L.FT_ERR_STATE and "Vocoder not loaded" in msg:
                raise RuntimeError("Vocoder not loaded")  # synthesizer.py:599-600
            raise HipError(f"{what} failed ({st}): {msg}")

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        a = self.args
        sd = fold_weight_norm(sd)
        want = None
        for k, v in sd.items():
            t = v.detach().float().contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            st = self.lib.ft_load_weight(self._h, k.encode(), C.c_void_p(t.data_ptr()), L.FT_F32, shape, t.dim())
            if st == L.FT_ERR_ARG and b"unknown weight name" in self.lib.ft_last_error(self._h):
                continue  # encoder / pre_module / training-only tensors of codec.pth
            self._check(st, f"ft_load_weight({k})")
        tab = _rope_table(self.max_frames, a.tf_head_dim, a.tf_rope_base)
        shape = (C.c_int64 * 3)(*tab.shape)
        self._check(self.lib.ft_load_weight(self._h, b"rope.codec", C.c_void_p(tab.data_ptr()), L.FT_F32, shape, 3), "rope.codec")
        if self.with_encoder:
            rate, npos = 1, 1
            for r, nt in zip(a.encoder_rates, a.encoder_transformer_layers):
                rate *= r
                if nt > 0:
                    npos = max(npos, self.max_enc_frames * a.encode_frame_length // rate)
            tab2 = _rope_table(npos, 64, a.tf_rope_base)   # encoder transformers: head_dim 64 (synthesizer.py:249)
            shape2 = (C.c_int64 * 3)(*tab2.shape)
            self._check(self.lib.ft_load_weight(self._h, b"rope.codec_enc", C.c_void_p(tab2.data_ptr()), L.FT_F32, shape2, 3),
                        "rope.codec_enc")
        self._check(self.lib.ft_finalize_weights(self._h), "ft_finalize_weights")

    @classmethod
    def synthetic(cls, device: int = 0, max_frames: int = 2048, seed: int = 0, args: Optional[CodecArgs] = None,
                  with_encoder: bool = False):
        from .weights import random_codec_state_dict
        eng = cls(args, device=device, max_frames=max_frames, with_encoder=with_encoder)
        eng.load_state_dict(random_codec_state_dict(eng.args, seed, with_encoder=eng.with_encoder))
        return eng

    def encode(self, audio: np.ndarray) -> np.ndarray:
        """vocoder.encode of encode_reference (synthesizer.py:345-352, vocoder.py:885-904): mono float audio at the
        codec sample rate -> (n_codebooks + 1, T') int64 codes, T' = ceil(len / encode_frame_length)."""
        if not self.with_encoder:
            raise RuntimeError("codec encoder not built (CodecHipEngine(..., with_encoder=True))")
        audio = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
        T = (audio.shape[0] + self.enc_frame_len - 1) // self.enc_frame_len
        codes = np.zeros((self.R, max(T, 1)), dtype=np.int32)
        n = C.c_int32(0)
        self._check(self.lib.ft_codec_encode(self._h, audio.ctypes.data_as(C.c_void_p), audio.shape[0],
                                             codes.ctypes.data_as(C.c_void_p), C.byref(n)), "ft_codec_encode")
        assert n.value == T, (n.value, T)
        return codes.astype(np.int64)

    def rvq_encode(self, z: np.ndarray) -> np.ndarray:
        """Test hook: the quantiser search alone on pre-quantiser latents z (T, latent_dim) f32."""
        z = np.ascontiguousarray(z, dtype=np.float32)
        codes = np.zeros((self.R, z.shape[0]), dtype=np.int32)
        self._check(self.lib.ft_codec_rvq_encode(self._h, z.ctypes.data_as(C.c_void_p), z.shape[0],
                                                 codes.ctypes.data_as(C.c_void_p)), "ft_codec_rvq_encode")
        return codes

    # ft_test_codec_trace_buffer kinds: main bf16 output, Snake'd copy, f32 output; a carrying launch of a streamed decode:
    # the carried rows as placed in front of the chunk, the whole carry left for the next chunk
    TRACE_KINDS = ("bf", "act", "f32", "front", "carry")

    def trace_variants(self) -> List[dict]:
        """Test hook: the GEMM instantiations gemm() can pick, by id: name and row / column tile."""
        out = []
        for i in range(self.lib.ft_test_codec_trace_variants()):
            bm, bn = C.c_int32(0), C.c_int32(0)
            name = self.lib.ft_test_codec_trace_variant(i, C.byref(bm), C.byref(bn))
            out.append({"id": i, "name": name.decode(), "bm": bm.value, "bn": bn.value})
        return out

    def trace(self, call, first: int = 0, count: int = 0):
        """Test hook (ft_test_codec_trace_*): run call() - ONE decode of one item, ONE encode, ONE chunk of a stream
        (CodecStream.decode) or ONE batched call (decode_streams of at most 64 plain streams) - traced.  Returns
        (call's result, launches): per launch in launch order a dict name / rows / cols / variant / halo / ntap / K and,
        for launches [first, first + count), "out": {"bf" | "act" | "f32": (rows, cols) array}, bf16 as uint16 bits.
        A carrying launch of a streamed call ("*.roll", "*.kvin", "*.kvout") has "chunk" (its chunk's index in the
        call, where the others have ntap) and "out": {"front" | "carry": ...}.  trace_chunks() gives the chunk table."""
        self._check(self.lib.ft_test_codec_trace_arm(self._h, int(first), int(count)), "ft_test_codec_trace_arm")
        res = call()
        n = self.lib.ft_test_codec_trace_count(self._h)
        if n < 0:
            raise HipError("codec trace: a copy failed or a launch wrote with a row stride other than its columns")
        launches = []
        name = C.create_string_buffer(96)
        info = (C.c_int32 * 8)()
        for i in range(n):
            self._check(self.lib.ft_test_codec_trace_launch(self._h, i, name, 96, info), "ft_test_codec_trace_launch")
            rec = {"name": name.value.decode(), "rows": info[0], "cols": info[1], "variant": info[2], "halo": info[4],
                   "ntap": info[5], "K": info[6], "kinds": [], "out": {}}
            if rec["name"].endswith((".roll", ".kvin", ".kvout")):
                rec["chunk"] = rec.pop("ntap")
            for j in range(info[3]):
                kind, f32, elems = C.c_int32(0), C.c_int32(0), C.c_int64(0)
                self._check(self.lib.ft_test_codec_trace_buffer(self._h, i, j, C.byref(kind), C.byref(f32), C.byref(elems), None),
                            "ft_test_codec_trace_buffer")
                k = self.TRACE_KINDS[kind.value]
                rec["kinds"].append(k)
                if info[7]:
                    a = np.empty((info[0], info[1]), dtype=np.float32 if f32.value else np.uint16)
                    assert a.size == elems.value, (rec["name"], a.shape, elems.value)
                    self._check(self.lib.ft_test_codec_trace_buffer(self._h, i, j, C.byref(kind), C.byref(f32), C.byref(elems),
                                                                    a.ctypes.data_as(C.c_void_p)), "ft_test_codec_trace_buffer")
                    rec["out"][k] = a
            launches.append(rec)
        return res, launches

    def trace_chunks(self) -> List[dict]:
        """Test hook (ft_test_codec_trace_chunks): the chunks of the last traced call, in call order: P (first frame in
        the call), L (frames), t0 (rope position), nh (carried K/V rows).  Empty after a one-shot call."""
        n = C.c_int32(0)
        tab = np.zeros((64, 4), dtype=np.int32)
        self._check(self.lib.ft_test_codec_trace_chunks(self._h, C.byref(n), tab.ctypes.data_as(C.c_void_p)),
                    "ft_test_codec_trace_chunks")
        return [dict(zip(("P", "L", "t0", "nh"), (int(v) for v in row))) for row in tab[:n.value]]

    def stream(self, sample_rate: Optional[int] = None, speed: Optional[float] = None,
               pitch: Optional[float] = None, fx: Optional[OutputFx] = None, live_loudness: Optional[float] = None) -> "CodecStream":
        """A streamed decode with carried state: the chunks' waveforms concatenate to the waveform of one decode.
        `sample_rate`, `speed`, `pitch` (OutputFx.of), or `fx`, the checked value itself.
        `sample_rate`: the stream's output is resampled on the device; it holds back the samples whose
        filter taps reach past the input so far, until a later chunk, decode(final=True) or finish().
        `speed`: the waveform is time-scaled on the device first; the stream holds back the samples that
        a later frame of the stage still adds to, in the same way.
        `pitch` (semitones): the waveform is pitch-shifted on the device (a plain shift: formants move with
        the pitch) between the two; the stream's length does not change.
        `live_loudness` (LUFS): the stream is ridden toward that loudness on the device, behind the other stages, by a gain
        that looks one second ahead (ft_codec_stream_begin_live); the stream holds back up to 1.1 s of output until a
        later chunk or the final one, and its length does not change."""
        return CodecStream(self, sample_rate, speed, pitch, fx, live_loudness)

    MAX_STREAMS_PER_CALL = 64     # ft_codec_stream_decode_many

    def _stream_groups(self, streams, chunks):
        """The streams of one native call after the other: (i, j, streams[i:j], lens, codes, handles), at most 64 streams
        and max_frames frames together in each (a single chunk goes alone whatever its length: the call judges it)."""
        i = 0
        while i < len(streams):
            j, total = i, 0
            while j < len(streams) and j - i < self.MAX_STREAMS_PER_CALL and (j == i or total + chunks[j].shape[1] <= self.max_frames):
                total += chunks[j].shape[1]
                j += 1
            group = streams[i:j]
            lens = np.array([c.shape[1] for c in chunks[i:j]], dtype=np.int32)
            codes = np.ascontiguousarray(np.concatenate([c.reshape(-1) for c in chunks[i:j]]))
            handles = (C.c_void_p * len(group))(*[s._h.value for s in group])
            yield i, j, group, lens, codes, handles
            i = j

    def decode_streams(self, streams: Sequence["CodecStream"], chunks: Sequence[np.ndarray],
                       final: Optional[Sequence[bool]] = None) -> List[np.ndarray]:
        """The next chunk of each of several distinct streams of this engine, in one pass through the codec per native
        call (ft_codec_stream_decode_many): chunks[j] (n_codebooks+1, T_j) integer -> float32 (T_j * frame_len,), bit
        for bit what streams[j].decode(chunks[j]) gives.  More than 64 streams, or more than max_frames frames together,
        take several calls (the streams of calls that went through stay advanced if a later one fails).
        Streams at other rates, speeds or pitches (stream(sample_rate=..., speed=..., pitch=...)) may be mixed in
        (ft_codec_stream_decode_many_at): theirs are the time-scaled / resampled samples the chunk completes, bit for
        bit what streams[j].decode(chunks[j], final[j]) gives;
        final[j] also emits the stream's tail and closes it for decoding (a chunk of 0 frames is allowed then)."""
        streams = list(streams)
        chunks = [np.ascontiguousarray(np.asarray(c), dtype=np.int32) for c in chunks]
        if len(streams) != len(chunks):
            raise ValueError("decode_streams: one chunk per stream")
        for c in chunks:
            assert c.ndim == 2 and c.shape[0] == self.R, c.shape
        for st in streams:
            st.fx.no_level("decode_streams")
        if final is not None or any(s.fx for s in streams):
            return self._decode_streams_at(streams, chunks, [False] * len(streams) if final is None else list(final))
        out: List[np.ndarray] = []
        for _, _, group, lens, codes, handles in self._stream_groups(streams, chunks):
            audio = np.empty(int(lens.sum()) * self.frame_len, dtype=np.float32)
            self._check(self.lib.ft_codec_stream_decode_many(self._h, len(group), handles, codes.ctypes.data_as(C.c_void_p),
                                                             lens.ctypes.data_as(C.c_void_p), audio.ctypes.data_as(C.c_void_p)),
                        "ft_codec_stream_decode_many")
            off = 0
            for s, T in zip(group, lens):
                s.frames += int(T)
                out.append(audio[off:off + int(T) * self.frame_len])
                off += int(T) * self.frame_len
        return out

    def _decode_streams_at(self, streams, chunks, final) -> List[np.ndarray]:
        if len(final) != len(streams):
            raise ValueError("decode_streams: one final flag per stream")
        out: List[np.ndarray] = []
        for i, j, group, lens, codes, handles in self._stream_groups(streams, chunks):
            fin = np.array([1 if f else 0 for f in final[i:j]], dtype=np.int32)
            # room for everything each stream can emit: its outputs up to the end of the chunk, less those it gave
            cap = sum(s._cap(int(T) * self.frame_len) for s, T in zip(group, lens))
            audio = np.empty(max(cap, 1), dtype=np.float32)
            out_lens = np.zeros(len(group), dtype=np.int64)
            self._check(self.lib.ft_codec_stream_decode_many_at(
                self._h, len(group), handles, codes.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
                fin.ctypes.data_as(C.c_void_p), audio.ctypes.data_as(C.c_void_p), out_lens.ctypes.data_as(C.c_void_p)),
                "ft_codec_stream_decode_many_at")
            off = 0
            for s, T, n, f in zip(group, lens, out_lens, fin):
                s._advance(int(T), int(n), bool(f))
                out.append(audio[off:off + int(n)])
                off += int(n)
        return out

    @property
    def max_level_samples(self) -> int:
        """The longest waveform loudness() takes: the longest item a decode gives, max_frames frames at speed 0.5 and 48 kHz."""
        return -(-2 * int(self.max_frames) * self.frame_len * 48000 // CODEC_RATE)

    def loudness(self, x: np.ndarray, sample_rate: Optional[int] = None, target: Optional[float] = None):
        """The level stage alone on a host waveform at `sample_rate` (None: the codec's rate), on the device
        (ft_codec_loudness): measured - integrated loudness per BS.1770, sample peak - and, with `target` (LUFS, as
        decode's `loudness`), levelled.  Returns (LevelInfo, y): y is x times the one gain, x's own samples without a target."""
        fx = OutputFx.of(sample_rate=sample_rate, loudness=target)
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        y = np.empty(len(x), dtype=np.float32)
        info = L.ft_level_info()
        self._check(self.lib.ft_codec_loudness(self._h, x.ctypes.data_as(C.c_void_p), len(x), fx.wav_rate, fx.native_level,
                                               C.byref(info), y.ctypes.data_as(C.c_void_p)), "ft_codec_loudness")
        return LevelInfo.of(info), y

    def ride(self, x: np.ndarray, sample_rate: Optional[int] = None, target: Optional[float] = None, nodes: bool = False):
        """The ride stage alone on a host waveform at `sample_rate` (None: the codec's rate), on the device (ft_codec_ride):
        x as one stream ridden toward `target` (LUFS, as stream's `live_loudness`; None: x's own samples).  Returns y, or
        (y, g) with `nodes`: the ceil(n / H) + 1 gains at the hop borders."""
        fx = OutputFx.of(sample_rate=sample_rate, live_loudness=target)
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        y = np.empty(len(x), dtype=np.float32)
        H = fx.wav_rate // 10
        g = np.empty(-(-len(x) // H) + 1, dtype=np.float32)
        self._check(self.lib.ft_codec_ride(self._h, x.ctypes.data_as(C.c_void_p), len(x), fx.wav_rate, fx.native_live,
                                           y.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)), "ft_codec_ride")
        return (y, g) if nodes else y

    def ride_plan(self, sample_rate: Optional[int], n_in: int, final: bool = False):
        """(final nodes, samples emitted) of a live stream after n_in samples at sample_rate (ft_ride_plan; host only)."""
        k, n = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.ft_ride_plan(OutputFx.of(sample_rate=sample_rate).wav_rate, int(n_in), 1 if final else 0,
                                          C.byref(k), C.byref(n)), "ft_ride_plan")
        return k.value, n.value

    def test_ride_streams(self, xs: Sequence[np.ndarray], sample_rate: int, target: int, cuts: Sequence[int]):
        """Test hook (ft_test_ride_streams): the waveforms xs as carried streams of the ride stage alone, fed in
        len(cuts) + 1 calls cut at the sample positions `cuts`; target in hundredths of a LUFS.  Returns (ys, nodes,
        emitted): per stream its samples and nodes, and emitted (len(cuts) + 1, B)."""
        xs = [np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1)) for x in xs]
        B = len(xs)
        n = np.array([len(x) for x in xs], dtype=np.int64)
        stride = int(max(1, n.max()))
        H = int(sample_rate) // 10
        x = np.zeros((B, stride), dtype=np.float32)
        for b, it in enumerate(xs):
            x[b, :len(it)] = it
        cuts = np.ascontiguousarray(np.asarray(list(cuts), dtype=np.int64).reshape(-1))
        y = np.zeros((B, stride), dtype=np.float32)
        g = np.zeros((B, stride // H + 2), dtype=np.float32)
        emitted = np.zeros((len(cuts) + 1, B), dtype=np.int64)
        self._check(self.lib.ft_test_ride_streams(self._h, x.ctypes.data_as(C.c_void_p), B, stride, n.ctypes.data_as(C.c_void_p),
                                                  int(sample_rate), int(target), cuts.ctypes.data_as(C.c_void_p), len(cuts),
                                                  y.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
                                                  emitted.ctypes.data_as(C.c_void_p)), "ft_test_ride_streams")
        return ([y[b, :n[b]] for b in range(B)], [g[b, :-(-int(n[b]) // H) + 1] for b in range(B)], emitted)

    def test_level_hops(self) -> np.ndarray:
        """Test hook (ft_test_level_hops): the hop sums of the last levelled call."""
        n = C.c_int64(0)
        self._check(self.lib.ft_test_level_hops(self._h, None, 0, C.byref(n)), "ft_test_level_hops")
        e = np.zeros(max(n.value, 1), dtype=np.float64)
        self._check(self.lib.ft_test_level_hops(self._h, e.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "ft_test_level_hops")
        return e[:n.value]

    def test_resample(self, x: np.ndarray, sample_rate: int) -> np.ndarray:
        """Test hook (ft_test_resample): the resampler alone on a waveform at the codec rate (zeros around it)."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        rate = int(sample_rate)
        y = np.empty(max(1, int(self.lib.ft_resampled_len(rate, len(x)))), dtype=np.float32)
        n = C.c_int64(0)
        self._check(self.lib.ft_test_resample(self._h, x.ctypes.data_as(C.c_void_p), len(x), rate,
                                              y.ctypes.data_as(C.c_void_p), C.byref(n)), "ft_test_resample")
        return y[:n.value]

    def test_timescale(self, x: np.ndarray, speed_pct: int):
        """Test hook (ft_test_timescale): the time-scale stage alone on a waveform at the codec rate (zeros around it).
        Returns (y, d): the timescaled_len samples and the alignment d_k the stage chose for every frame."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        pct = int(speed_pct)
        n_out = max(1, int(self.lib.ft_timescaled_len(pct, len(x))))
        y = np.empty(n_out, dtype=np.float32)
        d = np.zeros((n_out + 511) // 512 + 1, dtype=np.int32)
        n, k = C.c_int64(0), C.c_int32(0)
        self._check(self.lib.ft_test_timescale(self._h, x.ctypes.data_as(C.c_void_p), len(x), pct, y.ctypes.data_as(C.c_void_p),
                                               C.byref(n), d.ctypes.data_as(C.c_void_p), C.byref(k)), "ft_test_timescale")
        return y[:n.value], d[:k.value]

    def test_pitch(self, x: np.ndarray, speed_pct: int, cents: int):
        """Test hook (ft_test_pitch): the time-scale stage at its rational rate and the pitch stage on a waveform at the
        codec rate (zeros around it).  Returns (y, mid, d): the timescaled_len samples, the time-scaled intermediate the
        pitch stage read (x itself where that stage is absent) and the alignments d_k of its frames (none then)."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        pct, cents = int(speed_pct), int(cents)
        y = np.empty(max(1, -(-100 * len(x) // max(pct, 1))), dtype=np.float32)
        mid = np.empty(2 * len(x) + 1, dtype=np.float32)
        d = np.zeros((len(mid) + 511) // 512 + 1, dtype=np.int32)
        n, m, k = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._check(self.lib.ft_test_pitch(self._h, x.ctypes.data_as(C.c_void_p), len(x), pct, cents, y.ctypes.data_as(C.c_void_p),
                                           C.byref(n), mid.ctypes.data_as(C.c_void_p), C.byref(m), d.ctypes.data_as(C.c_void_p),
                                           C.byref(k)), "ft_test_pitch")
        return y[:n.value], mid[:m.value], d[:k.value]

    @staticmethod
    def _join_params(params) -> "L.ft_join_params":
        """(threshold, hop, keep, fade) -> the native struct, the threshold rounded to float32."""
        threshold, hop, keep, fade = params
        return L.ft_join_params(float(np.float32(threshold)), int(hop), int(keep), int(fade))

    def test_join(self, items: Sequence[np.ndarray], params, gaps: Sequence[int], started: int = 0,
                  capacity: Optional[int] = None, y: Optional[np.ndarray] = None, stride: Optional[int] = None):
        """Test hook (ft_test_join): the join stage alone on host waveforms.  Returns (y, total, cuts): y holds `capacity`
        samples (default: sum of the items and gaps plus 8), the sentinel pattern past `total`."""
        items = [np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1)) for x in items]
        B = len(items)
        n = np.array([len(x) for x in items], dtype=np.int64)
        stride = int(max(1, n.max() if B else 1)) if stride is None else int(stride)
        x = np.zeros((max(B, 1), stride), dtype=np.float32)
        for b, it in enumerate(items):
            x[b, :min(len(it), stride)] = it[:stride]
        g = np.ascontiguousarray(np.asarray(gaps, dtype=np.int64).reshape(-1))
        cap = int(n.sum() + g.sum()) + 8 if capacity is None else int(capacity)
        if y is None:
            y = np.zeros(max(cap, 1), dtype=np.float32)
        total = C.c_int64(0)
        cuts = np.zeros((max(B, 1), 2), dtype=np.int64)
        jp = self._join_params(params)
        self._check(self.lib.ft_test_join(self._h, x.ctypes.data_as(C.c_void_p), B, stride, n.ctypes.data_as(C.c_void_p),
                                          C.byref(jp), g.ctypes.data_as(C.c_void_p), int(started),
                                          y.ctypes.data_as(C.c_void_p), cap, C.byref(total), cuts.ctypes.data_as(C.c_void_p)),
                    "ft_test_join")
        return y, total.value, cuts[:B]

    MAX_CLIPS_PER_INTAKE = 64     # ft_codec_intake, ft_codec_encode_items
    MAX_INTAKE_BYTES = 1 << 30

    def _intake_args(self, what, clips, params, loudness, channel):
        """The checked arguments of an intake call: (items, keep-alive, join params, level).  clips: (WAV bytes, WavInfo of
        wavfile.parse_wav) each; the frames are handed to the device as they lie in the bytes."""
        from .wavfile import FORMATS, WIDTH
        clips = list(clips)
        if not 1 <= len(clips) <= self.MAX_CLIPS_PER_INTAKE:
            raise ValueError(f"{what}: {len(clips)} clips, a call takes 1 to {self.MAX_CLIPS_PER_INTAKE}")
        if channel is not None and (isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or channel < 0):
            raise ValueError(f"{what}: channel must be None or a channel index, got {channel!r}")
        level = OutputFx.of(loudness=loudness).native_level
        jp = self._join_params(params)
        if not jp.threshold >= 0 or jp.hop < 1 or jp.keep < 0 or jp.fade < 0:
            raise ValueError(f"{what}: bad join parameters {tuple(params)!r}")
        items = (L.ft_intake_item * len(clips))()
        keep, raw = [], 0
        for b, (data, info) in enumerate(clips):
            if info.fmt not in FORMATS:
                raise ValueError(f"{what}: clip {b}: unknown sample format {info.fmt!r}")
            if channel is not None and channel >= info.channels:
                raise ValueError(f"{what}: clip {b}: channel {channel} of a file with {info.channels} channels")
            if self.lib.ft_intake_len(int(info.rate), 0) < 0:
                raise ValueError(f"{what}: clip {b}: unsupported input sample rate {info.rate}: integers in [8000, 192000] whose "
                                 "ratio to 44100 reduces to L / M with L <= 640 and a filter window within the kernel's stage")
            buf = np.frombuffer(data, dtype=np.uint8)
            size = info.n_frames * info.channels * WIDTH[info.fmt]
            if info.n_frames < 1 or info.data_offset < 0 or info.data_offset + size > len(buf):
                raise ValueError(f"{what}: clip {b}: its frames lie outside its bytes")
            raw += -(-size // 16) * 16
            keep.append(buf)
            items[b] = L.ft_intake_item(buf.ctypes.data + info.data_offset, info.n_frames, info.rate, info.channels,
                                        FORMATS.index(info.fmt), -1 if channel is None else int(channel))
        if raw > self.MAX_INTAKE_BYTES:
            raise ValueError(f"{what}: {raw} raw bytes, a call takes {self.MAX_INTAKE_BYTES}")
        return items, keep, jp, level

    def intake(self, clips, params=(0.0, 1, 0, 0), loudness: Optional[float] = None, channel: Optional[int] = None):
        """The reference intake without the encoder (ft_codec_intake): clips - (WAV bytes, WavInfo) each, at most 64 and
        2^30 raw bytes - decoded, mixed down (`channel`: that channel alone), resampled to 44.1 kHz, levelled toward
        `loudness` (LUFS, as decode's; None: measured only) and trimmed and faded by the join stage with `params`
        ((threshold, hop, keep, fade); (0, 1, 0, 0): nothing), all on the device.  Returns (pieces, reports): the float32
        samples the encoder would be given, per clip, and one IntakeReport each."""
        items, keep, jp, level = self._intake_args("intake", clips, params, loudness, channel)
        B = len(items)
        cap = sum(int(self.lib.ft_intake_len(it.rate, it.n_frames)) for it in items)
        audio = np.empty(max(cap, 1), dtype=np.float32)
        lens = np.zeros(B, dtype=np.int64)
        infos = (L.ft_intake_info * B)()
        self._check(self.lib.ft_codec_intake(self._h, B, items, C.byref(jp), level, audio.ctypes.data_as(C.c_void_p), cap,
                                             lens.ctypes.data_as(C.c_void_p), infos), "ft_codec_intake")
        del keep
        ends = np.cumsum(lens)
        return [audio[int(e - n):int(e)] for e, n in zip(ends, lens)], [IntakeReport.of(i) for i in infos]

    def encode_items(self, clips, params=(0.0, 1, 0, 0), loudness: Optional[float] = None, channel: Optional[int] = None):
        """intake() with the encoder behind it, the prepared pieces never leaving the device (ft_codec_encode_items).
        Returns (codes, reports): per clip the (n_codebooks + 1, frames) int64 codes - what encode() gives for the piece
        intake() returns, bit for bit - or None where the report's status is not 0."""
        if not self.with_encoder:
            raise RuntimeError("codec encoder not built (CodecHipEngine(..., with_encoder=True))")
        items, keep, jp, level = self._intake_args("encode_items", clips, params, loudness, channel)
        B = len(items)
        cap = sum(-(-int(self.lib.ft_intake_len(it.rate, it.n_frames)) // self.enc_frame_len) for it in items)
        codes = np.zeros(self.R * max(cap, 1), dtype=np.int32)
        infos = (L.ft_intake_info * B)()
        self._check(self.lib.ft_codec_encode_items(self._h, B, items, C.byref(jp), level, codes.ctypes.data_as(C.c_void_p), cap,
                                                   infos), "ft_codec_encode_items")
        del keep
        out, at = [], 0
        for i in infos:
            if i.status != 0:
                out.append(None)
                continue
            out.append(codes[at:at + self.R * i.frames].reshape(self.R, i.frames).astype(np.int64))
            at += self.R * i.frames
        return out, [IntakeReport.of(i) for i in infos]

    def room(self, audio: np.ndarray, clip, regions=(), sample_rate: Optional[int] = None, params=None, ceiling: bool = True):
        """The room stage on a host waveform at `sample_rate` (None: the codec's rate), on the device (ft_codec_room): `clip` -
        (WAV bytes, WavInfo of wavfile.parse_wav), a room's impulse response - prepared by the intake launches, brought to the
        output rate, cut, faded and normalised; the programme, weighted by `regions` - (a, e, send) each, a send in hundredths
        of a dB of attenuation or -1 for muted; sorted and disjoint, at most 4096 - convolved with it, added to the dry
        programme and, with `ceiling`, held under -1 dBFS (False: a mix stage follows and has the ceiling).  `params`: a
        room.RoomParams (room.room_params makes one from a Room), or None for a default Room's.  Returns (y, RoomReport); y
        is the programme's length plus the tail."""
        from .room import Room, RoomParams, room_params
        what = "room"
        rate = OutputFx.of(sample_rate=sample_rate).wav_rate
        if params is None:
            params = room_params(Room(b""), rate)
        if not isinstance(params, RoomParams):
            raise ValueError(f"{what}: params must be a RoomParams, got {type(params).__name__}")
        if not isinstance(ceiling, bool):
            raise ValueError(f"{what}: ceiling must be True or False, got {ceiling!r}")
        items, keep, _, _ = self._intake_args(what, [clip], (0.0, 1, 0, 0), None, None if params.channel < 0 else params.channel)
        x = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
        if len(x) < 1:
            raise ValueError(f"{what}: an empty programme")
        table = send_region_table(what, regions, len(x))
        rp = L.ft_room_params(params.channel, params.normalize, params.wet, params.dry, params.send, 1 if ceiling else 0,
                              params.offset, params.length, params.fade, params.predelay, params.tail)
        nh = int(self.lib.ft_resampled_len(rate, int(self.lib.ft_intake_len(items[0].rate, items[0].n_frames))))
        N = C.c_int64(0)
        self._check(self.lib.ft_room_plan(rate, len(x), nh, C.byref(rp), None, C.byref(N)), "ft_room_plan")
        y = np.empty(N.value, dtype=np.float32)
        total = C.c_int64(0)
        info = L.ft_room_info()
        self._check(self.lib.ft_codec_room(self._h, x.ctypes.data_as(C.c_void_p), len(x), rate, *table, items, C.byref(rp),
                                           y.ctypes.data_as(C.c_void_p), N.value, C.byref(total), C.byref(info)), "ft_codec_room")
        del keep
        return y[:total.value], RoomReport.of(info)

    def flac(self, audio: np.ndarray, sample_rate: Optional[int] = None, blocksize: int = 4096):
        """A finished waveform as a FLAC file, packed on the device (ft_codec_flac): `audio` is float32 - quantised there by
        _to_wav_bytes's rule, so the file decodes to the 16-bit WAV's samples - or int16, taken as it is; (N,) mono or (N, 2)
        left then right.  Fixed predictors only: the stream is stated to the bit in include/fishtts_hip.h.  Returns
        (bytes, FlacReport)."""
        what = "flac"
        rate = OutputFx.of(sample_rate=sample_rate).wav_rate
        if isinstance(blocksize, bool) or not isinstance(blocksize, (int, np.integer)) or int(blocksize) not in FLAC_BLOCKSIZES:
            raise ValueError(f"{what}: blocksize must be one of {FLAC_BLOCKSIZES}, got {blocksize!r}")
        x = _flac_samples(what, audio)
        n, channels = x.shape[0], x.ndim
        cap = int(self.lib.ft_flac_bound(n, channels, int(blocksize)))
        if cap < 0:
            raise ValueError(f"{what}: {n} samples are more than a call takes (2^28)")
        out = np.empty(cap, dtype=np.uint8)
        fp = L.ft_flac_params(int(blocksize), 0)
        total = C.c_int64(0)
        info = L.ft_flac_info()
        self._check(self.lib.ft_codec_flac(self._h, x.ctypes.data_as(C.c_void_p), 1 if x.dtype == np.int16 else 0, n, channels, rate,
                                           C.byref(fp), out.ctypes.data_as(C.c_void_p), cap, C.byref(total), C.byref(info)),
                    "ft_codec_flac")
        return out[:total.value].tobytes(), FlacReport.of(info)

    def flac_stream(self, sample_rate: Optional[int] = None, channels: int = 1, blocksize: int = 4096, dtype=np.float32) -> FlacStream:
        """A stream of the live FLAC stage (ft_codec_flac_stream_begin) for `channels` (1 or 2) of `dtype` samples - float32,
        quantised on the device by flac()'s rule, or int16, taken as they are.  The FlacStream's pushes concatenate to
        flac(whole)[42:] byte for byte however they are cut, and its head() after the final push is flac(whole)[:42]."""
        what = "flac_stream"
        rate = OutputFx.of(sample_rate=sample_rate).wav_rate
        if isinstance(blocksize, bool) or not isinstance(blocksize, (int, np.integer)) or int(blocksize) not in FLAC_BLOCKSIZES:
            raise ValueError(f"{what}: blocksize must be one of {FLAC_BLOCKSIZES}, got {blocksize!r}")
        if isinstance(channels, bool) or channels not in (1, 2):
            raise ValueError(f"{what}: channels must be 1 or 2, got {channels!r}")
        try:
            dt = np.dtype(dtype)
        except TypeError:
            dt = None
        if dt not in (np.dtype(np.float32), np.dtype(np.int16)):
            raise ValueError(f"{what}: dtype must be float32 or int16, got {dtype!r}")
        fp = L.ft_flac_params(int(blocksize), 0)
        h = C.c_void_p()
        self._check(self.lib.ft_codec_flac_stream_begin(self._h, int(channels), 1 if dt == np.int16 else 0, rate, C.byref(fp),
                                                        C.byref(h)), "ft_codec_flac_stream_begin")
        return FlacStream(self, h, dt, int(channels), int(blocksize))

    def _room_live_args(self, what: str, clip, sample_rate, params):
        """(rate, IR item array, what keeps its bytes alive, ft_room_params with ceiling 0, tail) of a live room call, checked
        as room() checks them; the tail is Room's tl for these values (ft_room_plan)."""
        from .room import Room, RoomParams, room_params
        rate = OutputFx.of(sample_rate=sample_rate).wav_rate
        if params is None:
            params = room_params(Room(b""), rate)
        if not isinstance(params, RoomParams):
            raise ValueError(f"{what}: params must be a RoomParams, got {type(params).__name__}")
        items, keep, _, _ = self._intake_args(what, [clip], (0.0, 1, 0, 0), None, None if params.channel < 0 else params.channel)
        rp = L.ft_room_params(params.channel, params.normalize, params.wet, params.dry, params.send, 0,
                              params.offset, params.length, params.fade, params.predelay, params.tail)
        nh = int(self.lib.ft_resampled_len(rate, int(self.lib.ft_intake_len(items[0].rate, items[0].n_frames))))
        N = C.c_int64(0)
        self._check(self.lib.ft_room_plan(rate, 1, nh, C.byref(rp), None, C.byref(N)), "ft_room_plan")
        return rate, items, keep, rp, N.value - 1

    def room_stream(self, clip, sample_rate: Optional[int] = None, params=None) -> RoomStream:
        """A stream of the live room stage (ft_codec_room_stream_begin): the impulse response `clip` is prepared here, as
        room() prepares it, and stays on the device; the RoomStream's pushes concatenate to room(..., ceiling=False) of the
        whole programme with every push's regions moved to the timeline, bit for bit, however they are cut.  The stage has no
        ceiling: a mix stream behind it (mix_stream, with bedless=True where there is no bed) holds the piece under -1 dBFS."""
        rate, items, keep, rp, tail = self._room_live_args("room_stream", clip, sample_rate, params)
        h = C.c_void_p()
        self._check(self.lib.ft_codec_room_stream_begin(self._h, rate, items, C.byref(rp), C.byref(h)), "ft_codec_room_stream_begin")
        del keep                                           # (begin has prepared the response: its bytes are no longer read)
        return RoomStream(self, h, tail)

    def room_live(self, audio, clip, regions=(), sample_rate: Optional[int] = None, params=None):
        """The live room stage on a whole host waveform (ft_codec_room_live): what a room stream gives for it in one final
        push - room(..., ceiling=False), bit for bit.  `audio` may be empty: the tail alone, zeros.  Returns (y, RoomReport)."""
        what = "room_live"
        rate, items, keep, rp, tail = self._room_live_args(what, clip, sample_rate, params)
        x = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))
        table = send_region_table(what, regions, len(x))
        cap = len(x) + tail
        y = np.empty(max(cap, 1), dtype=np.float32)
        total = C.c_int64(0)
        info = L.ft_room_info()
        self._check(self.lib.ft_codec_room_live(self._h, x.ctypes.data_as(C.c_void_p), len(x), rate, *table, items, C.byref(rp),
                                                y.ctypes.data_as(C.c_void_p), cap, C.byref(total), C.byref(info)), "ft_codec_room_live")
        del keep
        return y[:total.value], RoomReport.of(info)

    def test_room_conv(self, xs: np.ndarray, hn: np.ndarray, predelay: int, N: int) -> np.ndarray:
        """Test hook: the room stage's convolution launches alone on the taps hn (ft_test_room_conv) -> c[0 .. N)."""
        xs = np.ascontiguousarray(np.asarray(xs, dtype=np.float32).reshape(-1))
        hn = np.ascontiguousarray(np.asarray(hn, dtype=np.float32).reshape(-1))
        c = np.empty(max(int(N), 1), dtype=np.float32)
        self._check(self.lib.ft_test_room_conv(self._h, xs.ctypes.data_as(C.c_void_p), len(xs), hn.ctypes.data_as(C.c_void_p),
                                               len(hn), int(predelay), int(N), c.ctypes.data_as(C.c_void_p)), "ft_test_room_conv")
        return c[:int(N)]

    def mix(self, x: np.ndarray, bed, sample_rate: Optional[int] = None, params=None, nodes: bool = False):
        """The mix stage on a host waveform at `sample_rate` (None: the codec's rate), on the device (ft_codec_mix): `bed` -
        (WAV bytes, WavInfo of wavfile.parse_wav) - prepared by the intake launches, brought to the output rate, looped or
        cut to the programme's length, ducked where x is loud, added to x and held under -1 dBFS.  `params`: a
        mix.MixParams (mix.bed_params makes one from a Bed), or None for a default Bed's.  Returns (y, MixReport), or
        (y, MixReport, D) with `nodes`: the duck D_k in hundredths of a dB at the hops + 1 hop borders."""
        return self._mix_whole("mix", x, bed, None, sample_rate, params, nodes)

    def mix_stereo(self, x: np.ndarray, bed, regions=(), sample_rate: Optional[int] = None, params=None, nodes: bool = False):
        """The stereo mix stage on a mono host waveform (ft_codec_mix_stereo): mix() with two channels out.  `regions`:
        (a, e, pan) each - samples [a, e) of x sit at `pan`, an integer in [-100, 100] with -100 hard left; sorted and
        disjoint, at most 4096; what no region holds sits in the centre.  `bed`: as mix()'s, its first two channels the two
        sides (a mono file, or a `channel` in params: that channel on both), or None for a panned programme without a bed.
        Returns (y, MixReport), or (y, MixReport, D) with `nodes`; y is (N, 2) float32, left then right."""
        return self._mix_whole("mix_stereo", x, bed, list(regions), sample_rate, params, nodes)

    def _mix_whole(self, what: str, x, bed, regions, sample_rate, params, nodes: bool):
        """mix(), and with `regions` (None: mono) mix_stereo(): the plan, the buffers, the call and the report."""
        stereo = regions is not None
        rate, items, keep, mp = self._mix_args(what, bed, sample_rate, params, bedless=stereo)
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        if len(x) < 1:
            raise ValueError(f"{what}: an empty programme")
        table = pan_region_table(what, regions, len(x)) if stereo else ()
        N, hop, nn = C.c_int64(0), C.c_int32(0), C.c_int64(0)
        self._check(self.lib.ft_mix_plan(rate, len(x), mp.lead, mp.tail, C.byref(N), C.byref(hop), C.byref(nn)), "ft_mix_plan")
        y = np.empty((N.value, 2) if stereo else N.value, dtype=np.float32)
        D = np.empty(nn.value, dtype=np.int32)
        total = C.c_int64(0)
        info = L.ft_mix_info()
        fn = "ft_codec_mix_stereo" if stereo else "ft_codec_mix"
        self._check(getattr(self.lib, fn)(self._h, x.ctypes.data_as(C.c_void_p), len(x), rate, *table, items, C.byref(mp),
                                          y.ctypes.data_as(C.c_void_p), N.value, C.byref(total),
                                          D.ctypes.data_as(C.c_void_p) if nodes else None, C.byref(info)), fn)
        del keep
        rep = MixReport.of(info)
        return (y[:total.value], rep, D) if nodes else (y[:total.value], rep)

    @staticmethod
    def _mix_params(params) -> "L.ft_mix_params":
        return L.ft_mix_params(params.bed_loudness, params.channel, params.depth, params.threshold, params.attack, params.release,
                               params.lead, params.tail, params.fade_in, params.fade_out, params.offset, params.loop, 0)

    def _mix_args(self, what: str, bed, sample_rate, params, bedless: bool = False):
        """(rate, bed item array, what keeps its bytes alive, ft_mix_params) of a mix call, checked as mix() checks them.
        `bedless`: the call takes None for the bed (the item array is then None)."""
        from .mix import Bed, MixParams, bed_params
        rate = OutputFx.of(sample_rate=sample_rate).wav_rate
        if params is None:
            params = bed_params(Bed(b""), rate)
        if not isinstance(params, MixParams):
            raise ValueError(f"{what}: params must be a MixParams, got {type(params).__name__}")
        items, keep = None, None
        if bed is not None or not bedless:
            items, keep, _, _ = self._intake_args(what, [bed], (0.0, 1, 0, 0), None, None if params.channel < 0 else params.channel)
        return rate, items, keep, self._mix_params(params)

    def mix_live_plan(self, sample_rate: Optional[int], params, n_in: int, final: bool = False):
        """(samples emitted, final limiter nodes) of a mix stream after n_in programme samples (ft_mix_live_plan; host only)."""
        mp = self._mix_params(params)
        n, k = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.ft_mix_live_plan(OutputFx.of(sample_rate=sample_rate).wav_rate, C.byref(mp), int(n_in),
                                              1 if final else 0, C.byref(n), C.byref(k)), "ft_mix_live_plan")
        return n.value, k.value

    def mix_live(self, x: np.ndarray, bed, sample_rate: Optional[int] = None, params=None, nodes: bool = False):
        """The live mix stage on a whole host waveform (ft_codec_mix_live): what a mix stream gives for x in one final push -
        mix()'s bed, duck and sum, held under -1 dBFS by a look-ahead limiter instead of one gain.  x may be empty.  Returns
        (y, MixLiveReport), or (y, MixLiveReport, D, L) with `nodes`: the duck and the limiter's depth in hundredths of a dB at
        the hops + 1 hop borders."""
        return self._mix_live("mix_live", x, bed, None, sample_rate, params, nodes)

    def mix_live_stereo(self, x: np.ndarray, bed, regions=(), sample_rate: Optional[int] = None, params=None, nodes: bool = False):
        """The live stereo mix stage on a whole mono host waveform (ft_codec_mix_live_stereo): what a stereo mix stream gives
        for x in one final push - mix_live() with two channels out, x panned by `regions` and the bed's two sides kept apart
        as in mix_stereo(), one limiter for both channels.  x may be empty; `bed` may be None.  Returns (y, MixLiveReport), or
        (y, MixLiveReport, D, L) with `nodes`; y is (N, 2) float32, left then right."""
        return self._mix_live("mix_live_stereo", x, bed, list(regions), sample_rate, params, nodes)

    def _mix_live(self, what: str, x, bed, regions, sample_rate, params, nodes: bool):
        """mix_live(), and with `regions` (None: mono) mix_live_stereo(): the plan, the buffers, the call and the report."""
        stereo = regions is not None
        rate, items, keep, mp = self._mix_args(what, bed, sample_rate, params, bedless=stereo)
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
        table = pan_region_table(what, regions, len(x)) if stereo else ()
        N = mp.lead + len(x) + mp.tail
        nn = -(-N // (rate // 50)) + 1
        y = np.empty((max(N, 1), 2) if stereo else max(N, 1), dtype=np.float32)
        D, Lk = np.empty(nn, dtype=np.int32), np.empty(nn, dtype=np.int32)
        total = C.c_int64(0)
        info = L.ft_mix_live_info()
        fn = "ft_codec_mix_live_stereo" if stereo else "ft_codec_mix_live"
        self._check(getattr(self.lib, fn)(self._h, x.ctypes.data_as(C.c_void_p), len(x), rate, *table, items, C.byref(mp),
                                          y.ctypes.data_as(C.c_void_p), N, C.byref(total),
                                          D.ctypes.data_as(C.c_void_p) if nodes else None,
                                          Lk.ctypes.data_as(C.c_void_p) if nodes else None, C.byref(info)), fn)
        del keep
        rep = MixLiveReport.of(info)
        return (y[:total.value], rep, D, Lk) if nodes else (y[:total.value], rep)

    def mix_stream(self, bed, sample_rate: Optional[int] = None, params=None, stereo: bool = False,
                   bedless: bool = False) -> MixStream:
        """A stream of the live mix stage (ft_codec_mix_stream_begin): the bed is prepared here and stays on the device; the
        MixStream's pushes concatenate to mix_live() of the whole programme, bit for bit, however they are cut.  `stereo`: a
        stream of the live stereo mix stage (ft_codec_mix_stream_begin_stereo) - a StereoMixStream, whose
        push(x, regions=(), final=False) takes the pan regions of that push, relative to it, and returns (frames, 2) arrays
        that concatenate to mix_live_stereo(); `bed` may then be None.  `bedless` (mono, `bed` None): the limiter alone
        (ft_codec_mix_stream_begin_bare) - the live mix stage with the bed term +0.0, for a stream with a room and no bed;
        `params` None: mix.bare_params()."""
        if not isinstance(bedless, bool):
            raise ValueError(f"mix_stream: bedless must be True or False, got {bedless!r}")
        if bedless and (stereo or bed is not None):
            raise ValueError("mix_stream: bedless=True is the mono stream without a bed (a stereo stream takes bed=None as it is)")
        if bedless and params is None:
            from .mix import bare_params
            params = bare_params()                         # no duck window to wait for: 160 ms held back
        rate, items, keep, mp = self._mix_args("mix_stream", bed, sample_rate, params, bedless=stereo or bedless)
        fn = "ft_codec_mix_stream_begin_stereo" if stereo else "ft_codec_mix_stream_begin"
        h = C.c_void_p()
        if bedless:
            fn = "ft_codec_mix_stream_begin_bare"
            self._check(self.lib.ft_codec_mix_stream_begin_bare(self._h, rate, C.byref(mp), C.byref(h)), fn)
            return MixStream(self, h, mp, rate)
        self._check(getattr(self.lib, fn)(self._h, rate, items, C.byref(mp), C.byref(h)), fn)
        del keep                                           # (begin has prepared the bed: its bytes are no longer read)
        return (StereoMixStream if stereo else MixStream)(self, h, mp, rate)

    MAX_ITEMS_PER_JOIN = 64       # ft_codec_decode_join

    def decode_join(self, codes_list: Sequence[np.ndarray], sample_rate: Optional[int] = None, speed: Optional[float] = None,
                    pitch: Optional[float] = None, params=(0.0, 1, 0, 0), gaps: Optional[Sequence[int]] = None,
                    started: bool = False, fx: Optional[OutputFx] = None, loudness: Optional[float] = None,
                    levels: Optional[list] = None, item_fx: Optional[Sequence[OutputFx]] = None):
        """The utterances of one document - codes_list[i] (n_codebooks+1, T_i) integer - decoded at `sample_rate`, `speed`
        and `pitch` (as decode) and joined on the device into one waveform (ft_codec_decode_join): each trimmed to its
        loud part, faded at the cuts and laid out behind gaps[i] samples of silence.  `params`: (threshold, hop, keep,
        fade), sample counts at the output rate; (0, 1, 0, 0) is plain concatenation with gaps.  `started`: audio of the
        document went out before this call (the first piece then gets its gap too).  Consecutive items go into native
        calls of at most 64 items and max_frames frames (ft_join_groups), `started` carried from call to call, the calls'
        outputs concatenated here - a piece depends on its own item only, so the grouping does not show.  `loudness` (LUFS,
        as decode): every item is levelled on its own before the join finds its edges (ft_codec_decode_join_level), so the
        threshold acts on the levelled samples - an absolute threshold such as synthesize_long's silence_db then means the
        same for every item; `levels`: a list that receives one LevelInfo per item.  `item_fx`: one checked OutputFx per item
        instead of the call's one chain - the lines of a script, each at its own pace, pitch and level
        (ft_codec_decode_join_items): item i's samples before the join are those of decode(codes_list[i], fx=item_fx[i]), bit
        for bit; the chains travel with their items through the grouping; all share one rate (the result is one waveform)
        and none is live, ValueError otherwise; `levels` then receives every item's LevelInfo, the empty result for an item
        without a level.  Returns (audio float32, cuts (n, 2) int64: the samples [a, e) kept of every item)."""
        if item_fx is not None:
            item_fx = list(item_fx)
            if len(item_fx) != len(codes_list):
                raise ValueError("decode_join: one item_fx entry per item")
            for f in item_fx:
                if not isinstance(f, OutputFx):
                    raise ValueError(f"decode_join: item_fx holds {f!r}, expected a checked OutputFx")
                f.no_live()
            if len({f.wav_rate for f in item_fx}) > 1:
                raise ValueError("decode_join: the items of a call share one sample rate (the result is one waveform), got "
                                 f"{sorted({f.wav_rate for f in item_fx})}")
            if item_fx:
                fx = OutputFx(rate=item_fx[0].rate)
        fx = OutputFx.of(sample_rate, speed, pitch, loudness) if fx is None else fx
        fx.no_live()
        items = [np.ascontiguousarray(np.asarray(c), dtype=np.int32) for c in codes_list]
        for c in items:
            if c.ndim != 2 or c.shape[0] != self.R:
                raise ValueError(f"decode_join: codes of shape {c.shape}, expected ({self.R}, T)")
        n = len(items)
        g = np.zeros(n, dtype=np.int64) if gaps is None else np.ascontiguousarray(np.asarray(gaps, dtype=np.int64).reshape(-1))
        if len(g) != n:
            raise ValueError("decode_join: one gap per item")
        if n and g.min() < 0:
            raise ValueError("decode_join: a negative gap")
        jp = self._join_params(params)
        if not jp.threshold >= 0 or jp.hop < 1 or jp.keep < 0 or jp.fade < 0:
            raise ValueError(f"decode_join: bad join parameters {tuple(params)!r}")
        lens = np.array([c.shape[1] for c in items], dtype=np.int32)
        ends = np.zeros(max(n, 1), dtype=np.int32)
        ng = self.lib.ft_join_groups(lens.ctypes.data_as(C.c_void_p), n, int(self.max_frames), ends.ctypes.data_as(C.c_void_p))
        if ng < 0:
            raise ValueError(f"decode_join: an item longer than max_frames ({self.max_frames}) frames")
        out, cuts, i, begun = [], np.zeros((n, 2), dtype=np.int64), 0, bool(started)
        for j in (int(e) for e in ends[:ng]):
            B, T = j - i, max(1, int(lens[i:j].max()))
            block = np.zeros((B, self.R, T), dtype=np.int32)
            for b, c in enumerate(items[i:j]):
                block[b, :, :c.shape[1]] = c
            glens = np.ascontiguousarray(lens[i:j])
            chains = [fx] * B if item_fx is None else item_fx[i:j]
            cap = sum(f.out_len(int(t) * self.frame_len) for f, t in zip(chains, glens)) + int(g[i:j].sum())
            audio = np.empty(max(cap, 1), dtype=np.float32)
            total = C.c_int64(0)
            gcuts = np.zeros((B, 2), dtype=np.int64)
            ggaps = np.ascontiguousarray(g[i:j])
            if item_fx is not None:
                infos = (L.ft_level_info * B)()
                native = (L.ft_item_fx * B)(*[L.ft_item_fx(f.pct or 100, f.cents or 0, f.native_level) for f in chains])
                self._check(self.lib.ft_codec_decode_join_items(
                    self._h, block.ctypes.data_as(C.c_void_p), B, T, glens.ctypes.data_as(C.c_void_p), fx.wav_rate, native,
                    C.byref(jp), ggaps.ctypes.data_as(C.c_void_p), 1 if begun else 0, audio.ctypes.data_as(C.c_void_p), cap,
                    C.byref(total), gcuts.ctypes.data_as(C.c_void_p), infos), "ft_codec_decode_join_items")
                if levels is not None:
                    levels.extend(LevelInfo.of(i) for i in infos)
            elif fx.level is None:
                self._check(self.lib.ft_codec_decode_join(
                    self._h, block.ctypes.data_as(C.c_void_p), B, T, glens.ctypes.data_as(C.c_void_p),
                    *fx.native, C.byref(jp), ggaps.ctypes.data_as(C.c_void_p), 1 if begun else 0, audio.ctypes.data_as(C.c_void_p), cap,
                    C.byref(total), gcuts.ctypes.data_as(C.c_void_p)), "ft_codec_decode_join")
            else:
                infos = (L.ft_level_info * B)()
                self._check(self.lib.ft_codec_decode_join_level(
                    self._h, block.ctypes.data_as(C.c_void_p), B, T, glens.ctypes.data_as(C.c_void_p),
                    *fx.native, fx.native_level, C.byref(jp), ggaps.ctypes.data_as(C.c_void_p), 1 if begun else 0,
                    audio.ctypes.data_as(C.c_void_p), cap, C.byref(total), gcuts.ctypes.data_as(C.c_void_p), infos),
                    "ft_codec_decode_join_level")
                if levels is not None:
                    levels.extend(LevelInfo.of(i) for i in infos)
            out.append(audio[:total.value])
            cuts[i:j] = gcuts
            begun = begun or total.value > 0
            i = j
        return (np.concatenate(out) if out else np.zeros(0, dtype=np.float32)), cuts

    def decode(self, codes: np.ndarray, lens: Optional[np.ndarray] = None, sample_rate: Optional[int] = None,
               speed: Optional[float] = None, pitch: Optional[float] = None, fx: Optional[OutputFx] = None,
               loudness: Optional[float] = None, levels: Optional[list] = None) -> np.ndarray:
        """codes (B, n_codebooks+1, T) or (n_codebooks+1, T) integer -> float32 (B, T*frame_len).
        `sample_rate`, `speed`, `pitch` (OutputFx.of), or `fx`, the checked value itself: (B, max_b fx.out_len(lens[b] *
        frame_len)); row b holds its fx.out_len samples, zeros after them.
        `sample_rate`: resampled on the device.  `speed`: time-scaled on the device (before the resampler).
        `pitch` (semitones): pitch-shifted on the device, between the two; a plain shift (formants move with the pitch)
        that leaves every length as it is.  `loudness` (LUFS): every row is brought to that integrated loudness on the
        device, behind the other stages (ft_codec_decode_level); `levels`: a list that receives one LevelInfo per row."""
        fx = OutputFx.of(sample_rate, speed, pitch, loudness) if fx is None else fx
        fx.no_live()
        codes = np.asarray(codes)
        if codes.ndim == 2:
            codes = codes[None]
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        B, R, T = codes.shape
        assert R == self.R, codes.shape
        lens_a = np.full(B, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
        if fx:
            width = max(fx.out_len(int(n) * self.frame_len) for n in lens_a)
            audio = np.empty((B, max(width, 1)), dtype=np.float32)
            out_lens = np.zeros(B, dtype=np.int64)
            if fx.level is not None:
                infos = (L.ft_level_info * B)()
                self._check(self.lib.ft_codec_decode_level(self._h, codes.ctypes.data_as(C.c_void_p), B, T,
                                                           lens_a.ctypes.data_as(C.c_void_p), *fx.native, fx.native_level,
                                                           audio.ctypes.data_as(C.c_void_p), out_lens.ctypes.data_as(C.c_void_p),
                                                           infos), "ft_codec_decode_level")
                if levels is not None:
                    levels.extend(LevelInfo.of(i) for i in infos)
                return audio[:, :width]
            self._check(self.lib.ft_codec_decode_fxp(self._h, codes.ctypes.data_as(C.c_void_p), B, T,
                                                     lens_a.ctypes.data_as(C.c_void_p), *fx.native,
                                                     audio.ctypes.data_as(C.c_void_p), out_lens.ctypes.data_as(C.c_void_p)),
                        "ft_codec_decode_fxp")
            return audio[:, :width]
        audio = np.empty((B, T * self.frame_len), dtype=np.float32)     # no stage (the launch trace arms through this entry point)
        self._check(self.lib.ft_codec_decode(self._h, codes.ctypes.data_as(C.c_void_p), B, T,
                                             lens_a.ctypes.data_as(C.c_void_p), audio.ctypes.data_as(C.c_void_p)),
                    "ft_codec_decode")
        return audio


class CodecStream:
    """Successive chunks of ONE utterance's codes (fish_tts/synthesizer.py:513-528 decodes each chunk from zero state;
    here the causal codec's context - the last 127 frames' K/V of every transformer layer, the last rows of every
    convolution input - is carried)."""

    def __init__(self, engine: CodecHipEngine, sample_rate: Optional[int] = None, speed: Optional[float] = None,
                 pitch: Optional[float] = None, fx: Optional[OutputFx] = None, live_loudness: Optional[float] = None):
        self.engine = engine
        self.fx = (OutputFx.of(sample_rate, speed, pitch, live_loudness=live_loudness) if fx is None else fx).no_level("a codec stream")   # falsy: no output stage, nothing held back
        self._h = C.c_void_p()
        if not self.fx:
            engine._check(engine.lib.ft_codec_stream_begin(engine._h, C.byref(self._h)), "ft_codec_stream_begin")
        elif self.fx.live is not None:
            engine._check(engine.lib.ft_codec_stream_begin_live(engine._h, *self.fx.native, self.fx.native_live, C.byref(self._h)),
                          "ft_codec_stream_begin_live")
        else:
            engine._check(engine.lib.ft_codec_stream_begin_fxp(engine._h, *self.fx.native, C.byref(self._h)),
                          "ft_codec_stream_begin_fxp")
        self.frames = 0
        self.samples_out = 0       # samples handed out so far (a stream at another rate, speed or pitch)
        self.finished = False      # its tail went out: no further chunk
        engine._streams.add(self)      # the engine ends its open streams before it destroys the native context

    rate = property(lambda self: self.fx.rate)      # None: the codec's own rate
    pct = property(lambda self: self.fx.pct)        # None: the model's own pace
    cents = property(lambda self: self.fx.cents)    # None: the model's own pitch
    live = property(lambda self: self.fx.live)      # None: no ride stage

    @property
    def closes_on_final(self) -> bool:
        """A final chunk closes the stream for decoding only where it has a stage: the tail that went out cannot be taken
        back.  Without one there is no tail, and the stream goes on."""
        return bool(self.fx)

    def _cap(self, n_in: int) -> int:
        """Most samples the next call can give for n_in more codec samples."""
        return self.fx.out_len(self.frames * self.engine.frame_len + n_in) - self.samples_out if self.fx else n_in

    def _advance(self, T: int, n_out: int, final: bool) -> None:
        self.frames += T
        self.samples_out += n_out
        self.finished = self.finished or (final and self.closes_on_final)

    def finish(self) -> np.ndarray:
        """The held-back tail of a stream at another rate, speed or pitch (the input taken as zero past its end); the
        stream takes no further chunk.  Empty at the codec's own rate, pace and pitch, and once the tail went out."""
        if not self.fx or self.finished:
            return np.zeros(0, dtype=np.float32)
        return self.engine.decode_streams([self], [np.zeros((self.engine.R, 0), dtype=np.int32)], [True])[0]

    def decode(self, codes: np.ndarray, final: bool = False) -> np.ndarray:
        """codes (n_codebooks+1, T) integer -> float32 (T * frame_len,): the next T frames of the stream.  At another
        rate: the resampled samples these frames complete; final=True also gives the tail (finish)."""
        e = self.engine
        codes = np.ascontiguousarray(np.asarray(codes), dtype=np.int32)
        assert codes.ndim == 2 and codes.shape[0] == e.R, codes.shape
        if self.fx:
            return e.decode_streams([self], [codes], [final])[0]
        T = codes.shape[1]
        audio = np.empty(T * e.frame_len, dtype=np.float32)
        e._check(e.lib.ft_codec_stream_decode(e._h, self._h, codes.ctypes.data_as(C.c_void_p), T,
                                              audio.ctypes.data_as(C.c_void_p)), "ft_codec_stream_decode")
        self.frames += T
        return audio

    def close(self) -> None:
        if self._h:
            self.engine.lib.ft_codec_stream_end(self.engine._h, self._h)   # the stream knows its context: a closed engine is fine
            self._h = C.c_void_p()
        self.engine._streams.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
