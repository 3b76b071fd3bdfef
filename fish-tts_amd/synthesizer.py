"""Public API of fish-tts on the MI355X path: get_instance / reset_instance / FishTTS / VoiceProfile with the
signatures, defaults and exceptions of fish_tts/synthesizer.py:47-719.  The dual-AR decode and the DAC decode
run in libfishtts_hip.so; this file is host logic only (threads, queues, WAV packing)."""
from __future__ import annotations

import contextlib
import io
import logging
import queue
import threading
import time
import wave
from dataclasses import dataclass, field
from pathlib import Path
from typing import Iterator, List, Literal, Optional, Tuple

import numpy as np

logger = logging.getLogger(__name__)

_instance: "FishTTS | None" = None
_instance_lock = threading.Lock()


@dataclass
class VoiceProfile:
    """Encoded reference audio: (num_codebooks, T) integer codes + transcript (synthesizer.py:47-65)."""
    codes: np.ndarray
    text: str = ""
    name: str = ""

    def save(self, path) -> None:
        np.save(path, self.codes)

    @classmethod
    def load(cls, path, text: str = "", name: str = "") -> "VoiceProfile":
        codes = np.load(path)
        if not name:
            name = Path(path).stem
        return cls(codes=codes, text=text, name=name)


@dataclass
class _PrefillCache:
    prompt_text: List[str] = field(default_factory=list)
    prompt_tokens: List[np.ndarray] = field(default_factory=list)
    profiles: List[VoiceProfile] = field(default_factory=list)


class FishTTS:
    """TTS synthesizer: DualARTransformer + DAC vocoder on one MI355X (one process per GPU)."""

    def __init__(self, model_dir=None, device: Literal["cpu", "cuda"] = "cuda",
                 precision: Literal["bf16", "fp16", "fp32"] = "bf16", warmup: bool = True, *,
                 _synthetic: Optional[dict] = None, gpu_index: int = 0, cache_reference_kv: bool = True,
                 max_batch: int = 1, batch_streams: int = 1):
        """`max_batch` (extension): utterance slots for synthesize_batch (lock-step batch with refill).  From 5 slots, at
        the model widths the kernels cover, `precision` "bf16" and "fp16" run the batch's frames on the MFMA launches
        (five per layer); "fp32" and narrower engines on the multi-row GEMV launches (ARHipEngine.frame_path()).
        `batch_streams` (extension): synthesize_batch of more than `max_batch` texts runs that many lock-step batches
        side by side (one engine - context, stream, weight copy - per batch, created on first use): a lock-step frame
        leaves most of the chip idle, so independent batches overlap (batch.run_batch_streams; three is the measured
        optimum at 32 slots each).
        `cache_reference_kv` (extension): keep the K/V of the reference part of the prompt on
        the device per voice, so a cloned-voice call prefills only the new text (the reference re-prefills ~700
        prompt positions per call: synthesizer.py:363-377, inference.py:779-793)."""
        from .generation import PrefixCache
        self._prefix_cache = PrefixCache() if cache_reference_kv else None
        self._max_batch = int(max_batch)
        self._batch_streams = max(1, int(batch_streams))
        self._more_engines: list = []
        self._engine_factory = None
        self.device = device
        self._precision = precision
        self._warmup = warmup
        self._engine = None
        self._tokenizer = None
        self._vocoder = None
        self._is_warmed_up = False
        self._prefill_cache = _PrefillCache()
        self._prefill_lock = threading.Lock()
        self._gen_lock = threading.Lock()  # AR calls on one context are serialised
        self._server = None                # an open BatchServer (serve()): it holds _gen_lock and serves synthesize*
        self._gpu_index = gpu_index
        if device != "cuda":
            raise RuntimeError("fish_tts_amd runs the hot path on an MI355X only: device must be 'cuda' "
                               "(there is no CPU fallback)")
        if _synthetic is not None:
            self._load_synthetic(**_synthetic)
        else:
            self._model_dir = self._ensure_model(model_dir)
            self._load_models()
        if warmup:
            self._run_warmup()

    # ------------------------------------------------------------------ loading
    def _ensure_model(self, model_dir) -> Path:
        if model_dir is not None:
            return Path(model_dir)
        # the reference downloads fishaudio/openaudio-s1-mini here (synthesizer.py:146-156)
        raise RuntimeError("model_dir is required: this build does not download checkpoints "
                           "(pass the directory holding config.json / model.pth / codec.pth / tokenizer.tiktoken)")

    def _load_models(self) -> None:
        import torch

        from .ar_engine import ARHipEngine
        from .codec_engine import CodecHipEngine
        from .config import DualARModelArgs
        from .tokenizer import IM_END_TOKEN, load_tokenizer
        from .weights import load_checkpoint
        t0 = time.perf_counter()
        args = DualARModelArgs.from_pretrained(str(self._model_dir))
        self._tokenizer = load_tokenizer(self._model_dir)
        tok = self._tokenizer

        def make_engine():
            eng = ARHipEngine(args, tok.semantic_begin_id, tok.semantic_end_id, tok.get_token_id(IM_END_TOKEN),
                              precision=self._precision, device=self._gpu_index, max_batch=self._max_batch,
                              max_new_tokens=2048 + 8)
            eng.load_state_dict(load_checkpoint(self._model_dir))
            return eng
        self._engine_factory = make_engine
        self._engine = make_engine()
        logger.info("Transformer loaded in %.1fs", time.perf_counter() - t0)
        codec_path = self._model_dir / "codec.pth"
        if codec_path.exists():
            sd = torch.load(codec_path, map_location="cpu", weights_only=True)
            inner = sd["state_dict"] if "state_dict" in sd else sd
            has_encoder = any(k.startswith(("encoder.", "generator.encoder.")) for k in inner)
            self._vocoder = CodecHipEngine(device=self._gpu_index, max_frames=2048 + 8, with_encoder=has_encoder)
            self._vocoder.load_state_dict(sd)
            logger.info("Vocoder loaded (bf16 contractions, f32 accumulate)")
        else:
            logger.warning("codec.pth not found, vocoder not loaded")

    def _load_synthetic(self, args, tokenizer, codec_args=None, seed: int = 0, with_codec: bool = True,
                        max_new_tokens: int = 2048 + 8, std=None, with_encoder: bool = False):
        from .ar_engine import ARHipEngine
        from .codec_engine import CodecHipEngine
        from .tokenizer import IM_END_TOKEN
        from .weights import random_state_dict
        import torch
        self._tokenizer = tokenizer
        dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(self._precision, torch.float32)

        def make_engine():
            eng = ARHipEngine(args, tokenizer.semantic_begin_id, tokenizer.semantic_end_id,
                              tokenizer.get_token_id(IM_END_TOKEN), precision=self._precision,
                              device=self._gpu_index, max_batch=self._max_batch, max_new_tokens=max_new_tokens)
            eng.load_state_dict(random_state_dict(args, seed=seed, dtype=dtype, std=std))
            return eng
        self._engine_factory = make_engine
        self._engine = make_engine()
        if with_codec:
            self._vocoder = CodecHipEngine.synthetic(device=self._gpu_index, max_frames=max_new_tokens, seed=seed,
                                                     args=codec_args, with_encoder=with_encoder)

    @classmethod
    def synthetic(cls, args, tokenizer, codec_args=None, precision="bf16", seed: int = 0, warmup: bool = False,
                  with_codec: bool = True, max_new_tokens: int = 2048 + 8, std=None, gpu_index: int = 0,
                  cache_reference_kv: bool = True, max_batch: int = 1, batch_streams: int = 1) -> "FishTTS":
        """Random-init model of the given shapes (no checkpoint on disk): benches, smoke tests."""
        return cls(None, "cuda", precision, warmup, gpu_index=gpu_index, cache_reference_kv=cache_reference_kv,
                   max_batch=max_batch, batch_streams=batch_streams,
                   _synthetic=dict(args=args, tokenizer=tokenizer, codec_args=codec_args, seed=seed,
                                   with_codec=with_codec, max_new_tokens=max_new_tokens, std=std))

    def _run_warmup(self) -> None:
        logger.info("Running warmup (captures the frame graph)...")
        t0 = time.perf_counter()
        try:
            from .generation import generate_long
            with self._gen_lock:
                for response in generate_long(engine=self._engine, tokenizer=self._tokenizer, text="Hello.",
                                              max_new_tokens=50, temperature=0.7, top_p=0.8, repetition_penalty=1.1,
                                              prompt_text=[], prompt_tokens=[]):
                    if response.action == "next":
                        break
            self._is_warmed_up = True
            logger.info("Warmup complete in %.1fs", time.perf_counter() - t0)
        except Exception as e:  # noqa: BLE001  (the reference only logs a failed warmup, synthesizer.py:322-323)
            logger.warning("Warmup failed: %s", e)

    def encode_reference(self, audio_bytes: bytes, text: str) -> VoiceProfile:
        """WAV bytes + transcript -> VoiceProfile (synthesizer.py:325-357): the codec *encoder* on the GPU
        (SURVEY.md §8-f F4)."""
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        audio = self._read_wav(audio_bytes)
        srv = getattr(self, "_server", None)
        if srv is not None:
            with srv.codec_lock:              # the server's codec worker shares the codec context
                codes = self._vocoder.encode(audio)
        else:
            codes = self._vocoder.encode(audio)
        return VoiceProfile(codes=codes.astype(np.int64), text=text)

    # ------------------------------------------------------------------ reference intake (extension)
    def _intake(self, clips, silence_db, loudness, channel, encode: bool):
        """(results, reports) of engine.encode_items / engine.intake over clips (WAV bytes each), in calls of at most 64
        clips and 2^30 raw bytes; every argument is checked before any device work."""
        from .codec_engine import CodecHipEngine, OutputFx
        from .longform import join_params
        from .wavfile import WIDTH, parse_wav
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        OutputFx.of(loudness=loudness)
        params = tuple(join_params(44100, 0, 0, silence_db)[0])
        if channel is not None and (isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or channel < 0):
            raise ValueError(f"channel must be None or a channel index, got {channel!r}")
        parsed = []
        for i, data in enumerate(clips):
            try:
                info = parse_wav(data)
            except ValueError as e:
                raise ValueError(f"clip {i}: {e}") from None
            if channel is not None and channel >= info.channels:
                raise ValueError(f"clip {i}: channel {channel} of a file with {info.channels} channels")
            if self._vocoder.lib.ft_intake_len(info.rate, 0) < 0:
                raise ValueError(f"clip {i}: unsupported input sample rate {info.rate}")
            parsed.append((data, info))
        groups, cur, raw = [], [], 0
        for c in parsed:
            size = -(-c[1].n_frames * c[1].channels * WIDTH[c[1].fmt] // 16) * 16
            if cur and (len(cur) == CodecHipEngine.MAX_CLIPS_PER_INTAKE or raw + size > CodecHipEngine.MAX_INTAKE_BYTES):
                groups.append(cur)
                cur, raw = [], 0
            cur.append(c)
            raw += size
        if cur:
            groups.append(cur)
        call = self._vocoder.encode_items if encode else self._vocoder.intake
        out, reports = [], []
        srv = getattr(self, "_server", None)
        for g in groups:
            if srv is not None:
                with srv.codec_lock:              # the server's codec worker shares the codec context
                    o, r = call(g, params, loudness, channel)
            else:
                o, r = call(g, params, loudness, channel)
            out += o
            reports += r
        return out, reports

    def _intake_refusals(self, reports) -> None:
        a = self._vocoder.args
        for i, r in enumerate(reports):
            if r.status == 1:
                raise ValueError(f"clip {i}: nothing in it is louder than silence_db: there is nothing to encode")
            if r.status == 2:
                takes = self._vocoder.max_enc_frames * self._vocoder.enc_frame_len / 44100.0
                raise ValueError(f"clip {i}: {r.kept / 44100.0:.2f} s are kept, the encoder takes {takes:.2f} s "
                                 f"(max_reference_seconds = {a.max_reference_seconds:g}); the clip is not cut: its transcript "
                                 "would no longer match")

    def encode_references(self, clips: List[Tuple[bytes, str]], silence_db: Optional[float] = -45.0,
                          loudness: Optional[float] = None, channel: Optional[int] = None,
                          reports: Optional[list] = None) -> List[VoiceProfile]:
        """Extension: a voice library onboarded in one go - (WAV bytes, transcript) each -> one VoiceProfile each, every
        clip prepared on the GPU (ft_codec_encode_items): any WAV of 8-, 16-, 24-, 32-bit PCM or 32-bit float, 1 to 8
        channels (mixed down; `channel`: that channel alone), plain or WAVE_FORMAT_EXTENSIBLE header, at an input rate in
        [8000, 192000] (resampled by a polyphase FIR, not a whole-clip FFT on the host); leading and trailing silence below
        `silence_db` dBFS trimmed with 5 ms fades (None: nothing is trimmed or faded); with `loudness` (LUFS in [-50, -5], as
        synthesize_at's) the clip is levelled to it before the trim, the peak held at -1 dBFS - the model follows its
        prompt's level.  The clips go in calls of at most 64 clips and 2^30 raw bytes, each call one launch chain.  `reports`:
        a list that receives one IntakeReport per clip.  ValueError before any device work for a bad WAV, rate or argument;
        after it, naming the clip, for one with nothing above silence_db and for one whose kept part is longer than
        max_reference_seconds."""
        clips = list(clips)
        codes, reps = self._intake([c[0] for c in clips], silence_db, loudness, channel, True) if clips else ([], [])
        if reports is not None:
            reports.extend(reps)
        self._intake_refusals(reps)
        return [VoiceProfile(codes=c, text=t) for c, (_, t) in zip(codes, clips)]

    def encode_reference_at(self, audio_bytes: bytes, text: str, silence_db: Optional[float] = -45.0,
                            loudness: Optional[float] = None, channel: Optional[int] = None,
                            report: Optional[list] = None) -> VoiceProfile:
        """Extension: encode_reference for any WAV, prepared on the GPU - encode_references of one clip.  With
        silence_db=None and loudness=None a 16-bit mono 44.1 kHz file gives encode_reference's codes, bit for bit.
        `report`: a list that receives the clip's IntakeReport."""
        return self.encode_references([(audio_bytes, text)], silence_db, loudness, channel, report)[0]

    def prepare_reference(self, audio_bytes: bytes, silence_db: Optional[float] = -45.0, loudness: Optional[float] = None,
                          channel: Optional[int] = None):
        """Extension: (float32 audio at 44.1 kHz, IntakeReport) - what encode_reference_at would hand to the encoder, for a
        caller who wants to hear what was kept (ft_codec_intake).  Nothing is refused after the call: the report tells."""
        audio, reps = self._intake([audio_bytes], silence_db, loudness, channel, False)
        return audio[0], reps[0]

    def measure_loudness(self, wav_bytes: bytes) -> float:
        """Extension: the integrated loudness (LUFS, ITU-R BS.1770-4) of a 16-bit mono WAV, measured on the GPU at the WAV's
        own rate by the stage that `loudness=` runs (CodecHipEngine.loudness) - the figure to pass as `loudness=` to match
        a reference clip.  -inf for a clip with nothing above the absolute gate.  ValueError: not 16-bit mono, a rate that is
        no accepted `sample_rate`, or a clip longer than the longest utterance the codec decodes
        (CodecHipEngine.max_level_samples: over three minutes at 48 kHz with the codec's 2056 frames)."""
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        with wave.open(io.BytesIO(wav_bytes), "rb") as wf:
            if wf.getnchannels() != 1 or wf.getsampwidth() != 2:
                raise ValueError("measure_loudness: a 16-bit mono WAV is needed")
            rate = wf.getframerate()
            audio = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0
        _output_fx(rate, None, None)                  # (ValueError for a rate the output stages do not take)
        if len(audio) > self._vocoder.max_level_samples:
            raise ValueError(f"measure_loudness: {len(audio)} samples, the stage takes {self._vocoder.max_level_samples}")
        srv = getattr(self, "_server", None)
        if srv is not None:
            with srv.codec_lock:              # the server's codec worker shares the codec context
                info, _ = self._vocoder.loudness(audio, rate)
        else:
            info, _ = self._vocoder.loudness(audio, rate)
        return info.lufs

    @staticmethod
    def _read_wav(audio_bytes: bytes) -> np.ndarray:
        """synthesizer.py:613-631: 16-bit PCM -> float32 / 32768, Fourier resampling to 44.1 kHz if needed."""
        with wave.open(io.BytesIO(audio_bytes), "rb") as wf:
            sample_rate = wf.getframerate()
            audio = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0
        if sample_rate != 44100:
            from scipy import signal
            audio = signal.resample(audio, int(len(audio) * 44100 / sample_rate))
        return audio

    # ------------------------------------------------------------------ references (synthesizer.py:363-429)
    def set_references(self, profiles: List[VoiceProfile]) -> None:
        with self._prefill_lock:
            self._prefill_cache = _PrefillCache(prompt_text=[p.text for p in profiles],
                                                prompt_tokens=[np.asarray(p.codes) for p in profiles],
                                                profiles=list(profiles))
            logger.info("Set %d reference(s)", len(profiles))

    def add_reference(self, profile: VoiceProfile) -> None:
        with self._prefill_lock:
            self._prefill_cache.profiles.append(profile)
            self._prefill_cache.prompt_text.append(profile.text)
            self._prefill_cache.prompt_tokens.append(np.asarray(profile.codes))

    def clear_references(self) -> None:
        with self._prefill_lock:
            self._prefill_cache = _PrefillCache()

    def get_references(self) -> List[VoiceProfile]:
        with self._prefill_lock:
            return list(self._prefill_cache.profiles)

    @property
    def num_references(self) -> int:
        return len(self._prefill_cache.profiles)

    def _get_prompt_data(self, references):
        if references is not None:
            return [p.text for p in references], [np.asarray(p.codes) for p in references]
        with self._prefill_lock:
            return list(self._prefill_cache.prompt_text), list(self._prefill_cache.prompt_tokens)

    # ------------------------------------------------------------------ synthesis
    def synthesize(self, text: str, references: Optional[List[VoiceProfile]] = None, temperature: float = 0.7,
                   top_p: float = 0.8, repetition_penalty: float = 1.1, max_tokens: int = 2048) -> bytes:
        """Text -> WAV bytes (synthesizer.py:431-481).  While a BatchServer is open (serve()) the call joins its batch.
        The reference's signature; synthesize_at also takes an output sample rate, a speaking rate and a pitch shift."""
        return self.synthesize_at(text, references, temperature, top_p, repetition_penalty, max_tokens)

    def synthesize_at(self, text: str, references: Optional[List[VoiceProfile]] = None, temperature: float = 0.7,
                      top_p: float = 0.8, repetition_penalty: float = 1.1, max_tokens: int = 2048,
                      sample_rate: Optional[int] = None, speed: Optional[float] = None,
                      pitch: Optional[float] = None, loudness: Optional[float] = None, format: str = "wav") -> bytes:
        """Extension: synthesize() with the WAV at `sample_rate` (resampled on the GPU; None or 44100: the codec's own
        rate, byte for byte synthesize()'s result; an unsupported rate raises ValueError before any work -
        codec_engine.output_rate) and at speaking rate `speed` (a factor in [0.5, 2.0], the waveform time-scaled on the
        GPU at unchanged pitch before the resampler; None or 1.0: the model's own pace, byte for byte synthesize()'s
        result; anything else raises ValueError before any work - codec_engine.output_speed), shifted by `pitch`
        semitones (in [-12, 12], in steps of a cent; a plain shift on the GPU between the two stages - formants move with
        the pitch - that leaves the length as it is; None or 0: the model's own pitch, byte for byte the result without
        it; a value outside the range, or one whose speed / 2^(pitch / 12) leaves [0.5, 2], raises ValueError before any
        work - codec_engine.output_pitch, output_fx), and levelled to `loudness` LUFS (a target in [-50, -5]: the
        utterance's integrated loudness per ITU-R BS.1770-4 is measured on the GPU behind the other stages and one gain
        brings it to the target, the sample peak held at -1 dBFS; None: the model's own level, byte for byte the result
        without it; anything else raises ValueError before any work - codec_engine.OutputFx.of).  `format`: "wav", or "flac"
        for a FLAC file of the same 16-bit samples, packed losslessly on the GPU (the FLAC stage, CodecHipEngine.flac); any
        other value raises ValueError before any work."""
        from .generation import generate_long
        from .serve import ServerClosed
        fx = _output_fx(sample_rate, speed, pitch, loudness)
        _check_format(format)
        srv = getattr(self, "_server", None)
        if srv is not None:
            try:
                return srv.synthesize(text, references, temperature, top_p, repetition_penalty, max_tokens, fx=fx,
                                      **_format_kw(format))
            except ServerClosed:
                pass                          # closed meanwhile: served here, once the server has let go of _gen_lock
        prompt_text, prompt_tokens = self._get_prompt_data(references)
        codes_list = []
        with self._gen_lock:
            for response in generate_long(engine=self._engine, tokenizer=self._tokenizer, text=text,
                                          max_new_tokens=max_tokens, temperature=temperature, top_p=top_p,
                                          repetition_penalty=repetition_penalty, prompt_text=prompt_text,
                                          prompt_tokens=prompt_tokens, prefix_cache=self._prefix_cache):
                if response.action == "sample":
                    codes_list.append(response.codes)
                elif response.action == "next":
                    break
        if not codes_list:
            raise RuntimeError("No audio generated")
        return self._decode_to_wav(np.concatenate(codes_list, axis=1), fx, **_format_kw(format))

    def _batch_utterances(self, texts: List[str], references, temperature: float, top_p: float,
                          repetition_penalty: float, max_tokens: int, seed: int, seeds: Optional[List[int]],
                          made: Optional[dict] = None, text_references: Optional[list] = None):
        """The engines and Utterances of a batch run (synthesize_batch, synthesize_batch_stream); call with _gen_lock
        held.  More engines than the first one when batch_streams > 1 and the texts outnumber max_batch (created on first
        use, kept); a voice's K/V prefix from the cache, spread over the engines; utterance i draws with seed + i, or
        seeds[i].  `made` (a dict the caller owns): the voice is one made up for this call - its prefix is built directly with
        engine.build_prefix, once per engine, kept in `made` and freed by the caller; the cache of the user's voices is
        not touched.  `text_references` (one entry per text): text i speaks in the voice text_references[i], a list of
        VoiceProfile, its prefix from the cache; an entry of None means `references` (and `made`), as without the
        argument."""
        cache = self._prefix_cache
        _check_sampling(temperature, top_p, repetition_penalty)
        if seeds is not None and len(seeds) != len(texts):
            raise ValueError("seeds must have one entry per text")
        if text_references is not None and len(text_references) != len(texts):
            raise ValueError("text_references must have one entry per text")
        call_prompt = self._get_prompt_data(references)
        utts = []
        engines = [self._engine]
        if self._batch_streams > 1 and len(texts) > self._max_batch:
            while len(self._more_engines) < self._batch_streams - 1:      # created on first use, kept
                self._more_engines.append(self._engine_factory())
            engines += self._more_engines
        for i, text in enumerate(texts):
            own_voice = text_references is not None and text_references[i] is not None
            utt, n_prefix = self._utterance(text, self._get_prompt_data(text_references[i]) if own_voice else call_prompt,
                                            (temperature, top_p, repetition_penalty, max_tokens),
                                            seeds[i] if seeds is not None else seed + i)
            if cache is not None and n_prefix >= cache.min_positions:
                # a saved prefix lives in one engine's memory and pins its utterance there: spread them evenly
                eng = engines[i % len(engines)]
                if made is None or own_voice:
                    utt.prefix = cache.get(eng, utt.prompt[:, :n_prefix])
                else:
                    if id(eng) not in made:
                        made[id(eng)] = eng.build_prefix(np.ascontiguousarray(utt.prompt[:, :n_prefix], dtype=np.int32))
                    utt.prefix = made[id(eng)]
            utts.append(utt)
        return engines, utts

    def _utterance(self, text: str, prompt, sampling, seed: int):
        """(Utterance, n_prefix) of one text behind `prompt` = (reference texts, reference codes), as generate_long builds
        and checks it; `sampling` = (temperature, top_p, repetition_penalty, max_tokens)."""
        from .batch import Utterance
        from .prompt import build_prompt_split
        temperature, top_p, repetition_penalty, max_tokens = sampling
        _check_sampling(temperature, top_p, repetition_penalty)
        enc, n_prefix = build_prompt_split(self._tokenizer, text, *prompt, self._engine.args.num_codebooks)
        if enc.shape[1] > self._engine.args.max_seq_len - 2048:
            raise ValueError(f"Prompt is too long: {enc.shape[1]} > {self._engine.args.max_seq_len - 2048}")
        return Utterance(enc, max_tokens, temperature, top_p, repetition_penalty, seed), n_prefix

    def _run_utterances(self, engines, utts, on_frames=None, on_done=None) -> None:
        """Runs the utterances of _batch_utterances: one lock-step batch with refill, or several side by side."""
        from .batch import run_batch, run_batch_streams
        if len(engines) > 1:
            run_batch_streams(engines, utts, on_frames=on_frames, on_done=on_done)
        else:
            run_batch(self._engine, utts, on_frames=on_frames, on_done=on_done)

    def synthesize_batch(self, texts: List[str], references: Optional[List[VoiceProfile]] = None,
                         temperature: float = 0.7, top_p: float = 0.8, repetition_penalty: float = 1.1,
                         max_tokens: int = 2048, seed: int = 0, seeds: Optional[List[int]] = None,
                         sample_rate: Optional[int] = None, speed: Optional[float] = None,
                         pitch: Optional[float] = None, loudness: Optional[float] = None,
                         format: str = "wav") -> List[bytes]:
        """Extension (BASELINE configs[2]): many texts -> WAV bytes each, decoded `max_batch` at a time in lock step
        with refill (fish_tts_amd.batch); utterance i uses seed + i, or seeds[i] when `seeds` is given (a sharded run
        passes the GLOBAL indices so an utterance draws the same noise on any number of GPUs).  Same per-utterance
        semantics as synthesize(), `sample_rate`, `speed`, `pitch` and `loudness` (as synthesize_at; every utterance is
        levelled on its own) and `format` included."""
        fx = _output_fx(sample_rate, speed, pitch, loudness)
        _check_format(format)
        self._no_server("synthesize_batch")
        with self._gen_lock:
            engines, utts = self._batch_utterances(texts, references, temperature, top_p, repetition_penalty, max_tokens,
                                                   seed, seeds)
            self._run_utterances(engines, utts)
        out = []
        for u in utts:
            codes = u.codes()
            if codes.shape[1] == 0:
                raise RuntimeError("No audio generated")
            out.append(self._decode_to_wav(codes, fx, **_format_kw(format)))
        return out

    def synthesize_batch_stream(self, texts: List[str], references: Optional[List[VoiceProfile]] = None,
                                chunk_tokens: int = 20, min_first_chunk: int = 10, temperature: float = 0.7,
                                top_p: float = 0.8, repetition_penalty: float = 1.1, max_tokens: int = 2048,
                                seed: int = 0, seeds: Optional[List[int]] = None,
                                sample_rate: Optional[int] = None,
                                speed: Optional[float] = None,
                                pitch: Optional[float] = None, loudness: Optional[float] = None,
                                live_loudness: Optional[float] = None,
                                format: Optional[str] = None, live_format=None,
                                flac_report: Optional[list] = None) -> Iterator[Tuple[int, bytes]]:
        """Extension: synthesize_batch's utterances streamed while the batch generates.  Yields (i, pcm) - int16 mono
        PCM chunks of utterance i as synthesize_stream(seamless=True) gives them: exactly `min_first_chunk` frames, then
        `chunk_tokens` frames each, then the remainder - and (i, b"") once after its last chunk.  Chunks of different
        utterances interleave as they become ready.  The codes of utterance i are those synthesize_batch decodes (same
        engines, seeds, K/V prefixes); its PCM concatenates to one stateful streamed decode of them (CodecStream), bit
        for bit, whatever else is in flight: the codec worker decodes every ready chunk in one batched call
        (CodecHipEngine.decode_streams, one chunk per utterance).  Generation holds _gen_lock on its own thread;
        abandoning the generator stops it within one burst and releases the lock (fish_tts_amd.batch_stream).
        `sample_rate` (as synthesize_at): each utterance's stream resamples on the GPU; the chunk before its (i, b"") holds
        the resampler's tail, so its PCM concatenates to the resampled waveform of one streamed decode.
        `speed` (as synthesize_at): each utterance's stream is time-scaled on the GPU through one carried stage (before
        the resampler, if any); the chunk before its (i, b"") holds the tail in the same way.
        `pitch` (as synthesize_at): each utterance's stream is pitch-shifted on the GPU through one carried stage (between
        the two); the tail travels in the same way.
        `loudness`: ValueError here, before any work - the level needs the whole utterance (synthesize_batch has it).
        `live_loudness` (LUFS in [-50, -5]) is what a stream takes instead: each utterance's stream is ridden toward that
        loudness on the GPU by a gain that looks one second ahead, last in its chain (as synthesize_stream).
        `format` is refused (ValueError): see _no_streamed_format.  `live_format` ("flac" or a flacfile.LiveFlac; as
        synthesize_stream): one FLAC stream per utterance - the (i, bytes) of utterance i concatenate to a FLAC stream of its
        own, with its own head, that decodes to exactly the PCM the call yields without it; its last frames go out before its
        (i, b""), which stays the end mark.  `flac_report` receives (i, FlacReport, the final 42-byte head) as each ends."""
        from .batch_stream import stream_utterances
        _no_streamed_format(format, "synthesize_batch_stream")
        live = _live_format(live_format)
        fx = _output_fx(sample_rate, speed, pitch, loudness, live_loudness).no_level("synthesize_batch_stream")
        self._no_server("synthesize_batch_stream")
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        texts = list(texts)

        def run(on_frames, on_done) -> None:
            with self._gen_lock:
                engines, utts = self._batch_utterances(texts, references, temperature, top_p, repetition_penalty,
                                                       max_tokens, seed, seeds)
                self._run_utterances(engines, utts, on_frames, on_done)

        chunks = stream_utterances(run, len(texts), self._vocoder, chunk_tokens=chunk_tokens,
                                   min_first_chunk=min_first_chunk, fx=fx)
        if live is None:
            return chunks
        from .flacfile import flac_tagged_chunks
        return flac_tagged_chunks(chunks, lambda: self._vocoder.flac_stream(fx.wav_rate, 1, live.blocksize, np.int16),
                                  self._codec_locked, flac_report)

    # ------------------------------------------------------------------ long texts (extension)
    def _long_plan(self, text, pause, paragraph_pause, silence_db, max_chars, min_chars, sample_rate, speed, pitch,
                   loudness=None, stereo: bool = False, pan=0.0):
        """Every check of a long-text call, before any device work: its segments.SegmentPlan - every segment in the call's
        voice, one chain of output stages for all; with `stereo` the piece is one line at `pan`.  ValueError for a bad
        value, a `stereo` that is no bool, a pan without stereo."""
        from .longform import join_params, split_text
        from .script import native_pan
        from .segments import SegmentPlan
        if not isinstance(stereo, bool):
            raise ValueError(f"stereo must be True or False, got {stereo!r}")
        place = native_pan("pan", pan)
        if place != 0 and not stereo:
            raise ValueError(f"pan={pan!r} needs stereo=True (the streams are mono)")
        fx = _output_fx(sample_rate, speed, pitch, loudness)
        jp, gap, pgap = join_params(fx.rate, pause, paragraph_pause, silence_db)
        segs = split_text(text, max_chars, min_chars)
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        return SegmentPlan([s.text for s in segs], [None] * len(segs), [pgap if s.paragraph else gap for s in segs], tuple(jp),
                           fx.wav_rate, fx, pans=[place] if stereo else None)

    def _segment_calls(self, plan, references, sampling, seed: int):
        """The keyword arguments of segments.join_wav / join_chunks for a checked call: the vocoder, the open BatchServer
        (asked when the work begins: a stream's first next()), and the segments through that server or as lock-step batches
        on this instance's engines (_batch_utterances with _gen_lock held: the voices' prefixes from the cache, one made up
        for this call in `made`)."""
        from . import segments

        def has_voice() -> bool:
            return bool(self._get_prompt_data(references)[1])

        def run(idx, seg_refs, refs, seeds, made, on_frames, on_done) -> None:
            engines, utts = self._batch_utterances([plan.texts[i] for i in idx], refs, *sampling, 0, seeds, made=made,
                                                   text_references=seg_refs)
            self._run_utterances(engines, utts, on_frames, lambda j: on_done(j, utts[j].codes()))

        return dict(
            vocoder=self._vocoder, server=lambda: getattr(self, "_server", None),
            serve_=lambda srv: segments.serve(srv, plan, references, has_voice, sampling, seed, self._prefix_cache),
            generate_=lambda emit, stopped: segments.generate(plan, references, has_voice, seed, run, self._gen_lock, emit,
                                                              stopped))

    def synthesize_long(self, text: str, references: Optional[List[VoiceProfile]] = None, temperature: float = 0.7,
                        top_p: float = 0.8, repetition_penalty: float = 1.1, max_tokens: int = 2048, seed: int = 0,
                        pause: float = 0.2, paragraph_pause: float = 0.5, silence_db: Optional[float] = -45.0,
                        max_chars: int = 200, min_chars: int = 24, sample_rate: Optional[int] = None,
                        speed: Optional[float] = None, pitch: Optional[float] = None,
                        loudness: Optional[float] = None, bed=None, stereo: bool = False, pan: float = 0.0,
                        room=None, format: str = "wav") -> bytes:
        """Extension: a text of any length -> one WAV.  The text is split into segments of at most `max_chars` bytes at
        sentence ends (longform.split_text; pieces below `min_chars` join a neighbour), every segment is an utterance of
        its own - `max_tokens` frames at most each, segment i drawing with seed + i - and all of them run as ONE lock-step
        batch with refill over the engine's `max_batch` slots, the voice prefix restored per slot from the cache (with
        max_batch=1 the call degrades to a loop; the result is built the same way).  The codec then decodes the segments
        and joins them on the GPU (CodecHipEngine.decode_join): each is trimmed to its loud part - 5 ms windows with a
        sample at or above `silence_db` dB full scale, 30 ms kept around them - faded over 5 ms at both cuts, and laid out
        behind `pause` seconds of silence, `paragraph_pause` after a paragraph break; silence_db=None trims and fades
        nothing.  One voice throughout: with no reference voice (neither `references` nor set_references) segment 0 is
        generated first and then serves, text and codes, as the reference of every other segment.  `sample_rate`,
        `speed`, `pitch` as synthesize_at, applied per segment before the join.  `loudness` (as synthesize_at): every
        segment is levelled to the target on its own, before the join - the sentences of the document then stand at one
        level, and `silence_db` is judged on the levelled samples.  While a BatchServer is open the segments
        join its batch.  `bed` (a mix.Bed): music or room tone under the joined piece, ducked where it speaks (the mix
        stage, CodecHipEngine.mix; bed=None: the call as it always was).  `stereo`: a two-channel WAV - the voice at `pan`
        in [-1, 1], -1 hard left, over the bed's own left and right (the stereo mix stage, CodecHipEngine.mix_stereo; with
        or without a bed).  `room` (a room.Room): a convolution reverb on the joined piece, before the bed and the panning
        (the room stage, CodecHipEngine.room); the piece rings on for the room's tail.  ValueError before any device work: a
        bad value in `room` or a response file the intake does not read, a pan without stereo or outside [-1, 1], pause /
        paragraph_pause outside [0, 5] s, silence_db outside
        [-90, 0], max_chars outside [16, 1000], min_chars outside [0, max_chars], no text, a bad sample_rate / speed / pitch /
        loudness, a bad value in `bed` or a bed file the intake does not read, a `format` other than "wav" or "flac" (as
        synthesize_at: the finished piece, mono or stereo, as a FLAC file of the WAV's samples)."""
        from . import segments
        _check_format(format)
        plan = self._long_plan(text, pause, paragraph_pause, silence_db, max_chars, min_chars, sample_rate, speed, pitch,
                               loudness, stereo, pan)
        mixed = self._bed_args(bed, plan.rate, silence_db)
        roomed = self._room_args(room, plan.rate)
        sampling = (temperature, top_p, repetition_penalty, max_tokens)
        audio, _ = segments.join_wav(plan, **self._segment_calls(plan, references, sampling, seed), bed=mixed, room=roomed)
        return self._to_file_bytes(audio, plan.rate, format)

    def synthesize_long_stream(self, text: str, references: Optional[List[VoiceProfile]] = None, temperature: float = 0.7,
                               top_p: float = 0.8, repetition_penalty: float = 1.1, max_tokens: int = 2048, seed: int = 0,
                               pause: float = 0.2, paragraph_pause: float = 0.5, silence_db: Optional[float] = -45.0,
                               max_chars: int = 200, min_chars: int = 24, sample_rate: Optional[int] = None,
                               speed: Optional[float] = None, pitch: Optional[float] = None,
                               loudness: Optional[float] = None, bed=None, live_bed=None, live_stereo: bool = False,
                               live_pan: float = 0.0, room=None, live_room=None,
                               format: Optional[str] = None, live_format=None,
                               flac_report: Optional[list] = None) -> Iterator[bytes]:
        """Extension: synthesize_long's audio as int16 PCM chunks in text order, while the batch generates.  Whenever the
        next segments not yet handed out are complete, the longest such run is decoded and joined as one group
        (decode_join, whether audio went out before carried along) - a piece depends on its own segment only, so the
        chunks concatenate to synthesize_long's PCM byte for byte - with `loudness` too: a group holds whole segments, and
        each is levelled on its own.  No empty chunk is yielded.  The arguments are checked
        here, at the call; generation holds _gen_lock on its own thread and stops within one burst when the generator is
        abandoned.  `bed` is refused (ValueError): see _no_streamed_bed.  `live_bed` (a mix.Bed): the bed under the stream -
        every joined group goes through a stream of the live mix stage (CodecHipEngine.mix_stream), which holds the piece
        under -1 dBFS with a look-ahead limiter instead of bed='s one gain and holds back under half a second; with a `lead`
        longer than that the music starts while the first sentence is still generating.  The chunks then concatenate to
        CodecHipEngine.mix_live over the plain stream's audio.  Its values are checked here, as bed='s are.
        `live_stereo`: the stream in stereo - interleaved int16 chunks, the voice at `live_pan` in [-1, 1] (-1 hard left)
        over the live_bed's own left and right, or without a bed (the live stereo mix stage,
        CodecHipEngine.mix_stream(stereo=True): one limiter for both channels, so the image stays where it is); where neither
        ceiling binds the chunks concatenate to synthesize_long(stereo=True, pan=live_pan)'s PCM.  ValueError: a live_pan
        other than 0 without live_stereo, or outside [-1, 1].  `room` is refused (ValueError): see _no_streamed_room.
        `live_room` (a room.Room): the streamed form - every joined group goes through a stream of the live room stage
        (CodecHipEngine.room_stream) before the mixer, which carries the room's tail from group to group and holds nothing
        back; the stream ends `tail` longer.  The room stage's ceiling - one gain for the piece - has no streamed form, so the
        limiter of the live mix stage holds the piece instead: the live_bed's or the live_stereo stream's, or, with neither, a
        limiter of its own (CodecHipEngine.mix_stream(None, bedless=True)); where it does not bind, the chunks concatenate to
        CodecHipEngine.room(..., ceiling=False) over the plain stream's audio.  Its values are checked here, as room='s are.
        `format` is refused (ValueError): see _no_streamed_format.  `live_format` ("flac", or a flacfile.LiveFlac for another
        blocksize): the chunks are the bytes of one FLAC stream instead of PCM, packed on the GPU behind every other stage (the
        live FLAC stage, CodecHipEngine.flac_stream; 2 channels with live_stereo).  The first chunk begins with a 42-byte head
        whose sizes and sample count read "unknown", which every FLAC reader takes; a group that completes no frame yields
        nothing, and the last chunk holds the short last frame.  The stream decodes to exactly the PCM chunks of the same call
        without live_format; it holds back under one blocksize of samples (93 ms at 4096 and 44.1 kHz).  `flac_report` (a
        list) receives (FlacReport, head) at the end: a caller who wrote the chunks to a file may overwrite its first 42
        bytes with `head`, and the file is then byte for byte what format="flac" would have made of the same samples."""
        from . import segments
        from .script import native_pan
        _no_streamed_format(format, "synthesize_long_stream")
        live = _live_format(live_format)
        _no_streamed_bed(bed, "synthesize_long_stream", live_bed)
        _no_streamed_room(room, "synthesize_long_stream")
        if not isinstance(live_stereo, bool):
            raise ValueError(f"live_stereo must be True or False, got {live_stereo!r}")
        if native_pan("live_pan", live_pan) != 0 and not live_stereo:
            raise ValueError(f"live_pan={live_pan!r} needs live_stereo=True: a mono stream has no left and right")
        plan = self._long_plan(text, pause, paragraph_pause, silence_db, max_chars, min_chars, sample_rate, speed, pitch,
                               loudness, live_stereo, live_pan)
        mixed = self._bed_args(live_bed, plan.rate, silence_db)
        roomed = self._room_args(live_room, plan.rate)
        sampling = (temperature, top_p, repetition_penalty, max_tokens)
        return segments.join_chunks(plan, **self._segment_calls(plan, references, sampling, seed), live_bed=mixed,
                                    live_stereo=live_stereo, live_room=roomed, live_format=live, flac_report=flac_report)

    # ------------------------------------------------------------------ music bed (extension)
    def _bed_args(self, bed, rate: int, silence_db=None):
        """Every check of a call's `bed=`, before any device work: None without one, else (clip, mix.MixParams) as
        CodecHipEngine.mix takes them - the Bed's values in their native form at output rate `rate` (mix.bed_params), its
        WAV read (wavfile.parse_wav) and judged as the intake judges a clip.  ValueError for a bad value."""
        if bed is None:
            return None
        from .mix import bed_bytes, bed_params
        from .wavfile import parse_wav
        mp = bed_params(bed, rate, silence_db)
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        data = bed_bytes(bed)
        clip = (data, parse_wav(data))
        self._vocoder._intake_args("bed", [clip], (0.0, 1, 0, 0), None, bed.channel)
        return clip, mp

    # ------------------------------------------------------------------ room (extension)
    def _room_args(self, room, rate: int):
        """Every check of a call's `room=`, before any device work: None without one, else (clip, room.RoomParams) as
        CodecHipEngine.room takes them - the Room's values in their native form at output rate `rate` (room.room_params), its
        WAV read (wavfile.parse_wav) and judged as the intake judges a clip.  ValueError for a bad value."""
        if room is None:
            return None
        from .room import room_bytes, room_params
        from .wavfile import parse_wav
        rp = room_params(room, rate)
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        data = room_bytes(room)
        clip = (data, parse_wav(data))
        self._vocoder._intake_args("room", [clip], (0.0, 1, 0, 0), None, room.channel)
        return clip, rp

    def reverb(self, wav_bytes: bytes, room, report: Optional[list] = None, format: str = "wav") -> bytes:
        """Extension: a finished 16-bit mono WAV - at 44.1 kHz or any rate `sample_rate=` takes - through `room` (a
        room.Room) -> one WAV at the same rate, the room's tail longer (the room stage, CodecHipEngine.room, with its
        ceiling).  `report`: a list that receives the RoomReport.  ValueError before any device work: not 16-bit mono, no
        sample, an unsupported rate, a bad Room, a `format` other than "wav" or "flac" (as synthesize_at)."""
        _check_format(format)
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        with wave.open(io.BytesIO(wav_bytes), "rb") as wf:
            if wf.getnchannels() != 1 or wf.getsampwidth() != 2:
                raise ValueError("reverb: a 16-bit mono WAV is needed")
            rate = wf.getframerate()
            audio = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0
        if not len(audio):
            raise ValueError("reverb: the WAV holds no sample")
        rate = _output_fx(rate, None, None).wav_rate            # (ValueError for a rate the output stages do not take)
        if room is None:
            raise ValueError("reverb: a Room is needed")
        clip, rp = self._room_args(room, rate)
        srv = getattr(self, "_server", None)
        with (srv.codec_lock if srv is not None else contextlib.nullcontext()):   # the server's codec worker shares the codec context
            y, rep = self._vocoder.room(audio, clip, (), sample_rate=rate, params=rp, ceiling=True)
        if report is not None:
            report.append(rep)
        return self._to_file_bytes(y, rate, format)

    def mix(self, wav_bytes: bytes, bed, silence_db: Optional[float] = None, report: Optional[list] = None,
            stereo: bool = False, format: str = "wav") -> bytes:
        """Extension: a finished 16-bit mono WAV - at 44.1 kHz or any rate `sample_rate=` takes - with `bed` (a mix.Bed)
        under it -> one WAV at the same rate, `lead` + `tail` longer (the mix stage, CodecHipEngine.mix).  `silence_db`:
        what counts as speech where the Bed has no threshold_db (None: -45).  `report`: a list that receives the
        MixReport.  `stereo`: a two-channel WAV - the programme (still mono) in the centre over the bed's own left and
        right (CodecHipEngine.mix_stereo).  ValueError before any device work: not 16-bit mono, no sample, an unsupported
        rate, a bad Bed, a `format` other than "wav" or "flac" (as synthesize_at)."""
        _check_format(format)
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        with wave.open(io.BytesIO(wav_bytes), "rb") as wf:
            if wf.getnchannels() != 1 or wf.getsampwidth() != 2:
                raise ValueError("mix: a 16-bit mono WAV is needed")
            rate = wf.getframerate()
            audio = np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16).astype(np.float32) / 32768.0
        if not len(audio):
            raise ValueError("mix: the WAV holds no sample")
        if not isinstance(stereo, bool):
            raise ValueError(f"mix: stereo must be True or False, got {stereo!r}")
        rate = _output_fx(rate, None, None).wav_rate            # (ValueError for a rate the output stages do not take)
        if bed is None:
            raise ValueError("mix: a Bed is needed")
        clip, mp = self._bed_args(bed, rate, silence_db)
        srv = getattr(self, "_server", None)
        with (srv.codec_lock if srv is not None else contextlib.nullcontext()):   # the server's codec worker shares the codec context
            if stereo:
                y, rep = self._vocoder.mix_stereo(audio, clip, (), sample_rate=rate, params=mp)
            else:
                y, rep = self._vocoder.mix(audio, clip, sample_rate=rate, params=mp)
        if report is not None:
            report.append(rep)
        return self._to_file_bytes(y, rate, format)

    def to_flac(self, wav_bytes: bytes, blocksize: int = 4096) -> bytes:
        """Extension: a finished 16-bit PCM WAV, mono or stereo, at any rate `sample_rate=` takes -> a FLAC file of its
        samples, packed on the GPU (the FLAC stage, CodecHipEngine.flac, with the samples taken as they are: lossless).
        ValueError before any device work: not a WAV, not 16-bit PCM, more than two channels, no sample, an unsupported
        rate, a bad blocksize."""
        from .wavfile import parse_wav
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        info = parse_wav(wav_bytes)
        if info.fmt != "s16":
            raise ValueError(f"to_flac: a 16-bit PCM WAV is needed, this one is {info.fmt}: the stage writes 16-bit samples, "
                             "and anything else would not come back bit for bit")
        if info.channels > 2:
            raise ValueError(f"to_flac: a mono or stereo WAV is needed, this one has {info.channels} channels")
        rate = _output_fx(info.rate, None, None).wav_rate       # (ValueError for a rate the output stages do not take)
        pcm = np.frombuffer(wav_bytes, dtype="<i2", count=info.n_frames * info.channels, offset=info.data_offset)
        pcm = pcm.astype(np.int16).reshape(-1) if info.channels == 1 else pcm.astype(np.int16).reshape(-1, 2)
        return self._flac_bytes(pcm, rate, blocksize, lock=True)

    # ------------------------------------------------------------------ scripts (extension)
    def _script_plan(self, lines, voices, references, pause, paragraph_pause, line_pause, silence_db, max_chars, min_chars,
                     sample_rate, speed, pitch, loudness, marks, stereo: bool = False, pans=None, room: bool = False,
                     sends=None):
        """Every check of a script call, before any device work: its segments.SegmentPlan, from script.plan_script - every
        segment with its line's references (None where it speaks in the call's voice) and its line's own chain of output
        stages.  ValueError for a bad value, an unknown voice, or more voices than the prefix cache holds: the cache frees
        its least recently used entry on insert, and an Utterance of the batch still holds the prefix it was given."""
        from .script import plan_script
        from .segments import SegmentPlan
        if marks is not None and not isinstance(marks, list):
            raise ValueError(f"marks must be None or a list, got {type(marks).__name__}")
        plan = plan_script(lines, voices, pause, paragraph_pause, line_pause, silence_db, max_chars, min_chars,
                           sample_rate, speed, pitch, loudness, stereo, pans, room, sends)
        used = []
        for v in plan.voices:
            if v is not None and v not in used:
                used.append(v)
        for v in used:
            if not isinstance(voices[v], (list, tuple)) or not all(isinstance(p, VoiceProfile) for p in voices[v]):
                raise ValueError(f"voices[{v!r}] must be a list of VoiceProfile")
        cache = self._prefix_cache
        if cache is not None:
            # the call's own voice goes through the cache too, unless it is made up for this call
            count = len(used) + (1 if None in plan.voices and self._get_prompt_data(references)[1] else 0)
            engines = self._batch_streams if self._batch_streams > 1 and len(plan.texts) > self._max_batch else 1
            if count * engines > cache.capacity:
                raise ValueError(f"a script of {count} voices" + (f" on {engines} engines" if engines > 1 else "") +
                                 f": the reference cache holds {cache.capacity} prefixes, and every voice of the batch needs "
                                 "its own to stay (split the script, or build the instance with cache_reference_kv=False)")
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        return SegmentPlan(plan.texts, [None if v is None else list(voices[v]) for v in plan.voices], plan.gaps,
                           tuple(plan.jp), plan.rate, plan.fx, plan.line_of, plan.n_lines, plan.pans, plan.sends)

    def synthesize_script(self, lines, voices=None, references: Optional[List[VoiceProfile]] = None, temperature: float = 0.7,
                          top_p: float = 0.8, repetition_penalty: float = 1.1, max_tokens: int = 2048, seed: int = 0,
                          pause: float = 0.2, paragraph_pause: float = 0.5, line_pause: float = 0.4,
                          silence_db: Optional[float] = -45.0, max_chars: int = 200, min_chars: int = 24,
                          sample_rate: Optional[int] = None, speed: Optional[float] = None, pitch: Optional[float] = None,
                          loudness: Optional[float] = None, marks: Optional[list] = None, bed=None, stereo: bool = False,
                          pans: Optional[dict] = None, room=None, sends: Optional[dict] = None,
                          format: str = "wav") -> bytes:
        """Extension: a script - a dialogue, a narrated piece with quoted speakers - as one WAV.  `lines`: a list of
        script.Line (text, voice, speed, pitch, loudness, volume, pause), or an SSML string (script.parse_ssml: speak, p, s,
        voice, break, prosody); `voices`: name -> list of VoiceProfile.  Every line is split as synthesize_long splits a text
        and ALL segments of all lines run as one lock-step batch with refill, segment i (counted over the whole script)
        drawing with seed + i, each with its own voice's prompt and K/V prefix.  A line without a voice speaks in
        `references` / set_references; with neither, synthesize_long's rule holds for those lines alone (their first segment
        becomes their voice).  The codec decodes every segment through its line's own chain - `speed`, `pitch`, `loudness`
        are the line's, or the call's where the line has None; `volume` dB is added to the loudness target - and joins them
        on the GPU (CodecHipEngine.decode_join with item_fx), behind `pause` / `paragraph_pause` inside a line and the
        line's `pause` or `line_pause` in front of it.  One `sample_rate` per call.  `marks` (a list) receives one
        (start_sample, end_sample) per line at the output rate, from the join's cuts and gaps.  A script of one plain Line
        is synthesize_long of its text, byte for byte.  While a BatchServer is open the segments join its batch.
        `bed` (a mix.Bed): as synthesize_long's; `marks` then count from the start of the mixed piece (the join's marks plus
        the bed's `lead` in samples).  `stereo`: a two-channel WAV - every line at its place, its `pan` or else its voice's
        in `pans` (voice name -> pan in [-1, 1], -1 hard left) or else the centre, over the bed's own left and right (the
        stereo mix stage, CodecHipEngine.mix_stereo, with or without a bed; the lines' marks are its regions); `marks` count
        frames.  `room` (a room.Room): as synthesize_long's, with `sends` - a dict from a voice name or a line index to that
        voice's or that line's send into the room, dB in [-60, 0] or -math.inf for a line the room does not hear (a narrator
        kept dry among reverberant speakers); a line takes its own entry, else its voice's, else 0 dB.  `marks` do not move:
        the room adds only its tail.  ValueError before any device work: `sends` without `room`, a bad send or key,
        a pan or `pans` without stereo, a pan outside [-1, 1], a `pans` key that
        is no voice of the call, no line, an unknown voice, a bad value in a line or in the call, a bad
        line_pause, more distinct voices than the reference cache holds (8; not with cache_reference_kv=False), a `format`
        other than "wav" or "flac" (as synthesize_long: with stereo= the FLAC file has two channels)."""
        from . import segments
        from .script import line_marks
        _check_format(format)
        plan = self._script_plan(lines, voices, references, pause, paragraph_pause, line_pause, silence_db, max_chars,
                                 min_chars, sample_rate, speed, pitch, loudness, marks, stereo, pans, room is not None, sends)
        mixed = self._bed_args(bed, plan.rate, silence_db)
        roomed = self._room_args(room, plan.rate)
        sampling = (temperature, top_p, repetition_penalty, max_tokens)
        audio, cuts = segments.join_wav(plan, **self._segment_calls(plan, references, sampling, seed), bed=mixed, room=roomed)
        if marks is not None:
            found = [None] * plan.n_lines
            line_marks(plan.line_of, plan.gaps, cuts, found, at=0 if mixed is None else mixed[1].lead)
            marks.extend(found)
        return self._to_file_bytes(audio, plan.rate, format)

    def synthesize_script_stream(self, lines, voices=None, references: Optional[List[VoiceProfile]] = None,
                                 temperature: float = 0.7, top_p: float = 0.8, repetition_penalty: float = 1.1,
                                 max_tokens: int = 2048, seed: int = 0, pause: float = 0.2, paragraph_pause: float = 0.5,
                                 line_pause: float = 0.4, silence_db: Optional[float] = -45.0, max_chars: int = 200,
                                 min_chars: int = 24, sample_rate: Optional[int] = None, speed: Optional[float] = None,
                                 pitch: Optional[float] = None, loudness: Optional[float] = None,
                                 marks: Optional[list] = None, bed=None, live_bed=None, live_stereo: bool = False,
                                 live_pans: Optional[dict] = None, room=None, sends: Optional[dict] = None, live_room=None,
                                 live_sends: Optional[dict] = None, format: Optional[str] = None, live_format=None,
                                 flac_report: Optional[list] = None) -> Iterator[bytes]:
        """Extension: synthesize_script's audio as int16 PCM chunks in script order, while the batch generates
        (as synthesize_long_stream: the longest ready run of segments is decoded and joined as one group, whether audio went
        out before carried along, every segment through its own chain).  The chunks concatenate to synthesize_script's PCM
        byte for byte; no empty chunk is yielded.  `marks` fills as groups go out: a line's entry is added once its last
        segment went out, and in the end the list is synthesize_script's.  The arguments are checked here, at the call.
        `bed` is refused (ValueError): see _no_streamed_bed.  `live_bed` (a mix.Bed): as synthesize_long_stream's; `marks`
        then count from the start of the mixed piece (the join's marks plus the bed's `lead` in samples).  `live_stereo`: the
        stream in stereo - interleaved int16 chunks, every line at its place, its `pan` or else its voice's in `live_pans`
        (voice name -> pan in [-1, 1], -1 hard left) or else the centre, over the live_bed's own left and right or without a
        bed (the live stereo mix stage, CodecHipEngine.mix_stream(stereo=True): every joined group is pushed with the regions
        of its lines, one limiter for both channels); where neither ceiling binds the chunks concatenate to
        synthesize_script(stereo=True, pans=live_pans)'s PCM; `marks` count frames.  ValueError: `live_pans` without
        live_stereo; a Line.pan without it stays refused, as a stereo value on a mono stream.  `room` and `sends` are refused
        (ValueError): see _no_streamed_room.  `live_room` (a room.Room): as synthesize_long_stream's, with `live_sends` -
        sends='s dict and rules: every joined group is pushed with the send regions of its lines, a line that crosses a group
        keeping its send.  `marks` do not move: the room adds only its tail, behind the last line.  On a live_stereo stream
        the tail stays at the pan of the last line heard.  ValueError: `live_sends` without `live_room`.  `format` is refused
        (ValueError): see _no_streamed_format.  `live_format` and `flac_report`: as synthesize_long_stream's - one FLAC stream
        behind every other stage, of 2 channels on a live_stereo stream; `marks` count samples (frames) of the decoded
        stream, as they count those of the PCM."""
        from . import segments
        from .script import line_marks
        _no_streamed_format(format, "synthesize_script_stream")
        live = _live_format(live_format)
        _no_streamed_bed(bed, "synthesize_script_stream", live_bed)
        _no_streamed_room(room, "synthesize_script_stream", sends)
        if not isinstance(live_stereo, bool):
            raise ValueError(f"live_stereo must be True or False, got {live_stereo!r}")
        if live_pans is not None and not live_stereo:
            raise ValueError("live_pans needs live_stereo=True: a mono stream has no left and right")
        if live_sends is not None and live_room is None:
            raise ValueError("live_sends needs live_room=: without a room there is nothing to send to")
        plan = self._script_plan(lines, voices, references, pause, paragraph_pause, line_pause, silence_db, max_chars,
                                 min_chars, sample_rate, speed, pitch, loudness, marks, live_stereo, live_pans,
                                 live_room is not None, live_sends)
        mixed = self._bed_args(live_bed, plan.rate, silence_db)
        roomed = self._room_args(live_room, plan.rate)
        sampling = (temperature, top_p, repetition_penalty, max_tokens)
        found = [None] * plan.n_lines
        state = {"at": 0 if mixed is None else mixed[1].lead, "started": False, "told": 0}

        def on_cuts(first, cuts) -> None:
            end = first + len(cuts)
            state["at"], state["started"] = line_marks(plan.line_of[first:end], plan.gaps[first:end], cuts, found,
                                                       state["at"], state["started"])
            done = plan.n_lines if end == len(plan.texts) else plan.line_of[end]     # the lines whose last segment went out
            marks.extend(found[state["told"]:done])
            state["told"] = max(state["told"], done)

        return segments.join_chunks(plan, **self._segment_calls(plan, references, sampling, seed),
                                    on_cuts=None if marks is None else on_cuts, live_bed=mixed, live_stereo=live_stereo,
                                    live_room=roomed, live_format=live, flac_report=flac_report)

    def synthesize_stream(self, text: str, references: Optional[List[VoiceProfile]] = None, chunk_tokens: int = 20,
                          min_first_chunk: int = 10, **kwargs) -> Iterator[bytes]:
        """Streaming synthesis: AR generation on this thread, codec decode on a worker thread with two bounded
        queues; each chunk is decoded independently from zero context (synthesizer.py:483-584).

        Extension `seamless=True` (keyword): the codec is strictly causal, so a chunk can be decoded with the context its
        predecessors left (the last 127 frames' K/V of the transformer layers, the last rows of every convolution input:
        CodecStream / ft_codec_stream_*) - no restart artefacts at chunk boundaries (the stateful streaming decode of
        SURVEY.md section 8-f F4), at the cost of one chunk each.  The result does not depend on the chunking, bit for
        bit; it equals the non-streaming decode of the same codes up to summation order (the stream always runs the
        kernel variants of a nominal 215-frame utterance: bit-equal at about that length, relative RMS <= 2e-2 measured at
        60 and 300 frames).  One stream carries at most `max_frames` frames (2056 here: the codec's rotation table); a
        longer synthesis starts a fresh stream there - that one boundary is decoded from zero state, as the reference
        decodes every chunk.

        While a BatchServer is open (serve()) the request joins its batch (BatchServer.synthesize_stream).

        Extension `sample_rate=` (keyword, as synthesize_at; checked at the first next()): seamless=False chunks are
        resampled each on its own, as independent waveforms; a seamless stream resamples through one carried resampler
        (a last PCM chunk holds its tail), so its chunks concatenate to the resampled waveform of one streamed decode.

        Extension `speed=` (keyword, as synthesize_at; checked at the first next()): seamless=False chunks are time-scaled
        each on its own, as independent waveforms; a seamless stream runs one carried time-scale stage (in front of the
        resampler, if any; a last PCM chunk holds the tail), so its chunks concatenate to the time-scaled waveform of one
        streamed decode.

        Extension `pitch=` (keyword, as synthesize_at; checked at the first next()): seamless=False chunks are shifted each
        on its own, as independent waveforms; a seamless stream runs one carried pitch stage (between the time-scale stage
        and the resampler), so its chunks concatenate to the shifted waveform of one streamed decode.

        `loudness=` raises ValueError (at the first next(), before any work): the level needs the whole utterance, and a
        stream hands out audio before its end (synthesize_at, synthesize_long_stream take it).

        Extension `live_loudness=` (keyword; LUFS in [-50, -5]; checked at the first next()): with seamless=True the stream
        is ridden toward that loudness on the GPU by a carried look-ahead gain rider, last in the chain (CodecStream /
        ft_codec_stream_begin_live): a gain that follows the loudness of the programme so far, moves at most 0.5 dB per
        100 ms, looks one second ahead and holds the sample peak at -1 dBFS.  First audio comes one second of output
        (about 22 frames) later, and the result does not depend on the chunking, bit for bit.  A fresh stream at
        `max_frames`, or the cut at `max_tokens`, starts a fresh ride state: the level is not carried over that one
        boundary.  seamless=False chunks are independent waveforms - levelling each on its own would jump - so that
        combination raises ValueError (at the first next(), before any work).  The one-shot and long-form calls do not
        take it: they have `loudness=`.

        `format=` raises ValueError (at the first next(), before any work): see _no_streamed_format.

        Extension `live_format=` (keyword; "flac", or a flacfile.LiveFlac for another blocksize; checked at the first next()):
        the chunks are the bytes of one FLAC stream instead of PCM.  The very int16 samples of every PCM chunk are pushed
        into a stream of the live FLAC stage (CodecHipEngine.flac_stream, opened at the first next(); under the codec lock of
        an open BatchServer) and the frames they complete are yielded: the first chunk begins with a 42-byte head whose
        sizes and sample count read "unknown", a PCM chunk that completes no frame yields nothing, the last chunk holds the
        short last frame.  The stream decodes to exactly the PCM the same call yields without live_format.  `flac_report=`
        (keyword, a list) receives (FlacReport, the final 42-byte head) at the end; a file of the chunks with its first 42
        bytes overwritten by that head is byte for byte to_flac() of the PCM's WAV."""
        _no_streamed_format(kwargs.get("format"), "synthesize_stream")
        live, report = _live_format(kwargs.pop("live_format", None)), kwargs.pop("flac_report", None)
        chunks = self._stream_pcm(text, references, chunk_tokens, min_first_chunk, **kwargs)
        if live is None:
            yield from chunks
            return
        from .flacfile import flac_chunks
        rate = _output_fx(kwargs.get("sample_rate"), kwargs.get("speed"), kwargs.get("pitch"), kwargs.get("loudness"),
                          kwargs.get("live_loudness")).wav_rate
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        yield from flac_chunks(chunks, lambda: self._vocoder.flac_stream(rate, 1, live.blocksize, np.int16), self._codec_locked,
                               report)

    def _stream_pcm(self, text: str, references: Optional[List[VoiceProfile]] = None, chunk_tokens: int = 20,
                    min_first_chunk: int = 10, **kwargs) -> Iterator[bytes]:
        """synthesize_stream's int16 PCM chunks (its docstring states them)."""
        from .generation import generate_long
        from .serve import ServerClosed
        _no_streamed_format(kwargs.pop("format", None), "synthesize_stream")
        fx = _output_fx(kwargs.pop("sample_rate", None), kwargs.pop("speed", None), kwargs.pop("pitch", None),
                        kwargs.pop("loudness", None), kwargs.pop("live_loudness", None)).no_level("synthesize_stream")
        if fx.live is not None and not kwargs.get("seamless", False):
            raise ValueError("live_loudness needs seamless=True: seamless=False chunks are independent waveforms, and "
                             "levelling each on its own would jump")
        srv = getattr(self, "_server", None)
        if srv is not None:
            chunks = srv.synthesize_stream(text, references, chunk_tokens, min_first_chunk, fx=fx, **kwargs)
            try:
                try:
                    first = next(chunks)      # the request is queued here
                except ServerClosed:
                    chunks = None             # closed meanwhile: served here, once the server has let go of _gen_lock
                except StopIteration:
                    return
                if chunks is not None:
                    yield first
                    yield from chunks
                    return
            finally:
                if chunks is not None:
                    chunks.close()            # (an abandoned stream cancels its request)
        seamless = bool(kwargs.get("seamless", False))
        prompt_text, prompt_tokens = self._get_prompt_data(references)
        codes_queue: "queue.Queue" = queue.Queue(maxsize=3)
        audio_queue: "queue.Queue" = queue.Queue(maxsize=3)
        error_holder: List[Exception] = []

        def decoder_worker():
            stream = None
            try:
                if seamless:
                    if self._vocoder is None:
                        raise RuntimeError("Vocoder not loaded")
                    stream = self._vocoder.stream(fx=fx)  # carried state: K/V of the last 127 frames, conv tails
                while True:
                    codes = codes_queue.get()
                    if codes is None:
                        break
                    if stream is None:
                        audio_queue.put(self._decode_to_pcm(codes, **fx.kw))
                    else:
                        codes = np.asarray(codes)
                        if stream.frames + codes.shape[1] > self._vocoder.max_frames:   # the rotation table ends here
                            if fx:                              # the old stream's output-stage tail first
                                audio_queue.put((stream.finish() * 32767).astype(np.int16).tobytes())
                            stream.close()
                            stream = self._vocoder.stream(fx=fx)
                        audio = stream.decode(codes)
                        if len(audio) or fx.emits_empty:   # (a time-scale, pitch or ride stage completed nothing: nothing to hand out)
                            audio_queue.put((audio * 32767).astype(np.int16).tobytes())
                if stream is not None and fx:
                    audio_queue.put((stream.finish() * 32767).astype(np.int16).tobytes())   # the output stages' tail
            except Exception as e:  # noqa: BLE001
                error_holder.append(e)
            finally:
                if stream is not None:
                    stream.close()
                audio_queue.put(None)

        worker = threading.Thread(target=decoder_worker, daemon=True)
        worker.start()

        def worker_gone() -> bool:
            # the worker records its exception BEFORE its final put(None) (which may itself wait for queue space)
            return bool(error_holder) or not worker.is_alive()

        pending: List[Optional[bytes]] = []   # audio taken off the queue while a put was waiting, in order

        def hand_over(item) -> bool:
            """Puts item on the bounded codes queue without ever blocking on a stuck or dead worker: keeps draining
            the audio queue meanwhile.  False = the worker is gone (its error is raised at the end)."""
            while True:
                if worker_gone():
                    return False
                try:
                    codes_queue.put(item, timeout=0.005)
                    return True
                except queue.Full:
                    pass
                try:
                    pending.append(audio_queue.get_nowait())
                except queue.Empty:
                    pass

        try:
            buffer, is_first_chunk, total_tokens = [], True, 0
            tail_chunk, worker_ok = None, True
            with self._gen_lock:
                for response in generate_long(engine=self._engine, tokenizer=self._tokenizer, text=text,
                                              max_new_tokens=kwargs.get("max_tokens", 2048),
                                              temperature=kwargs.get("temperature", 0.7), top_p=kwargs.get("top_p", 0.8),
                                              repetition_penalty=kwargs.get("repetition_penalty", 1.1),
                                              prompt_text=prompt_text, prompt_tokens=prompt_tokens, streaming=True,
                                              prefix_cache=self._prefix_cache):
                    if response.action == "sample":
                        buffer.append(response.codes)
                        total_tokens += response.codes.shape[1]
                        threshold = min_first_chunk if is_first_chunk else chunk_tokens
                        if total_tokens >= threshold:
                            chunk = np.concatenate(buffer, axis=1)
                            buffer, total_tokens, is_first_chunk = [], 0, False
                            # Both queues are bounded.  The reference blocks in put() here and joins the worker before
                            # draining (synthesizer.py:556-578): harmless when the AR loop is the slow side, a deadlock
                            # once it is faster than the codec (worker stuck on a full audio queue).  Keep draining; and
                            # stop generating when the worker has died (its exception is re-raised below, as the
                            # reference does at synthesizer.py:583-584).
                            worker_ok = hand_over(chunk)
                            while pending:
                                audio = pending.pop(0)
                                if audio is not None:
                                    yield audio
                            if not worker_ok:
                                break
                            while not audio_queue.empty():
                                audio = audio_queue.get_nowait()
                                if audio is not None:
                                    yield audio
                    elif response.action == "next":
                        if buffer:
                            tail_chunk = np.concatenate(buffer, axis=1)
                        break
        finally:
            # hand over the tail and the stop mark (the consumer may have abandoned the generator: then pending audio
            # is dropped); a dead worker takes nothing more
            for item in ([tail_chunk] if tail_chunk is not None else []) + [None]:
                if not hand_over(item):
                    break
        got_end = False
        for audio in pending:                 # drained while handing over, in order
            if audio is None:
                got_end = True
            else:
                yield audio
        while not got_end:                    # the worker always ends with a None
            try:
                audio = audio_queue.get(timeout=0.05)
            except queue.Empty:
                if worker.is_alive():
                    continue
                # the worker may have put its last chunk and the end mark between the time-out and this check
                while True:
                    try:
                        audio = audio_queue.get_nowait()
                    except queue.Empty:
                        break
                    if audio is not None:
                        yield audio
                break
            if audio is None:
                break
            yield audio
        worker.join()
        if error_holder:
            raise error_holder[0]

    # ------------------------------------------------------------------ continuous batching (extension)
    def serve(self, burst: int = 8) -> "BatchServer":
        """Extension: a BatchServer (fish_tts_amd.serve) over this instance's first AR engine - concurrent synthesize /
        synthesize_stream calls, from any number of threads, join one continuous lock-step batch (max_batch slots) at
        the next burst boundary and stream their audio back.  While it is open, this instance's own synthesize and
        synthesize_stream are served by it, synthesize_batch and synthesize_batch_stream raise RuntimeError.  A context
        manager; after close() the instance behaves exactly as before.  Waits for a running synthesis to end."""
        from .serve import BatchServer
        if getattr(self, "_server", None) is not None:
            raise RuntimeError("a BatchServer is already open on this instance")
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        self._gen_lock.acquire()            # held while the server owns the engine; released by _server_closed
        try:
            self._server = BatchServer(self._engine, self._vocoder, burst, prepare=self._serve_prepare,
                                       decode_wav=self._decode_to_wav, decode_pcm=self._decode_to_pcm,
                                       prefix_cache=self._prefix_cache, on_close=self._server_closed)
        except BaseException:
            self._gen_lock.release()
            raise
        return self._server

    def _server_closed(self, server) -> None:
        if self._server is server:
            self._server = None
            self._gen_lock.release()

    def _no_server(self, what: str) -> None:
        if getattr(self, "_server", None) is not None:
            raise RuntimeError(f"{what} is not available while a BatchServer is open (serve()): close it first, or "
                               "send the texts through the server")

    def _serve_prepare(self, text: str, references, temperature: float, top_p: float, repetition_penalty: float,
                       max_tokens: int, seed: int):
        """A BatchServer request on the caller's thread: the prompt as generate_long builds and checks it."""
        return self._utterance(text, self._get_prompt_data(references), (temperature, top_p, repetition_penalty, max_tokens),
                               seed)

    # ------------------------------------------------------------------ codes -> audio (synthesizer.py:586-648)
    def _decode_to_wav(self, codes: np.ndarray, fx=None, format: str = "wav") -> bytes:
        """The file of a call that decodes codes (the BatchServer's decode_wav too: its worker holds the codec lock)."""
        audio, rate = self._decode_codes(codes, fx), self.sample_rate if fx is None else fx.wav_rate
        return self._to_wav_bytes(audio, rate) if format == "wav" else self._flac_bytes(audio, rate)

    def _to_file_bytes(self, audio: np.ndarray, sample_rate: int, format: str) -> bytes:
        """A finished waveform as the file `format` names: _to_wav_bytes, or the FLAC stage on the same float32 samples."""
        return self._to_wav_bytes(audio, sample_rate) if format == "wav" else self._flac_bytes(audio, sample_rate, lock=True)

    def _flac_bytes(self, audio: np.ndarray, sample_rate: int, blocksize: int = 4096, lock: bool = False) -> bytes:
        """CodecHipEngine.flac's bytes; `lock`: under an open BatchServer's codec lock (its worker shares the codec context)."""
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        srv = getattr(self, "_server", None) if lock else None
        with (srv.codec_lock if srv is not None else contextlib.nullcontext()):
            return self._vocoder.flac(audio, sample_rate, blocksize)[0]

    @contextlib.contextmanager
    def _codec_locked(self):
        """Held around a call's own use of the codec context: an open BatchServer's codec lock (its worker shares the
        context), asked anew each time - a server may open or close while a stream runs."""
        srv = getattr(self, "_server", None)
        with (srv.codec_lock if srv is not None else contextlib.nullcontext()):
            yield

    def _decode_to_pcm(self, codes: np.ndarray, fx=None) -> bytes:
        return (self._decode_codes(codes, fx) * 32767).astype(np.int16).tobytes()  # no clip on the PCM path (synthesizer.py:594)

    def _decode_codes(self, codes: np.ndarray, fx=None) -> np.ndarray:
        """codes (n_codebooks+1, T) -> the waveform through the output stages `fx` (a checked codec_engine.OutputFx; None:
        none)."""
        if self._vocoder is None:
            raise RuntimeError("Vocoder not loaded")
        codes = np.asarray(codes)
        if codes.ndim == 2:
            codes = codes[None]
        return np.squeeze(self._vocoder.decode(codes, fx=fx), axis=0)

    @staticmethod
    def _to_wav_bytes(audio: np.ndarray, sample_rate: int = 44100) -> bytes:
        """A 16-bit WAV: mono, or - from an (N, 2) array, left then right - two interleaved channels."""
        stereo = getattr(audio, "ndim", 1) == 2
        if stereo and audio.shape[1] != 2:
            raise ValueError(f"a two-channel waveform is (N, 2), got {audio.shape}")
        audio = np.clip(audio, -1.0, 1.0)
        audio_int16 = np.ascontiguousarray((audio * 32767).astype(np.int16))
        buffer = io.BytesIO()
        with wave.open(buffer, "wb") as wf:
            wf.setnchannels(2 if stereo else 1)
            wf.setsampwidth(2)
            wf.setframerate(sample_rate)
            wf.writeframes(audio_int16.tobytes())
        return buffer.getvalue()

    @property
    def sample_rate(self) -> int:
        return 44100

    @property
    def precision(self) -> str:
        return self._precision


def _check_sampling(temperature: float, top_p: float, repetition_penalty: float) -> None:
    assert 0 < top_p <= 1, "top_p must be in (0, 1]"
    assert 0 < repetition_penalty < 2, "repetition_penalty must be in (0, 2)"
    assert 0 < temperature < 2, "temperature must be in (0, 2)"


def _check_format(format) -> None:
    """batch_stream.checked_format: the one check of `format=` (imported when first needed, as the engines are)."""
    from .batch_stream import checked_format
    checked_format(format)


def _live_format(live_format):
    """batch_stream.checked_live_format: the one check of `live_format=` (imported when first needed, as the engines are)."""
    from .batch_stream import checked_live_format
    return checked_live_format(live_format)


def _format_kw(format: str) -> dict:
    """`format` as the keyword of a call that takes it defaulted: nothing for "wav" - a decoder handed in by a caller, which
    may know of no format, is then called as it always was (as OutputFx.kw)."""
    return {} if format == "wav" else {"format": format}


def _no_streamed_format(format, what: str) -> None:
    """A stream takes no `format=`: that keyword names the file a whole call returns, and the FLAC stage behind it packs a
    finished waveform.  `live_format=` is what a stream takes instead: the live FLAC stage, which carries the samples of an
    unfinished frame from push to push."""
    if format is not None:
        raise ValueError(f"format needs the whole piece: {what} hands out int16 PCM chunks before the piece's end, and the FLAC "
                         "stage packs a finished waveform; synthesize the piece with format=, or to_flac() a finished WAV")


def _no_streamed_room(room, what: str, sends=None) -> None:
    """A stream takes no `room=`: the room stage convolves the whole piece in one call - its tail rings past every later
    line, and its ceiling is one gain known only when the last sample is.  `live_room=` (with `live_sends=`) is the streamed
    form: the same convolution carried from push to push (the live room stage), a limiter in the ceiling's place."""
    if room is not None or sends is not None:
        raise ValueError(f"room needs the whole piece: {what} hands out audio before its end, while the room stage's tail "
                         "rings over everything that follows and its ceiling is one gain for the piece; use synthesize_long / "
                         "synthesize_script with room=, or reverb() on the finished WAV; use live_room= (and live_sends=) for a "
                         "room on the stream")


def _no_streamed_bed(bed, what: str, live_bed=None) -> None:
    """A stream takes no `bed=`: the mix stage holds the whole piece under the -1 dBFS ceiling with ONE gain, known only when
    the last sample is (as `loudness=` was before `live_loudness=`).  `live_bed=` is the streamed form: the same bed under a
    look-ahead limiter (the live mix stage)."""
    if bed is not None and live_bed is not None:
        raise ValueError(f"{what}: bed= and live_bed= are two ways to hold one ceiling; give one (a stream takes live_bed=)")
    if bed is not None:
        raise ValueError(f"bed needs the whole piece: {what} hands out audio before its end, and the mix stage's ceiling - one "
                         "gain over the whole mixed piece - is known only there (synthesize the piece, or mix() a finished WAV); "
                         "use live_bed= for a bed under the stream")


def _output_fx(sample_rate, speed, pitch, loudness=None, live_loudness=None):
    """codec_engine.OutputFx.of: the checked output stages of a call (imported when first needed, as the engines are)."""
    from .codec_engine import OutputFx
    return OutputFx.of(sample_rate, speed, pitch, loudness, live_loudness)


def get_instance(model_dir=None, device: Literal["cpu", "cuda"] = "cuda",
                 precision: Literal["bf16", "fp16", "fp32"] = "bf16", warmup: bool = True) -> FishTTS:
    """Process-wide singleton; later calls return the first instance and ignore their arguments
    (synthesizer.py:661-710)."""
    global _instance
    if _instance is not None:
        return _instance
    with _instance_lock:
        if _instance is not None:
            return _instance
        logger.info("Creating singleton FishTTS instance...")
        _instance = FishTTS(model_dir=model_dir, device=device, precision=precision, warmup=warmup)
        return _instance


def reset_instance() -> None:
    global _instance
    with _instance_lock:
        if _instance is not None:
            logger.info("Resetting singleton FishTTS instance")
            _instance = None
