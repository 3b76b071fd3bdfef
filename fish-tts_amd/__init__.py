"""fish_tts_amd: MI355X-native (gfx950) hot path of smolGura/fish-tts — dual-AR semantic-token decode and
DAC codec decode as hand-written HIP kernels behind the reference's public API
(get_instance / FishTTS.synthesize / synthesize_stream / VoiceProfile)."""
__version__ = "0.1.0"

from .codec_engine import FlacReport, IntakeReport, MixLiveReport, MixReport, RoomReport  # noqa: F401
from .config import CodecArgs, DualARModelArgs, s1_mini_args  # noqa: F401
from .flacfile import FlacInfo, LiveFlac, stream_info  # noqa: F401
from .mix import Bed  # noqa: F401
from .room import Room  # noqa: F401
from .script import Line, parse_ssml, plan_script  # noqa: F401
from .serve import BatchServer  # noqa: F401
from .synthesizer import FishTTS, VoiceProfile, get_instance, reset_instance  # noqa: F401
from .tokenizer import ByteTokenizer, TokenLayout  # noqa: F401
from .wavfile import WavInfo, parse_wav  # noqa: F401

__all__ = ["FishTTS", "VoiceProfile", "get_instance", "reset_instance", "BatchServer", "DualARModelArgs", "CodecArgs",
           "s1_mini_args", "ByteTokenizer", "TokenLayout", "Line", "parse_ssml", "plan_script", "IntakeReport", "WavInfo", "parse_wav",
           "Bed", "MixReport", "MixLiveReport", "Room", "RoomReport", "FlacReport", "FlacInfo", "LiveFlac", "stream_info"]
