"""`stereo=` without a GPU: script.plan_script's pans (Line.pan, `pans`, the refusals), script.pan_regions' merging,
segments.join_wav handing the joined piece, the regions from the cuts and the bed to the stereo mix stage - on the fake codec
of tests/test_segments_host.py - and the two-channel WAV writer."""
import io
import threading
import wave

import numpy as np
import pytest

import fish_tts_amd.segments as S
from fish_tts_amd.script import Line, line_marks, native_pan, pan_regions, plan_script
from tests.test_segments_host import LONG, MIXED, JoinCodec, _codes, _kw, _no_server, _plan

T = "Some text is here."
VOICES = {"anna": [], "ben": []}


def test_every_line_gets_its_place():
    lines = [Line(T, voice="anna"), Line(T, voice="ben"), Line(T), Line(T, voice="anna", pan=1.0), Line(T, pan=-0.004),
             Line(T + " " + T + " " + T, voice="ben", pan=0)]
    p = plan_script(lines, VOICES, stereo=True, pans={"anna": -0.5, "ben": 0.375})
    assert p.pans == [-50, 38, 0, 100, 0, 0] and len(p.pans) == p.n_lines         # round(100 pan); the line's own pan wins
    assert plan_script(lines[:3], VOICES, stereo=True).pans == [0, 0, 0]          # neither: the centre
    assert plan_script(lines[:3], VOICES).pans is None                            # mono: the plan as it was
    assert plan_script(lines[:3], VOICES)[:8] == plan_script(lines[:3], VOICES, stereo=True)[:8]
    assert Line(T).pan is None and Line._fields[-1] == "pan" and Line(T, "anna", 1.0, 0.0, -20.0, 1.0, 0.5, -1.0).pan == -1.0
    assert [native_pan("pan", v) for v in (-1, -0.37, 0, 0.01, 0.004, 1)] == [-100, -37, 0, 1, 0, 100]


def test_refusals_before_any_work():
    nan = float("nan")
    bad = [dict(lines=[Line(T, pan=0.5)]), dict(lines=[Line(T, pan=0.0)]), dict(pans={"anna": 0.5}), dict(pans={}),
           dict(stereo=1), dict(stereo=None), dict(stereo=True, pans={"carl": 0.5}), dict(stereo=True, pans=[("anna", 0.5)]),
           dict(stereo=True, pans={None: 0.5})]
    for v in (1.01, -1.0001, nan, True, "0.5", [0.5], float("inf")):
        bad += [dict(stereo=True, lines=[Line(T, pan=v)]), dict(stereo=True, pans={"anna": v})]
    bad.append(dict(stereo=True, pans={"anna": None}))
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            plan_script(kw.pop("lines", [Line(T)]), VOICES, **kw)
            pytest.fail(f"accepted: {kw}")
    with pytest.raises(ValueError, match="no voice"):
        plan_script([Line(T)], None, stereo=True, pans={"anna": 0.5})
    with pytest.raises(ValueError, match="line 1: pan"):
        plan_script([Line(T), Line(T, pan=2)], VOICES, stereo=True)
    # 4096 regions after merging is the most: runs of lines at one place count once, the centre does not count
    flip = [Line(T, pan=(0.5 if i % 2 else -0.5)) for i in range(4097)]
    assert len(plan_script(flip[:4096], stereo=True).pans) == 4096
    with pytest.raises(ValueError, match="4097 pan regions"):
        plan_script(flip, stereo=True)
    assert plan_script([Line(T, pan=0.5)] * 5000, stereo=True).n_lines == 5000          # one run
    assert plan_script([Line(T, pan=(0.5 if i % 2 else 0)) for i in range(8192)], stereo=True).n_lines == 8192


def test_regions_from_marks_and_merging():
    marks = [(0, 10), (15, 30), (30, 30), (35, 50), (55, 60), None, (60, 70), (75, 80)]
    assert pan_regions([-50, -50, 20, -50, 0, 99, 50, 50], marks) == [(0, 50, -50), (60, 80, 50)]
    #   lines 0, 1 and 3 merge - line 2 has no audio and separates nothing; the centred line 4 gives no region and separates;
    #   line 5 never began
    assert pan_regions([10, 0, 10], [(0, 5), (5, 9), (9, 12)]) == [(0, 5, 10), (9, 12, 10)]
    assert pan_regions([10, -10, 10], [(0, 5), (5, 9), (9, 12)]) == [(0, 5, 10), (5, 9, -10), (9, 12, 10)]
    assert pan_regions([0, 0], [(0, 5), (5, 9)]) == [] and pan_regions([7], [None]) == [] and pan_regions([7], [(3, 3)]) == []
    # from the join's own cuts and gaps: the regions lie where line_marks puts the lines
    line_of, gaps, cuts = [0, 0, 1, 2], [10, 20, 30, 40], [(2, 9), (0, 5), (4, 4), (1, 8)]
    found = [None] * 3
    line_marks(line_of, gaps, cuts, found)
    assert found == [(0, 32), (32, 32), (72, 79)] and pan_regions([-100, 100, 25], found) == [(0, 32, -100), (72, 79, 25)]


class StereoCodec(JoinCodec):
    def __init__(self, held=None):
        super().__init__(held)
        self.calls = []

    def mix_stereo(self, x, bed, regions=(), sample_rate=None, params=None, nodes=False):
        self.calls.append(dict(x=np.array(x), bed=bed, regions=list(regions), rate=sample_rate, params=params,
                               locked=self.held.locked() if self.held is not None else None))
        return np.stack([x, -x], 1), "report"

    def mix(self, *a, **k):
        raise AssertionError("a stereo plan goes through the stereo mix stage")


@pytest.mark.parametrize("bed", [None, ("clip", "params")], ids=["no-bed", "bed"])
def test_join_wav_hands_the_piece_and_the_regions_to_the_stereo_stage(bed):
    codes = [_codes(i, 3 + i) * 1000 for i in range(4)]
    plan = _plan(MIXED)._replace(line_of=[0, 0, 1, 2], n_lines=3, pans=[-50, 0, 50])

    def generate(emit, stopped):
        for i in (2, 0, 3, 1):
            emit(i, codes[i])
    codec = StereoCodec()
    audio, cuts = S.join_wav(plan, **_kw(codec, None, _no_server, generate), bed=bed)
    (call,) = codec.calls
    mono = np.concatenate([np.asarray(c)[0].astype(np.float32) / 1e6 for c in codes])
    assert np.array_equal(call["x"], mono) and call["rate"] == plan.rate
    assert (call["bed"], call["params"]) == (bed if bed is not None else (None, None))
    found = [None] * 3
    line_marks(plan.line_of, plan.gaps, cuts, found)
    assert call["regions"] == [(found[0][0], found[0][1], -50), (found[2][0], found[2][1], 50)]
    assert audio.shape == (len(mono), 2) and np.array_equal(audio[:, 0], mono)
    # a long text: one line over the piece
    codec = StereoCodec()
    S.join_wav(_plan(LONG)._replace(pans=[30]), **_kw(codec, None, _no_server, generate), bed=bed)
    found = [None]
    line_marks([0] * 4, _plan(LONG).gaps, cuts, found)
    assert codec.calls[0]["regions"] == [(0, found[0][1], 30)]
    codec = StereoCodec()
    S.join_wav(_plan(LONG)._replace(pans=[0]), **_kw(codec, None, _no_server, generate), bed=bed)
    assert codec.calls[0]["regions"] == []                 # stereo, everything in the centre
    # a mono plan never gets there
    plain = JoinCodec()
    audio, _ = S.join_wav(_plan(LONG), **_kw(plain, None, _no_server, generate))
    assert audio.ndim == 1


def test_the_stereo_stage_runs_under_the_servers_codec_lock():
    lock = threading.Lock()
    codes = [_codes(i, 4) * 1000 for i in range(4)]

    class Srv:
        codec_lock = lock
    codec = StereoCodec(held=lock)
    serve = lambda srv: ([lambda c=c: c for c in codes], lambda cancel=False: None)      # noqa: E731
    S.join_wav(_plan(LONG)._replace(pans=[-100]), **_kw(codec, Srv(), serve, None))
    assert codec.calls[0]["locked"] is True and codec.joins[0]["locked"] is True


def test_the_two_channel_wav_writer():
    from fish_tts_amd.synthesizer import FishTTS
    y = np.array([[0.5, -0.5], [1.5, -1.5], [0.0, 0.25]], dtype=np.float32)
    data = FishTTS._to_wav_bytes(y, 16000)
    with wave.open(io.BytesIO(data), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()) == (2, 2, 16000, 3)
        frames = np.frombuffer(wf.readframes(3), dtype=np.int16)
    assert frames.tolist() == [16383, -16383, 32767, -32767, 0, 8191]                     # left, right, frame by frame
    assert FishTTS._to_wav_bytes(y[::-1], 16000) != data and len(FishTTS._to_wav_bytes(y[:, ::-1], 16000)) == len(data)
    mono = FishTTS._to_wav_bytes(y[:, 0], 16000)
    with wave.open(io.BytesIO(mono), "rb") as wf:
        assert (wf.getnchannels(), wf.getnframes()) == (1, 3) and wf.readframes(3) == np.array([16383, 32767, 0], np.int16).tobytes()
    for shape in ((3, 3), (3, 1)):
        with pytest.raises(ValueError):
            FishTTS._to_wav_bytes(np.zeros(shape, dtype=np.float32))
