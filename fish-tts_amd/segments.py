"""The segments of one call, host side: what FishTTS.synthesize_long, synthesize_script and their streams share once their
arguments are checked.  A SegmentPlan says what to speak and how to join it; generate runs the segments as lock-step
batches on the instance's own engines, serve hands them to an open BatchServer as requests for codes, and join_wav /
join_chunks decode and join what either gives (CodecHipEngine.decode_join).  A long text is a script of one plain line:
every segment speaks in the call's voice and all share one chain of output stages.  Plain Python: neither torch nor the
native library is imported here, and the engine, the vocoder and the server come in as arguments, so all of it runs on fakes.

The reference speaks one text in one voice as one utterance (fish_tts/synthesizer.py:431-481) and has nothing of the kind."""
from __future__ import annotations

import contextlib
import queue
import threading
from typing import Iterator, List, NamedTuple, Optional, Sequence


class SegmentPlan(NamedTuple):
    texts: List[str]                   # the segments, in order
    refs: list                         # every segment's references (a list of VoiceProfile); None: the call's voice
    gaps: List[int]                    # samples of silence before every segment, at the output rate
    jp: tuple                          # the join parameters (longform.JoinParams)
    rate: int                          # the output rate (Hz)
    fx: object                         # the checked output stages (codec_engine.OutputFx): ONE for all segments (a long
                                       # text: ft_codec_decode_join / _join_level) or a list, one per segment (a script:
                                       # ft_codec_decode_join_items)
    line_of: Optional[List[int]] = None   # a script: the line every segment came from (its marks) ...
    n_lines: int = 0                   # ... and the number of its lines
    pans: Optional[List[int]] = None   # a stereo call: every line's pan in hundredths (a long text is one line); None: mono
    sends: Optional[List[int]] = None  # a script with a room: every line's send in hundredths of a dB of attenuation, -1 muted

    def fx_of(self, first: int = 0, end: Optional[int] = None) -> dict:
        """decode_join's keywords for the output stages of segments first .. end - 1."""
        return dict(item_fx=self.fx[first:end]) if isinstance(self.fx, list) else dict(fx=self.fx)


class Stopped(Exception):
    """The consumer of a stream went away: generation stops at its next block of frames."""


def first_alone(seg_refs: Sequence, has_voice: bool) -> Optional[int]:
    """The voice rule: the segment that must run first and alone, because its text and codes become the voice of the other
    segments in the call's voice - the first of those, when the call has no reference voice and there is more than one of
    them.  None: nobody waits for anybody."""
    own = [i for i, r in enumerate(seg_refs) if r is None]
    return own[0] if len(own) > 1 and not has_voice else None


def _first_alone(plan: SegmentPlan, has_voice) -> Optional[int]:
    """first_alone, asking has_voice() only where the answer depends on it."""
    k = first_alone(plan.refs, False)
    return None if k is None or has_voice() else k


def generate(plan: SegmentPlan, references, has_voice, seed: int, run, lock, emit, stopped) -> None:
    """The codes of every segment, emit(i, codes) as each is complete (from any thread).  Segment i speaks in plan.refs[i],
    or (None) in the call's voice `references`, and draws with seed + i; all go through one lock-step batch with refill:
    run(idx, seg_refs, references, seeds, made, on_frames, on_done) builds and runs the segments `idx` - idx[j] in
    seg_refs[j] or the call's voice, with seeds[j] - calling on_frames(j, block) as frames arrive and on_done(j, codes) when
    idx[j] is complete.  Without any reference voice (`has_voice()`, asked with `lock` - the generation lock - held) the
    segment first_alone names runs first, on its own, and is the voice of the others in the call's voice: run then gets
    `made`, a dict in which it keeps the prefixes it builds for that voice, one per engine; they are freed when the call
    ends, so the cache of the user's voices is neither entered nor evicted from.  `stopped()`: the consumer went away."""
    from .synthesizer import VoiceProfile

    def guard(j, block):
        if stopped():
            raise Stopped()

    def batch(idx, refs, made=None) -> dict:
        got = {}

        def done(j, codes):
            got[idx[j]] = codes
            emit(idx[j], codes)
        run(idx, [plan.refs[i] for i in idx], refs, [seed + i for i in idx], made, guard, done)
        return got

    made = None
    with lock:
        try:
            rest = list(range(len(plan.texts)))
            k = _first_alone(plan, has_voice)
            if k is not None:
                codes0 = batch([k], references)[k]
                rest.remove(k)
                if codes0.shape[1]:
                    references, made = [VoiceProfile(codes=codes0, text=plan.texts[k])], {}
            if rest:
                batch(rest, references, made)
        finally:
            for pf in (made or {}).values():
                pf.free()


def serve(srv, plan: SegmentPlan, references, has_voice, sampling, seed: int, prefix_cache):
    """generate through an open BatchServer: the segments as requests whose output is their codes
    (BatchServer.submit_codes).  Returns the requests' results as a list of callables in segment order, each blocking until
    its codes are there, and a release() to call when all were taken (cancel=True: the open requests are given up).  The
    segments with a voice of their own are queued first; then, without any reference voice, the segment first_alone names
    is awaited and made the voice of the others, its prefix in a one-entry PrefixCache of this call (`prefix_cache`: the
    instance's, None without one) that the server retires.  ServerClosed (nothing was handed out yet): what was queued
    is cancelled, and the caller serves the segments itself."""
    from .generation import PrefixCache
    from .serve import ServerClosed
    from .synthesizer import VoiceProfile
    texts = plan.texts
    own, reqs, taken = None, {}, {}

    def release(cancel: bool = False) -> None:
        if cancel:
            for r in reqs.values():
                srv.cancel(r)                # (nothing happens to a request that has ended)
        if own is not None:
            srv.retire_cache(own)        # freed on the server's scheduler thread, once none of its requests can use it

    try:
        for k, r in enumerate(plan.refs):
            if r is not None:
                reqs[k] = srv.submit_codes(texts[k], r, *sampling, seed + k)
        k = _first_alone(plan, has_voice)
        if k is not None:
            taken[k] = srv.take_codes(srv.submit_codes(texts[k], references, *sampling, seed + k))
            if taken[k].shape[1]:
                references = [VoiceProfile(codes=taken[k], text=texts[k])]
                if prefix_cache is not None:
                    own = PrefixCache(capacity=1, min_positions=prefix_cache.min_positions)
        for k, r in enumerate(plan.refs):
            if r is None and k not in taken:
                reqs[k] = srv.submit_codes(texts[k], references, *sampling, seed + k, voice_cache=own)
    except ServerClosed:
        release(cancel=True)             # (a closing server still finishes what it took, then frees the prefix)
        raise
    return [(lambda c=taken[k]: c) if k in taken else (lambda r=reqs[k]: srv.take_codes(r)) for k in range(len(texts))], release


def codes_served(srv, serve_) -> Optional[list]:
    """[codes of every segment] from serve_(srv) -> (takes, release), as serve gives them; None: no server (`srv` None, or
    it closed before it took the segments) - the caller generates."""
    from .serve import ServerClosed
    if srv is None:
        return None
    try:
        takes, release = serve_(srv)
    except ServerClosed:
        return None
    try:
        return [t() for t in takes]
    finally:
        release()


def join_wav(plan: SegmentPlan, *, vocoder, server, serve_, generate_, bed=None, room=None):
    """(audio, cuts) of the whole call: the codes from serve_(srv) while a BatchServer srv = server() is open (None: there
    is none), else from generate_(emit, stopped); one decode_join, under the server's codec lock when it served them.
    `bed`: (clip, mix.MixParams) - the joined piece then goes through the mix stage (vocoder.mix) under the same lock, and
    `audio` is the mixed piece: `lead` samples longer in front, `tail` behind (the cuts are the join's own).  A plan with
    `pans` goes through the stereo mix stage instead (vocoder.mix_stereo), with or without a bed: the regions are the lines'
    marks from the cuts (script.pan_regions), and `audio` is (N, 2).
    `room`: (clip, room.RoomParams) - the joined piece first goes through the room stage (vocoder.room) under the same lock,
    behind the join and before either mix stage: the lines' sends (plan.sends) are its regions, it holds the ceiling itself
    only where no mix stage follows, and the mix stages see the piece it lengthened by its tail.  In a stereo call the room
    runs on the mono programme: the pan region that ends with the programme is extended over the tail, so the wet signal is
    panned with the line that excites it.  The cuts and the lines' marks do not move."""
    from .room import send_regions
    from .script import line_marks, pan_regions
    srv = server()
    codes = codes_served(srv, serve_)
    lock = contextlib.nullcontext() if codes is None else srv.codec_lock
    if codes is None:
        got = {}
        generate_(got.__setitem__, lambda: False)
        codes = [got[i] for i in range(len(plan.texts))]
    with lock:
        audio, cuts = vocoder.decode_join(codes, params=plan.jp, gaps=plan.gaps, **plan.fx_of())
        line_of = plan.line_of if plan.line_of is not None else [0] * len(plan.texts)
        dry_len = len(audio)
        if room is not None and len(audio):
            sends = ()
            if plan.sends is not None:
                found = [None] * len(plan.sends)
                line_marks(line_of, plan.gaps, cuts, found)
                sends = send_regions(plan.sends, found)
            audio, _ = vocoder.room(audio, room[0], sends, sample_rate=plan.rate, params=room[1],
                                    ceiling=plan.pans is None and bed is None)
        if plan.pans is not None and len(audio):
            found = [None] * len(plan.pans)
            line_marks(line_of, plan.gaps, cuts, found)
            regions = pan_regions(plan.pans, found)
            if regions and regions[-1][1] == dry_len < len(audio):
                regions[-1] = (regions[-1][0], len(audio), regions[-1][2])     # the room's tail stays where the last line is
            audio, _ = vocoder.mix_stereo(audio, None if bed is None else bed[0], regions,
                                          sample_rate=plan.rate, params=None if bed is None else bed[1])
        elif bed is not None and len(audio):
            audio, _ = vocoder.mix(audio, bed[0], sample_rate=plan.rate, params=bed[1])
    if not len(audio):
        raise RuntimeError("No audio generated")
    return audio, cuts


def join_chunks(plan: SegmentPlan, *, vocoder, server, serve_, generate_, on_cuts=None, live_bed=None,
                live_stereo: bool = False, live_room=None, live_format=None, flac_report=None) -> Iterator[bytes]:
    """The int16 PCM chunks of the segments as they become ready in order: serve_(srv) -> (takes, release) through an open
    BatchServer srv = server() - asked at the first next(), so a stream made before a server opens and read while it is
    open joins its batch - else generate_(emit, stopped) on a thread of its own; every ready run decoded and joined as one
    group (longform.ready_prefixes, decode_join with `started`).  on_cuts(first, cuts): what the join kept of the group that
    starts at segment `first`, before its chunk goes out.  Abandoning the generator sets stopped() and cancels the open
    requests.  `live_bed`: (clip, mix.MixParams) - every joined group then goes through a stream of the live mix stage
    (vocoder.mix_stream, opened at the first next()) under the same lock as its decode_join: what an empty push emits - the
    bed alone, where `lead` is longer than the stage holds back - goes out before any group, then what each group's push
    emits, then what the final push leaves; the stream is closed when the generator ends or is abandoned.  `live_stereo`
    (the plan then has `pans`): the mixer is a stream of the live stereo mix stage (vocoder.mix_stream(stereo=True)), opened
    with or without a `live_bed`; every group is pushed with the regions of that group (script.push_regions: the lines'
    marks from the group's cuts through pan_regions, clipped to the push and in its coordinates), and the chunks are
    interleaved int16, left then right.
    `live_room`: (clip, room.RoomParams) - every joined group first goes through a stream of the live room stage
    (vocoder.room_stream, opened with the mixer) under the same lock as its decode_join, with the send regions of that group
    (room.push_send_regions over plan.sends; none for a long text), and then into the mixer: the live stereo stream, the live
    bed stream or, where neither was asked for, the bare limiter (vocoder.mix_stream(None, bedless=True)) - the room stage
    has no ceiling on a stream.  A group comes out of the room as long as it went in, so the cuts and the lines' marks do not
    move; at the end the room's final push gives its tail, which goes into the mixer's final push - on a stereo stream under
    one pan region at the pan of the last line heard, Room's "extended over the tail" rule.  The room stream is closed with
    the mixer.
    `live_format`: a flacfile.LiveFlac - the chunks are the bytes of one FLAC stream instead of PCM: a stream of the live FLAC
    stage (vocoder.flac_stream, opened with the mixer at the first next(); 2 channels with `live_stereo`) sits where pcm() is and
    is pushed the float32 the mixer or the join gave, under the same lock - its quantiser is pcm()'s clip-and-truncate rule, so
    the stream decodes to exactly the PCM chunks of the same call without it.  The unknown-values head goes out in front of
    the first frames; a push that completes no frame yields nothing; a final push at the end flushes the short last frame,
    and `flac_report` (a list) receives (FlacReport, the final 42-byte head).  The stream is closed with the mixer."""
    import numpy as np

    from .longform import ready_prefixes
    from .serve import ServerClosed
    q: "queue.Queue" = queue.Queue()
    stop = threading.Event()
    srv, lock, release = server(), contextlib.nullcontext(), None
    if srv is not None:
        try:
            takes, release = serve_(srv)
            lock = srv.codec_lock
        except ServerClosed:
            srv = None                       # closed meanwhile: served here, once the server has let go of the engine

    def feed_served() -> None:
        try:
            for i, take in enumerate(takes):
                q.put((i, take()))
        except BaseException as e:  # noqa: BLE001
            q.put(e)

    def feed_own() -> None:
        try:
            generate_(lambda i, c: q.put((i, c)), stop.is_set)
        except Stopped:
            pass
        except BaseException as e:  # noqa: BLE001
            q.put(e)

    def pcm(audio) -> bytes:
        if flac is not None:                 # the frames these samples complete (none: nothing goes out)
            with lock:
                return flac.push(audio)
        return (np.clip(audio, -1.0, 1.0) * 32767).astype(np.int16).tobytes()   # the WAV's samples

    feeder = threading.Thread(target=feed_own if srv is None else feed_served, daemon=True)
    feeder.start()
    started = False
    mixer = roomer = flac = None
    line_of = plan.line_of if plan.line_of is not None else [0] * len(plan.texts)
    place = (0, False, 0)                    # where the next group begins, whether audio went out, the pan of the last line heard
    if live_room is not None:
        from .room import push_send_regions
        sent = (0, False, 0)                 # the same for the sends: ..., the send of the last line heard
    if live_stereo:
        from .script import push_regions
        if plan.pans is None:
            raise ValueError("live_stereo needs a plan with pans")
    try:
        if live_format is not None:
            from .flacfile import LiveFlacFeed
            with lock:
                flac = LiveFlacFeed(vocoder.flac_stream(plan.rate, 2 if live_stereo else 1, live_format.blocksize), flac_report)
        if live_bed is not None or live_stereo or live_room is not None:
            with lock:
                if live_stereo:
                    mixer = vocoder.mix_stream(None if live_bed is None else live_bed[0], sample_rate=plan.rate,
                                               params=None if live_bed is None else live_bed[1], stereo=True)
                elif live_bed is not None:
                    mixer = vocoder.mix_stream(live_bed[0], sample_rate=plan.rate, params=live_bed[1])
                else:
                    mixer = vocoder.mix_stream(None, sample_rate=plan.rate, bedless=True)
                if live_room is not None:
                    roomer = vocoder.room_stream(live_room[0], sample_rate=plan.rate, params=live_room[1])
                head = mixer.push(None)
            if len(head) and (chunk := pcm(head)):
                yield chunk
        for first, group in ready_prefixes(q, len(plan.texts)):
            end = first + len(group)
            with lock:
                audio, cuts = vocoder.decode_join(group, params=plan.jp, gaps=plan.gaps[first:end], started=started,
                                                  **plan.fx_of(first, end))
                if roomer is not None:
                    sends = ()
                    if plan.sends is not None:
                        sends, *sent = push_send_regions(plan.sends, line_of[first:end], plan.gaps[first:end], cuts, *sent)
                    if len(audio):
                        audio = roomer.push(audio, sends)
                if live_stereo:
                    regions, *place = push_regions(plan.pans, line_of[first:end], plan.gaps[first:end], cuts, *place)
                    out = mixer.push(audio, regions) if len(audio) else audio
                else:
                    out = audio if mixer is None or not len(audio) else mixer.push(audio)
            if on_cuts is not None:
                on_cuts(first, cuts)
            if len(audio):
                started = True
            if len(out) and (chunk := pcm(out)):
                yield chunk
        if mixer is not None and started:
            with lock:
                if roomer is None:
                    rest = mixer.push(None, final=True)
                else:
                    tail = roomer.push(None, final=True)
                    if live_stereo:
                        rest = mixer.push(tail, [(0, len(tail), place[2])] if len(tail) and place[2] != 0 else [], final=True)
                    else:
                        rest = mixer.push(tail, final=True)
            if len(rest) and (chunk := pcm(rest)):
                yield chunk
        if flac is not None and started:
            with lock:
                chunk = flac.push(None, final=True)
            if chunk:
                yield chunk
    finally:
        stop.set()
        if release is not None:
            release(cancel=True)
        feeder.join()
        if mixer is not None or roomer is not None or flac is not None:
            with lock:
                if flac is not None:
                    flac.close()
                if roomer is not None:
                    roomer.close()
                if mixer is not None:
                    mixer.close()
    if not started:
        raise RuntimeError("No audio generated")
