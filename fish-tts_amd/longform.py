"""Long texts, host side: split_text cuts a document into the segments FishTTS.synthesize_long speaks one by one (each an
utterance of its own in the lock-step batch) and join_params turns its pause / silence arguments into what the device join
stage takes (ft_codec_decode_join).  Plain Python: neither torch nor the native library is imported here.

The reference speaks one text as one utterance (fish_tts/models/inference.py:741-846 does not split either), which caps a
text at max_tokens frames and at max_seq_len - 2048 prompt positions."""
from __future__ import annotations

import math
import queue
from numbers import Real
from typing import Iterator, List, NamedTuple, Optional, Tuple

CODEC_RATE = 44100

TERMINATORS = ".!?…"                       # . ! ? and the ellipsis
CLOSERS = "\"'”’)]»"             # " ' right double / single quote ) ] and the right guillemet
CJK_TERMINATORS = "。！？；"    # ideographic full stop, fullwidth ! ? ;
CJK_CLOSERS = "」』）”"        # right corner brackets, fullwidth ), right double quote
CUT_MARKS = ",;:—、，；："  # , ; : em dash, ideographic comma, fullwidth , ; :
ABBREVIATIONS = frozenset("mr mrs ms dr prof sr jr st vs etc no fig e.g i.e".split())

MAX_PAUSE = 5.0            # seconds
MIN_SILENCE_DB, MAX_SILENCE_DB = -90.0, 0.0


class Segment(NamedTuple):
    text: str
    paragraph: bool        # a paragraph break precedes this segment


def _blen(s: str) -> int:
    return len(s.encode("utf-8"))


def _paragraphs(text: str) -> List[str]:
    """Paragraphs (separated by blank or whitespace-only lines), every run of whitespace inside one made a single space."""
    out, cur = [], []
    for line in text.replace("\r\n", "\n").replace("\r", "\n").split("\n") + [""]:
        if line.strip():
            cur.append(line)
        elif cur:
            out.append(" ".join(" ".join(cur).split()))
            cur = []
    return [p for p in out if p]


def _keeps_going(p: str, dot: int) -> bool:
    """A lone `.` at p[dot] that closes an initial or one of ABBREVIATIONS: no sentence end."""
    start = dot
    while start > 0 and not p[start - 1].isspace():
        start -= 1
    token = p[start:dot]
    return (len(token) == 1 and token.isalpha()) or token.lower() in ABBREVIATIONS


def _sentences(p: str) -> List[str]:
    out, start, i, n = [], 0, 0, len(p)
    while i < n:
        c = p[i]
        end = -1
        if c in TERMINATORS:
            j = i
            while j < n and p[j] in TERMINATORS:
                j += 1
            k = j
            while k < n and p[k] in CLOSERS:
                k += 1
            if (k == n or p[k].isspace()) and not (j == i + 1 and c == "." and _keeps_going(p, i)):
                end = k
            i = k
        elif c in CJK_TERMINATORS:
            k = i
            while k < n and p[k] in CJK_TERMINATORS:      # (a run such as "!?" closes one sentence, not two)
                k += 1
            while k < n and p[k] in CJK_CLOSERS:
                k += 1
            end = i = k
        else:
            i += 1
        if end >= 0:
            out.append(p[start:end].strip())
            start = end
    out.append(p[start:].strip())
    return [s for s in out if s]


def _cut(s: str, max_chars: int) -> List[str]:
    """A sentence longer than max_chars bytes, cut after the last CUT_MARKS character that fits, else at the last whitespace
    that does, else at the largest character boundary."""
    out = []
    while _blen(s) > max_chars:
        mark = space = fit = used = 0
        for i, c in enumerate(s):
            if i and c.isspace() and used <= max_chars:
                space = i
            used += _blen(c)
            if used > max_chars:
                break
            fit = i + 1
            if c in CUT_MARKS:
                mark = i + 1
        at = mark or space or fit
        out.append(s[:at].strip())
        s = s[at:].strip()
    out.append(s)
    return [x for x in out if x]


def _merge(pieces: List[str], max_chars: int, min_chars: int) -> List[str]:
    out, i = [], 0
    while i < len(pieces):
        cur = pieces[i]
        i += 1
        while _blen(cur) < min_chars and i < len(pieces) and _blen(cur) + 1 + _blen(pieces[i]) <= max_chars:
            cur = cur + " " + pieces[i]
            i += 1
        out.append(cur)
    if len(out) >= 2 and _blen(out[-1]) < min_chars and _blen(out[-2]) + 1 + _blen(out[-1]) <= max_chars:
        out[-2:] = [out[-2] + " " + out[-1]]
    return out


def split_text(text: str, max_chars: int = 200, min_chars: int = 24) -> List[Segment]:
    """The segments of a document, in order.  Sizes are UTF-8 byte counts.  Paragraphs are split at sentence ends (a run of
    . ! ? or an ellipsis with closing quotes / brackets, before whitespace or the paragraph's end - but not the dot of an
    initial or of a common abbreviation; a CJK terminator with its closers, whatever follows); a sentence longer than
    `max_chars` is cut at punctuation, else at whitespace, else anywhere; pieces shorter than `min_chars` join a neighbour
    of the same paragraph where the two fit.  Every segment is non-empty and at most `max_chars` bytes, and the segments
    hold the document's characters, whitespace aside.  ValueError: sizes out of range, or nothing to speak."""
    for name, v in (("max_chars", max_chars), ("min_chars", min_chars)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 16 <= max_chars <= 1000:
        raise ValueError(f"max_chars must lie in [16, 1000], got {max_chars}")
    if not 0 <= min_chars <= max_chars:
        raise ValueError(f"min_chars must lie in [0, max_chars], got {min_chars}")
    if not isinstance(text, str):
        raise ValueError(f"text must be a string, got {type(text).__name__}")
    out: List[Segment] = []
    for p in _paragraphs(text):
        pieces = [x for s in _sentences(p) for x in _cut(s, max_chars)]
        for k, seg in enumerate(_merge(pieces, max_chars, min_chars)):
            out.append(Segment(seg, k == 0 and bool(out)))
    if not out:
        raise ValueError("No text to synthesize")
    return out


class JoinParams(NamedTuple):
    threshold: float       # a window is loud when a sample's magnitude reaches it (rounded to float32 by the engine)
    hop: int               # window length, samples at the output rate
    keep: int              # samples kept around the loud part
    fade: int              # fade length at each cut


def _seconds(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, Real) or not 0.0 <= float(v) <= MAX_PAUSE:   # (a nan fails)
        raise ValueError(f"{name} must be a number of seconds in [0, {MAX_PAUSE:g}], got {v!r}")
    return int(round(1000.0 * float(v)))


def join_params(rate: Optional[int], pause=0.2, paragraph_pause=0.5, silence_db: Optional[float] = -45.0):
    """(JoinParams, pause samples, paragraph pause samples) of a synthesize_long call at output rate `rate` (None: 44100).
    hop = fade = rate // 200 (5 ms), keep = 30 ms, a pause of ms milliseconds = (ms rate + 500) // 1000 samples,
    threshold = 10^(silence_db / 20); silence_db None: nothing is trimmed or faded (threshold = keep = fade = 0).
    ValueError for a pause outside [0, 5] s or a silence_db outside [-90, 0]."""
    R = CODEC_RATE if rate is None else int(rate)
    ms, pms = _seconds("pause", pause), _seconds("paragraph_pause", paragraph_pause)
    hop = max(1, R // 200)
    if silence_db is None:
        jp = JoinParams(0.0, hop, 0, 0)
    else:
        if isinstance(silence_db, bool) or not isinstance(silence_db, Real) or \
                not MIN_SILENCE_DB <= float(silence_db) <= MAX_SILENCE_DB:
            raise ValueError(f"silence_db must be None or lie in [{MIN_SILENCE_DB:g}, {MAX_SILENCE_DB:g}], got {silence_db!r}")
        jp = JoinParams(math.pow(10.0, float(silence_db) / 20.0), hop, (30 * R + 500) // 1000, hop)
    return jp, (ms * R + 500) // 1000, (pms * R + 500) // 1000


def ready_prefixes(q: "queue.Queue", n: int) -> Iterator[Tuple[int, list]]:
    """The items 0 .. n-1 of a document in order, in runs: `q` delivers (i, item) in any order (or an exception, which is
    raised here); whenever the next items not yet handed out are there, yields (first index, [the longest such run])."""
    have, nxt = {}, 0
    while nxt < n:
        item = q.get()
        while True:
            if isinstance(item, BaseException):
                raise item
            have[item[0]] = item[1]
            try:
                item = q.get_nowait()
            except queue.Empty:
                break
        j = nxt
        while j in have:
            j += 1
        if j > nxt:
            yield nxt, [have.pop(k) for k in range(nxt, j)]
            nxt = j
