"""CPU: the text splitter of synthesize_long (fish_tts_amd/longform.py) - its three properties on a fixed corpus and on
200 seeded random texts, literal expected splits, the argument checks, the join parameters and the ordered hand-out of
segments (ready_prefixes).  The module loads without torch, ctypes or the native library."""
import os
import queue
import random
import subprocess
import sys

import pytest

from fish_tts_amd.longform import Segment, join_params, ready_prefixes, split_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CORPUS = [
    "Dr. Smith met Mrs. Jones at St. Mary's. They talked, e.g. about fig. 3 vs. fig. 4, etc. and left.",
    "J. R. R. Tolkien wrote it. A. A. Milne did not.",
    "Pi is about 3.14. Version 2.0.1 is out! Cost: $4.50?",
    'She said "Stop!" He asked "Why?" and then (quietly) left.) The end...',
    "“Really?!” she asked… ‘Yes.’ »Gut.» [Done.] Fine",
    "今天天气很好。我们去公园吧！好不好？「好」。他说：“走吧。”然后就走了；没有回头",
    "これはペンです。あれは？",
    "word " * 140,                                         # 700 bytes, no punctuation
    "x" * 300,                                             # one 300-byte word
    "é" * 150 + " " + "ü" * 150,                           # two-byte characters at the cut
    "First paragraph, line one.\r\nStill the first.\r\n\r\nSecond paragraph.\r\r\n \t \nThird one here.",
    "A long clause, then another one; and a third: all of them — with dashes — go on and on and on, " * 4,
    "Short. Tiny. Ok. And now a sentence that is clearly long enough to stand alone. Hm.",
    "Hi.",
    "  \n\n   leading and trailing space   \n\n ",
    "No terminator at the end",
    "Mixed 中文 and English. 然后继续。And back.",
    "a.b.c. d.e. f",
]


def _nows(s):
    return "".join(s.split())


def _check(text, max_chars, min_chars):
    segs = split_text(text, max_chars, min_chars)
    assert segs and not segs[0].paragraph
    for s in segs:
        assert isinstance(s, Segment) and s.text and s.text == s.text.strip()
        assert len(s.text.encode("utf-8")) <= max_chars, (s, max_chars)
    assert _nows("".join(s.text for s in segs)) == _nows(text)
    return segs


@pytest.mark.parametrize("sizes", [(200, 24), (16, 0), (16, 16), (40, 10), (1000, 0), (64, 64)])
def test_properties_on_the_corpus(sizes):
    for text in CORPUS:
        _check(text, *sizes)


def test_properties_on_random_texts():
    rng = random.Random(1234)
    alphabet = ["a", "b", "word", "Dr", "e.g", "x", "Z", "é", "中", "文", "。", "！", "？", "；", "、", "，", ".", "!", "?", "…",
                ",", ";", ":", "—", '"', "'", "”", "’", ")", "]", "»", "」", "』", "）", " ", " ", " ", "  ", "\n", "\r\n", "\r",
                "\n\n", "\t", "3.14", "(", " ", "　"]
    n = 0
    while n < 200:
        text = "".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 400)))
        if not text.strip():
            continue
        max_chars = rng.choice([16, 17, 31, 64, 200, 1000])
        _check(text, max_chars, rng.randrange(0, max_chars + 1))
        n += 1


def test_one_short_sentence_is_one_segment():
    for text in ["Hello  there,\n general Kenobi.", "No end mark", "  One!  ", "Dr. No came.", "中文一句。", "x" * 200]:
        for max_chars in (200, 1000):
            assert split_text(text, max_chars, 24) == [Segment(" ".join(text.split()), False)]


LITERAL = [
    ("One two three four five six. Seven eight nine ten eleven twelve.", 200, 24,
     ["One two three four five six.", "Seven eight nine ten eleven twelve."]),
    ("Dr. Smith and Mr. J. Doe arrived at the station. They were late for the meeting.", 200, 24,
     ["Dr. Smith and Mr. J. Doe arrived at the station.", "They were late for the meeting."]),
    ("The value is 3.14 and not more. That much is certain, friend.", 200, 24,
     ["The value is 3.14 and not more.", "That much is certain, friend."]),
    ('He shouted "Stop right there!" and everyone froze. Nobody moved again.', 200, 0,
     ['He shouted "Stop right there!"', "and everyone froze.", "Nobody moved again."]),   # (quotes after a terminator end it)
    ('"Is it really over now?" she asked him. (It was not.) He nodded...', 200, 0,
     ['"Is it really over now?"', "she asked him.", "(It was not.)", "He nodded..."]),
    ("今天天气很好。我们去公园吧！好不好？", 200, 0, ["今天天气很好。", "我们去公园吧！", "好不好？"]),
    ("他说「走吧。」然后就走了", 200, 0, ["他说「走吧。」", "然后就走了"]),
    ("Hi. Yes. This sentence is long enough to stand alone all right. No.", 200, 24,
     ["Hi. Yes. This sentence is long enough to stand alone all right. No."]),
    ("aaaa bbbb cccc dddd eeee ffff", 16, 0, ["aaaa bbbb cccc", "dddd eeee ffff"]),
    ("aaaa, bbbb cccc dddd eeee", 16, 0, ["aaaa,", "bbbb cccc dddd", "eeee"]),
    ("abcdefghijklmnopqrstuvwxyz", 16, 0, ["abcdefghijklmnop", "qrstuvwxyz"]),
    ("ééééééééé", 16, 0, ["éééééééé", "é"]),
    ("First one here.\r\n\r\nSecond one here.\r \rThird.", 200, 24, ["First one here.", "Second one here.", "Third."]),
    ("e.g. this is not split here. But here it is, of course.", 200, 24,
     ["e.g. this is not split here.", "But here it is, of course."]),
]


@pytest.mark.parametrize("case", LITERAL, ids=[str(i) for i in range(len(LITERAL))])
def test_literal_splits(case):
    text, max_chars, min_chars, want = case
    assert [s.text for s in split_text(text, max_chars, min_chars)] == want


def test_paragraph_flags_and_no_merge_across_paragraphs():
    segs = split_text("One. Two.\n\nThree.\n \nFour is the last paragraph of them. Five.", 200, 24)
    assert segs == [Segment("One. Two.", False), Segment("Three.", True),
                    Segment("Four is the last paragraph of them. Five.", True)]


def test_bad_arguments():
    for text in ["", "   ", "\r\n \n\t", "　"]:
        with pytest.raises(ValueError, match="No text to synthesize"):
            split_text(text)
    for kw in [dict(max_chars=15), dict(max_chars=1001), dict(min_chars=-1), dict(max_chars=50, min_chars=51),
               dict(max_chars=20.0), dict(min_chars=True), dict(max_chars="200")]:
        with pytest.raises(ValueError):
            split_text("Some text.", **kw)
    with pytest.raises(ValueError):
        split_text(None)


def test_join_params():
    jp, gap, pgap = join_params(None)
    assert tuple(jp) == (10 ** (-45 / 20), 220, 1323, 220) and (gap, pgap) == (8820, 22050)
    jp, gap, pgap = join_params(8000, 0.013, 5, -6.0)
    assert (jp.hop, jp.keep, jp.fade) == (40, 240, 40) and (gap, pgap) == (104, 40000)
    assert abs(jp.threshold - 0.5011872336272722) < 1e-15
    jp, gap, pgap = join_params(16000, 0, 0, None)
    assert tuple(jp) == (0.0, 80, 0, 0) and (gap, pgap) == (0, 0)
    assert join_params(22050, 0.0004, 0.0005)[1:] == (0, 0) and join_params(44100, 0.001, 0.0015)[1:] == (44, 88)
    for kw in [dict(pause=-0.001), dict(pause=5.001), dict(pause=float("nan")), dict(pause="1"), dict(pause=True),
               dict(pause=None), dict(paragraph_pause=-1), dict(paragraph_pause=6), dict(paragraph_pause=float("inf")),
               dict(silence_db=0.1), dict(silence_db=-90.5), dict(silence_db=float("nan")), dict(silence_db="-45"),
               dict(silence_db=False)]:
        with pytest.raises(ValueError):
            join_params(None, **kw)


def test_ready_prefixes_hands_out_runs_in_order():
    q = queue.Queue()
    for i in (2, 0):
        q.put((i, f"c{i}"))
    it = ready_prefixes(q, 5)
    assert next(it) == (0, ["c0"])
    q.put((4, "c4"))
    q.put((1, "c1"))
    assert next(it) == (1, ["c1", "c2"])
    q.put((3, "c3"))
    assert next(it) == (3, ["c3", "c4"])
    with pytest.raises(StopIteration):
        next(it)
    q.put((1, "x"))
    q.put(KeyError("boom"))
    with pytest.raises(KeyError):
        list(ready_prefixes(q, 3))


def test_module_loads_without_torch_or_the_native_library():
    code = ("import sys, importlib.util as u\n"
            "spec = u.spec_from_file_location('longform', sys.argv[1])\n"
            "m = u.module_from_spec(spec); sys.modules['longform'] = m; spec.loader.exec_module(m)\n"
            "assert m.split_text('A. B.')[0].text == 'A. B.'\n"
            "assert 'torch' not in sys.modules and 'ctypes' not in sys.modules and 'numpy' not in sys.modules\n")
    path = os.path.join(ROOT, "fish-tts_amd", "longform.py")
    subprocess.run([sys.executable, "-S", "-c", code, path], check=True)
