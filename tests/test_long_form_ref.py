"""tests/long_form_ref.py (rules C15s and C15j restated) against expectations written out by hand: five fixed texts with their chunks - closers, ellipsis,
line breaks, a clause fallback, an over-budget word, merging against no merging - and joins of tiny arrays with every value spelled out; then two
properties of the join.  The token count used here is the synthetic vocabulary's: one piece per punctuation mark, per run of letters the vocabulary
knows as a word and per run of digits; bytes outside ASCII give none."""
import re

import numpy as np
import pytest

import long_form_ref as lfr
import output_format_ref as ofr


def count(span: bytes) -> int:
    return min(len(re.findall(rb"[!-/:-@\[-`{-~]|[A-Za-z]+|[0-9]+", span)), 256)


# (text, max_tokens, the chunks)
FIXED = [
    # closers behind the mark: " ) and U+2019 are stripped before the last byte is looked at; no merging: one sentence per chunk
    ("He said \"stop.\" She asked (why?) Then ‘go!’ end", 0, ["He said \"stop.\"", "She asked (why?)", "Then ‘go!’", "end"]),
    # U+2026 ends a sentence; so does a line break in the whitespace behind a word (\r\n\r\n holds one), a \t does not
    ("Wait… what\nis\tthis\r\n\r\nok fine", 0, ["Wait…", "what", "is\tthis", "ok fine"]),
    # merging with B = 6 and no sentence end: the last clause end in reach, then a bare cut at the last word that fits
    ("one two, three four five six ten two five one", 6, ["one two,", "three four five six ten two", "five one"]),
    # a single word over the budget (7 pieces, B = 3) is a chunk of its own
    ("a b.c.d.e f g", 3, ["a", "b.c.d.e", "f g"]),
    # the same text without merging, with B = 8 (the LAST sentence end in reach) and with B = 255 (everything fits).  Where the budget matters every
    # word is one of the synthetic vocabulary's, so the model file's tokenizer counts what `count` above counts
    ("Go there. How are they? We are fine. Stop.", 0, ["Go there.", "How are they?", "We are fine.", "Stop."]),
    ("Go there. How are they? We are fine. Stop.", 8, ["Go there. How are they?", "We are fine. Stop."]),
    ("Go there. How are they? We are fine. Stop.", 255, ["Go there. How are they? We are fine. Stop."]),
]


@pytest.mark.parametrize("case", range(len(FIXED)))
def test_fixed_texts_give_the_chunks_written_out(case):
    text, max_tokens, want = FIXED[case]
    raw = text.encode("utf-8")
    spans = lfr.split(raw, max_tokens, count)
    assert [raw[b:e].decode("utf-8") for b, e in spans] == want
    assert all(0 <= b < e <= len(raw) for b, e in spans) and all(spans[i][1] < spans[i + 1][0] for i in range(len(spans) - 1))


def test_spans_are_byte_offsets():
    raw = "Wait… what\nis\tthis\r\n\r\nok fine".encode("utf-8")                       # U+2026 is three bytes
    assert lfr.split(raw, 0, count) == [(0, 7), (8, 12), (13, 20), (24, 31)]
    assert lfr.split(b"  a b.c.d.e  f g ", 3, count) == [(2, 3), (4, 11), (13, 16)]


def test_word_flags():
    flags = {raw[b:e]: (s, c) for raw in [b'a. b." c.\') d, e;] f: - x-y g\xe2\x80\x94 \xe2\x80\x93 h\xe2\x80\xa6\xc2\xbb i\xc2\xbb "'] for b, e, s, c in lfr.words(raw)}
    assert flags == {b"a.": (True, False), b'b."': (True, False), b"c.')": (True, False), b"d,": (False, True), b"e;]": (False, True), b"f:": (False, True),
                     b"-": (False, True), b"x-y": (False, False), b"g\xe2\x80\x94": (False, False), b"\xe2\x80\x93": (False, True),
                     b"h\xe2\x80\xa6\xc2\xbb": (True, False), b"i\xc2\xbb": (False, False), b'"': (False, False)}


def test_edges_of_the_splitter():
    assert lfr.split(b"", 0, count) == [] and lfr.split(b" \t\r\n\f\v ", 5, count) == []
    assert lfr.split(b"word", 1, count) == [(0, 4)]
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            lfr.split(b"a b", bad, count)
    assert len(lfr.split(b"a. " * 64, 0, count)) == 64
    with pytest.raises(ValueError):
        lfr.split(b"a. " * 65, 0, count)
    # without merging a sentence end in reach wins over the end of the text; with merging the end of the text wins
    assert lfr.split(b"a b. c d", 0, count) == [(0, 4), (5, 8)] and lfr.split(b"a b. c d", 10, count) == [(0, 8)]


def _f32(*v):
    return np.array(v, np.float32)


def test_join_of_tiny_arrays_value_by_value():
    segs = [_f32(1, 2, 3), _f32(0, 0.25), _f32(4, -5)]
    p = dict(gap_samples=2, fade_samples=0, trim_threshold=0.5, trim_pad_frames=0)
    assert lfr.layout(segs, p) == ([(0, 3), (3, 0), (5, 2)], 7)                                 # the silent segment takes no room and no second gap
    assert lfr.join24(segs, p).tolist() == [1.0, 2.0, 3.0, 0.0, 0.0, 4.0, -5.0]
    p["fade_samples"] = 1                                                                     # W = [0.5 - 0.5 cos(pi / 2)] = [0.5]: both ends of every range
    assert lfr.fade_table(1).tolist() == [0.5]
    assert lfr.join24(segs, p).tolist() == [0.5, 2.0, 1.5, 0.0, 0.0, 2.0, -2.5]
    p["fade_samples"] = 2                                                                     # W = [0.5 - 0.5 cos(pi / 4), 0.5 - 0.5 cos(3 pi / 4)]
    w0, w1 = np.float32(0.5 - 0.5 * np.cos(np.pi * 0.25)), np.float32(0.5 - 0.5 * np.cos(np.pi * 0.75))
    assert lfr.fade_table(2).tolist() == [float(w0), float(w1)] and abs(w0 - 0.14644662) < 1e-7 and abs(w1 - 0.8535534) < 1e-7
    assert lfr.join24(segs, p).tolist() == [float(np.float32(1) * w0), float(np.float32(2) * w1), float(np.float32(3) * w0), 0.0, 0.0,
                                            float(np.float32(4) * w0), float(np.float32(-5) * w0)]
    p.update(trim_threshold=0.0, fade_samples=0, gap_samples=1)                               # threshold 0: the quiet segment is kept, a gap on either side of it
    assert lfr.join24(segs, p).tolist() == [1.0, 2.0, 3.0, 0.0, 0.0, 0.25, 0.0, 4.0, -5.0]
    p.update(trim_threshold=6.0)
    assert lfr.layout(segs, p) == ([(0, 0), (0, 0), (0, 0)], 0) and len(lfr.join24(segs, p)) == 0 and len(lfr.joined(segs, p, 8000, ofr.MULAW)) == 0


def test_activity_frame_by_frame():
    x = np.zeros(500, np.float32)
    x[250] = -1.0                                                                             # frame 1 of [0, 240) [240, 480) [480, 500)
    assert lfr.activity(x, 1.0, 0) == (240, 480) and lfr.activity(x, 1.0, 1) == (0, 500) and lfr.activity(x, 1.0, 3) == (0, 500)
    assert lfr.activity(x, 1.5, 0) == (0, 0) and lfr.activity(x, 0.0, 0) == (0, 500)
    x[250] = 0.0
    x[499] = 0.5
    assert lfr.activity(x, 0.5, 0) == (480, 500) and lfr.activity(x, 0.5, 1) == (240, 500)
    x[0] = 0.5
    assert lfr.activity(x, 0.5, 0) == (0, 500)
    assert lfr.activity(np.zeros(241, np.float32), 0.0, 0) == (0, 241)


def test_no_trim_no_fade_no_gap_is_concatenation_and_24000_f32_is_join24():
    rng = np.random.default_rng(15)
    segs = [rng.standard_normal(n).astype(np.float32) for n in (1, 239, 240, 241, 777)]
    p = dict(gap_samples=0, fade_samples=0, trim_threshold=0.0, trim_pad_frames=0)
    assert lfr.join24(segs, p).tobytes() == np.concatenate(segs).tobytes()
    for q in (p, dict(gap_samples=7, fade_samples=100, trim_threshold=1.5, trim_pad_frames=1)):
        assert lfr.joined(segs, q, 24000, ofr.F32).tobytes() == lfr.join24(segs, q).tobytes()
        assert lfr.joined(segs, q, 8000, ofr.S16).tobytes() == ofr.to_format(ofr.resample(lfr.join24(segs, q), 24000, 8000), ofr.S16).tobytes()
