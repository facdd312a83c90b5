"""Rules C15s and C15j restated in Python / numpy: the splitter of a long text and the join of the chunks' audio.

C15s  split(text, max_tokens, count): byte spans [begin, end) of the chunks.  Whitespace is space \\t \\n \\r \\f \\v, a word a maximal run of other bytes,
count(bytes) the WordPiece count of a span with n_max = 257 (256: over).  A word ends a sentence if, with trailing closers (" ' ) ] } U+201D U+2019 U+00BB)
stripped, its last byte is . ! ? or it ends in U+2026, or if the whitespace behind it holds a \\n; it ends a clause if the stripped last byte is , ; : or the
whole word is - U+2013 U+2014.  max_tokens 0: B = 255, no merging; 1 .. 255: B = max_tokens, greedy merging.  From word s, E = the last word up to which every
count(s .. e) <= B (E = s when the word alone is over).  E the last word: the chunk is s .. end (without merging the first sentence end in [s, E] still ends
it).  Else: the sentence end in [s, E] (LAST with merging, FIRST without), else the last clause end, else E.  More than 64 chunks: an error.

C15j  activity / layout / join24 / joined: frames of 240 samples, active iff max |x| >= threshold; kept range [240 max(a - pad, 0), min(240 (b + 1 + pad), n));
fade W[k] = f32(0.5 - 0.5 cos(pi (k + 0.5) / F)) applied as one f32 product where d = min(k, K - 1 - k) < F; gap_samples of +0 between consecutive non-empty
kept ranges; joined = format(C14r(J, 24000 -> rate)) (tests/output_format_ref.py)."""
import numpy as np

import output_format_ref as ofr

WHITESPACE = b" \t\n\r\f\v"
CLOSERS = (b'"', b"'", b")", b"]", b"}", "”".encode(), "’".encode(), "»".encode())
ELLIPSIS = "…".encode()
DASHES = (b"-", "–".encode(), "—".encode())
MAX_CHUNKS = 64
FRAME = 240
DEFAULT_JOIN = dict(gap_samples=6000, fade_samples=0, trim_threshold=0.0, trim_pad_frames=0)


# ---- C15s ------------------------------------------------------------------------------------------------------------------------------------------------
def words(text: bytes):
    """[(begin, end, ends a sentence, ends a clause)]"""
    out, i, n = [], 0, len(text)
    while i < n:
        while i < n and text[i] in WHITESPACE:
            i += 1
        if i >= n:
            break
        e = i
        while e < n and text[e] not in WHITESPACE:
            e += 1
        g = e
        while g < n and text[g] in WHITESPACE:
            g += 1
        w = text[i:e]
        s = w
        while True:
            for c in CLOSERS:
                if s.endswith(c):
                    s = s[:len(s) - len(c)]
                    break
            else:
                break
        sentence = b"\n" in text[e:g] or s[-1:] in (b".", b"!", b"?") or s.endswith(ELLIPSIS)
        clause = s[-1:] in (b",", b";", b":") or w in DASHES
        out.append((i, e, sentence, clause))
        i = g
    return out


def split(text: bytes, max_tokens: int, count):
    """count(bytes) -> the WordPiece count of the span with n_max = 257"""
    if not 0 <= max_tokens <= 255:
        raise ValueError("max_tokens is 0 or 1 .. 255")
    merge, B = max_tokens > 0, max_tokens if max_tokens > 0 else 255
    ws = words(text)
    chunks, s = [], 0
    while s < len(ws):
        fits = lambda e: count(text[ws[s][0]:ws[e][1]]) <= B
        E = s
        if fits(s):
            while E + 1 < len(ws) and fits(E + 1):
                E += 1
        sent = [e for e in range(s, E + 1) if ws[e][2]]
        clause = [e for e in range(s, E + 1) if ws[e][3]]
        last = E == len(ws) - 1
        if merge:
            cut = E if last else sent[-1] if sent else clause[-1] if clause else E
        else:
            cut = sent[0] if sent else E if last else clause[-1] if clause else E
        if len(chunks) == MAX_CHUNKS:
            raise ValueError("more than 64 chunks")
        chunks.append((ws[s][0], ws[cut][1]))
        s = cut + 1
    return chunks


# ---- C15j ------------------------------------------------------------------------------------------------------------------------------------------------
def _params(params):
    p = dict(DEFAULT_JOIN)
    p.update(params or {})
    return p


def activity(x, threshold: float, pad: int):
    """the kept range [start, stop) of a segment; (0, 0) if no frame is active"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n = len(x)
    thr = np.float32(threshold)
    act = [j for j in range((n + FRAME - 1) // FRAME) if np.abs(x[FRAME * j:FRAME * (j + 1)]).max() >= thr]
    if not act:
        return 0, 0
    return FRAME * max(act[0] - pad, 0), min(FRAME * (act[-1] + 1 + pad), n)


def fade_table(F: int) -> np.ndarray:
    k = np.arange(F, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (k + 0.5) / F)).astype(np.float32) if F else np.zeros(0, np.float32)


def layout(segments, params=None):
    """([(first sample in J, kept samples)] per segment, N); an empty range sits where the next one would start"""
    p = _params(params)
    out, pos, seen = [], 0, False
    for x in segments:
        a, b = activity(x, p["trim_threshold"], p["trim_pad_frames"])
        if b > a:
            if seen:
                pos += p["gap_samples"]
            seen = True
        out.append((pos, b - a))
        pos += b - a
    return out, pos


def join24(segments, params=None) -> np.ndarray:
    """J: the joined signal at 24 kHz in f32"""
    p = _params(params)
    W = fade_table(p["fade_samples"])
    lay, N = layout(segments, p)
    J = np.zeros(N, np.float32)
    for x, (pos, K) in zip(segments, lay):
        if not K:
            continue
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        a, _ = activity(x, p["trim_threshold"], p["trim_pad_frames"])
        y = x[a:a + K].copy()
        k = np.arange(K)
        d = np.minimum(k, K - 1 - k)
        m = d < len(W)
        y[m] = (y[m] * W[d[m]]).astype(np.float32)
        J[pos:pos + K] = y
    return J


def joined(segments, params=None, rate: int = 24000, fmt: int = ofr.F32, h=None) -> np.ndarray:
    """format(C14r(J, 24000 -> rate)); h: the pair's table [L][2 HALF] (output_format_ref.taps by default)"""
    J = join24(segments, params)
    if not len(J):
        return np.zeros(0, ofr.DTYPE[fmt])
    return ofr.to_format(ofr.resample(J, 24000, rate, h=h), fmt)
