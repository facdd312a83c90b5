"""Rule C14r and the sample formats restated in numpy: the rational resampler between 24 kHz and the other supported rates, s16 and mu-law.

For a pair (rate_in, rate_out): g = gcd, L = rate_out / g, M = rate_in / g, c = 0.99 min(1, L / M), W = 6 / c, HALF = ceil(W) + 1, 2 HALF taps per phase at
j = -HALF + 1 .. HALF:   h[p][j] = c sinc(c u) cos^2(pi u / (2 W)) for |u| < W, else 0,   u = p / L - j   (double precision, this expression order, rounded once
to f32).  Output m: base = floor(m M / L), phase = (m M) mod L,
    acc = +0;  for j ascending, zero taps included:  acc = fma32(x[base + j], h[phase][j + HALF - 1], acc)                    (tests/resample_ref.py: fma32_vec)
with x = +0 outside the recording, no renormalisation, n_out = ceil(n L / M).  rate_in == rate_out: the samples themselves.
s16: r = rint(y * 32768) (ties to even) clamped to [-32768, 32767].  mu-law (G.711) from the s16 value s: sign = 0x80 if s < 0, mag = min(|s|, 32635) + 132,
e = floor(log2 mag) - 7, man = (mag >> (e + 3)) & 15, byte = ~(sign | e << 4 | man) & 0xFF."""
from math import gcd

import numpy as np

from resample_ref import fma32_vec

RATES = (8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
PAIRS = [(24000, r) for r in RATES if r != 24000] + [(r, 24000) for r in RATES if r != 24000]          # the 14 pairs with a filter
MAX_SAMPLES = 4096 * 320
F32, S16, MULAW = 0, 1, 2
BYTES = {F32: 4, S16: 2, MULAW: 1}
DTYPE = {F32: np.float32, S16: np.int16, MULAW: np.uint8}


def supported(rate_in: int, rate_out: int) -> bool:
    return rate_in in RATES and rate_out in RATES and 24000 in (rate_in, rate_out)


def lmh(rate_in: int, rate_out: int):
    """(L, M, HALF)"""
    g = gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    c = 0.99 * min(1.0, L / M)
    return L, M, int(np.ceil(6.0 / c)) + 1


def taps64(rate_in: int, rate_out: int) -> np.ndarray:
    """[L][2 HALF] in double precision"""
    L, M, half = lmh(rate_in, rate_out)
    c = 0.99 * min(1.0, L / M)
    W = 6.0 / c
    j = np.arange(-half + 1, half + 1)
    out = np.zeros((L, 2 * half), np.float64)
    for p in range(L):
        u = p / L - j
        out[p] = c * np.sinc(c * u) * np.where(np.abs(u) < W, np.cos(np.pi * u / (2.0 * W)) ** 2, 0.0)
    return out


def taps(rate_in: int, rate_out: int) -> np.ndarray:
    return taps64(rate_in, rate_out).astype(np.float32)


def n_out(n: int, rate_in: int, rate_out: int) -> int:
    if rate_in == rate_out:
        return n
    L, M, _ = lmh(rate_in, rate_out)
    return (n * L + M - 1) // M


def _gather(x, m, rate_in, rate_out):
    """xs [len(m)][2 HALF]: the samples x[base + j] of outputs m (zero outside the recording), and the phases"""
    L, M, half = lmh(rate_in, rate_out)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    m = np.asarray(m, np.int64)
    base, phase = (m * M) // L, (m * M) % L
    idx = base[:, None] + np.arange(-half + 1, half + 1)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    xs = np.where(ok, x[np.clip(idx, 0, len(x) - 1)], np.float32(0.0)).astype(np.float32)
    return xs, phase


def resample(x, rate_in: int, rate_out: int, m=None, h=None) -> np.ndarray:
    """C14r on the outputs m (all of them by default) with the taps h [L][2 HALF] (taps() by default)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if rate_in == rate_out:
        return x.copy() if m is None else x[np.asarray(m, np.int64)]
    L, M, half = lmh(rate_in, rate_out)
    if m is None:
        m = np.arange(n_out(len(x), rate_in, rate_out))
    h = taps(rate_in, rate_out) if h is None else np.asarray(h, np.float32).reshape(L, 2 * half)
    xs, phase = _gather(x, m, rate_in, rate_out)
    acc = np.zeros(len(xs), np.float32)
    for k in range(2 * half):
        acc = fma32_vec(xs[:, k], h[phase, k], acc)
    return acc


def exact(x, rate_in: int, rate_out: int, m=None):
    """(the float64 sum with the float64 taps, sum_j |h_j| |x_j|) of every output: the yardstick and the scale of the rounding bound"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if m is None:
        m = np.arange(n_out(len(x), rate_in, rate_out))
    xs, phase = _gather(x, m, rate_in, rate_out)
    h = taps64(rate_in, rate_out)[phase]
    return (xs.astype(np.float64) * h).sum(axis=1), (np.abs(xs.astype(np.float64)) * np.abs(h)).sum(axis=1)


def to_s16(y) -> np.ndarray:
    v = (np.asarray(y, np.float32) * np.float32(32768.0)).astype(np.float32)
    return np.clip(np.rint(v), -32768.0, 32767.0).astype(np.int16)


def mulaw_of_s16(s) -> np.ndarray:
    s = np.asarray(s, np.int16).astype(np.int64)
    sign = np.where(s < 0, 0x80, 0)
    mag = np.minimum(np.abs(s), 32635) + 132
    e = np.floor(np.log2(mag.astype(np.float64))).astype(np.int64) - 7          # mag < 2^15: log2 of an integer in double never crosses a power of two
    man = (mag >> (e + 3)) & 15
    return (~(sign | (e << 4) | man) & 0xFF).astype(np.uint8)


def to_format(y, fmt: int) -> np.ndarray:
    """format(resample_f32(x)): f32 as is, s16, or mu-law of the s16 value"""
    if fmt == F32:
        return np.asarray(y, np.float32)
    s = to_s16(y)
    return s if fmt == S16 else mulaw_of_s16(s)
