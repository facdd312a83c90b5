"""Rule C13r restated: the 24 kHz -> 16 kHz resampler in f32.  Output m sits at input time t = 1.5 m; base = floor(t), phase = m % 2;
    acc = +0;  for j = -10 .. 11 ascending, zero taps included:  acc = fma32(x[base + j], h[phase][j + 10], acc)        (tests/test_canon_orders.py: fma32)
with x = +0 outside the recording, no renormalisation, n_out = (2 n + 2) // 3.  h = the f32 roundings of the double-precision taps of
voice.resample_24k_to_16k (bark.cpp_amd/voice.py): c = 0.99 * 2 / 3, W = 6 / c, h(u) = c sinc(c u) cos^2(pi u / (2 W)) for |u| < W else 0, u = phase / 2 - j.

fma32_vec is fma32 on arrays: the product of two f32 is exact in float64; the sum with c is formed in float64 with its rounding error (TwoSum) and, where it
is inexact, moved to the neighbour with an odd last bit (round to odd), after which the cast to f32 rounds once (53 >= 2 * 24 + 2 bits) - a plain float64
sum would round twice.  tests/test_resample_ref.py holds it to fma32 on random triples, double-rounding cases among them."""
import numpy as np

HALF = 11
N_TAPS = 2 * HALF
J = np.arange(-HALF + 1, HALF + 1)                       # -10 .. 11
MAX_SAMPLES = 4096 * 320


def taps64() -> np.ndarray:
    """[2][22] in double precision, voice.py's formula"""
    c = 0.99 * 2.0 / 3.0
    W = 6.0 / c
    out = np.zeros((2, N_TAPS), np.float64)
    for phase in (0, 1):
        u = 0.5 * phase - J
        out[phase] = c * np.sinc(c * u) * np.where(np.abs(u) < W, np.cos(np.pi * u / (2.0 * W)) ** 2, 0.0)
    return out


def taps() -> np.ndarray:
    return taps64().astype(np.float32)


def n_out(n: int) -> int:
    return (2 * n + 2) // 3


def fma32_vec(a, b, c) -> np.ndarray:
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b                                             # exact: 48 significant bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c = s + err exactly
    bits = np.atleast_1d(s).view(np.int64).copy()
    err, s1 = np.atleast_1d(err), np.atleast_1d(s)
    need = (err != 0.0) & ((bits & 1) == 0)
    away = (err > 0.0) == (s1 > 0.0)                      # the exact sum lies beyond s in magnitude
    bits = np.where(need, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32).reshape(np.shape(s))


def _gather(x, m):
    """xs [len(m)][22]: the samples x[base + j] of outputs m (zero outside the recording), and the phases"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    m = np.asarray(m, np.int64)
    base = (3 * m) // 2
    idx = base[:, None] + J[None, :]
    ok = (idx >= 0) & (idx < len(x))
    xs = np.where(ok, x[np.clip(idx, 0, len(x) - 1)], np.float32(0.0)).astype(np.float32)
    return xs, (m & 1)


def resample(x, m=None, h=None) -> np.ndarray:
    """C13r on the outputs m (all (2 n + 2) // 3 of them by default), with the taps h [2][22] (taps() by default)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if m is None:
        m = np.arange(n_out(len(x)))
    h = taps() if h is None else np.asarray(h, np.float32).reshape(2, N_TAPS)
    xs, phase = _gather(x, m)
    acc = np.zeros(len(xs), np.float32)
    for k in range(N_TAPS):
        acc = fma32_vec(xs[:, k], h[phase, k], acc)
    return acc


def abs_weight(x, m=None) -> np.ndarray:
    """sum_j |h_j| |x_j| of every output, in double precision: the scale of the rounding bounds"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if m is None:
        m = np.arange(n_out(len(x)))
    xs, phase = _gather(x, m)
    return (np.abs(xs.astype(np.float64)) * np.abs(taps64()[phase])).sum(axis=1)


def dense_signal(n: int, seed: int = 0) -> np.ndarray:
    """n samples at 24 kHz with energy everywhere: two tones, a slow sweep and seeded Gaussian noise.  A prefix of a longer signal is NOT the shorter one's."""
    t = np.arange(n, dtype=np.float64) / 24000.0
    x = 0.3 * np.sin(2 * np.pi * 180.0 * t) + 0.2 * np.sin(2 * np.pi * (300.0 + 40.0 * t) * t) + 0.1 * np.sin(2 * np.pi * 2500.0 * t + 0.5)
    x += 0.1 * np.random.default_rng([seed, 13]).standard_normal(n)
    return x.astype(np.float32)
