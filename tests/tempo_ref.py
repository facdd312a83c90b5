"""Rule C16t restated: the speaking rate of a 24 kHz f32 recording by waveform-similarity overlap-add, every fmaf through
resample_ref.fma32_vec.  x: n samples, p = speed_permille in 500 .. 2000; p == 1000 is the identity and nothing below runs.
    W = 720 (frame), HS = 360 (synthesis hop), D = 240 (search radius);  w[k] = f32(0.5 - 0.5 cos(2 pi k / 720)) formed in double, a committed table
    n_out = ceil(1000 n / p), K = ceil(n_out / HS) frames, x reads +0 outside [0, n)
    pos[-1] = -HS, pos[0] = 0; for k >= 1: a = floor(k HS p / 1000), t[j] = x[pos[k - 1] + HS + j],
        score(d) = the fmaf chain from +0 over t[j] x[a + d + j], j = 0 .. HS - 1 ascending, d in [-D, D],
        scanned in the order 0, -1, +1, -2, +2, .., -D, +D, a candidate replaces the best only with a strictly greater score; pos[k] = a + the winner
    y[m] = fmaf(w[j], x[pos[k] + j], w[HS + j] * x[pos[k - 1] + HS + j]),  k = m // HS, j = m - k HS  (one rounded product, one fmaf)
The window is an argument: the tests pass the library's own table (bark_hip_tempo_window)."""
import numpy as np

from resample_ref import fma32_vec

W, HS, D = 720, 360, 240
N_CAND = 2 * D + 1
P_MIN, P_MAX = 500, 2000
MAX_SAMPLES = 4096 * 320
MAX_ABS = 65520.0
_DELTA = np.arange(-D, D + 1)
SCAN = np.argsort(np.where(_DELTA == 0, 0, np.where(_DELTA < 0, -2 * _DELTA - 1, 2 * _DELTA)), kind="stable")      # candidate indices d + D in scan order


def window64() -> np.ndarray:
    k = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / 720.0)


def window() -> np.ndarray:
    return window64().astype(np.float32)


def out_len(n: int, p: int) -> int:
    return (1000 * int(n) + int(p) - 1) // int(p)


def n_frames(n: int, p: int) -> int:
    return (out_len(n, p) + HS - 1) // HS


def nominal(k: int, p: int) -> int:
    return (int(k) * HS * int(p)) // 1000


def tempo(x, p: int, w=None, want_pos: bool = False):
    """C16t of one recording; want_pos: (y, pos[K]) - at p == 1000 the positions are the nominal ones, k HS"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n, p = len(x), int(p)
    assert n >= 1 and P_MIN <= p <= P_MAX
    K = n_frames(n, p)
    if p == 1000:
        return (x.copy(), np.arange(K, dtype=np.int32) * HS) if want_pos else x.copy()
    w = window() if w is None else np.ascontiguousarray(w, np.float32).reshape(W)
    lead = HS + D + 8
    xz = np.zeros(lead + nominal(K, p) + D + W + 8 + n, np.float32)
    xz[lead:lead + n] = x

    def get(i0, count):
        return xz[lead + i0:lead + i0 + count]

    y = np.zeros(K * HS, np.float32)
    pos = np.zeros(K, np.int32)
    prev = -HS
    for k in range(K):
        cur = 0
        if k >= 1:
            a = nominal(k, p)
            t = get(prev + HS, HS)
            cand = np.lib.stride_tricks.sliding_window_view(get(a - D, N_CAND + HS - 1), HS)      # [481][360]: row c is x[a - D + c ..]
            acc = np.zeros(N_CAND, np.float32)
            for j in range(HS):
                acc = fma32_vec(np.full(N_CAND, t[j], np.float32), cand[:, j], acc)
            cur = a + int(_DELTA[SCAN[int(np.argmax(acc[SCAN]))]])                                # the first maximum in scan order
        pos[k] = cur
        y[k * HS:(k + 1) * HS] = fma32_vec(w[:HS], get(cur, HS), w[HS:] * get(prev + HS, HS))
        prev = cur
    y = y[:out_len(n, p)].copy()
    return (y, pos) if want_pos else y
