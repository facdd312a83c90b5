"""Rule C8n restated in Python: the top-k / nucleus filter of the semantic and coarse samples, then C8's multinomial
pick as libstdc++'s std::discrete_distribution makes it.  Independent of the engine: a stable sort, exact integers for the nucleus, literal
sequential sums for the softmax.  Used by test_nucleus_sampling_host.py (emulated engine) and test_gpu_nucleus_sampling.py (device)."""
import math
from fractions import Fraction

import numpy as np


def _exp_f32(d, fast=False):
    """(float) exp((double) d) per element, with the C library's exp (what the host path and the reference use).  fast: numpy's exp, which can
    differ from it in the last bit of the double (then, rarely, in the float) - for bulk checks that recheck any disagreement without it."""
    if fast:
        return np.exp(np.asarray(d, np.float64)).astype(np.float32)
    return np.array([math.exp(float(v)) for v in np.asarray(d, np.float64)], np.float64).astype(np.float32)


def order(l):
    """pi: ids by logit descending, ties (-0.0 == 0.0 included) by ascending id."""
    l = np.asarray(l, np.float32)
    return np.lexsort((np.arange(l.size), -l.astype(np.float64)))


def weights(l, fast=False):
    """w_i = floor(e_i 2^40), e_i = (float) exp((double) (l_i - max)): exact integers."""
    l = np.asarray(l, np.float32)
    e = _exp_f32((l - l.max()).astype(np.float32), fast)
    return [int(math.floor(float(v) * 2.0 ** 40)) for v in e]


def keep_mask_fast(l, top_k, top_p):
    """keep_mask with numpy's exp and array prefix sums (integers: still exact) - bulk checks"""
    l = np.asarray(l, np.float32)
    n = l.size
    pi = order(l)
    J = n
    if top_p < 1.0:
        e = _exp_f32((l - l.max()).astype(np.float32), True)
        w = np.floor(e.astype(np.float64) * 2.0 ** 40).astype(np.int64)
        fr = Fraction(float(np.float32(top_p)))
        T = (fr.numerator * int(w.sum())) // fr.denominator          # W <= top_p * S  <=>  W <= floor(top_p * S) for an integer W
        ws = w[pi]
        excl = np.concatenate([[0], np.cumsum(ws)[:-1]])
        J = max(1, int(np.count_nonzero(excl <= T)))
    F = J
    if 0 < top_k < J:
        v = l[pi[top_k - 1]]
        F = top_k + int(np.count_nonzero(l[pi[top_k:J]] >= v))
    keep = np.zeros(n, bool)
    keep[pi[:F]] = True
    return keep


def keep_mask(l, top_k, top_p):
    """bool [n]: the ids the filter keeps (top-p on the untempered logits, then top-k)."""
    l = np.asarray(l, np.float32)
    n = l.size
    pi = order(l)
    J = n
    if top_p < 1.0:
        w = weights(l)
        S = sum(w)
        T = Fraction(float(np.float32(top_p))) * S            # the comparison is exact, on the float value of top_p
        J, run = 0, 0
        for j in range(n):
            if j > 0 and run > T:
                break
            J = j + 1
            run += w[pi[j]]
    F = J
    if 0 < top_k < J:
        v = l[pi[top_k - 1]]
        F = top_k
        while F < J and l[pi[F]] >= v:                       # ties with the top_k-th logit stay
            F += 1
    keep = np.zeros(n, bool)
    keep[pi[:F]] = True
    return keep


def multinomial(l, temp, u, keep=None, fast=False):
    """C8's draw: l / temp, max, (float) exp((double) .), float sum in index order, p_i = e_i / sum; libstdc++'s discrete_distribution on u
    (double accumulate, normalise, partial_sum, last one pinned to 1.0, lower_bound).  Returns (id, p_{n-1})."""
    x = np.asarray(l, np.float32).copy()
    if keep is not None:
        x[~keep] = -np.inf
    x = (x / np.float32(temp)).astype(np.float32)
    mx = x.max()
    d = (x - mx).astype(np.float32)
    e = np.zeros(x.size, np.float32)
    fin = np.isfinite(d)
    e[fin] = _exp_f32(d[fin], fast)
    fs = np.cumsum(e, dtype=np.float32)[-1]                   # sequential float sum
    p = (e / fs).astype(np.float32)
    if p.size < 2:
        return 0, float(p[-1])
    p64 = p.astype(np.float64)
    s = np.cumsum(p64)[-1]
    cp = np.cumsum(p64 / s)
    cp[-1] = 1.0
    return int(np.searchsorted(cp, u, side="left")), float(p[-1])


def sample(l, temp, top_k, top_p, u):
    """C8n: filter, then the draw.  Returns (id, eos_p)."""
    return multinomial(l, temp, u, keep_mask(l, top_k, top_p))


def bin_edges(l, temp, top_k, top_p):
    """the running sums cp of the draw (u within 1e-9 of one of them is an adversarial draw)"""
    keep = keep_mask_fast(l, top_k, top_p)
    x = np.asarray(l, np.float32).copy()
    x[~keep] = -np.inf
    x = (x / np.float32(temp)).astype(np.float32)
    d = (x - x.max()).astype(np.float32)
    e = np.zeros(x.size, np.float32)
    fin = np.isfinite(d)
    e[fin] = _exp_f32(d[fin], True)
    p = (e / np.cumsum(e, dtype=np.float32)[-1]).astype(np.float32).astype(np.float64)
    return np.cumsum(p / np.cumsum(p)[-1])


def exact_path_forced(l, temp, top_k, top_p, u, margin=5e-7):
    """True when u lies within `margin` of an end of the bin it picks.  C8's device sampler then takes its exact path (its own running sums are
    within ~1.3e-7 of these, and it settles anything within 1e-6 of an end exactly), whose eos_p is the sequential value: bit-equal here."""
    cp = bin_edges(l, temp, top_k, top_p)
    cp[-1] = 1.0
    j = int(np.searchsorted(cp, u, side="left"))
    prev = cp[j - 1] if j > 0 else 0.0
    return bool(cp[j] - u < margin or u - prev < margin)


class MT19937:
    """std::mt19937 (32-bit Mersenne twister, default seeding) and std::generate_canonical<double, 53> on it (two words per draw)."""

    def __init__(self, seed):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.i = 624

    def word(self):
        if self.i >= 624:
            mt = self.mt
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.i = 0
        y = self.mt[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF

    def canonical(self):
        lo = self.word()
        hi = self.word()
        r = (float(lo) + float(hi) * 4294967296.0) / 18446744073709551616.0
        return r if r < 1.0 else math.nextafter(1.0, 0.0)
