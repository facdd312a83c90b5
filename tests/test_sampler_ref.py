"""The restatement of the greedy sample and the semantic stop rule (tests/sampler_ref.py) without a GPU: pinned to the oracle's semantic stage loop
(ids and the eos_p trace, bit for bit - pyoracle exposes no sampler of its own) and to hand-built rows whose answer follows from reasoning."""
import math
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sampler_ref as S  # noqa: E402

TEXT = "the quick brown fox jumps over the lazy dog"
ULP1 = 2.0 ** -24                                                   # spacing of the floats just below 1.0


def _rn_f32(x: Fraction) -> Fraction:
    """x > 0 rounded to the nearest float32 (ties to even), exactly; normal range"""
    e = math.floor(math.log2(x))
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    q = x / Fraction(2) ** (e - 23)                                 # in [2^23, 2^24)
    m = q.numerator // q.denominator
    r = q - m
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and m % 2 == 1):
        m += 1
    return m * Fraction(2) ** (e - 23)


def test_greedy_equals_the_oracle_stage_loop(toy_oracle):
    """the oracle's logits, one row per step, through greedy(): every id and every eos_p of orc.semantic's own loop, and its stopping point"""
    orc = toy_oracle
    n_steps = 24
    prompt = orc.tokenize(TEXT)
    for min_eos_p in (0.2, 1.4e-4):
        p = orc.params(temp=0.0, fine_temp=0.0, min_eos_p=min_eos_p, n_steps_text_encoder=n_steps)
        ids, trace = orc.semantic(prompt, p, want_eos_trace=True)
        eos_token = 10000                                              # semantic_vocab_size (bark_oracle.cpp Params)
        logits, n_past = orc.gpt_eval(0, prompt, 0, True)
        out = []
        for i in range(n_steps):
            if i > 0:
                logits, n_past = orc.gpt_eval(0, [out[-1]], n_past, False)
            tok, eos_p = S.greedy(logits, False)
            assert np.float32(eos_p) == trace[i], (min_eos_p, i, eos_p, trace[i])
            if S.stop(tok, eos_p, eos_token, p.min_eos_p):
                break
            out.append(tok)
        assert out == ids.tolist(), (min_eos_p, out, ids.tolist())


def test_equal_maxima_the_lower_index_wins():
    for pre in (0, 1):
        l = np.array([-6.0, 2.5, -7.0, 2.5, -5.5, 2.5], np.float32)
        assert S.greedy(l, pre)[0] == 1
        assert S.greedy(l[::-1].copy(), pre)[0] == 0
        assert S.greedy(np.array([-0.0, 0.0, -0.0], np.float32), pre)[0] == 0          # -0 and +0 are one value
        assert S.greedy(np.full(1025, 0.25, np.float32), pre) == (0, float(np.float32(1.0) / np.float32(1025.0)))
    assert S.greedy(np.array([3.0], np.float32), 0) == (0, 1.0)


def test_tie_cut_is_where_the_exponential_rounds_to_one():
    """e = (float) exp(d) is 1.0f down to d = -2^-25 and 1 - 2^-24 for the float just below it: the kernel's kTieCut"""
    cut = np.float32(-2.0 ** -25)
    below = np.nextafter(cut, np.float32(-1))
    for d, e in ((np.float32(-2.0 ** -26), 1.0), (cut, 1.0), (below, 1.0 - ULP1), (np.float32(-1e-7), 1.0 - 2 * ULP1)):
        assert float(np.float32(math.exp(float(d)))) == e, d
    bg = [-5.0, -6.0]
    assert S.greedy(np.array([cut, 0.0] + bg, np.float32), 1)[0] == 0                   # e = 1 twice: the lower index
    assert S.greedy(np.array([np.float32(-1e-6), 0.0] + bg, np.float32), 1)[0] == 1


def test_one_ulp_below_at_a_lower_index_goes_by_the_rounded_quotients():
    """M = 1.0 at index 1, 1 - 2^-24 at index 0: e = 1 - 2^-24 and 1 (d is exact).  The lower index wins exactly when RN(e_0 / S) == RN(1 / S) for
    the float sum S - worked out in rationals; both outcomes occur among the backgrounds"""
    lo = np.float32(1.0 - ULP1)
    outcomes = set()
    for bg in ([], [-4.0], [1.0 - math.log(3.0)], [-0.5, -0.25], [0.5, 0.25, -1.0], [0.9] * 5, [-2.0] * 40, [0.75] * 300):
        l = np.array([lo, 1.0] + bg, np.float32)
        d = (l - np.float32(1.0)).astype(np.float32)
        assert float(d[0]) == -ULP1
        e = [np.float32(math.exp(float(v))) for v in d]
        assert float(e[0]) == 1.0 - ULP1 and float(e[1]) == 1.0
        s = np.float32(0.0)
        for v in e:
            s = np.float32(s + v)                                     # the reference's sequential float sum
        p0 = _rn_f32(Fraction(float(e[0])) / Fraction(float(s)))
        p1 = _rn_f32(Fraction(1) / Fraction(float(s)))
        assert p0 <= p1
        want = 0 if p0 == p1 else 1
        assert all(_rn_f32(Fraction(float(v)) / Fraction(float(s))) <= p1 for v in e[2:])
        tok, eos_p = S.greedy(l, 1)
        assert tok == want, (bg, tok, want)
        assert Fraction(eos_p) == _rn_f32(Fraction(float(e[-1])) / Fraction(float(s))), bg
        outcomes.add(want)
    assert outcomes == {0, 1}


def test_unscaled_rows_are_divided_by_the_float_0_7_first():
    l = np.array([0.7, 0.35, 1.4 - 2.0 ** -23, 1.4], np.float32)
    assert np.array_equal(S.scaled(l, 0), l / np.float32(0.7)) and S.scaled(l, 1) is l
    x = (l / np.float32(0.7)).astype(np.float32)
    assert S.greedy(l, 0) == S.greedy(x, 1)
    # the division can merge two raw logits into one scaled value, and then the lower index wins: around 1.5 a step of one ulp becomes 0.71 ulp of
    # the quotient (1.5 / 0.7 lies in the next binade)
    fl = [np.float32(1.5)]
    for _ in range(8):
        fl.append(np.nextafter(fl[-1], np.float32(9)))
    merged = [(u, v) for u, v in zip(fl, fl[1:]) if np.float32(u / np.float32(0.7)) == np.float32(v / np.float32(0.7))]
    assert merged
    for u, v in merged:
        assert S.greedy(np.array([u, v, -9.0], np.float32), 0)[0] == 0 and S.greedy(np.array([u, v, -9.0], np.float32), 1)[0] == 1


def test_stop_rule():
    l = np.array([0.0, -1.0, -2.0, -0.5], np.float32)
    tok, eos_p = S.greedy(l, 1)
    assert tok == 0 and 0.0 < eos_p < 1.0
    assert eos_p == float(S.probabilities(l, 1)[0, -1])
    assert S.stop(tok, eos_p, eos_token=-1, min_eos_p=eos_p)                             # >=, not >
    assert not S.stop(tok, eos_p, eos_token=-1, min_eos_p=float(np.nextafter(np.float32(eos_p), np.float32(2))))
    assert S.stop(tok, eos_p, eos_token=0, min_eos_p=2.0)                                # the pick is the eos token: eos_p does not matter
    assert not S.stop(tok, eos_p, eos_token=3, min_eos_p=2.0)
    # the threshold is compared as a float: 0.2 is the float 0.2f, as in the engine's parameter struct
    assert S.stop(1, float(np.float32(0.2)), -1, 0.2)


def test_numpy_exponential_form_agrees_or_is_redecided():
    rng = np.random.default_rng(11)
    L = (rng.standard_normal((40, 777)) * 3.0).astype(np.float32)
    ids, eos = S.greedy_rows(L, 0, fast=True)
    for r in range(len(L)):
        tok, e = S.greedy(L[r], 0)
        assert tok == ids[r] and abs(e - float(eos[r])) <= 2.0 ** -22 * e
    assert S.near_ties(np.array([[0.0, -3e-7, -5e-7, -1.0]], np.float32), 1).tolist() == [2]
