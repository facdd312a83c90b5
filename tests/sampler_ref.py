"""Rule C8's greedy sample (gpt_argmax_sample) and the semantic stop rule restated in Python, after the statement above sample_greedy_kernel
(bark.cpp_amd/csrc/misc_kernels.hip) and the sampling section of oracle/bark_oracle.cpp: the reference's arithmetic literally, none of the
kernel's shortcuts.  Independent of the engine.  Used by test_sampler_ref.py (pinned to the oracle's stage loop), test_gpu_decode_sampler.py
(device) and, through it, test_emulated_decode_sampler.py.  Multinomial rows stay with nucleus_ref.multinomial / sample."""
import numpy as np

from nucleus_ref import _exp_f32

INT32_MAX = 2 ** 31 - 1
# the kernel's constants, for the tests' statements about which path a row takes (the restatement itself does not use them)
TIE_CUT = np.float32(-2.0 ** -25)
NEAR_TIE = np.float32(-4.0e-7)
EOS_BAND = 2.0e-3


def scaled(l, prescaled):
    """the logits the softmax sees: l / 0.7f in float unless the LM head has already divided"""
    l = np.asarray(l, np.float32)
    return l if prescaled else (l / np.float32(0.7)).astype(np.float32)


def probabilities(l, prescaled, fast=False):
    """p [.., n] float32: max, e_i = (float) exp((double) (l_i - max)), float sum in index order, p_i = e_i / sum.  fast: numpy's exp (bulk checks
    that re-decide any disagreement without it)"""
    x = np.atleast_2d(scaled(l, prescaled))
    d = (x - x.max(axis=1, keepdims=True)).astype(np.float32)
    e = np.zeros(d.shape, np.float32)
    fin = np.isfinite(d)
    e[fin] = _exp_f32(d[fin], fast)
    fs = np.add.accumulate(e, axis=1, dtype=np.float32)[:, -1:]            # sequential float sum
    return (e / fs).astype(np.float32)


def greedy(l, prescaled, fast=False):
    """one row: (id, eos_p) - the first index of the largest probability, the probability of the last logit"""
    p = probabilities(l, prescaled, fast)[0]
    return int(np.argmax(p)), float(p[-1])


def greedy_rows(L, prescaled, fast=True):
    """rows [R, n]: (ids int64 [R], eos_p float32 [R])"""
    p = probabilities(L, prescaled, fast)
    return np.argmax(p, axis=1), p[:, -1].copy()


def stop(tok, eos_p, eos_token, min_eos_p):
    """the semantic stage's stop rule on one sample"""
    return bool(tok == eos_token or np.float32(eos_p) >= np.float32(min_eos_p))


def near_ties(L, prescaled):
    """per row: how many logits lie within NEAR_TIE of the maximum (the maximum itself included).  More than one: the kernel must take its exact path."""
    x = np.atleast_2d(scaled(L, prescaled))
    d = (x - x.max(axis=1, keepdims=True)).astype(np.float32)
    return np.count_nonzero(d >= NEAR_TIE, axis=1)
