"""The weight block formats read independently of engine and oracle (tests/block_formats_ref.py: a numpy dequantiser written from ggml's
definitions).

The engine is held bit-equal to the oracle on quantised files (tests/test_gpu_weight_formats.py, tests/test_gpu_parity.py), but one author
wrote both: had both misread a format the same way - the fifth-bit word of q5_0 / q5_1, the nibble halves, the minimum of q4_1 / q5_1 -
they would compute the same scrambled model and agree.  Here the oracle on a quantised file must compute what plain f32 arithmetic
computes on the file's dequantised twin (every quantised matrix replaced by its dequantised values, f32 weights x f32 activations), up to
ggml's q8 rounding of the activations, the one thing the twin leaves out.  Three deliberately wrong readings are the negative controls:
each must miss by at least ten times the tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import block_formats_ref as bf  # noqa: E402
from test_quantize import _blocks  # noqa: E402

FMTS = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0")
FTYPE = {"q4_0": 2002, "q4_1": 2003, "q8_0": 2007, "q5_0": 2008, "q5_1": 2009}
LEVELS = {"q4_0": (-8, 7), "q4_1": (0, 15), "q5_0": (-16, 15), "q5_1": (0, 31), "q8_0": (-127, 127)}
N_THREADS = 8
# Per evaluation of bf.evaluations, with Δ = logits(quantised file) - logits(twin) and σ = std(logits of the twin):
#   max |Δ| <= TAU * σ  and  rms(Δ) <= TAU_RMS * σ.
# Measured on the seed-0 toy / mini models, all five formats: rms(Δ) / σ = 0.007 - 0.014 (toy 0.007 - 0.010, mini 0.010 - 0.014), max |Δ| / σ
# = 0.028 - 0.061 (toy <= 0.044, mini <= 0.061).  The maximum is 3.5 - 5.7 times the rms: the extreme of noise over 10^4 logits (decode and
# prompt rows) to 10^6 (fine passes), not a structure - and q8_0 weights, 15 times finer than q4_0's, show the same spread, so it is the
# activations' q8 rounding (relative error ~ 1 / (127 * sqrt(12)) of a block's largest value per element) that moves the logits.  The wrong
# readings below move them by 3.3 - 7.0 sigma.
TAU = 0.08
TAU_RMS = 0.02
WRONG = [("swap_nibbles", f) for f in ("q4_0", "q4_1", "q5_0", "q5_1")] + [("qh_wrong_half", f) for f in ("q5_0", "q5_1")] + \
        [("drop_min", f) for f in ("q4_1", "q5_1")]


def _exact_level_blocks(fmt, rng, n):
    """n blocks that hold nothing but levels * d (+ m), d a power of two and m a multiple of d: the quantiser recovers every level and
    the dequantiser every weight exactly.  -> (levels [n, 32], weights [n, 32])"""
    lo, hi = LEVELS[fmt]
    q = rng.integers(lo, hi + 1, (n, 32))
    rows, k = np.arange(n), rng.integers(0, 32, n)
    c = np.zeros(n, np.int64)
    if fmt in ("q4_1", "q5_1"):                      # the minimum (level 0) and the maximum fix m and d = (max - min) / hi
        q[rows, k] = 0
        q[rows, (k + rng.integers(1, 32, n)) % 32] = hi
        c = rng.integers(-40, 9, n)                  # m = c * d
    elif fmt == "q8_0":                              # d = amax / 127
        q[rows, k] = rng.choice([-127, 127], n)
    else:                                            # d = (the first element of largest magnitude) / -8 or / -16
        q[rows, k] = lo
    s = 2.0 ** -rng.integers(4, 11, n)
    return q, ((q + c[:, None]) * s[:, None]).astype(np.float32)


@pytest.mark.parametrize("fmt", FMTS)
def test_dequantiser_inverts_the_quantiser_restatements(fmt):
    """Dequantising the blocks of tests/test_quantize.py's numpy copies of ggml's quantisers: every weight within its block's |d| (the
    f16 rounding of d and m aside), and exactly the weights of blocks built from levels - which pins every element to its nibble and
    its fifth bit."""
    rng = np.random.default_rng(FMTS.index(fmt))
    w = np.concatenate([rng.standard_normal(32 * 256) * 0.02, rng.standard_normal(32 * 64) * 3.0, rng.uniform(-1.0, 1.0, 32 * 64) + 0.5])
    w = w.astype(np.float32)
    raw = _blocks(fmt, w).tobytes()
    d = np.abs(bf.block_scales(fmt, raw))
    err = np.abs(bf.dequantize(fmt, raw).reshape(-1, 32) - w.reshape(-1, 32))
    assert np.all(err <= d[:, None] * (1 + 2.0 ** -6)), float(np.max(err / d[:, None]))
    q, wx = _exact_level_blocks(fmt, rng, 512)
    raw = _blocks(fmt, wx).tobytes()
    assert np.array_equal(bf.levels(fmt, raw), q)
    assert np.array_equal(bf.dequantize(fmt, raw), wx.reshape(-1))


def _oracle_evaluations(path, ftype):
    from oracle.pyoracle import Oracle
    o = Oracle(path, n_threads=N_THREADS)
    try:
        assert o.hparams(0)["ftype"] == ftype
        return bf.evaluations(o, bf.evaluation_inputs())
    finally:
        o.close()


def _twin_evaluations(src, tmp_path, variant=None):
    twin = str(tmp_path / "twin.bin")
    try:
        seen = bf.write_dequantized_twin(src, twin, variant)
        return seen, _oracle_evaluations(twin, 0)
    finally:
        if os.path.exists(twin):
            os.remove(twin)


def _spread(got, ref, rms=False):
    """evaluation -> max |got - ref| / std(ref), or rms(got - ref) / std(ref)"""
    out = {}
    for k in ref:
        d = got[k].astype(np.float64) - ref[k]
        out[k] = float((np.sqrt(np.mean(d * d)) if rms else np.max(np.abs(d))) / np.std(ref[k].astype(np.float64)))
    return out


@pytest.fixture(scope="module")
def quantised_evaluations(toy_model, mini_model, quantized_model):
    """(preset, fmt) -> the oracle's evaluations on the quantised file, computed once"""
    cache = {}

    def get(preset, fmt):
        if (preset, fmt) not in cache:
            cache[(preset, fmt)] = _oracle_evaluations(quantized_model({"toy": toy_model, "mini": mini_model}[preset], fmt), FTYPE[fmt])
        return cache[(preset, fmt)]
    return get


@pytest.mark.parametrize("preset", ["toy", "mini"])
@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_on_a_quantised_file_is_plain_arithmetic_on_its_dequantised_twin(fmt, preset, request, quantized_model, quantised_evaluations, tmp_path):
    src = quantized_model(request.getfixturevalue(preset + "_model"), fmt)
    seen, ref = _twin_evaluations(src, tmp_path)
    assert set(seen) == {0, bf.TYPE_OF[fmt]}, seen           # the GPT sections: quantised matrices, f32 vectors
    got = quantised_evaluations(preset, fmt)
    r = _spread(got, ref)
    assert max(r.values()) <= TAU, r
    assert min(r.values()) > 0, r                            # the activations are rounded to q8 on the quantised file
    r = _spread(got, ref, rms=True)
    assert max(r.values()) <= TAU_RMS, r


@pytest.mark.parametrize("variant,fmt", WRONG, ids=[f"{v}-{f}" for v, f in WRONG])
def test_a_wrong_reading_of_the_format_misses_by_ten_times_the_tolerance(variant, fmt, toy_model, quantized_model, quantised_evaluations, tmp_path):
    _, ref = _twin_evaluations(quantized_model(toy_model, fmt), tmp_path, variant)
    r = _spread(quantised_evaluations("toy", fmt), ref)
    assert max(r.values()) >= 10 * TAU, r
