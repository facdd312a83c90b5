"""Rule C13r on a CPU: the committed tap table of the library is the f32 rounding of voice.py's formula, the length formula, the vectorised FMA step of
tests/resample_ref.py against the exact fma32 of tests/test_canon_orders.py, and the f32 reference against voice.resample_24k_to_16k within a derived bound."""
import ctypes as C

import numpy as np

import codec_encoder_ref as cref
import resample_ref as rr
from test_canon_orders import fma32


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def test_the_committed_taps_are_the_f32_roundings_of_voice_py_s_formula():
    lib = _pkg().load_library()
    got = np.full(44, np.nan, np.float32)
    assert lib.bark_hip_resample_taps(got.ctypes.data) == 44
    want = rr.taps().reshape(-1)
    assert got.tobytes() == want.tobytes() and np.count_nonzero(got) == 37      # all 44 entries, the signs of the zero taps included
    # the formula here is voice.py's: the two phases of resample_24k_to_16k, read back through unit impulses
    voice = _pkg().voice
    x = np.zeros(64, np.float32); x[30] = 1.0
    y = voice.resample_24k_to_16k(x)
    for m in range(14, 27):
        j = 30 - (3 * m) // 2
        if -10 <= j <= 11:
            assert y[m] == want.reshape(2, 22)[m & 1, j + 10], m
    assert lib.bark_hip_resample_taps(None) == -1


def test_length_formula():
    voice = _pkg().voice
    for n in range(1, 51):
        assert rr.n_out(n) == -(-2 * n // 3) == len(voice.resample_24k_to_16k(np.zeros(n, np.float32))) == len(rr.resample(np.zeros(n, np.float32)))


def _double_rounding_triples(n, rng):
    """a b = +-2^(e - 24) (1 - 2^-46) beside c = 2^e (odd significand): the exact sum lies just off a tie of f32, a float64 sum lands ON it"""
    e1, e2 = rng.integers(-20, 20, n), rng.integers(-20, 20, n)
    a = np.ldexp(np.float32(1.0) + np.float32(2.0 ** -23), e1).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], np.float32), n)
    b = np.ldexp(np.float32(1.0) - np.float32(2.0 ** -23), e2).astype(np.float32)
    k = 2 * rng.integers(0, 1 << 22, n) + 1
    c = np.ldexp((1.0 + k * 2.0 ** -23), e1 + e2 + 24).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], np.float32), n)
    return a, b, c


def test_vectorised_fma_is_fma32():
    rng = np.random.default_rng(7)
    n = 4000
    parts = [(rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)),
             (rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32) * np.float32(1e-3), rng.standard_normal(n).astype(np.float32) * np.float32(50.0)),
             _double_rounding_triples(n, rng)]
    a, b, c = (np.concatenate([p[i] for p in parts]) for i in range(3))
    a[:4], b[:4], c[:4] = [0.0, 1.0, -0.0, 0.5], [3.0, 0.0, 2.0, -2.0], [0.0, -0.0, 0.0, 1.0]
    got = rr.fma32_vec(a, b, c)
    want = np.array([fma32(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert len(a) >= 10000 and got.tobytes() == want.tobytes()
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)      # rounds twice
    assert int((naive != want).sum()) > 1000                 # the cases that tell the two apart are in the sample


def test_reference_is_within_the_derived_bound_of_voice_py():
    """Per output: 22 FMA roundings (each at most 2^-24 of a partial sum that never exceeds sum |h_j| |x_j|), the rounding of the taps (2^-24 |h_j| each: one
    more share of the same sum) and numpy's final cast (one more), with first-order slack for the float64 sum itself: 25 x 2^-24 x sum_j |h_j| |x_j|."""
    voice = _pkg().voice
    for x in (cref.fixture_signal(24000), np.random.default_rng(11).standard_normal(5000).astype(np.float32), cref.fixture_signal(23)):
        want = voice.resample_24k_to_16k(x)
        got = rr.resample(x)
        bound = 25.0 * 2.0 ** -24 * rr.abs_weight(x)
        dev = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(f"n={len(x)}: worst |f32 reference - voice.py| / bound = {float((dev / np.maximum(bound, 1e-300)).max()):.3f}")
        assert got.shape == want.shape and np.all(dev <= bound)
