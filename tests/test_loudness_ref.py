"""tests/loudness_ref.py (rule C17l) pinned without a GPU: the coefficient formulas against the ITU's 48 kHz table, a calibration tone,
the hop form against a one-chain K-weighting filter, gate cases worked out by hand, and the ceiling and the cap."""
import math

import numpy as np

import loudness_ref as lr


def _noise(n, amp, seed):
    return np.random.default_rng([17, seed]).uniform(-amp, amp, n).astype(np.float32)


def _composite():
    return np.concatenate([_noise(24000, 0.3, 2), _noise(24000, 0.003, 3), np.zeros(24000, np.float32)])


def test_formulas_give_the_itu_table_at_48_khz_and_the_committed_values_at_24():
    t = lr.ITU_48K
    want = np.array([*t["shelf_b"], *t["shelf_a"], *t["hp_a"]])
    assert np.abs(lr.formulas(48000.0) - want).max() <= 1e-12
    k = lr.constants()
    assert np.allclose(k[:7], [1.4879002209622763, -2.2462054681411368, 0.904909123246438, -1.3902346051928203, 0.5368384812603979, -1.9801441262289323, 0.9802428178592764],
                       rtol=4e-16, atol=0.0)
    assert abs(k[7] / 10.0 ** -6.9309 - 1.0) <= 1e-14 and k[8] == 9600.0 * k[7]
    assert lr.target_ms(-2300) == 10.0 ** ((-23.0 + 0.691) / 10.0) and abs(lr.lufs_of(lr.target_ms(-1600)) + 16.0) < 1e-12


def test_a_997_hz_sine_of_amplitude_a_tenth_reads_minus_23():
    """BS.1770's calibration: a full-scale 997 Hz sine reads -3.01 LKFS, so amplitude 0.1 reads -23.01; at 24 kHz the prototypes give -22.984"""
    x = (0.1 * np.sin(2.0 * np.pi * 997.0 * np.arange(72000) / 24000.0)).astype(np.float32)
    m = lr.measure(x)
    assert abs(m["lufs"] + 23.01) <= 0.1 and abs(m["lufs"] + 22.984) <= 1e-3
    assert (m["n_blocks"], m["n_abs"], m["n_gated"], m["flags"]) == (27, 27, 27, 0)


def _one_chain(x, k):
    """the same gates over ONE K-weighting filter run from the first sample to the last (scipy.signal.lfilter in f64)"""
    try:
        from scipy.signal import lfilter
    except ImportError:                                                     # the same transposed direct form II, sample by sample
        def lfilter(b, a, x):
            out, s1, s2 = np.zeros(len(x)), 0.0, 0.0
            for i, v in enumerate(x.tolist()):
                o = b[0] * v + s1
                s1 = b[1] * v - a[1] * o + s2
                s2 = b[2] * v - a[2] * o
                out[i] = o
            return out
    y = lfilter(k[0:3], [1.0, k[3], k[4]], np.asarray(x, np.float32).astype(np.float64))
    y = lfilter([1.0, -2.0, 1.0], [1.0, k[5], k[6]], y)
    Hn = len(x) // lr.HOP
    return lr.gates((y[:Hn * lr.HOP] ** 2).reshape(Hn, lr.HOP).sum(axis=1), k)


def test_the_hop_form_agrees_with_a_one_chain_filter():
    """Measured: the integrated loudness of the hop form (runs of 7200 samples from zero state, the first 4800 outputs discarded) differs from the one-chain
    filter's by 3.6e-15 dB on 3 s of seeded noise of amplitude 0.1 and by 5.3e-15 dB on the loud / quiet / silent composite (8.3e-16 of the mean square):
    the filters' own f64 rounding, the impulse response beyond 4800 samples sums to 4.4e-20.  Bound: a thousand times the larger figure."""
    k = lr.constants()
    for x in (_noise(72000, 0.1, 3), _composite()):
        a, (M, J, c1, c2) = lr.measure(x), _one_chain(x, k)
        assert (a["n_blocks"], a["n_abs"], a["n_gated"]) == (J, c1, c2)
        assert abs(a["lufs"] - lr.lufs_of(M)) <= 5.4e-12


def test_gate_cases_worked_out_by_hand():
    k = lr.constants()
    # silence: every hop sums to +0, both blocks fail the absolute gate
    s = lr.measure(np.zeros(12000, np.float32))
    assert not s["z"].any() and (s["n_blocks"], s["n_abs"], s["n_gated"], s["flags"]) == (2, 0, 0, lr.UNMEASURABLE) and s["mean_square"] == 0.0 and s["lufs"] == -math.inf
    y, info = lr.level(np.zeros(12000, np.float32), lr.target_ms(-1600))
    assert info["gain"] == 1.0 and not y.any()
    # amplitude 1e-4: a mean square near 3.3e-9 (-85 LUFS) against the gate's 1.17e-7 (-70 LUFS): measured hops, no block passes
    x = _noise(14400, 1e-4, 1)
    u = lr.measure(x)
    assert u["z"].all() and (u["z"] * 4 < k[8]).all() and (u["n_blocks"], u["n_abs"], u["n_gated"], u["flags"]) == (3, 0, 0, lr.UNMEASURABLE)
    y, info = lr.level(x, lr.target_ms(-1600))
    assert info["gain"] == 1.0 and y.tobytes() == x.tobytes()
    # under 4 hops there is no block at all
    assert lr.gates(np.ones(3), k) == (0.0, 0, 0, 0)
    # a z table in binary fractions: S = 16, 12.0625, 8.125, 4.1875, 0.25, all over the absolute gate; sum1 = 40.625, a tenth of it is 4.0625 against
    # S c1 = 80, 60.3125, 40.625, 20.9375, 1.25: the last block falls to the relative gate; sum2 = 40.375
    M, J, c1, c2 = lr.gates(np.array([4.0, 4.0, 4.0, 4.0, 0.0625, 0.0625, 0.0625, 0.0625]), k)
    assert (J, c1, c2) == (5, 5, 4) and M == 40.375 / 38400.0
    # the comparisons are strict: a block AT the absolute gate fails, a block AT a tenth of the mean fails
    g = k[8]
    assert lr.gates(np.array([g, 0.0, 0.0, 0.0]), k) == (0.0, 1, 0, 0)
    M, J, c1, c2 = lr.gates(np.array([19.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), k)       # S = 19, 1, 1, 1, 1: c1 = 5, sum1 = 23 - every block over 0.46
    assert (J, c1, c2) == (5, 5, 5) and M == 23.0 / 48000.0
    # the signal of the GPU tests: loud, 40 dB quieter, silent
    c = lr.measure(_composite())
    assert 0 < c["n_gated"] < c["n_abs"] < c["n_blocks"] == 27 and c["flags"] == 0


def test_ceiling_and_cap_bind():
    tms = lr.target_ms(-1600)
    x = _noise(12000, 0.01, 4)
    free = lr.level(x, tms, 0.0, 0.0)[1]
    assert free["flags"] == 0 and free["gain"] == np.float32(np.sqrt(np.float64(tms) / np.float64(free["mean_square"]))) and free["gain"] > 10.0
    capped = lr.level(x, tms, 0.0, 10.0)[1]
    assert capped["flags"] == lr.CAP_BOUND and capped["gain"] == 10.0
    x[7000] = -0.9
    y, spike = lr.level(x, tms, 1.0, 10.0)
    assert spike["flags"] == lr.CEILING_BOUND and spike["peak"] == np.float32(0.9) and spike["gain"] == np.float32(1.0 / np.float64(np.float32(0.9)))
    assert np.abs(y).max() <= 1.0 and y.tobytes() == (x * spike["gain"]).tobytes()
    half = lr.level(x, tms, 0.5, 10.0)[1]
    assert half["gain"] == np.float32(np.float64(0.5) / np.float64(np.float32(0.9)))
    loud = lr.level(_noise(12000, 0.5, 6), lr.target_ms(-3000), 1.0, 10.0)[1]          # a gain under 1: neither binds
    assert loud["flags"] == 0 and loud["gain"] < 1.0
    ys = lr.level_many([x, x], [tms, 0], 1.0, 10.0)
    assert ys[0][0].tobytes() == y.tobytes() and ys[1][0].tobytes() == x.tobytes() and ys[1][1]["gain"] == 1.0
