"""tests/output_format_ref.py (rule C14r and the sample formats) held to three checks that need no device: at 24000 -> 16000 it is rule
C13r's restatement bit for bit; for every pair the f32 chain stays within its derived rounding bound of the float64 sum; and every pair resamples a tone to
the tone.  The formats are held to G.711's known values and to rint's ties."""
import numpy as np
import pytest

import output_format_ref as ofr
import resample_ref as rr

PAIR_IDS = [f"{a}-{b}" for a, b in ofr.PAIRS]


def tone(n, rate, freq=1000.0, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(n, dtype=np.float64) / rate)).astype(np.float32)


def test_there_are_14_pairs_and_the_largest_tables_are_the_stated_ones():
    assert len(ofr.PAIRS) == 14 and all(ofr.supported(a, b) for a, b in ofr.PAIRS)
    assert not ofr.supported(11025, 24000) and not ofr.supported(16000, 48000) and ofr.supported(24000, 24000)
    shape = {p: ofr.taps(*p).shape for p in ofr.PAIRS}
    assert shape[(22050, 24000)] == (160, 16) and shape[(24000, 44100)] == (147, 16) and shape[(44100, 24000)] == (80, 26) and shape[(24000, 8000)] == (1, 40)
    assert max(s[1] for s in shape.values()) == 40 and sum(s[0] * s[1] for s in shape.values()) == 9768


def test_at_24000_to_16000_the_rule_is_c13r_bit_for_bit():
    assert ofr.lmh(24000, 16000) == (2, 3, rr.HALF)
    h = ofr.taps(24000, 16000)
    assert h.shape == (2, rr.N_TAPS) and np.array_equal(h, rr.taps())                        # == on floats: equal apart from the sign of a zero
    nz = h != 0.0
    assert h[nz].tobytes() == rr.taps()[nz].tobytes()
    for x in (rr.dense_signal(5000), np.random.default_rng(5).standard_normal(2311).astype(np.float32), rr.dense_signal(1), rr.dense_signal(23)):
        assert ofr.n_out(len(x), 24000, 16000) == rr.n_out(len(x))
        assert ofr.resample(x, 24000, 16000).tobytes() == rr.resample(x).tobytes()
        assert ofr.resample(x, 24000, 16000, h=rr.taps()).tobytes() == rr.resample(x).tobytes()


@pytest.mark.parametrize("pair", ofr.PAIRS, ids=PAIR_IDS)
def test_chain_is_within_the_derived_bound_of_the_float64_sum(pair):
    """Per output: n_taps FMA roundings (each at most 2^-24 of a partial sum that never exceeds sum |h_j| |x_j|), the rounding of the taps (one more share of
    the same sum) and first-order slack for the float64 sum and the final cast: (n_taps + 3) x 2^-24 x sum_j |h_j| |x_j| (tests/test_resample_ref.py's form)."""
    n_taps = 2 * ofr.lmh(*pair)[2]
    for x in (tone(3000, pair[0]), rr.dense_signal(3000), np.random.default_rng(11).standard_normal(2000).astype(np.float32)):
        got = ofr.resample(x, *pair)
        want, weight = ofr.exact(x, *pair)
        bound = (n_taps + 3) * 2.0 ** -24 * weight
        dev = np.abs(got.astype(np.float64) - want)
        print(f"{pair}: worst |chain - float64 sum| / bound = {float((dev / np.maximum(bound, 1e-300)).max()):.3f}")
        assert got.shape == want.shape == (ofr.n_out(len(x), *pair),) and np.all(dev <= bound)


@pytest.mark.parametrize("pair", ofr.PAIRS, ids=PAIR_IDS)
def test_a_1_khz_tone_stays_the_tone(pair):
    """Away from the edges - 4 HALF (floor(L / M) + 1) outputs at each end: HALF input samples of filter reach in output samples, four times over for the
    window's tail - the resampled tone lies within 1e-3 of the ideal one."""
    L, M, half = ofr.lmh(*pair)
    x = tone(pair[0] // 5, pair[0])
    y = ofr.resample(x, *pair).astype(np.float64)
    ideal = 0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(len(y), dtype=np.float64) / pair[1])
    edge = 4 * half * (L // M + 1)
    assert len(y) > 4 * edge
    err = float(np.abs(y - ideal)[edge:len(y) - edge].max())
    print(f"{pair}: worst |resampled - ideal| = {err:.2e}")
    assert err <= 1e-3


def test_identity_and_lengths():
    x = rr.dense_signal(777)
    assert ofr.resample(x, 24000, 24000).tobytes() == x.tobytes() and ofr.n_out(777, 24000, 24000) == 777
    for a, b in ofr.PAIRS:
        for n in (1, 2, 3, 1000, ofr.MAX_SAMPLES):
            assert ofr.n_out(n, a, b) == -((-n * b) // a)                                  # ceil(n rate_out / rate_in)


def test_s16_rounds_ties_to_even_and_saturates():
    lsb = np.float32(1.0 / 32768.0)
    y = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.0, 32766.5, 32767.0, 32767.5, 40000.0, -32768.0, -32768.5, -61000.0], np.float32) * lsb
    assert ofr.to_s16(y).tolist() == [0, 2, 2, 0, -2, -2, 0, 32766, 32767, 32767, 32767, -32768, -32768, -32768]
    assert ofr.to_s16(np.array([1.0, -1.0, 1.87, -1.87], np.float32)).tolist() == [32767, -32768, 32767, -32768]


def test_mulaw_known_values_and_all_65536():
    assert ofr.mulaw_of_s16(np.array([0, -1, 32767, -32768], np.int16)).tolist() == [0xFF, 0x7F, 0x80, 0x00]
    s = np.arange(-32768, 32768).astype(np.int16)
    b = ofr.mulaw_of_s16(s).astype(np.int64)
    # G.711 decode of every byte lands within the segment's step of the clipped value, and the code is monotonic in s on either side of zero
    u = ~b & 0xFF
    e, man = (u >> 4) & 7, u & 15
    dec = np.where(u & 0x80, -1, 1) * ((((man << 3) + 132) << e) - 132)
    clipped = np.clip(s.astype(np.int64), -32635, 32635)
    assert np.all(np.abs(dec - clipped) <= (1 << (e + 3)))
    pos, neg = b[s >= 0], b[s < 0][::-1]
    assert np.all(np.diff(pos) <= 0) and np.all(np.diff(neg) <= 0) and len(set(b.tolist())) == 256
    assert ofr.to_format(np.array([0.25], np.float32), ofr.MULAW).tolist() == ofr.mulaw_of_s16(np.array([8192], np.int16)).tolist()
