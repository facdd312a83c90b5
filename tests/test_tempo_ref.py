"""Rule C16t on the CPU: the committed window against its formula, the length formula, and what the restated rule
(tests/tempo_ref.py, run with the library's own table) does to silence and to a two-tone signal - the search stays within its radius, moves nearly every
frame of a tonal signal, and the result keeps the tones where they were."""
import os

import numpy as np
import pytest

import tempo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from bark_amd_loader import load_package
    return load_package().load_library()


@pytest.fixture(scope="module")
def window():
    w = np.zeros(tr.W, np.float32)
    assert _lib().bark_hip_tempo_window(w.ctypes.data) == tr.W
    return w


def test_committed_window_is_the_double_formula_rounded_once(window):
    assert window.view(np.uint32).tolist() == tr.window().view(np.uint32).tolist()
    assert window[0] == 0.0 and window[360] == 1.0 and window[180] == 0.5
    s = window[:tr.HS].astype(np.float64) + window[tr.HS:].astype(np.float64)               # exact in double
    assert np.abs(s - 1.0).max() <= 2.0 ** -24                                             # within one f32 rounding of 1
    text = open(os.path.join(ROOT, "bark.cpp_amd", "csrc", "codec_kernels.hip")).read()
    assert "static const float kTempoWindow[kTempoFrame] = {" in text and "cosf(" not in text.split("kTempoWindow[kTempoFrame]")[1]


@pytest.mark.parametrize("p", [500, 999, 1001, 2000])
def test_length_formula(p, window):
    lib = _lib()
    for n in (1, 2, 359, 360, 361, 719, 720, 721, 1081):
        want = -((-1000 * n) // p)                                                         # ceil(1000 n / p)
        assert tr.out_len(n, p) == want == lib.bark_hip_tempo_out_len(n, p)
        y, pos = tr.tempo(np.full(n, 0.5, np.float32), p, window, want_pos=True)
        assert len(y) == want and len(pos) == -(-want // tr.HS) and np.isfinite(y).all() and pos[0] == 0


def test_silence_keeps_every_frame_nominal(window):
    for p in (500, 750, 1250, 2000):
        y, pos = tr.tempo(np.zeros(3000, np.float32), p, window, want_pos=True)
        assert pos.tolist() == [tr.nominal(k, p) for k in range(len(pos))] and not y.any()


def test_identity_is_the_samples_themselves(window):
    x = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    y, pos = tr.tempo(x, 1000, window, want_pos=True)
    assert y.tobytes() == x.tobytes() and pos.tolist() == [0, 360, 720]


def test_scan_order_and_ties():
    d = (tr.SCAN - tr.D).tolist()
    assert d[:5] == [0, -1, 1, -2, 2] and d[-2:] == [-tr.D, tr.D] and sorted(d) == list(range(-tr.D, tr.D + 1))


def two_tones(n=12000):
    t = np.arange(n) / 24000.0
    return (0.5 * np.sin(2 * np.pi * 200.0 * t) + 0.3 * np.sin(2 * np.pi * 1310.0 * t)).astype(np.float32)


@pytest.mark.parametrize("p", [500, 750, 1250, 2000])
def test_two_tones_keep_their_pitch(p, window):
    x = two_tones()
    y, pos = tr.tempo(x, p, window, want_pos=True)
    nom = np.array([tr.nominal(k, p) for k in range(len(pos))])
    assert np.abs(pos - nom).max() <= tr.D                                                 # a position never leaves a +- 240
    assert np.count_nonzero(pos != nom) >= len(pos) // 2                                   # the search works: most frames move off the nominal position
    z = y[tr.W:len(y) - 2 * tr.W].astype(np.float64)                                       # the interior: away from the first frame and the recording's end
    spec = np.abs(np.fft.rfft(z * np.hanning(len(z)))) ** 2
    f = np.fft.rfftfreq(len(z), 1.0 / 24000.0)
    near = (np.abs(f - 200.0) <= 40.0) | (np.abs(f - 1310.0) <= 40.0)
    share = spec[~near].sum() / spec.sum()
    print(f"p={p}: energy outside the tones {share:.3g}, peak at {f[np.argmax(spec)]:.1f} Hz")
    assert share <= 1e-3
    # the peak lies in the 200 Hz tone's bin: inside the Hann analysis window's main lobe around 200 Hz, two bins (about 1 Hz each here) either way -
    # a frame that moved shifts the tone's phase, which can move the maximum of the lobe by a bin, never the tone out of it
    assert abs(f[np.argmax(spec)] - 200.0) <= 2.0 * (f[1] - f[0])
