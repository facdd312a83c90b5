"""Top-k / nucleus sampling (rule C8n) without a GPU: the Python restatement (tests/nucleus_ref.py) on hand-built cases, the
engine's filter + sampler launches (bark_hip_sample_rows_filtered) on the host-emulated engine (tests/simt/build_engine.py) against it, and the HTTP
server's parsing of the new request fields."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nucleus_ref as R  # noqa: E402

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _f32_below(x: Fraction) -> float:
    """the largest float32 < x (0 < x <= 1)"""
    f = np.float32(float(x))
    while Fraction(float(f)) >= x:
        f = np.nextafter(f, np.float32(0))
    return float(f)


def _f32_at_or_above(x: Fraction) -> float:
    f = np.float32(float(x))
    while Fraction(float(f)) < x:
        f = np.nextafter(f, np.float32(2))
    return float(f)


def test_top_k_1_keeps_the_argmax():
    l = np.array([0.5, 2.0, -1.0, 1.9, 2.0 - 2 ** -20], np.float32)
    assert np.flatnonzero(R.keep_mask(l, 1, 1.0)).tolist() == [1]
    for u in (1e-300, 0.3, 0.999999):
        assert R.sample(l, 0.7, 1, 1.0, u) == (1, 0.0)         # the last id went: eos_p is exactly 0
    assert R.sample(l, 0.7, 1, 1.0, 0.0)[0] == 0                 # libstdc++'s quirk, kept: u == 0 is lower_bound's first running sum (0)


def test_top_k_keeps_ties_with_the_kth_logit():
    l = np.array([3.0, 1.0, 2.0, 1.0, 0.0, 1.0], np.float32)
    assert np.flatnonzero(R.keep_mask(l, 3, 1.0)).tolist() == [0, 1, 2, 3, 5]
    assert R.keep_mask(l, 7, 1.0).all() and R.keep_mask(l, 6, 1.0).all()       # top_k >= n keeps everything


def test_nucleus_cut_inside_a_tie_group_goes_by_ascending_id():
    l = np.array([-3.0, 1.0, -9.0, 1.0, 1.0, 1.0], np.float32)       # four equal weights 2^40 at ids 1, 3, 4, 5
    w = R.weights(l)
    S = sum(w)
    assert w[1] == 2 ** 40
    # 1.5 weights of the group fit: the first two ids of the group (1, 3) stay; id 4's prefix (2 * 2^40) is above top_p * S
    top_p = _f32_at_or_above(Fraction(3, 2) * 2 ** 40 / S)
    assert np.flatnonzero(R.keep_mask(l, 0, top_p)).tolist() == [1, 3]
    # -0.0 and +0.0 are one logit value: a tie, split by id
    z = np.array([-0.0, 0.0, -0.0, -50.0], np.float32)
    assert np.flatnonzero(R.keep_mask(z, 0, 0.4)).tolist() == [0, 1]


def test_top_p_just_below_and_at_a_cumulative_weight():
    l = np.array([-1.0, 0.0, -2.0, -0.5], np.float32)
    w = R.weights(l)
    S = sum(w)
    pi = R.order(l).tolist()
    assert pi == [1, 3, 0, 2]
    edge = Fraction(w[1] + w[3], S)                               # the prefix in front of pi(2) = id 0
    assert np.flatnonzero(R.keep_mask(l, 0, _f32_below(edge))).tolist() == [1, 3]
    assert np.flatnonzero(R.keep_mask(l, 0, _f32_at_or_above(edge))).tolist() == [0, 1, 3]
    # a tiny top_p keeps the first id of pi only - also when it ties with the second
    assert np.flatnonzero(R.keep_mask(l, 0, 1e-30)).tolist() == [1]
    assert np.flatnonzero(R.keep_mask(np.array([1.0, 2.0, 2.0], np.float32), 0, 2 ** -40)).tolist() == [1]


def test_top_p_then_top_k_order():
    l = np.array([0.0, -0.1, -0.2, -5.0, -6.0], np.float32)
    # nucleus keeps ids 0..2 (+ the crossing one), then top_k = 2 cuts to the two largest survivors
    assert np.flatnonzero(R.keep_mask(l, 0, 0.7)).tolist() == [0, 1, 2]
    assert np.flatnonzero(R.keep_mask(l, 2, 0.7)).tolist() == [0, 1]
    assert np.flatnonzero(R.keep_mask(l, 4, 0.5)).tolist() == [0, 1]          # fewer survivors than top_k: nothing more goes


def test_filter_off_is_the_plain_multinomial():
    rng = np.random.default_rng(5)
    for _ in range(20):
        l = rng.standard_normal(300).astype(np.float32)
        u = rng.random()
        assert R.sample(l, 0.7, 0, 1.0, u) == R.multinomial(l, 0.7, u)
        assert R.keep_mask(l, 0, 1.0).all()


def test_mt19937_restatement_matches_the_standard_sequence():
    g = R.MT19937(5489)
    words = [g.word() for _ in range(10000)]
    assert words[0] == 3499211612 and words[-1] == 4123659995             # the C++ standard's check value: the 10000th word of mt19937()


def _rows(rng, count, n_choices):
    """random and adversarial rows: (logits, temp, top_k, top_p, u)"""
    out = []
    for r in range(count):
        n = int(rng.choice(n_choices))
        kind = r % 6
        if kind == 0:
            l = rng.standard_normal(n) * 4.0                            # peaked
        elif kind == 1:
            l = rng.standard_normal(n) * 0.01                           # flat
        elif kind == 2:
            l = np.round(rng.standard_normal(n) * 2.0) / 2.0            # wide tie groups
        elif kind == 3:
            l = np.full(n, 0.25); l[rng.integers(0, n, 3)] = 1.0       # everything tied but three ids
        elif kind == 4:
            l = rng.standard_normal(n) * 30.0                           # most weights are exactly 0
        else:
            l = rng.standard_normal(n); l[rng.integers(0, n, n // 4)] *= -0.0
        l = l.astype(np.float32)
        temp = float(rng.choice([0.7, 1.0, 0.3]))
        top_k = int(rng.choice([0, 0, 1, 2, 50, 1000, n, n + 5]))
        top_p = float(np.float32(rng.choice([1.0, 0.5, 0.9, 0.99, 1e-6, rng.random()])))
        if top_k == 0 and top_p == 1.0:
            top_p = 0.9
        u = float(rng.random())
        if r % 3 == 0:                                                  # u within 1e-9 of a bin edge of the filtered draw
            cp = R.bin_edges(l, temp, top_k, top_p)
            nz = np.flatnonzero(np.diff(np.concatenate([[0.0], cp])) > 0)
            j = int(rng.choice(nz))
            u = float(np.clip(cp[j] + rng.choice([-1e-9, 0.0, 1e-9, -1e-12]), 0.0, np.nextafter(1.0, 0.0)))
        out.append((l, temp, top_k, top_p, u))
    return out


def check_rows(ctx, rows, chunk=512):
    """ids bit-equal.  eos_p: exactly 0 where the last id was removed; bit-equal where u lies next to an end of its bin (the sampler's exact path:
    sequential sums); elsewhere C8's fast-path value - e_last over a TREE sum of the exponentials where the restatement sums in index order
    (sample_multinomial_kernel's eos_p, as for unfiltered rows) - within n 2^-23 relative.  Returns (mismatches, rows whose eos_p was held to the bit)."""
    bad = []
    n_bits = 0
    for c0 in range(0, len(rows), chunk):
        part = rows[c0:c0 + chunk]
        for n in sorted({r[0].size for r in part}):
            sel = [r for r in part if r[0].size == n]
            ids, eos = ctx.sample_rows_filtered(np.stack([r[0] for r in sel]), [r[1] for r in sel], [r[2] for r in sel], [r[3] for r in sel], [r[4] for r in sel])
            for (l, temp, k, p, u), i, e in zip(sel, ids, eos):
                ri, re = R.sample(l, temp, k, p, u)
                bits = re == 0.0 or R.exact_path_forced(l, temp, k, p, u)
                n_bits += bits and re != 0.0
                ok = i == ri and (e == re if bits else abs(e - re) <= n * 2.0 ** -23 * re)
                if not ok:
                    bad.append((n, temp, k, p, u, ri, re, int(i), float(e)))
    return bad, n_bits


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_nucleus")))


# runs in a child process: the library a process loads first is the one it keeps (bark_amd_loader caches it)
_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from bark_amd_loader import load_package
from tools.make_synth_model import ensure_model
import test_nucleus_sampling_host as H
pkg = load_package()
ctx = pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(temp=0.7), seed=0)
rng = np.random.default_rng(2024)
rows = H._rows(rng, 1900, [1024, 1024, 1024, 333]) + H._rows(rng, 100, [10048])
bad, n_bits = H.check_rows(ctx, rows)
print("BAD", len(bad), bad[:3])
print("EOS_BITS", n_bits)
l = np.zeros((1, 16), np.float32)
rej = 0
for k, p in ((-1, 0.5), (0, 0.0), (0, 1.5), (0, float("nan"))):
    try:
        ctx.sample_rows_filtered(l, [0.7], [k], [p], [0.5])
    except RuntimeError:
        rej += 1
for k, p in ((-1, 1.0), (0, 0.0), (0, -0.1), (0, 1.0001), (3, float("nan"))):
    try:
        ctx.set_sampling_filter(k, p)
    except ValueError:
        rej += 1
ctx.set_sampling_filter(50, 0.9)
ctx.set_sampling_filter(0, 1.0)
print("REJECTED", rej)
ctx.free()
"""


def test_emulated_filter_kernel_matches_the_restatement(sim_engine):
    """2 000 rows (n = 1024 and 10 048, random and adversarial, a third of them with u within 1e-9 of a bin edge) through the engine's own
    filter + sampler kernels, run work-item for work-item on the host; bad settings are refused at the C ABI"""
    env = dict(os.environ, BARK_HIP_LIBRARY=sim_engine)
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "BAD 0 []" in r.stdout, r.stdout[-3000:]
    n_bits = int(r.stdout.split("EOS_BITS ")[1].split()[0])
    assert n_bits >= 40, r.stdout[-3000:]                              # adversarial draws with eos_p > 0: held to the bit on the exact path
    assert "REJECTED 9" in r.stdout, r.stdout[-3000:]


def test_server_parses_top_k_and_top_p(tmp_path):
    exe = str(tmp_path / "http_filter_driver")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "bark.cpp_amd", "examples"),
                        os.path.join(ROOT, "tests", "http_filter_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(body):
        kv = dict(l.split("=", 1) for l in subprocess.run([exe, body], capture_output=True, text=True, check=True).stdout.splitlines())
        sk, vk = kv["top_k"].split(","); sp, vp = kv["top_p"].split(",")
        return (int(sk), int(vk)), (int(sp), float.fromhex(vp))

    assert run('{"text": "a", "top_k": 50, "top_p": 0.9}') == ((1, 50), (1, float(np.float32(0.9))))
    assert run('{"text": "a"}') == ((0, 0), (0, 1.0))
    assert run('{"top_p":1}')[1] == (1, 1.0) and run('{"top_k": 0}')[0] == (1, 0)
    assert run('{"top_k": -3}')[0] == (1, -3)                          # parsed; the server's range check answers 400
    assert run('{"top_k": 1.5}')[0][0] == -1 and run('{"top_k": "7"}')[0][0] == -1 and run('{"top_k": 1e12}')[0][0] == -1
    assert run('{"top_p": "0.5"}')[1][0] == -1 and run('{"top_p": nan}')[1][0] == -1 and run('{"top_p": }')[1][0] == -1
    assert run('{"top_p": 1e-3}')[1] == (1, float(np.float32(1e-3)))
    # the server's own checks: an invalid value is a 400 (batch_server.cpp)
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    assert 'json_int(body, "top_k"' in src and 'json_float(body, "top_p"' in src and "bark_hip_batcher_submit_filtered" in src
