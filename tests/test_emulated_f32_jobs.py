"""Lock-step jobs on f32 model files, without a GPU (host emulation of tests/simt: work-items as fibers, DPP / readlane as wave-wide rendezvous).

1. Kernel level, in the style of tests/test_simt_emulation.py: gemv_w32_slots_kernel - the f32 product of all live slots, every weight chunk read once per
   group of eight slots - through the product's own dispatch (launch_linear_w32 with a.batched) against gemv_w32_kernel slot after slot, bit for bit:
   K in {128, 768, 2048, 3072, 4096} (one and two K tiles in LDS; K = 4096 has no GPU test - an f32 bark-large file is 4.5 GB - so this case and the
   static LDS bound are its cover), 1 .. 64 slots (partial slot groups), M not a multiple of 16, with and without LayerNorm / LayerNorm bias / bias,
   the residual epilogue, and the coarse LM head's row selection by every slot's OWN step parity with mixed parities inside a group.
2. Engine level: a ragged toy job (3 utterances, then 2 more on the same context; greedy and sampled, a top-k / top-p filter, a voice prompt) on the
   WHOLE engine compiled for the host (tests/simt/build_engine.py) against the live oracle on the same f32 file, and the route it took
   (bark_hip_batch_lock_steps)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.environ.get("BARK_SIM_CSRC", os.path.join(ROOT, "bark.cpp_amd", "csrc"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    d = str(tmp_path_factory.mktemp("simt_w32"))
    for name in ("kernels.h", "quant_formats.h", "device_utils.h"):
        open(os.path.join(d, name), "w").write(build_engine.patch(open(os.path.join(CSRC, name)).read()))
    text = open(os.path.join(CSRC, "quant_kernels.hip")).read()
    assert re.search(r"void gemv_w32_slots_kernel\(", text), "the slot form of the f32 decode product is missing from quant_kernels.hip"
    open(os.path.join(d, "quant_kernels_sim.hip"), "w").write(build_engine.patch(text))      # the kernel source unchanged but for the generic host patches
    so = os.path.join(d, "libsim_w32.so")
    cmd = [CLANG, "-x", "c++", "-std=c++20", "-O1", "-mfma", "-mf16c", "-mavx2", "-ffp-contract=off", "-pthread", "-shared", "-fPIC", "-Wno-everything",
           "-I", os.path.join(ROOT, "tests", "simt"), "-I", d, os.path.join(ROOT, "tests", "simt", "sim_driver_w32.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    assert lib.sim_w32_state_size() == 32
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run(sim, route, W, x, g, b_ln, bias, out, st, K, M, B, parity_rows, epi, ld):
    return sim.sim_w32(route, _p(W), _p(x), _p(g), _p(b_ln), _p(bias), _p(out), _p(st), K, M, B, parity_rows, epi, ld)


M_ROWS = 37             # three row blocks of 16, the last one with 5 live rows


@pytest.mark.parametrize("K", [128, 768, 2048, 3072, 4096])
def test_f32_slot_product_equals_the_single_utterance_kernel(sim, K):
    rng = np.random.default_rng(K)
    M = M_ROWS
    W = (rng.standard_normal((2 * M, K)) * 0.05).astype(np.float32)            # two parity windows of M rows
    bias = (0.1 * rng.standard_normal(2 * M)).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    b_ln = (0.1 * rng.standard_normal(K)).astype(np.float32)
    fuses_ln = K <= 2048                                                       # one K tile in LDS: the whole LayerNorm-ed rows wait there
    for B in (1, 2, 7, 8, 9, 17, 64):
        x = (rng.standard_normal((B, K)) * (1 + rng.random((B, 1)))).astype(np.float32) + np.float32(0.3)
        st = np.zeros((B, 8), np.int32)                                        # StepState: n_past, cur_token, step, ...
        st[:, 2] = (np.arange(B) * 5 + (np.arange(B) // 3)) % 7                # mixed step parities inside every slot group
        assert B == 1 or len(set(st[:min(B, 8), 2] & 1)) == 2
        # (LayerNorm gain, LayerNorm bias, bias, parity_rows, epilogue): LM head shapes with and without parity, products without LayerNorm with the residual
        cases = [(None, None, bias, 0, 1), (None, None, None, 0, 3), (None, None, bias, M, 3)]
        if fuses_ln:
            cases += [(g, b_ln, bias, 0, 3), (g, None, None, 0, 3), (g, b_ln, bias, M, 3), (g, b_ln, bias, 0, 1)]
        for ln_g, ln_b, bs, par, epi in cases:
            # what the output holds before the launch: random logits rows with three columns of margin, or the residual rows
            first = rng.standard_normal((B, M + 3)).astype(np.float32) if epi == 3 else x[:, :M].copy() * np.float32(0.5)
            outs = []
            for route in (0, 1):
                out = first.copy()
                assert _run(sim, route, W, x, ln_g, ln_b, bs, out, st, K, M, B, par, epi, M + 3 if epi == 3 else M) == 0
                outs.append(out)
            tag = f"K={K} B={B} ln={ln_g is not None}/{ln_b is not None} bias={bs is not None} parity_rows={par} epi={epi}"
            assert outs[0].tobytes() == outs[1].tobytes(), tag + ": the slot product differs from gemv_w32_kernel slot by slot"
            assert (outs[0][:, :M] != first[:, :M]).all(), tag + ": outputs not written"
            if epi == 3:
                assert outs[0][:, M:].tobytes() == first[:, M:].tobytes(), tag + ": wrote beyond row M"
            if par and B > 1:
                # slots at odd steps took the second row window: their result differs from what the first window gives
                even = np.zeros_like(st); out0 = first.copy()
                assert _run(sim, 0, W, x, ln_g, ln_b, bs, out0, even, K, M, B, par, epi, M + 3) == 0
                odd = (st[:, 2] & 1) == 1
                assert (out0[~odd] == outs[0][~odd]).all() and (out0[odd][:, :M] != outs[0][odd][:, :M]).any(), tag
        if not fuses_ln:
            # the LayerNorm-fused form exists for n_embd <= 2048: the dispatch refuses, it does not fall back
            out = np.zeros((B, M), np.float32)
            assert _run(sim, 0, W, x, g, b_ln, bias, out, st, K, M, B, 0, 3, M) == -1
    # shapes the f32 products do not take at all
    out = np.zeros((2, M), np.float32)
    assert _run(sim, 0, W, np.zeros((2, 8192), np.float32), None, None, None, out, np.zeros((2, 8), np.int32), 8192, M, 2, 0, 3, M) == -1
    assert _run(sim, 0, W, np.zeros((2, 192), np.float32), None, None, None, out, np.zeros((2, 8), np.int32), 192, M, 2, 0, 3, M) == -1


# ---- the whole engine on the host: a ragged f32 job against the live oracle ----------------------------------------------------------------------------
_JOB_CHILD = r"""
import sys
root, path = sys.argv[1:3]
sys.path.insert(0, root)
import numpy as np
from bark_amd_loader import load_package
from oracle.pyoracle import Oracle
from tests import voice_prompt_ref as R
from tests.f32_jobs_ref import job_plan, job_reference, check_utterance
pkg = load_package()
orc = Oracle(path, n_threads=8)
ctx = pkg.BarkContext.load_model(path, pkg.default_params(), seed=3)
assert ctx.batch_lock_steps() is None
ctx.reserve_batch(8)
texts, reqs, flts, voices = job_plan(ctx, 5, max_cap=6)
pv = [None if v is None else pkg.VoicePrompt(v.semantic, v.coarse, v.fine) for v in voices]
for lo, hi in ((0, 3), (3, 5)):
    res = ctx.generate_batch(texts[lo:hi], params=reqs[lo:hi], filters=flts[lo:hi], voices=pv[lo:hi])
    steps = ctx.batch_lock_steps()
    assert steps is not None and steps[0] > 0 and steps[1] > 0, steps
    for i in range(lo, hi):
        check_utterance(f"emulated f32 job, utterance {i}", res[i - lo], job_reference(orc, texts[i], reqs[i], flts[i], voices[i]))
print("F32_JOB_SIM_OK")
ctx.free(); orc.close()
"""


def test_f32_job_on_the_host_emulated_engine_equals_the_oracle(tmp_path_factory, toy_f32_model):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    so = build_engine.build(str(tmp_path_factory.mktemp("sim_engine_f32")))
    env = dict(os.environ, BARK_HIP_LIBRARY=so)
    r = subprocess.run([sys.executable, "-c", _JOB_CHILD, ROOT, toy_f32_model], env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0 and "F32_JOB_SIM_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
