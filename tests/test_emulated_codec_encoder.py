"""The toy_enc selection of tests/test_gpu_codec_encoder.py and tests/test_gpu_codec_encoder_oracle.py on a CPU: the whole engine compiled for the host
(tests/simt/build_engine.py, as tests/test_emulated_voice_prompts.py runs the voiced stage calls) - the RVQ kernel against C11q at T <= 4, latents, taps
and codes at the lengths 1, 7 and 321 (the padding rule's short-input detour at every layer, a partial second frame); against the oracle bit for bit:
taps and codes at the same lengths in both convolution orders (the chain kernels of BARK_HIP_CROSSCHECK=1024 included), and the RVQ kernel on exact
ties.  The remaining toy_enc tests (24000-sample inputs, batches, clone, refusals, voice prompt, midpoint latents: minutes under emulation) sit behind
BARK_SIM_FULL=1."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_codec_encoder")))


def _pytest_on(sim_engine, k, workers, timeout, files=("tests/test_gpu_codec_encoder.py",)):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


BOTH = ("tests/test_gpu_codec_encoder.py", "tests/test_gpu_codec_encoder_oracle.py")


def test_rvq_rows_and_short_inputs_pass_on_the_host_emulated_engine(sim_engine):
    k = ("(test_rvq_kernel_equals and (T1- or T4-)) or ((test_latent_taps or test_codes_are) and (toy_enc-n1 or toy_enc-n7 or toy_enc-n321) and not n19)"
         " or (test_taps_and_codes_equal_the_oracle and (n1_ or n7_ or n321_)) or (test_both_convolution_orders and n1_7_321_) or test_rvq_kernel_on_exact_ties")
    _passed(_pytest_on(sim_engine, k, workers=6, timeout=1200, files=BOTH), 18)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="minutes of emulation: set BARK_SIM_FULL=1")
def test_every_toy_enc_test_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not small and not encodec_24khz", workers=8, timeout=3000, files=BOTH), 53)
