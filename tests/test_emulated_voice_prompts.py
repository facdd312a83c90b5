"""The voiced stage-call tests of tests/test_gpu_voice_prompts.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as
tests/test_emulated_engine.py runs the parity suite) against tests/voice_prompt_ref.py, bit for bit, without a GPU - toy model.  Tokenizer, semantic and
coarse stage calls run by default (about a minute each under emulation); the fine stage calls, bark_generate_audio and the pick kernels take several
minutes each and sit behind BARK_SIM_FULL=1."""
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
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_voice")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_voice_prompts.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_voiced_stage_calls_pass_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "test_voiced_semantic_and_coarse_stage_calls and toy", workers=6, timeout=2400), 6)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="minutes of emulation: set BARK_SIM_FULL=1")
def test_voiced_fine_stage_and_picks_pass_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "(test_voiced_fine_stage_call and toy) or (test_voiced_generate_audio and toy and greedy) or test_pick_kernels or test_refused_voice_prompts",
                       workers=8, timeout=3400), 11)
