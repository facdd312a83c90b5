"""A selection of tests/test_gpu_voice_from_audio.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as
tests/test_emulated_semantic_encoder.py runs the semantic encoder) - the resampler kernel against rule C13r at every length up to 24 000 samples, its unit
impulses, and the shortest composition (1079 samples: two semantic ids, four codec frames) through bark_hip_voice_from_audio.  The remaining toy tests (the
longest recording, one-second and 20-second compositions, generation, refusals: minutes under emulation) sit behind BARK_SIM_FULL=1; the server test needs the
product library."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILES = ("tests/test_gpu_voice_from_audio.py",)


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_voice_from_audio")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_resampler_and_shortest_composition_pass_on_the_host_emulated_engine(sim_engine):
    k = "test_resampler_is_c13r or test_resampler_unit_impulses or test_resampler_twice or (test_voice_from_audio_equals_its_parts and toy-n1079-)"
    _passed(_pytest_on(sim_engine, k, workers=4, timeout=1800), 32)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="minutes of emulation: set BARK_SIM_FULL=1")
def test_every_toy_test_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not small- and not test_native_batch_server", workers=8, timeout=3400), 37)
