"""A selection of tests/test_gpu_flac.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as tests/test_emulated_loudness.py runs
the loudness kernels) - the two FLAC kernels against rule C18f byte for byte on all fourteen lengths of the alternating and the click input, a ragged batch
of 5 in two orders and the refusals.  The other inputs, the batch of 64, the 300 frames and the routes that generate sit behind BARK_SIM_FULL=1; the server
test needs the product library."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILES = ("tests/test_gpu_flac.py",)


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_flac")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_kernels_pass_on_the_host_emulated_engine(sim_engine):
    k = "test_streams_and_frame_choices_equal_the_reference and (alternating or sine_click) or test_a_ragged_batch_of_5 or test_refusals_leave_the_context_usable"
    _passed(_pytest_on(sim_engine, k, workers=3, timeout=1800), 4)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="long under emulation: set BARK_SIM_FULL=1")
def test_every_test_but_the_server_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not test_native_batch_server", workers=8, timeout=3400), 25)
