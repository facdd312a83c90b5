"""A selection of tests/test_gpu_output_format.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as
tests/test_emulated_voice_from_audio.py runs the C13r resampler) - the rational resampler kernel against rule C14r for all 14 pairs and every length of the GPU
test, the formats, the s16 / mu-law tables, the ragged batches, the identity and the old kernel beside the new one.  The tests that generate (refusals, routes,
the request collector: half an hour under emulation) sit behind BARK_SIM_FULL=1; the server test needs the product library."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILES = ("tests/test_gpu_output_format.py",)


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_output_format")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_kernel_formats_and_ragged_batches_pass_on_the_host_emulated_engine(sim_engine):
    k = "test_kernel_is_c14r or test_impulses_and or test_every_s16 or test_ragged_batches or test_identity or test_old_kernel"
    _passed(_pytest_on(sim_engine, k, workers=4, timeout=1800), 36)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="half an hour of emulation: set BARK_SIM_FULL=1")
def test_every_test_but_the_server_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not test_native_batch_server", workers=8, timeout=3400), 39)
