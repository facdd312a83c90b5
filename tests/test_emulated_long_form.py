"""The kernel-level tests of tests/test_gpu_long_form.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as
tests/test_emulated_output_format.py runs the C14r resampler) - the activity kernel and the join kernel against rule C15j for every rate and format, runs of
one-sample segments, tiles in gaps and across seams, trim, fade, the old resampler beside the new kernel, repeats and clones.  The tests that generate
(generate_long, chained voices) and the refusals (they end by generating) sit behind BARK_SIM_FULL=1; the 2^25-sample join runs on the GPU only, and the server test needs the product library."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILES = ("tests/test_gpu_long_form.py",)


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_long_form")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_join_kernels_pass_on_the_host_emulated_engine(sim_engine):
    k = ("test_join_is_c15j or test_runs_of_one or test_a_tile_inside or test_output_counts or test_trim_by or test_silent_segments or test_fade_at or "
         "test_one_plain_segment or test_repeat_and_clone")
    _passed(_pytest_on(sim_engine, k, workers=4, timeout=1800), 12 + 2 + 1 + 3 + 1 + 1 + 2 + 8 + 1)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="long under emulation: set BARK_SIM_FULL=1")
def test_every_test_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not test_the_longest_joined and not test_native_batch_server", workers=8, timeout=3400), 35)
