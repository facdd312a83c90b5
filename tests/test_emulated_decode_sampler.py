"""tests/test_gpu_decode_sampler.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as tests/test_emulated_codec_encoder.py
does for the codec encoder), so that the rows built around the sampler's thresholds run through the engine's own kernels - work-item for work-item -
in the suite that needs no GPU: families A, B, D, E and G whole, the stop rule (C) and the mixed launches (F) at n = 1024, and the hook's refusals.
The emulator has no v_exp_f32, no 16 concurrent waves and no scheduler: the fast path's tree sum and the kernel's barrier ordering are held on the
device.  The large sizes of C and F, the multinomial margin rows (H) and the forced-exact child (I) sit behind BARK_SIM_FULL=1."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILE = "tests/test_gpu_decode_sampler.py"


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_decode_sampler")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", FILE, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_threshold_rows_pass_on_the_host_emulated_engine(sim_engine):
    k = "test_a_ or test_b_ or test_d_ or test_e_ or test_g_ or test_hook_ or ((test_c_ or test_f_) and n1024)"
    _passed(_pytest_on(sim_engine, k, workers=6, timeout=1200), 9)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="minutes of emulation: set BARK_SIM_FULL=1")
def test_every_decode_sampler_test_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not n1024 and (test_c_ or test_f_ or test_h_ or test_i_)", workers=6, timeout=3000), 5)
