"""A selection of tests/test_gpu_codec_decoder.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as
tests/test_emulated_codec_encoder.py runs the encoder's) - the batched decoder's host logic (row tables, graph keys, captures, refusals) and its
toy-width kernels against the oracle bit for bit: D1 at 1, 2, 7, 33 and 65 frames, D2's first seven lists and 32 x [3], D4 on toy, D5 without the
200-frame step, D6.  The remaining toy tests of that file (minutes under emulation) sit behind BARK_SIM_FULL=1; the mini and small widths and D3's child
processes need the device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILE = "tests/test_gpu_codec_decoder.py"


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_codec_decoder")))


def _pytest_on(sim_engine, k, workers, timeout):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", FILE, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


SELECTION = ("(test_lengths_taps_and_pcm and (T1_ or T2_ or T7_ or T33_ or T65_))"
             " or (test_ragged_batches and (list0_ or list1_ or list2_ or list3_ or list4_ or list5_ or list6_ or list8_))"
             " or (test_codebook_depths and toy) or (test_one_context and without_regrow) or test_refusals_leave")


def test_ragged_batches_graph_keys_and_refusals_pass_on_the_host_emulated_engine(sim_engine):
    # 5 lengths + 8 lists + 3 depths + the sequence + the refusals
    _passed(_pytest_on(sim_engine, SELECTION, workers=6, timeout=1500), 18)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="minutes of emulation: set BARK_SIM_FULL=1")
def test_every_toy_test_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not test_widths_and_orders and not small and not test_the_longest", workers=8, timeout=3000), 32)
