"""A selection of tests/test_gpu_semantic_encoder.py on a CPU: the whole engine compiled for the host (tests/simt/build_engine.py, as
tests/test_emulated_codec_encoder.py runs the codec encoder) - the token head's hook at T = 1 and 2, and taps and ids of hub_toy at 400 and 720 samples
(every new kernel: convolution 0 with its norm, the valid strided convolutions, the grouped positional convolution, the post-norm step, attention over one
and two keys), and of tests/test_gpu_semantic_encoder_oracle.py: the engine's own source, run on the host, equals the CPU oracle bit for bit at taps 0 - 5 and
the ids of 400, 720 and 2640 samples and at the head's logits and ids of 1 and 2 rows - before a GPU sees either.  The remaining hub_toy tests (16000-sample inputs, state, clone, refusals, generation: minutes under emulation) sit behind BARK_SIM_FULL=1."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FILES = ("tests/test_gpu_semantic_encoder.py",)
ORACLE_FILES = ("tests/test_gpu_semantic_encoder_oracle.py",)


@pytest.fixture(scope="module")
def sim_engine(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_engine
    return build_engine.build(str(tmp_path_factory.mktemp("sim_engine_semantic_encoder")))


def _pytest_on(sim_engine, k, workers, timeout, files=FILES):
    env = dict(os.environ); env["BARK_HIP_LIBRARY"] = sim_engine
    cmd = [sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-n", str(workers), "-k", k]
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _passed(r, at_least):
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-500:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= at_least, tail


def test_head_rows_and_short_inputs_pass_on_the_host_emulated_engine(sim_engine):
    k = "(test_head_hook and (T1- or T2-)) or ((test_taps_against_hf or test_ids_are_hf) and (hub_toy-n400- or hub_toy-n720-))"
    _passed(_pytest_on(sim_engine, k, workers=3, timeout=1200), 6)


def test_host_emulated_engine_equals_the_oracle_bit_for_bit(sim_engine):
    k = "(test_frame_count_edges and (n400_ or n720_ or n2640_)) or (test_head_alone and (T1_ or T2_))"
    _passed(_pytest_on(sim_engine, k, workers=3, timeout=1200, files=ORACLE_FILES), 5)


@pytest.mark.slow
@pytest.mark.skipif(os.environ.get("BARK_SIM_FULL") != "1", reason="minutes of emulation: set BARK_SIM_FULL=1")
def test_every_hub_toy_test_passes_on_the_host_emulated_engine(sim_engine):
    _passed(_pytest_on(sim_engine, "not hub_base and not from_audio_alone", workers=8, timeout=3000), 17)
