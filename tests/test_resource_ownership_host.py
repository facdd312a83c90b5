"""Who releases what in a context, checked without a GPU and without Python in the checked process: tests/resource_driver.cpp walks one
context of the host-emulated engine through codec growth and recapture, decode graphs and their invalidation, the timing and profiling hooks, pinned memory, a
refused call and a clone that outlives its original.  The engine's host-control translation units and the driver are compiled with AddressSanitizer
(tests/simt/build_asan_driver.py), whose runtime is linked into the executable: a double release, a use after a release or a leak is its report."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_a_context_releases_every_graph_event_and_buffer_once(tmp_path_factory, toy_model):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "simt"))
    import build_asan_driver
    exe = build_asan_driver.build(str(tmp_path_factory.mktemp("sim_engine_asan")), os.path.join(ROOT, "tests", "resource_driver.cpp"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, toy_model], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert r.stdout.split() == ["ok"]
    assert "Sanitizer" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-4000:]
