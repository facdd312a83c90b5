"""CPU test of the boundary of lock-step jobs on f32 model files: bark_hip_batch_lock_steps - the accessor that makes a job's route observable without
timing - is declared in the header with its signature, exported by the library, mirrored in the ctypes wrapper, and fails cleanly without a context."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from bark_amd_loader import load_package
    p = load_package()
    if not os.path.exists(p.library_path()):
        p.build_library()
    return p


def test_batch_lock_steps_is_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    assert re.search(r"BARK_API\s+int\s+bark_hip_batch_lock_steps\s*\(\s*struct\s+bark_context\s*\*\s*\w+\s*,\s*int32_t\s+\w+\[2\]\s*\)\s*;", header)
    lib = pkg.load_library()
    assert hasattr(lib, "bark_hip_batch_lock_steps")
    assert "bark_hip_batch_lock_steps" in pkg.api.EXPORTS
    fn = lib.bark_hip_batch_lock_steps
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(C.c_int32)]
    assert callable(getattr(pkg.BarkContext, "batch_lock_steps"))
    # bark.h stays byte-compatible with the reference: the accessor lives in the extension header only
    assert "lock_steps" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_batch_lock_steps_fails_cleanly_without_a_context_or_a_buffer(pkg):
    lib = pkg.load_library()
    out = (C.c_int32 * 2)(7, 7)
    assert lib.bark_hip_batch_lock_steps(None, out) == -1
    assert list(out) == [7, 7]


def test_header_and_documents_state_the_route_of_f32_files():
    header = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*BARK_API double bark_hip_time_slots", header, flags=re.S)
    assert m and "f32 model files" in m.group(1) and "f16 model files only" not in m.group(1)
    assert "slower plain kernels" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
