"""CPU tests of the sampler hook's boundary (bark_hip_sample_rows_state), in the style of tests/test_voice_abi.py: the export, the layout of its
settings struct through ctypes against the header, and the null-safe failures.  What a live context refuses (sizes, states, settings) is in
tests/test_gpu_decode_sampler.py::test_hook_refuses_bad_arguments, which tests/test_emulated_decode_sampler.py also runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from bark_amd_loader import load_package
    p = load_package()
    if not os.path.exists(p.library_path()):
        p.build_library()
    return p


def test_sampler_hook_export_and_struct_layout(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "bark_hip_sample_rows_state")
    assert "bark_hip_sample_rows_state" in pkg.api.EXPORTS
    header = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    assert "BARK_API int bark_hip_sample_rows_state(struct bark_context * bctx," in header
    body = header.split("struct bark_hip_sample_call {")[1].split("};")[0]
    fields = re.findall(r"^\s*int32_t (\w+);", body, re.M)
    V = pkg.api.BarkHipSampleCall
    assert [f for f, _ in V._fields_] == fields == ["mode", "eos_token", "token_base", "prescaled", "n_past_add", "per_row"]
    assert C.sizeof(V) == 24 and [getattr(V, f).offset for f, _ in V._fields_] == [0, 4, 8, 12, 16, 20]
    # the state travels as eight 32-bit words in the order of struct StepState
    kernels_h = open(os.path.join(ROOT, "bark.cpp_amd", "csrc", "kernels.h")).read()
    st = kernels_h.split("struct StepState {")[1].split("};")[0]
    assert tuple(re.findall(r"^\s*(?:int32_t|float)\s+(\w+);", st, re.M)) == pkg.BarkContext.STATE_FIELDS
    # bark.h stays byte-compatible with the reference
    assert "sample_rows" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_sampler_hook_fails_cleanly_without_a_context_or_arguments(pkg):
    lib = pkg.load_library()
    l = np.zeros((1, 8), np.float32)
    t, p, m = np.zeros(1, np.float32), np.ones(1, np.float32), np.full(1, 2.0, np.float32)
    k, ids, st = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 8), np.int32)
    u, eos = np.full(1, 0.5), np.zeros(1, np.float32)
    call = pkg.api.BarkHipSampleCall(0, -1, 0, 0, 1, 0)
    args = [l.ctypes.data, 1, 8, t.ctypes.data, k.ctypes.data, p.ctypes.data, u.ctypes.data, m.ctypes.data, C.byref(call), st.ctypes.data,
            ids.ctypes.data, eos.ctypes.data]
    assert lib.bark_hip_sample_rows_state(None, *args) == -1
    assert lib.bark_hip_sample_rows_state(None, None, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    assert not st.any() and ids[0] == 0                               # nothing was written
