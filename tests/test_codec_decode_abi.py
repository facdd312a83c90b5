"""CPU tests of the batched codec decoder's surface: bark_hip_codec_decode_many is in api.EXPORTS, declared in include/bark_mi355x.h and exported by
the cross-compiled libbark.so; the ctypes mirror's argument types are the header's; and everything the call refuses before any work - a null handle, null
arrays, a null matrix, a count outside 1 .. 32, a capacity below 320 sum T_i - returns -1 without a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bark_hip_codec_decode_many"
CTYPE_OF = {"struct bark_context *": C.c_void_p, "const int32_t * const *": C.POINTER(C.c_void_p), "const int *": C.c_void_p, "int": C.c_int,
            "float *": C.c_void_p}


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _declaration():
    header = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"BARK_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % NAME, header)
    assert m, f"{NAME} is not declared in bark_mi355x.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_point_is_listed_declared_and_exported():
    pkg = _pkg()
    lib = pkg.load_library()
    assert NAME in pkg.api.EXPORTS
    assert len(_declaration()) == 7
    assert hasattr(lib, NAME), f"libbark.so does not export {NAME}"
    assert callable(pkg.BarkContext.codec_decode_many)
    assert hasattr(lib, "bark_hip_codec_decode")                 # the single call stays


def test_mirror_argument_types_match_the_header():
    args = _declaration()
    types = [re.sub(r"\s*\w+$", "", a).strip() for a in args]            # drop the parameter's name
    assert types == ["struct bark_context *", "const int32_t * const *", "const int *", "int", "int", "float *", "int"], types
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["bctx", "codes", "T", "n", "n_q", "pcm_concat", "capacity"]
    lib = _pkg().load_library()
    fn = getattr(lib, NAME)
    assert list(fn.argtypes) == [CTYPE_OF[t] for t in types]
    assert fn.restype is C.c_int


def test_refused_before_any_work():
    """None of these reaches the engine: the handle below is not a context, so a call that got past the door would not return -1 - it would crash."""
    lib = _pkg().load_library()
    fn = getattr(lib, NAME)
    codes = [np.zeros((8, 3), np.int32) for _ in range(33)]
    ptrs = (C.c_void_p * 33)(*[c.ctypes.data for c in codes])
    T = np.full(33, 3, np.int32)
    pcm = np.zeros(320 * 3 * 33, np.float32)
    assert fn(None, ptrs, T.ctypes.data, 2, 8, pcm.ctypes.data, pcm.size) == -1                       # null handle
    fake = C.create_string_buffer(1 << 16)                      # stands in for a context: the calls below must not look inside
    h = C.addressof(fake)
    assert fn(h, None, T.ctypes.data, 2, 8, pcm.ctypes.data, pcm.size) == -1                          # null arrays
    assert fn(h, ptrs, None, 2, 8, pcm.ctypes.data, pcm.size) == -1
    assert fn(h, ptrs, T.ctypes.data, 2, 8, None, pcm.size) == -1
    holed = (C.c_void_p * 2)(codes[0].ctypes.data, None)
    assert fn(h, holed, T.ctypes.data, 2, 8, pcm.ctypes.data, pcm.size) == -1                         # a null matrix
    for n in (0, 33, -1):
        assert fn(h, ptrs, T.ctypes.data, n, 8, pcm.ctypes.data, pcm.size) == -1, n                   # n outside 1 .. 32
    assert fn(h, ptrs, T.ctypes.data, 2, 8, pcm.ctypes.data, 320 * 6 - 1) == -1                       # capacity below 320 sum T_i
    assert fn(h, ptrs, T.ctypes.data, 32, 8, pcm.ctypes.data, 320 * 96 - 1) == -1
    assert not pcm.any()
