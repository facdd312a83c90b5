#!/usr/bin/env python3
"""build_asan_driver.py OUT_DIR DRIVER - the host-emulated engine of build_engine.py (same patched sources, same flags) as a stand-alone program: DRIVER, a
C++ file with a main of its own that calls the C ABI, linked with the engine's objects.  The host-control translation units (HOST_CONTROL) and DRIVER are
compiled with AddressSanitizer and its runtime is linked into the executable; the kernel files stay as they are, because their work-items are hand-switched
fibers, which the sanitizer's stack bookkeeping does not follow.  A module of its own: build_engine.py stays the one recipe of libbark_sim.so, which every emulated test builds."""
import os
import subprocess
import sys

import build_engine as E

HOST_CONTROL = ["engine_load.hip", "engine.hip", "engine_codec.hip", "engine_batch.hip", "engine_timing.hip", "api.hip", "batcher.hip"]
ASAN = ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]


def build(out_dir: str, driver: str) -> str:
    src = os.path.join(out_dir, "src")
    os.makedirs(src, exist_ok=True)
    for name in os.listdir(E.CSRC):
        if name.endswith((".h", ".hip", ".cpp")):
            open(os.path.join(src, name), "w").write(E.patch(open(os.path.join(E.CSRC, name)).read()))
    flags = ["-std=c++20", "-O1", "-mfma", "-mf16c", "-mavx2", "-ffp-contract=off", "-pthread", "-fPIC", "-fvisibility=hidden", "-Wno-everything",      # as build_engine.build
             "-I", E.HERE, "-I", src, "-I", os.path.join(E.ROOT, "include")]
    procs, objs = [], []
    for name, path in [(name, os.path.join(src, name)) for name in E.HIP_SOURCES + E.CPP_SOURCES] + [("driver", driver)]:
        o = os.path.join(out_dir, name.rsplit(".", 1)[0] + ".o")
        objs.append(o)
        extra = ASAN if name in HOST_CONTROL or name == "driver" else []
        procs.append((name, subprocess.Popen([E.CLANG, "-x", "c++"] + flags + extra + ["-c", path, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for name, p in procs:
        log = p.communicate()[0].decode()
        if p.returncode != 0:
            raise RuntimeError(f"{name}: {log[-3000:]}")
    exe = os.path.join(out_dir, "driver_asan")
    r = subprocess.run([E.CLANG, "-pthread", "-o", exe] + ASAN + objs, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    return exe


if __name__ == "__main__":
    print(build(sys.argv[1], sys.argv[2]))
