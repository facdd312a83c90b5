"""CPU tests of the voice-prompt boundary: the new exports and struct layouts through ctypes (as tests/test_abi.py does for the old ones), the
null-safe failures, and the voice side of the HTTP server's request parsing (tests/http_voice_driver.cpp, the pattern of tests/http_filter_driver.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import voice_prompt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from bark_amd_loader import load_package
    p = load_package()
    if not os.path.exists(p.library_path()):
        p.build_library()
    return p


def test_voice_exports_and_struct_layout(pkg):
    lib = pkg.load_library()
    for name in ("bark_hip_set_voice_prompt", "bark_hip_generate_batch_voiced", "bark_hip_batcher_submit_voiced", "bark_hip_pick_rows"):
        assert hasattr(lib, name), name
        assert name in pkg.api.EXPORTS
    header = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    assert "struct bark_hip_voice_prompt {" in header
    # three (pointer, int32) pairs: x86-64 pads each count to the next pointer
    V = pkg.BarkHipVoicePrompt
    assert C.sizeof(V) == 48
    assert [getattr(V, f).offset for f, _ in V._fields_] == [0, 8, 16, 24, 32, 40]
    assert [f for f, _ in V._fields_] == ["semantic", "n_semantic", "coarse_Tx2", "n_coarse_frames", "fine_Tx8", "n_fine_frames"]
    # bark.h stays byte-compatible with the reference: nothing about voices in it
    assert "voice" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_voice_entry_points_fail_cleanly_without_a_context(pkg):
    lib = pkg.load_library()
    v = R.synthetic_voice(1, 35, 41, 41)
    st, keep = pkg.api._voice_struct(v)
    assert (st.n_semantic, st.n_coarse_frames, st.n_fine_frames) == (35, 41, 41)
    assert lib.bark_hip_set_voice_prompt(None, C.byref(st)) == -1
    assert lib.bark_hip_set_voice_prompt(None, None) == -1
    assert lib.bark_hip_generate_batch_voiced(None, None, 1, None, None, None) == -1
    assert lib.bark_hip_batcher_submit_voiced(None, b"x", None, None, C.byref(st)) == -1
    assert lib.bark_hip_pick_rows(None, None, 1, 1024, 0.0, None, None, None, None) == -1


def test_server_voice_table_and_request_field(tmp_path, pkg):
    exe = str(tmp_path / "http_voice_driver")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "bark.cpp_amd", "examples"),
                        os.path.join(ROOT, "tests", "http_voice_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    v = R.synthetic_voice(2, 50, 60, 70)
    path = str(tmp_path / "alice.bvp")
    pkg.voice.save(pkg.VoicePrompt(v.semantic, v.coarse, v.fine), path)
    checksum = int(v.semantic.astype(np.int64).sum() + 3 * v.coarse.astype(np.int64).sum() + 7 * v.fine.astype(np.int64).sum())

    def run(body, *args):
        return subprocess.run([exe, body, *args], capture_output=True, text=True, check=True).stdout.splitlines()

    assert run('{"text": "a", "voice": "alice"}', "alice=" + path) == ["load=ok", f"voice=1,50,60,70,{checksum}"]
    assert run('{"text": "a"}', "alice=" + path)[-1] == "voice=0,0,0,0,0"
    assert run('{"text": "a", "voice": "bob"}', "alice=" + path)[-1].startswith("voice=-1,")          # unknown name: the server answers 400
    assert run('{"text": "a", "voice": 3}', "alice=" + path)[-1].startswith("voice=-1,")
    assert run('{"voice": "alice"}')[-1].startswith("voice=-1,")                                       # no table
    assert run("{}", "alice")[0] == "load=--voice expects name=file"
    assert "cannot open" in run("{}", "alice=" + path + ".missing")[0]
    open(path, "ab").write(b"\0\0\0\0")
    assert "counts do not match" in run("{}", "alice=" + path)[0]
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    assert "request_voice(body, voice_table" in src and "bark_hip_batcher_submit_voiced" in src and '"--voice"' in src
