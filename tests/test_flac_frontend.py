"""bark_batch_server's output format without a device: request_format and answer_type of bark.cpp_amd/examples/http_util.h through
tests/flac_frontend_driver.cpp - "format": "flac" is parsed (and is the default under --format flac) and goes out as audio/flac, anything that is not one of
the four names is refused, every other answer is still a WAV; once more with AddressSanitizer and UBSan (a stand-alone host program).  The body of a FLAC
answer is checked on the GPU (tests/test_gpu_flac.py::test_native_batch_server_flac_format)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-I", os.path.join(ROOT, "bark.cpp_amd", "examples"),
                        os.path.join(ROOT, "tests", "flac_frontend_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flac_frontend")
    return _build(tmp, "driver", []), _build(tmp, "driver_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _parse(exe, fields, rate=24000, name="f32"):
    body = fields if isinstance(fields, str) else json.dumps(fields)
    r = subprocess.run([exe, "parse", body, str(rate), name], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stdout.strip()


def test_flac_is_parsed_and_a_wrong_value_refused(drivers):
    for exe in drivers:
        assert _parse(exe, {"text": "a", "format": "flac"}) == "ok 24000 3 audio/flac"
        assert _parse(exe, {"text": "a", "format": "flac", "sample_rate": 16000}) == "ok 16000 3 audio/flac"
        assert _parse(exe, {"text": "a", "sample_rate": 8000}, 48000, "flac") == "ok 8000 3 audio/flac"          # --format flac: the default form
        assert _parse(exe, {"text": "a"}, 44100, "flac") == "ok 44100 3 audio/flac"
        assert _parse(exe, {"text": "a", "format": "s16"}, 24000, "flac") == "ok 24000 1 audio/wav"               # a request may still ask for a WAV
        assert _parse(exe, {"text": "a"}) == "ok 24000 0 audio/wav" and _parse(exe, {"text": "a", "format": "mulaw"}) == "ok 24000 2 audio/wav"
        for bad in ("FLAC", "flac ", "ogg", "alaw", "", 3, True, None, ["flac"]):
            assert _parse(exe, {"text": "a", "format": bad}) == "bad", bad
        assert _parse(exe, {"text": "a", "format": "flac", "sample_rate": "x"}) == "bad"
        assert _parse(exe, '{"text": "a", "format": ') == "bad" and _parse(exe, '{"text": "a", "format": "fla') == "bad"


def test_the_server_speaks_flac():
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    assert "barkhttp::request_format(body, af.sample_rate, af.sample_format)" in src and "barkhttp::answer_type(af.sample_format)" in src
    assert src.count("answer_body(bytes, nb, af)") == 2 and "f32|s16|mulaw|flac" in src
    body = src[src.index("std::string answer_body("):src.index("bool format_valid(")]
    assert "BARK_HIP_SAMPLE_FLAC) return std::string(bytes.data(), (size_t) nb);" in body and "barkhttp::wav_samples(" in body
    assert src.index("barkhttp::request_format(body") < src.index("next_seed.fetch_add(1)")      # a refused value draws no seed
