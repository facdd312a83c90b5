"""The recording side of bark_batch_server without a device: parse_wav and write_voice_file of bark.cpp_amd/examples/http_util.h through
tests/voice_audio_driver.cpp - once as built, once more with AddressSanitizer and UBSan on the malformed inputs (a stand-alone host program)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def _build(tmp, name, extra):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", os.path.join(ROOT, "bark.cpp_amd", "examples"),
                        os.path.join(ROOT, "tests", "voice_audio_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("voice_audio")
    return _build(tmp, "driver", []), _build(tmp, "driver_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def chunk(cid, payload):
    return cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def fmt(tag, channels, rate, bits, extensible_sub=None):
    base = struct.pack("<HHIIHH", 0xFFFE if extensible_sub else tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if extensible_sub:
        base += struct.pack("<HHI", 22, bits, 4) + struct.pack("<H", extensible_sub) + GUID_TAIL
    return chunk(b"fmt ", base)


def riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


I16 = np.array([0, 1, -1, 32767, -32768, 12345, -4321, 7], "<i2")
F32 = np.array([0.0, 0.5, -0.25, 1.0, -1.0, 3.0e-8, 0.123], "<f4")
GOOD = {
    "pcm16": (riff(fmt(1, 1, 24000, 16), chunk(b"data", I16.tobytes())), 24000, I16.astype(np.float32) / np.float32(32768.0)),
    "float32": (riff(fmt(3, 1, 16000, 32), chunk(b"data", F32.tobytes())), 16000, F32.astype(np.float32)),
    "extensible_pcm16": (riff(fmt(1, 1, 24000, 16, extensible_sub=1), chunk(b"data", I16.tobytes())), 24000, I16.astype(np.float32) / np.float32(32768.0)),
    "extensible_float32": (riff(fmt(3, 1, 48000, 32, extensible_sub=3), chunk(b"data", F32.tobytes())), 48000, F32.astype(np.float32)),
    "odd_list_chunk": (riff(fmt(1, 1, 24000, 16), chunk(b"LIST", b"INFOabc"), chunk(b"data", I16.tobytes())), 24000, I16.astype(np.float32) / np.float32(32768.0)),
    "chunk_behind_data": (riff(fmt(1, 1, 24000, 16), chunk(b"data", I16.tobytes()), chunk(b"LIST", b"x")), 24000, I16.astype(np.float32) / np.float32(32768.0)),
}
_pcm16 = GOOD["pcm16"][0]
BAD = {
    "stereo": riff(fmt(1, 2, 24000, 16), chunk(b"data", I16.tobytes())),
    "eight_bit": riff(fmt(1, 1, 24000, 8), chunk(b"data", bytes(range(16)))),
    "pcm24": riff(fmt(1, 1, 24000, 24), chunk(b"data", bytes(range(18)))),
    "float64": riff(fmt(3, 1, 24000, 64), chunk(b"data", bytes(16))),
    "alaw": riff(fmt(6, 1, 8000, 8), chunk(b"data", bytes(16))),
    "extensible_other_subformat": riff(fmt(1, 1, 24000, 16, extensible_sub=6), chunk(b"data", I16.tobytes())),
    "data_beyond_the_body": _pcm16[:40] + struct.pack("<I", len(I16) * 2 + 1) + _pcm16[44:],
    "data_size_huge": _pcm16[:40] + struct.pack("<I", 0xFFFFFFFF) + _pcm16[44:],
    "no_fmt": riff(chunk(b"data", I16.tobytes())),
    "no_data": riff(fmt(1, 1, 24000, 16), chunk(b"LIST", b"abcd")),
    "empty_data": riff(fmt(1, 1, 24000, 16), chunk(b"data", b"")),
    "one_byte_of_data": riff(fmt(1, 1, 24000, 16), chunk(b"data", b"\x01")),
    "fmt_cut_short": riff(chunk(b"fmt ", struct.pack("<HHI", 1, 1, 24000)), chunk(b"data", I16.tobytes())),
    "fmt_size_beyond_the_body": b"RIFF" + struct.pack("<I", 30) + b"WAVEfmt " + struct.pack("<I", 4000) + bytes(18),
    "unknown_chunk_beyond_the_body": riff(fmt(1, 1, 24000, 16)) + b"LIST" + struct.pack("<I", 0xFFFFFFF0) + b"abc",
    "not_riff": b"RIFX" + _pcm16[4:],
    "not_wave": _pcm16[:8] + b"AVI " + _pcm16[12:],
    "empty": b"",
    "rate_zero": riff(fmt(1, 1, 0, 16), chunk(b"data", I16.tobytes())),
}


def _parse(exe, tmp_path, blob):
    src, dst = tmp_path / "in.wav", tmp_path / "out.f32"
    src.write_bytes(blob)
    r = subprocess.run([exe, "wav", str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    word = r.stdout.split()
    if word[0] == "err":
        assert len(word) > 1
        return None
    return int(word[1]), np.fromfile(dst, "<f4", int(word[2]))


@pytest.mark.parametrize("name", sorted(GOOD))
def test_parse_wav_takes(drivers, tmp_path, name):
    blob, rate, want = GOOD[name]
    for exe in drivers:
        got = _parse(exe, tmp_path, blob)
        assert got is not None and got[0] == rate and got[1].tobytes() == want.tobytes()


@pytest.mark.parametrize("name", sorted(BAD))
def test_parse_wav_refuses_with_a_message(drivers, tmp_path, name):
    for exe in drivers:
        assert _parse(exe, tmp_path, BAD[name]) is None


@pytest.mark.parametrize("name", ["pcm16", "extensible_float32", "odd_list_chunk"])
def test_every_truncation_is_refused(drivers, tmp_path, name):
    blob = GOOD[name][0]
    src = tmp_path / "in.wav"
    src.write_bytes(blob)
    for exe in drivers:
        r = subprocess.run([exe, "truncations", str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.split() == ["refused", str(len(blob)), "of", str(len(blob))]


def test_voice_file_round_trip_equals_voice_save(drivers, tmp_path):
    from bark_amd_loader import load_package
    voice = load_package().voice
    rng = np.random.default_rng(3)
    for n_sem, t in ((0, 0), (1, 1), (49, 75)):
        v = voice.VoicePrompt(rng.integers(0, 10000, n_sem), rng.integers(0, 1024, (t, 2)), rng.integers(0, 1024, (t, 8)))
        a, b = str(tmp_path / "a.bvp"), str(tmp_path / "b.bvp")
        v.save(a)
        for exe in drivers:
            r = subprocess.run([exe, "voice", a, b], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and r.stdout.split() == ["ok", str(n_sem), str(t), str(t)], r.stdout + r.stderr[-2000:]
            assert open(b, "rb").read() == open(a, "rb").read()
            assert voice.load(b) == v
    bad = tmp_path / "bad.bvp"
    bad.write_bytes(b"BVP1" + struct.pack("<3i", 5, 0, 0))
    for exe in drivers:
        r = subprocess.run([exe, "voice", str(bad), str(tmp_path / "c.bvp")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.startswith("err")
