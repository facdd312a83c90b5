"""CPU tests of the FLAC restatement (tests/flac_ref.py, rule C18f of DESIGN.md section 3): the decoder returns what the encoder was given on every input the
GPU tests use; both CRCs against a second, polynomial-division form; frames worked out by hand; the subframe choices the inputs were built for; and, if this
machine has a FLAC decoder of its own, that decoder's samples at every supported rate."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_ref as fr


@pytest.mark.parametrize("kind", fr.KINDS)
def test_decode_returns_what_encode_was_given(kind):
    for n in fr.LENGTHS:
        x = fr.signal(kind, n)
        stream = fr.encode(x, 24000)
        y, rate = fr.decode(stream)
        assert rate == 24000 and y.dtype == np.int16 and np.array_equal(x, y), (kind, n)
        assert len(stream) <= fr.max_bytes(n)
        assert max(len(f) for f, _ in fr.encode_frames(x, 24000)) <= fr.FRAME_STRIDE - 2


def _remainder(data: bytes, poly: int, width: int) -> int:
    """the message times x^width, divided by the polynomial as one long integer: the CRC without a register"""
    v = int.from_bytes(data, "big") << width
    for bit in range(v.bit_length() - 1, width - 1, -1):
        if v >> bit & 1:
            v ^= poly << (bit - width)
    return v


def test_both_crcs_against_polynomial_division():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 333):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert fr.crc8(data) == _remainder(data, 0x107, 8)
        assert fr.crc16(data) == _remainder(data, 0x18005, 16) == fr._crc16_fast(data)
    assert fr.crc8(b"") == 0 and fr.crc16(b"") == 0


def _bits(*fields) -> bytes:
    """(value, width) fields, most significant bit first, zero-padded to a byte"""
    s = "".join(format(v & ((1 << w) - 1), f"0{w}b") if w else "" for v, w in fields)
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big")


def _closed(header_without_crc: bytes, body: bytes) -> bytes:
    h = header_without_crc + bytes([fr.crc8(header_without_crc)])
    return h + body + fr.crc16(h + body).to_bytes(2, "big")


def test_a_constant_frame_by_hand():
    # 4096 samples of 7 at 24 kHz, frame 0: sync and fixed strategy FF F8, block 4096 = 1100, rate 24 kHz = 0111, mono 16 bit = 08, frame number 00
    want = _closed(bytes([0xFF, 0xF8, 0xC7, 0x08, 0x00]), bytes([0x00, 0x00, 0x07]))
    (got, info), = fr.encode_frames(np.full(4096, 7, np.int16), 24000)
    assert got == want and info[:3] == [0, 0, len(want)]
    # 5 samples of -2 at 12 kHz, frame 0: block size in 16 bits (0111, then 00 04), rate in kHz (1100, then 0C)
    want = _closed(bytes([0xFF, 0xF8, 0x7C, 0x08, 0x00, 0x00, 0x04, 0x0C]), bytes([0x00, 0xFF, 0xFE]))
    (got, info), = fr.encode_frames(np.full(5, -2, np.int16), 12000)
    assert got == want


def test_an_order_0_frame_of_16_samples_by_hand():
    # sums of |residual|: order 0 gives 24, order 1 gives 3 + 15 * 6 = 93: order 0.  16 = 2^4 and 1 > 0: partition orders 0 .. 4.  Zigzag: 3 -> 6, -3 -> 5.
    # One partition: k = 0 costs 4 + 16 + 88 = 108, k = 1 costs 4 + 32 + (3 + 2) * 8 = 76, k = 2 costs 4 + 48 + 8 = 60, k = 3 costs 4 + 64 = 68; escape: 3 bits of
    # width, 9 + 48 = 57 < 60.  Two partitions: 2 * (9 + 24) = 66.  So partition order 0, escape, width 3.
    x = np.asarray([3, -3] * 8, np.int16)
    body = _bits((0, 1), (8, 6), (0, 1), (0, 2), (0, 4), (15, 4), (3, 5), *[(v, 3) for v in x])
    want = _closed(bytes([0xFF, 0xF8, 0x77, 0x08, 0x00, 0x00, 0x0F]), body)
    (got, info), = fr.encode_frames(x, 24000)
    assert got == want and info[:2] == [8, 0]
    # the same samples in Rice codes where the escape is no shorter: 0 and -1 in turn, zigzag 0 and 1 - k = 0 costs 4 + 16 + 8 = 28, the escape 9 + 16 = 25 ...
    x = np.asarray([0, -1] * 8, np.int16)
    (got, info), = fr.encode_frames(x, 24000)
    assert got == _closed(bytes([0xFF, 0xF8, 0x77, 0x08, 0x00, 0x00, 0x0F]), _bits((0, 1), (8, 6), (0, 1), (0, 2), (0, 4), (15, 4), (1, 5), *[(v, 1) for v in x]))
    # ... and 0, 0, 0, -1: k = 0 costs 4 + 16 + 4 = 24 < 25: sixteen unary codes
    x = np.asarray([0, 0, 0, -1] * 4, np.int16)
    (got, info), = fr.encode_frames(x, 24000)
    assert got == _closed(bytes([0xFF, 0xF8, 0x77, 0x08, 0x00, 0x00, 0x0F]), _bits((0, 1), (8, 6), (0, 1), (0, 2), (0, 4), (0, 4), *[(1, 1), (1, 1), (1, 1), (1, 2)] * 4))


def test_an_escape_partition_by_hand():
    # 32 samples: sixteen of +-3 in turn, then sixteen zeros.  Order 0 (sum 48; order 1 gives 3 + 15 * 6 + 3 = 96).  Partition order 1: the first partition as
    # above (escape, width 3: 57 bits), the second all zero: k = 0 costs 4 + 16 = 20, the escape with width 0 costs 9.  66 bits; partition order 0 costs at
    # best k = 1: 4 + 64 + 40 = 108, k = 2: 4 + 96 + 8 = 108, escape 9 + 96 = 105; partition order 2: 2 * (9 + 24) + 2 * 9 = 84.
    x = np.asarray([3, -3] * 8 + [0] * 16, np.int16)
    body = _bits((0, 1), (8, 6), (0, 1), (0, 2), (1, 4), (15, 4), (3, 5), *[(v, 3) for v in x[:16]], (15, 4), (0, 5))
    want = _closed(bytes([0xFF, 0xF8, 0x77, 0x08, 0x00, 0x00, 0x1F]), body)
    (got, info), = fr.encode_frames(x, 24000)
    assert got == want and info[:2] == [8, 1]
    assert np.array_equal(fr.decode(fr.encode(x, 24000))[0], x)


def test_the_inputs_choose_what_they_were_built_for():
    code = lambda kind, n=4096: [i[0] for _, i in fr.encode_frames(fr.signal(kind, n), 24000)]
    assert code("silence") == [0] and code("constant", 12289) == [0, 0, 0, 0]
    assert code("alternating") == [1] and code("white", 8192) == [1, 1]
    assert code("ramp", 8192) == [10, 10]
    assert code("small_noise") == [8]
    po = [i[1] for _, i in fr.encode_frames(fr.signal("sine_click", 4096), 24000)]
    assert po[0] > 0 and code("sine_click")[0] in (9, 10, 11, 12)
    assert [i[:2] for _, i in fr.encode_frames(fr.signal("loud_first_partition", 4096), 24000)] == [[8, 4]]
    r4 = fr.residuals(fr.signal("alternating", 16).astype(np.int64), 4)
    assert int(np.abs(r4).max()) > 32768                                  # the residual the 16-bit samples cannot hold
    # the stream header: 42 bytes, STREAMINFO marked last, the sample count and an MD5 of zeros
    s = fr.encode(fr.signal("small_noise", 4097), 44100)
    assert s[:8] == b"fLaC\x80\x00\x00\x22" and s[8:12] == b"\x10\x00\x10\x00" and s[26:42] == bytes(16)
    assert int.from_bytes(s[18:26], "big") == (44100 << 44) | (15 << 36) | 4097


def _local_decoder():
    for mod in ("soundfile", "torchaudio"):
        if importlib.util.find_spec(mod) is not None:
            return mod
    for exe in ("ffmpeg", "flac", "sox"):
        if shutil.which(exe):
            return exe
    return None


def _decode_with(dec, path, tmp):
    if dec == "soundfile":
        import soundfile
        y, rate = soundfile.read(path, dtype="int16")
        return np.asarray(y, np.int16).reshape(-1), rate
    if dec == "torchaudio":
        import torchaudio
        y, rate = torchaudio.load(path, normalize=False)
        return y.numpy().reshape(-1).astype(np.int16), rate
    raw = os.path.join(tmp, "out.raw")
    cmd = {"ffmpeg": ["ffmpeg", "-y", "-loglevel", "error", "-i", path, "-f", "s16le", "-acodec", "pcm_s16le", raw],
           "flac": ["flac", "-d", "-f", "--force-raw-format", "--endian=little", "--sign=signed", "-o", raw, path],
           "sox": ["sox", path, "-t", "raw", "-e", "signed", "-b", "16", "-L", raw]}[dec]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    return np.fromfile(raw, "<i2"), None


def test_an_independent_decoder_agrees(tmp_path):
    dec = _local_decoder()
    if dec is None:
        pytest.skip("no FLAC decoder on this machine (soundfile, torchaudio, ffmpeg, flac, sox): the format is held to tests/flac_ref.py's decoder alone")
    for rate in fr.RATES:
        for kind in fr.KINDS:
            x = fr.signal(kind, 12289)
            path = str(tmp_path / f"{kind}_{rate}.flac")
            open(path, "wb").write(fr.encode(x, rate))
            y, got_rate = _decode_with(dec, path, str(tmp_path))
            assert np.array_equal(x, y), (dec, kind, rate)
            assert got_rate in (None, rate)
