"""Rule C18f restated on the CPU: the FLAC encoder of the output path, byte for byte, and a decoder that shares nothing with it.

encode(s16, rate) -> bytes         the stream the device and the host write together: marker, STREAMINFO, frames of 4096 samples
encode_frames(s16, rate) -> list   (bytes, [subframe code, partition order, byte length, CRC-16]) per frame - what bark_hip_flac_frames reports
decode(bytes) -> (s16, rate)       parses every header, checks both CRCs, handles CONSTANT, VERBATIM, FIXED 0 .. 4, Rice and escape partitions

The encoder works on numpy arrays frame by frame; the decoder is a plain bit reader.  Subframe code: 0 CONSTANT, 1 VERBATIM, 8 + o FIXED of order o (the
six type bits of the subframe header)."""
import numpy as np

BLOCK = 4096
MAX_PARTITION_ORDER = 4
MAX_RICE = 14
RATE_CODE = {8000: 0b0100, 12000: 0b1100, 16000: 0b0101, 22050: 0b0110, 24000: 0b0111, 32000: 0b1000, 44100: 0b1001, 48000: 0b1010}
RATES = tuple(sorted(RATE_CODE))
FRAME_STRIDE = 8208                      # the device's scratch slot: 11 header bytes + 1 + 2 * 4096 + 2, rounded up to 16


def max_bytes(n: int) -> int:
    """The bound bark_hip_flac_max_bytes states: marker and STREAMINFO, and every frame verbatim under the longest header."""
    frames = (n + BLOCK - 1) // BLOCK
    return 42 + frames * 14 + 2 * n


# ---- CRCs, bit by bit ------------------------------------------------------------------------------------------------------------------------------------
def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


_T16 = None


def _crc16_fast(data: bytes) -> int:
    """crc16 through a table made from crc16 itself (the streams of the long tests have megabytes)."""
    global _T16
    if _T16 is None:
        _T16 = [crc16(bytes([i])) for i in range(256)]
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


# ---- the encoder -----------------------------------------------------------------------------------------------------------------------------------------
def utf8_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    if v < 0x800:
        return bytes([0xC0 | (v >> 6), 0x80 | (v & 0x3F)])
    assert v < 0x10000
    return bytes([0xE0 | (v >> 12), 0x80 | ((v >> 6) & 0x3F), 0x80 | (v & 0x3F)])


def frame_header(frame_no: int, n: int, rate: int) -> bytes:
    code = RATE_CODE[rate]
    h = bytes([0xFF, 0xF8, ((0b1100 if n == BLOCK else 0b0111) << 4) | code, 0x08]) + utf8_number(frame_no)
    if n != BLOCK:
        h += bytes([(n - 1) >> 8, (n - 1) & 0xFF])
    if code == 0b1100:
        h += bytes([rate // 1000])
    return h + bytes([crc8(h)])


def residuals(s: np.ndarray, order: int) -> np.ndarray:
    """The FIXED predictor's residual of samples order .. n - 1 (int64)."""
    r = s.astype(np.int64)
    for _ in range(order):
        r = r[1:] - r[:-1]
    return r


def _bitlen(v: int) -> int:
    return int(v).bit_length()


def plan_partitions(u: np.ndarray, n: int, order: int):
    """(partition order, [(parameter or 15, escape width)], total bits of the partitions with their 4 / 9 header bits) for the zigzag residuals u."""
    best = None
    for po in range(MAX_PARTITION_ORDER + 1):
        if n % (1 << po) or (n >> po) <= order:
            break
        psz, total, plan = n >> po, 0, []
        for p in range(1 << po):
            a = u[max(p * psz - order, 0):(p + 1) * psz - order]
            cnt = len(a)
            k_best, b_best = 0, None
            for k in range(MAX_RICE + 1):
                b = 4 + cnt * (k + 1) + int((a >> k).sum())
                if b_best is None or b < b_best:
                    k_best, b_best = k, b
            w = _bitlen(int(a.max()))          # the signed width of the residuals: the bit length of the largest zigzag value (0: all zero)
            esc = 4 + 5 + cnt * w
            if esc < b_best:
                plan.append((15, w)); total += esc
            else:
                plan.append((k_best, 0)); total += b_best
        if best is None or total < best[2]:
            best = (po, plan, total)
    return best


class _Bits:
    def __init__(self, nbits_hint):
        self.pos, self.val, self.len = [], [], []
        self.at = 0

    def put(self, v, n):
        self.pos.append(np.asarray([self.at], np.int64)); self.val.append(np.asarray([v], np.int64)); self.len.append(np.asarray([n], np.int64))
        self.at += n

    def put_many(self, skip, v, n):
        """items i: skip[i] zero bits, then v[i] in n[i] bits"""
        adv = skip + n
        end = self.at + np.cumsum(adv)
        self.pos.append(end - n); self.val.append(v); self.len.append(n)
        self.at = int(end[-1]) if len(end) else self.at

    def bytes(self):
        nbytes = (self.at + 7) // 8
        bits = np.zeros(nbytes * 8, np.uint8)
        pos, val, ln = np.concatenate(self.pos), np.concatenate(self.val), np.concatenate(self.len)
        for b in range(int(ln.max()) if len(ln) else 0):
            m = ln > b
            bits[pos[m] + ln[m] - 1 - b] = (val[m] >> b) & 1
        return np.packbits(bits).tobytes()


def encode_frame(s: np.ndarray, frame_no: int, rate: int):
    s = np.asarray(s, np.int64)
    n = len(s)
    assert 1 <= n <= BLOCK
    head = frame_header(frame_no, n, rate)
    bw = _Bits(0)
    for b in head:
        bw.put(b, 8)
    code, po = 1, 0
    if np.all(s == s[0]):
        code = 0
        bw.put(0, 8)
        bw.put(int(s[0]) & 0xFFFF, 16)
    else:
        sums = [int(np.abs(residuals(s, o)).sum()) for o in range(min(4, n - 1) + 1)]
        order = int(np.argmin(sums))           # the first minimum: ties go to the lower order
        r = residuals(s, order)
        u = (r << 1) ^ (r >> 63)
        po_f, plan, total = plan_partitions(u, n, order)
        if 8 + 16 * order + 6 + total < 8 + 16 * n:
            code, po = 8 + order, po_f
            bw.put(code << 1, 8)
            for v in s[:order]:
                bw.put(int(v) & 0xFFFF, 16)
            bw.put(po, 6)                      # coding method 00, then the partition order
            psz = n >> po
            for p, (k, w) in enumerate(plan):
                a_u = u[max(p * psz - order, 0):(p + 1) * psz - order]
                a_r = r[max(p * psz - order, 0):(p + 1) * psz - order]
                bw.put(k, 4)
                if k == 15:
                    bw.put(w, 5)
                    if w:
                        bw.put_many(np.zeros(len(a_r), np.int64), a_r & ((1 << w) - 1), np.full(len(a_r), w, np.int64))
                else:
                    bw.put_many(a_u >> k, (1 << k) | (a_u & ((1 << k) - 1)), np.full(len(a_u), k + 1, np.int64))
        else:
            bw.put(1 << 1, 8)
            bw.put_many(np.zeros(n, np.int64), s & 0xFFFF, np.full(n, 16, np.int64))
    body = bw.bytes()
    c = _crc16_fast(body)
    out = body + bytes([c >> 8, c & 0xFF])
    return out, [code, po, len(out), c]


def encode_frames(s16, rate: int):
    s = np.asarray(s16).reshape(-1)
    assert rate in RATE_CODE and len(s) >= 1 and s.dtype == np.int16
    return [encode_frame(s[f:f + BLOCK], f // BLOCK, rate) for f in range(0, len(s), BLOCK)]


def stream_header(n: int, rate: int, min_frame: int, max_frame: int) -> bytes:
    """The 42 bytes the host writes: the marker and one STREAMINFO block marked last; the MD5 field is all zeros, which the format defines as not computed."""
    info = BLOCK.to_bytes(2, "big") * 2                            # min and max block size: 4096 whatever the length of the last frame
    info += min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
    info += ((rate << 44) | (0 << 41) | (15 << 36) | n).to_bytes(8, "big") + bytes(16)
    assert len(info) == 34
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info


def encode(s16, rate: int) -> bytes:
    frames = encode_frames(s16, rate)
    sizes = [len(f) for f, _ in frames]
    return stream_header(len(np.asarray(s16).reshape(-1)), rate, min(sizes), max(sizes)) + b"".join(f for f, _ in frames)


# ---- the decoder: written from the format, not from the encoder above --------------------------------------------------------------------------------------
class _Reader:
    def __init__(self, data: bytes, at: int = 0):
        self.d, self.byte, self.acc, self.have = data, at, 0, 0

    def bits(self, n: int) -> int:
        while self.have < n:
            self.acc = (self.acc << 8) | self.d[self.byte]; self.byte += 1; self.have += 8
        self.have -= n
        v = (self.acc >> self.have) & ((1 << n) - 1)
        self.acc &= (1 << self.have) - 1
        return v

    def signed(self, n: int) -> int:
        if n == 0:
            return 0
        v = self.bits(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self) -> int:
        q = 0
        while self.bits(1) == 0:
            q += 1
        return q

    def align(self):
        self.acc, self.have = 0, 0


_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
_DEC_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}


def decode(data: bytes):
    assert data[:4] == b"fLaC", "no marker"
    at, info = 4, None
    while True:
        last, kind, size = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        body = data[at + 4:at + 4 + size]
        at += 4 + size
        if kind == 0:
            assert size == 34
            x = int.from_bytes(body[10:18], "big")
            info = dict(min_block=int.from_bytes(body[0:2], "big"), max_block=int.from_bytes(body[2:4], "big"), min_frame=int.from_bytes(body[4:7], "big"),
                        max_frame=int.from_bytes(body[7:10], "big"), rate=x >> 44, channels=((x >> 41) & 7) + 1, bps=((x >> 36) & 31) + 1,
                        total=x & ((1 << 36) - 1), md5=body[18:34])
        if last:
            break
    assert info is not None and info["channels"] == 1 and info["bps"] == 16
    out, expect_no, sizes = [], 0, []
    while at < len(data):
        start = at
        rd = _Reader(data, at)
        assert rd.bits(14) == 0x3FFE and rd.bits(1) == 0, "no frame sync"
        assert rd.bits(1) == 0, "fixed block size strategy expected"
        bs_code, sr_code, ch, ss = rd.bits(4), rd.bits(4), rd.bits(4), rd.bits(3)
        assert rd.bits(1) == 0 and ch == 0 and ss == 0b100
        first = rd.bits(8)
        extra = 0
        while first & (0x80 >> extra):
            extra += 1
        no = first & (0xFF >> (extra + 1)) if extra else first
        for _ in range(max(extra - 1, 0)):
            c = rd.bits(8)
            assert c >> 6 == 2
            no = (no << 6) | (c & 0x3F)
        assert no == expect_no, "frame numbers count up from zero"
        expect_no += 1
        if bs_code == 1:
            n = 192
        elif 2 <= bs_code <= 5:
            n = 576 << (bs_code - 2)
        elif bs_code == 6:
            n = rd.bits(8) + 1
        elif bs_code == 7:
            n = rd.bits(16) + 1
        else:
            assert bs_code >= 8
            n = 256 << (bs_code - 8)
        if sr_code == 0:
            rate = info["rate"]
        elif sr_code == 12:
            rate = rd.bits(8) * 1000
        elif sr_code == 13:
            rate = rd.bits(16)
        elif sr_code == 14:
            rate = rd.bits(16) * 10
        else:
            rate = _DEC_RATES[sr_code]
        assert rate == info["rate"]
        assert crc8(data[start:rd.byte]) == rd.bits(8), "CRC-8 of the frame header"
        assert rd.bits(1) == 0
        kind = rd.bits(6)
        assert rd.bits(1) == 0, "no wasted bits in these streams"
        if kind == 0:
            s = [rd.signed(16)] * n
        elif kind == 1:
            s = [rd.signed(16) for _ in range(n)]
        else:
            assert 8 <= kind <= 12, "subframe type"
            order = kind - 8
            s = [rd.signed(16) for _ in range(order)]
            assert rd.bits(2) == 0, "4-bit Rice parameters"
            po = rd.bits(4)
            assert n % (1 << po) == 0 and (n >> po) > order - 1
            res = []
            for p in range(1 << po):
                cnt = (n >> po) - (order if p == 0 else 0)
                k = rd.bits(4)
                if k == 15:
                    w = rd.bits(5)
                    res += [rd.signed(w) for _ in range(cnt)]
                else:
                    for _ in range(cnt):
                        q = rd.unary()
                        v = (q << k) | rd.bits(k) if k else q
                        res.append((v >> 1) ^ -(v & 1))
            c = _FIXED[order]
            for r in res:
                s.append(r + sum(cj * s[-1 - j] for j, cj in enumerate(c)))
        rd.align()
        got = int.from_bytes(data[rd.byte:rd.byte + 2], "big")
        assert _crc16_fast(data[start:rd.byte]) == got, "CRC-16 of the frame"
        at = rd.byte + 2
        sizes.append(at - start)
        assert all(-32768 <= v <= 32767 for v in s)
        out += s
    assert len(out) == info["total"], "STREAMINFO's sample count"
    assert info["min_frame"] == min(sizes) and info["max_frame"] == max(sizes)
    assert info["min_block"] == info["max_block"] == BLOCK
    assert info["md5"] == bytes(16)
    return np.asarray(out, np.int16), info["rate"]


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------------------------------------
# around the predictor orders, the partition orders and the frame edges: orders limited by the block size (1 .. 5), 15 / 16 / 17 and 255 / 256 (which
# partition orders divide the block), a frame less one sample, a whole frame, a frame and one sample, two frames, three frames and one sample
LENGTHS = (1, 2, 4, 5, 15, 16, 17, 255, 256, 4095, 4096, 4097, 8192, 12289)
KINDS = ("silence", "constant", "alternating", "ramp", "white", "small_noise", "sine_click", "loud_first_partition")


def signal(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """n int16 samples: silence; a constant; +-32767 in turn (the order-4 residual passes 16 bits); a ramp that starts again with every frame (order 2 is
    exact); white noise at full scale (VERBATIM); noise in -3 .. 3 (small parameters); a sine with one click (mixed parameters across the partitions); a
    frame whose first sixteenth is loud and the rest silent."""
    t = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng([18, seed, n, KINDS.index(kind)])
    if kind == "silence":
        x = np.zeros(n, np.int64)
    elif kind == "constant":
        x = np.full(n, -1234, np.int64)
    elif kind == "alternating":
        x = np.where(t % 2 == 0, 32767, -32767)
    elif kind == "ramp":
        x = (t % BLOCK) * 7 - 14000
    elif kind == "white":
        x = rng.integers(-32768, 32768, n)
    elif kind == "small_noise":
        x = rng.integers(-3, 4, n)
    elif kind == "sine_click":
        x = np.round(8000.0 * np.sin(t * 0.05)).astype(np.int64)
        x[n // 2] = 32767
    else:
        assert kind == "loud_first_partition"
        x = np.zeros(n, np.int64)
        k = np.flatnonzero(t % BLOCK < max(min(n, BLOCK) // 16, 1))
        x[k] = rng.integers(-20000, 20001, len(k))
    return x.astype(np.int16)
