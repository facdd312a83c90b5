"""Rule C12h restated with torch on the CPU, in f32: the semantic encoder - HuBERT's feature encoder, projection, positional convolution
and first `output_layer` post-norm layers, then the token head (two LSTM layers, a linear layer, argmax) - reading the file tools/convert_hubert.py writes.
Plain tensor operations only (no nn.Module of HuggingFace, no nn.LSTM): what the engine's kernels are checked against, itself pinned to HuggingFace by
tests/test_semantic_encoder_ref.py.  `f16=True` rounds the input rows of every convolution, linear layer and LSTM product to f16 (the weights of the file
already are f16 values): the reference's own sensitivity to the engine's number formats.

Also here: the fixture signal (a formula, not a file) and the helpers the fixture generator and the tests share."""
from __future__ import annotations

import struct

import numpy as np
import torch
import torch.nn.functional as tf

MAGIC = 0x68756273
HPARAM_NAMES = ("C", "H", "n_head", "F", "n_layer_stored", "output_layer", "pos_kernel", "pos_groups", "D", "n_classes", "ftype")
TOY_LENGTHS = (400, 719, 720, 1040, 16000)
BASE_LENGTHS = (16000, 48000)
TAPS = ("conv0", "conv", "proj", "h0", "hL", "logits")      # stages 0..5 of bark_hip_semantic_encode_tap
CONV_STRIDES = (5, 2, 2, 2, 2, 2, 2)


def fixture_signal(n: int, seed: int = 0) -> np.ndarray:
    """n samples at 16 kHz: a chirp 100 Hz -> 3.5 kHz over 3 s (amplitude 0.4, modulated at 3 Hz), a 440 Hz tone (0.2) and seeded Gaussian noise (0.05).
    A prefix of a longer signal is the shorter signal."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    phase = 2.0 * np.pi * (100.0 * t + (3400.0 / 6.0) * t * t)
    x = 0.4 * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t)) * np.sin(phase) + 0.2 * np.sin(2.0 * np.pi * 440.0 * t)
    x += 0.05 * np.random.default_rng([seed, 12]).standard_normal(max(n, 48000))[:n]
    return x.astype(np.float32)


def frame_count(n: int) -> int:
    if n < 400:
        raise ValueError("a recording needs at least 400 samples")
    return (n - 400) // 320 + 1


def load(path: str):
    """-> (hparams dict, {name: f32 torch tensor})."""
    with open(path, "rb") as f:
        data = f.read()
    if struct.unpack_from("<I", data, 0)[0] != MAGIC:
        raise ValueError("not a semantic encoder file")
    hp = dict(zip(HPARAM_NAMES, struct.unpack_from("<11i", data, 4)))
    pos, W = 48, {}
    while pos < len(data):
        n_dims, name_len, ttype = struct.unpack_from("<3i", data, pos); pos += 12
        dims = struct.unpack_from(f"<{n_dims}i", data, pos); pos += 4 * n_dims
        name = data[pos:pos + name_len].decode(); pos += name_len
        count = int(np.prod(dims))
        a = np.frombuffer(data, dtype="<f2" if ttype == 1 else "<f4", count=count, offset=pos).astype(np.float32).reshape(tuple(reversed(dims)))
        pos += count * (2 if ttype == 1 else 4)
        W[name] = torch.from_numpy(a.copy())
    return hp, W


def _r(x, f16):
    return x.half().float() if f16 else x


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _ln(x, g, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * g + b


def head(hp, W, feats, f16: bool = False):
    """feats [T][H] -> (logits [T][n_classes], ids [T]): LSTM(H -> D, 2 layers, gates i f g o, zero state), Linear, argmax (ties: the lowest id)."""
    D = hp["D"]
    x = torch.as_tensor(np.asarray(feats, dtype=np.float32))
    for l in range(2):
        wi, wh = W[f"head.lstm.weight_ih_l{l}"], W[f"head.lstm.weight_hh_l{l}"]
        bi, bh = W[f"head.lstm.bias_ih_l{l}"], W[f"head.lstm.bias_hh_l{l}"]
        gi = _r(x, f16) @ wi.T + bi
        h, c, out = torch.zeros(D), torch.zeros(D), []
        for t in range(len(x)):
            g = gi[t] + (_r(h, f16) @ wh.T + bh)
            i, f, gg, o = torch.sigmoid(g[:D]), torch.sigmoid(g[D:2 * D]), torch.tanh(g[2 * D:3 * D]), torch.sigmoid(g[3 * D:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            out.append(h)
        x = torch.stack(out)
    logits = (_r(x, f16) @ W["head.out.weight"].T + W["head.out.bias"]).numpy()
    return logits, np.argmax(logits, axis=1).astype(np.int32)


def encode(hp, W, pcm, f16: bool = False):
    """pcm [n] (16 kHz) -> ({tap name: [rows][channels] f32}, ids [T])."""
    H, nh, L = hp["H"], hp["n_head"], hp["output_layer"]
    n = len(pcm)
    T = frame_count(n)
    taps = {}
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(pcm, dtype=np.float32)).reshape(1, 1, -1)
        # feature encoder: seven valid convolutions without bias; behind the first a norm per channel over time (biased variance), erf GELU behind each
        y = tf.conv1d(_r(x, f16), W["conv0.weight"], stride=CONV_STRIDES[0])
        mean = y.mean(-1, keepdim=True)
        var = ((y - mean) ** 2).mean(-1, keepdim=True)
        y = (y - mean) / torch.sqrt(var + 1e-5) * W["conv0.norm.weight"].reshape(1, -1, 1) + W["conv0.norm.bias"].reshape(1, -1, 1)
        y = _gelu(y)
        taps["conv0"] = y[0].T
        for i in range(1, 7):
            y = _gelu(tf.conv1d(_r(y, f16), W[f"conv{i}.weight"], stride=CONV_STRIDES[i]))
        feat = y[0].T                                                       # [T][C]
        assert feat.shape[0] == T
        taps["conv"] = feat
        # projection
        proj = _r(_ln(feat, W["proj.ln.weight"], W["proj.ln.bias"]), f16) @ W["proj.weight"].T + W["proj.bias"]
        taps["proj"] = proj
        # positional convolution (padding Kp / 2; for even Kp the last output frame is dropped), GELU, residual, encoder.layer_norm
        Kp = hp["pos_kernel"]
        pc = tf.conv1d(_r(proj, f16).T.unsqueeze(0), W["pos.weight"], W["pos.bias"], padding=Kp // 2, groups=hp["pos_groups"])[0].T
        pc = pc[:T]
        hcur = _ln(proj + _gelu(pc), W["enc.ln.weight"], W["enc.ln.bias"])
        taps["h0"] = hcur
        for l in range(L):
            p = f"layers.{l}."
            qkv = _r(hcur, f16) @ W[p + "attn.qkv.weight"].T + W[p + "attn.qkv.bias"]
            q, k, v = (qkv[:, i * H:(i + 1) * H].reshape(T, nh, 64).transpose(0, 1) for i in range(3))
            att = torch.softmax((q * 0.125) @ k.transpose(1, 2), dim=-1) @ v      # [nh][T][64]
            att = att.transpose(0, 1).reshape(T, H)
            hcur = _ln(hcur + (_r(att, f16) @ W[p + "attn.out.weight"].T + W[p + "attn.out.bias"]), W[p + "ln1.weight"], W[p + "ln1.bias"])
            ff = _gelu(_r(hcur, f16) @ W[p + "fc1.weight"].T + W[p + "fc1.bias"])
            hcur = _ln(hcur + (_r(ff, f16) @ W[p + "fc2.weight"].T + W[p + "fc2.bias"]), W[p + "ln2.weight"], W[p + "ln2.bias"])
        taps["hL"] = hcur
        logits, ids = head(hp, W, hcur.numpy(), f16)
        taps["logits"] = torch.from_numpy(logits)
    return {k: v.numpy().astype(np.float32) for k, v in taps.items()}, ids


def margins(logits: np.ndarray):
    """Per frame: top-two logit margin and the two ids."""
    order = np.argsort(-logits, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(logits))
    return (logits[rows, order[:, 0]] - logits[rows, order[:, 1]]).astype(np.float32), order.astype(np.int32)


# ---- inputs of the bit-exact tests against the CPU oracle (tests/test_gpu_semantic_encoder_oracle.py; their conditions: tests/test_oracle_semantic_encoder.py) ----
# S1: every length is the smallest input that reaches the edge its test names; 2580 samples give 515 / 257 / 128 / 63 / 31 / 15 / 7 rows behind the seven convolutions
ORACLE_S1 = (400, 719, 720, 2580, 2640, 2960, 5129, 5130, 5200, 5520, 10000, 10320, 10640, 20240, 20560, 20880, 40720, 41040, 41360, 327759, 327760, 328079)
ORACLE_LONG = 327759                 # from here on tap 0 (65 550 rows and more) is not compared
ORACLE_S2_N = 5200
ORACLE_S2_SIGNALS = ("zeros", "half", "alternating")
ORACLE_S3 = (("alternating09", 328079), ("fixture", 400), ("fixture", 10000), ("fixture", 10320), ("fixture", 10640), ("fixture", 20880))
ORACLE_S4_MASKS = (512, 1, 1024)     # BARK_HIP_CROSSCHECK: attn_rows_kernel at 1024 frames, gemv_rows_kernel for the products, the convolutions' C9 chains
ORACLE_S4_LENGTHS = (720, 10640, 327760)
ORACLE_S5_T = (1, 2, 63, 64, 65, 128, 129, 1024)
ORACLE_S6 = (16000, 48000)
# The seed of fixture_signal per (preset, length): 0 unless the oracle's near-midpoint census (Oracle.near_midpoints) of seed 0 is not zero along the input's path
# - then the first seed whose census is zero, in both convolution orders where S4 runs the input in both.  Held by tests/test_oracle_semantic_encoder.py.
ORACLE_SEEDS = {("hub_toy", 41040): 1, ("hub_toy", 41360): 1, ("hub_toy", 327759): 1, ("hub_toy", 327760): 2, ("hub_base", 48000): 4}
ORACLE_HEAD_SEEDS = {}               # the same for the seeded rows of S5, per T


def oracle_signal(n: int, kind: str = "fixture", preset: str = "hub_toy") -> np.ndarray:
    if kind == "fixture":
        return fixture_signal(n, ORACLE_SEEDS.get((preset, n), 0))
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "half":
        return np.full(n, 0.5, np.float32)
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if kind == "alternating":
        return alt
    if kind == "alternating09":
        return (np.float32(0.9) * alt).astype(np.float32)
    raise ValueError(kind)


def head_rows(T: int, H: int) -> np.ndarray:
    return np.random.default_rng([7, T, ORACLE_HEAD_SEEDS.get(T, 0)]).standard_normal((T, H)).astype(np.float32)


def tie_pairs(ids: np.ndarray, n_classes: int):
    """Two (low, high, source) triples for write_tie_hubert from the ids a head picks on some rows: for the most frequent id w1 its neighbour, (w1, w1 + 1, w1) -
    neighbouring lanes of the pick; for the second most frequent id w2 the class 64 below it, (w2 - 64, w2, w2) - the same lane one trip earlier, so the frames that
    picked w2 must now answer w2 - 64 - or, for w2 < 64, (w2, w2 + 64, w2).  `source` is the class whose row both receive: the one that is picked."""
    vals, counts = np.unique(ids, return_counts=True)
    order = vals[np.argsort(-counts, kind="stable")]
    w1, w2 = int(order[0]), int(order[1])
    a = (w1, w1 + 1, w1) if w1 + 1 < n_classes and w1 + 1 != w2 else (w1 - 1, w1, w1)
    b = (w2 - 64, w2, w2) if w2 >= 64 else (w2, w2 + 64, w2)
    if len({*a[:2], *b[:2]}) != 4:
        raise ValueError(f"tie pairs collide: {a} {b}")
    return a, b


def write_tie_hubert(src: str, dst: str, pairs):
    """Copy of a semantic-encoder file with duplicated classes: for every (low, high, source) of `pairs` row `source` (one of the two) of head.out.weight and
    its entry of head.out.bias are written to both `low` and `high`, so the two classes have equal logits in every frame (as codec_encoder_ref.write_tie_model
    duplicates codebook rows)."""
    data = bytearray(open(src, "rb").read())
    pos, where = 48, {}
    while pos < len(data):
        n_dims, name_len, ttype = struct.unpack_from("<3i", data, pos); pos += 12
        dims = struct.unpack_from(f"<{n_dims}i", data, pos); pos += 4 * n_dims
        name = bytes(data[pos:pos + name_len]).decode(); pos += name_len
        es = 2 if ttype == 1 else 4
        where[name] = (pos, dims, es)
        pos += int(np.prod(dims)) * es
    wpos, wdims, wes = where["head.out.weight"]
    bpos, _, bes = where["head.out.bias"]
    D = wdims[0]
    for low, high, source in pairs:
        for dstrow in (low, high):
            data[wpos + dstrow * D * wes:wpos + (dstrow + 1) * D * wes] = data[wpos + source * D * wes:wpos + (source + 1) * D * wes]
            data[bpos + dstrow * bes:bpos + (dstrow + 1) * bes] = data[bpos + source * bes:bpos + (source + 1) * bes]
    with open(dst, "wb") as f:
        f.write(bytes(data))
