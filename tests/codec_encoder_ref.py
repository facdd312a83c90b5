"""numpy restatement of the EnCodec 24 kHz encoder (HF modeling_encodec.py: EncodecConv1d / _pad1d, EncodecResnetBlock, EncodecLSTM, EncodecEncoder,
EncodecResidualVectorQuantizer.encode) on the tensors of a model file - the reference of the codec encoder's tests.  Everything in f32.

  pad1d            EncodecConv1d's causal reflect padding, restated the way HF builds it: an array that is padded, reflected and cut
  encode_latent    PCM [n] -> latent [H][T] and the activations the engine's taps hand out
  rvq_c11q         rule C11q: d_j = sum_d (r_d - e_jd)^2 as t = r_d - e_jd; p = t * t; acc = acc + p over d ascending, every
                   operation rounded to f32; argmin with ties to the lowest j; r <- r - e_j.  Bit for bit what rvq_encode_kernel computes.
  hf_margins       per frame and stage the f64 gap between the two smallest squared distances along HF's own greedy path (the decision rule of G2)
  decided_frames   G2's rule: the frames whose codes a latent deviating from HF's cannot flip
  write_tie_model / tie_latents / midpoint_latents / stage0_pick
                   the adversarial inputs of C11q (exact ties, midpoints of two rows, scaled midpoints) and the stage-0 loop in the stated order and in the
                   two orders a wrong kernel would most likely use (fused multiply-add, d descending)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RATIOS = (2, 4, 5, 8)
FIXTURE_LENGTHS = {"toy_enc": (1, 7, 319, 320, 321, 977, 24000), "small": (977, 24000)}


def fixture_signal(n: int) -> np.ndarray:
    """0.4 sin(2 pi 220 t) + 0.2 sin(2 pi 1333 t + 1) + 0.1 N(0, 1), default_rng(5); the first n samples of one 24000-sample draw"""
    t = np.arange(24000, dtype=np.float64) / 24000.0
    x = 0.4 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1333 * t + 1) + 0.1 * np.random.default_rng(5).standard_normal(24000)
    return x[:n].astype(np.float32)


def codec_tensors(path: str):
    """(hparams, {name: f32 array in torch order}) of the codec section"""
    from tools.make_hf_golden import read_model_file
    hp, tens = read_model_file(path)["codec"]
    return hp, {k: np.asarray(v, dtype=np.float32) for k, v in tens.items()}


def codebooks(tens, n_q: int) -> np.ndarray:
    return np.stack([tens[f"quantizer.vq.layers.{q}._codebook.embed"] for q in range(n_q)]).astype(np.float32)


def pad1d(x: np.ndarray, left: int, right: int) -> np.ndarray:
    """_pad1d(mode='reflect') on the last axis: an input not longer than the larger pad gets zeros appended first, and as many elements are cut off
    the END of the padded array afterwards"""
    L = x.shape[-1]
    extra = 0
    if L <= max(left, right):
        extra = max(left, right) - L + 1
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (extra,), x.dtype)], axis=-1)
    padded = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(left, right)], mode="reflect")
    return padded[..., :padded.shape[-1] - extra]


def conv1d(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride: int = 1) -> np.ndarray:
    """EncodecConv1d.forward (causal): x [cin][L], w [cout][cin][K] -> [cout][ceil(L / stride)]"""
    cout, cin, K = w.shape
    L = x.shape[1]
    n_out = -(-L // stride)
    xp = pad1d(x, K - stride, n_out * stride - L)
    assert xp.shape[1] == (n_out - 1) * stride + K
    cols = np.stack([xp[:, k:k + (n_out - 1) * stride + 1:stride] for k in range(K)], axis=1)      # [cin][K][n_out]
    y = w.reshape(cout, cin * K).astype(np.float32) @ cols.reshape(cin * K, n_out).astype(np.float32)
    return (y + np.reshape(b, (cout, 1))).astype(np.float32)


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0).astype(np.float64))).astype(np.float32)


def _sigmoid(x):
    return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)


def lstm2(x: np.ndarray, tens, prefix: str) -> np.ndarray:
    """nn.LSTM with two layers (gate order i, f, g, o) over x [D][T]; returns the second layer's outputs [D][T] (the skip is the caller's)"""
    seq = x.T.astype(np.float32)
    for layer in range(2):
        w_ih, w_hh = tens[f"{prefix}.weight_ih_l{layer}"], tens[f"{prefix}.weight_hh_l{layer}"]
        bias = tens[f"{prefix}.bias_ih_l{layer}"] + tens[f"{prefix}.bias_hh_l{layer}"]
        D = w_hh.shape[1]
        gi = seq @ w_ih.T + bias
        h = np.zeros(D, np.float32); c = np.zeros(D, np.float32)
        out = np.zeros_like(seq)
        for t in range(len(seq)):
            g = gi[t] + w_hh @ h
            i_t, f_t, o_t = _sigmoid(g[:D]), _sigmoid(g[D:2 * D]), _sigmoid(g[3 * D:])
            g_t = np.tanh(g[2 * D:3 * D].astype(np.float64)).astype(np.float32)
            c = f_t * c + i_t * g_t
            h = o_t * np.tanh(c.astype(np.float64)).astype(np.float32)
            out[t] = h
        seq = out
    return seq.T


def encode_latent(tens, pcm: np.ndarray):
    """-> (latent [H][T], taps): taps[0] first conv, [1..4] after each down-sampling conv, [5] LSTM + skip, [6] the latent - all [C][T']"""
    def cv(name, x, stride=1):
        return conv1d(x, tens[name + ".weight"], tens[name + ".bias"], stride)
    x = cv("encoder.model.0.conv.conv", np.asarray(pcm, np.float32).reshape(1, -1))
    taps = [x]
    idx = 1
    for ratio in RATIOS:
        h = cv(f"encoder.model.{idx}.block.1.conv.conv", elu(x))
        h = cv(f"encoder.model.{idx}.block.3.conv.conv", elu(h))
        x = cv(f"encoder.model.{idx}.shortcut.conv.conv", x) + h
        x = cv(f"encoder.model.{idx + 2}.conv.conv", elu(x), ratio)
        taps.append(x)
        idx += 3
    x = lstm2(x, tens, f"encoder.model.{idx}.lstm") + x
    taps.append(x)
    z = cv(f"encoder.model.{idx + 2}.conv.conv", elu(x))
    taps.append(z)
    return z, taps


def rvq_c11q(latents_TxH: np.ndarray, cbs: np.ndarray, n_q: int) -> np.ndarray:
    """C11q: latents [T][H] f32, codebooks [>= n_q][bins][H] f32 -> codes [n_q][T] int32"""
    r = np.array(latents_TxH, dtype=np.float32, copy=True)
    T, H = r.shape
    codes = np.zeros((n_q, T), np.int32)
    for q in range(n_q):
        e = cbs[q].astype(np.float32)
        acc = np.zeros((T, e.shape[0]), np.float32)
        for d in range(H):
            t = r[:, d, None] - e[None, :, d]      # f32 - f32 -> f32: one rounding
            p = t * t
            acc = acc + p
        j = np.argmin(acc, axis=1)                 # the first of equal minima: the lowest j
        codes[q] = j
        r = r - e[j]
    return codes


def hf_margins(latents_TxH: np.ndarray, cbs: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """[n_q][T] f64: second-smallest minus smallest squared distance at every stage, the residual following `codes` (HF's own picks)"""
    r = np.asarray(latents_TxH, np.float64).copy()
    n_q = codes.shape[0]
    out = np.zeros((n_q, len(r)))
    for q in range(n_q):
        e = cbs[q].astype(np.float64)
        d = (r * r).sum(1)[:, None] - 2.0 * (r @ e.T) + (e * e).sum(1)[None]
        s = np.sort(d, axis=1)
        out[q] = s[:, 1] - s[:, 0]
        r = r - e[codes[q]]
    return out


def decided_frames(z_TxH: np.ndarray, z_hf_TxH: np.ndarray, cbs: np.ndarray, codes_hf: np.ndarray) -> np.ndarray:
    """[T] bool: a frame is decided when at every stage HF's margin exceeds 4 |z[t] - z_hf[t]|_2 max_j |e_qj| - the deviation of z from HF's latent cannot
    flip one of its picks, so it must carry HF's codes"""
    margins = hf_margins(z_hf_TxH, cbs, codes_hf)                                           # [n_q][T]
    enorm = np.sqrt((cbs.astype(np.float64) ** 2).sum(-1)).max(-1)                          # [n_q]
    delta = np.sqrt(((np.asarray(z_TxH, np.float64) - z_hf_TxH) ** 2).sum(-1))              # [T]
    return (margins > 4.0 * delta[None, :] * enorm[:len(margins), None]).all(0)


# ---- adversarial inputs of C11q ---------------------------------------------------------------------------------------------------------------------
# (low row, its copy): both in one work-item of rvq_encode_kernel (j, j + 256), in neighbouring lanes, in different waves, the last row and a low one
TIE_PAIRS = ((10, 266), (20, 21), (30, 94), (5, 1023))
TIE_BOOKS = (0, 3)


def write_tie_model(src: str, dst: str) -> np.ndarray:
    """copy of a model file in which, in the codebooks TIE_BOOKS, the second row of every TIE_PAIRS entry is overwritten with the first; returns the
    patched codebooks [8][bins][H]"""
    import model_patch
    buf = bytearray(open(src, "rb").read())
    info = model_patch.walk(buf)["codec"]
    for q in TIE_BOOKS:
        t = info[f"quantizer.vq.layers.{q}._codebook.embed"]
        ttype = int(np.frombuffer(buf, "<i4", 1, t["ttype_off"])[0])
        assert ttype == 0 and len(t["dims"]) == 2, (ttype, t["dims"])               # f32 [bins][H]: dims = (H, bins)
        H, bins = t["dims"]
        assert t["end"] - t["data_off"] == 4 * H * bins and bins > max(max(p) for p in TIE_PAIRS)
        for lo, hi in TIE_PAIRS:
            a, b = t["data_off"] + 4 * H * lo, t["data_off"] + 4 * H * hi
            buf[b:b + 4 * H] = buf[a:a + 4 * H]
    tmp = dst + ".tmp%d" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(buf)
    os.replace(tmp, dst)
    return codebooks(codec_tensors(dst)[1], 8)


def tie_latents(cbs: np.ndarray) -> np.ndarray:
    """[17][H] latents on the codebooks of write_tie_model: for every duplicated row of codebook 0 the row itself (both distances 0) and the row plus
    N(0, 0.01) noise (equal non-zero distances); the same for codebook 3 behind random rows of codebooks 0 - 2, so that the tie arises at stage 3; the
    all-zero latent"""
    rng = np.random.default_rng(77)
    H = cbs.shape[2]
    out = []
    for lo, _ in TIE_PAIRS:
        out.append(cbs[0][lo].copy())
        out.append((cbs[0][lo] + 0.01 * rng.standard_normal(H)).astype(np.float32))
    for lo, _ in TIE_PAIRS:
        head = ((cbs[0][rng.integers(100, 1000)] + cbs[1][rng.integers(0, 1024)]) + cbs[2][rng.integers(0, 1024)]).astype(np.float32)
        out.append((head + cbs[3][lo]).astype(np.float32))
        out.append((head + cbs[3][lo] + 0.01 * rng.standard_normal(H)).astype(np.float32))
    out.append(np.zeros(H, np.float32))
    return np.stack(out).astype(np.float32)


def midpoint_latents(cbs: np.ndarray, T: int, scale: float = 1.0, seed: int = 0) -> np.ndarray:
    """[T][H]: scale * f32((e_a + e_b) / 2) for pairs of stage-0 rows.  scale 1: random pairs - in exact arithmetic the latent is equally far from both
    rows, so rounding alone decides the pick, and the residual carries the decision through the later stages.  Other scales: s (e_a + e_b) / 2 differs
    in its two squared distances by (1 - s)(|e_a|^2 - |e_b|^2), so the pairs are recomputed as neighbours in the order of the rows' norms - the pairs
    for which the scaled latent stays closest to equidistant."""
    rng = np.random.default_rng(4242 + seed)
    e = cbs[0].astype(np.float32)
    if scale == 1.0:
        a = rng.integers(0, len(e), T)
        b = (a + 1 + rng.integers(0, len(e) - 1, T)) % len(e)
    else:
        order = np.argsort((e.astype(np.float64) ** 2).sum(1), kind="stable")
        k = rng.integers(0, len(e) - 1, T)
        a, b = order[k], order[k + 1]
    mid = ((e[a].astype(np.float64) + e[b].astype(np.float64)) / 2).astype(np.float32)
    return (mid * np.float32(scale)).astype(np.float32)


def stage0_pick(latents_TxH: np.ndarray, e: np.ndarray, order: str = "c11q") -> np.ndarray:
    """[T] stage-0 picks of C11q's loop ("c11q") and of the same loop with acc = f32(f64(acc) + f64(t) f64(t)) ("fused": what a fused multiply-add
    computes) or with d running downwards ("descending") - the measures of how much an input set can tell these orders apart"""
    r = np.asarray(latents_TxH, np.float32)
    e = e.astype(np.float32)
    H = r.shape[1]
    acc = np.zeros((len(r), len(e)), np.float32)
    for d in (range(H - 1, -1, -1) if order == "descending" else range(H)):
        t = r[:, d, None] - e[None, :, d]
        if order == "fused":
            t64 = t.astype(np.float64)
            acc = (acc.astype(np.float64) + t64 * t64).astype(np.float32)
        else:
            acc = acc + t * t
    return np.argmin(acc, axis=1)
