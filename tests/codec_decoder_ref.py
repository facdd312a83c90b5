"""numpy restatement of the EnCodec 24 kHz decoder (HF modeling_encodec.py: EncodecResidualVectorQuantizer.decode, EncodecConv1d / _pad1d,
EncodecConvTranspose1d, EncodecResnetBlock, EncodecLSTM, EncodecDecoder) on the tensors of a model file - the reference of the codec decoder's tests.
Everything in f32; the convolution, its padding, the ELU and the LSTM are tests/codec_encoder_ref.py's.

  convtr1d        the causal transposed convolution: weight [cin][cout][2 s], the full output of (T - 1) s + K columns trimmed by K - s on the right
  decode          codes [n_q][T] -> (pcm [320 T], taps): taps[0] first conv, [1] LSTM + skip, [2..5] the four up-sampling blocks - all [C][T'], as the
                  engine and the oracle hand them out
  pad1d_without_extension / decode(..., pad=...)
                  the padding rule WITHOUT its short-input detour (reflection where numpy defines it, the edge value otherwise): the wrong decoder of the
                  blindness check
"""
import numpy as np

import codec_encoder_ref as enc

RATIOS = (8, 5, 4, 2)
codec_tensors, codebooks = enc.codec_tensors, enc.codebooks


def convtr1d(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride: int) -> np.ndarray:
    """EncodecConvTranspose1d.forward (causal, trim_right_ratio 1): x [cin][T], w [cin][cout][K] -> [cout][T stride]"""
    cin, cout, K = w.shape
    T = x.shape[1]
    full = np.zeros((cout, (T - 1) * stride + K), np.float32)
    for k in range(K):
        full[:, k:k + (T - 1) * stride + 1:stride] += w[:, :, k].T.astype(np.float32) @ x.astype(np.float32)
    full = full + np.reshape(b, (cout, 1))
    return full[:, :full.shape[1] - (K - stride)].astype(np.float32)


def pad1d_without_extension(x: np.ndarray, left: int, right: int) -> np.ndarray:
    """reflect padding that skips _pad1d's zero-extension of a short input: plain reflection where it is defined, the edge value otherwise"""
    mode = "reflect" if x.shape[-1] > max(left, right) else "edge"
    return np.pad(x, [(0, 0)] * (x.ndim - 1) + [(left, right)], mode=mode)


def _conv1d(x, w, b, pad):
    """EncodecConv1d.forward at stride 1 with the given padding rule; the one-channel last convolution stores a 0-d bias"""
    cout, cin, K = w.shape
    b = np.reshape(np.asarray(b, np.float32), (-1,)) * np.ones(cout, np.float32)
    if pad is enc.pad1d:
        return enc.conv1d(x, w, b)
    xp = pad(x, K - 1, 0)
    cols = np.stack([xp[:, k:k + x.shape[1]] for k in range(K)], axis=1)
    return (w.reshape(cout, cin * K) @ cols.reshape(cin * K, -1) + b[:, None]).astype(np.float32)


def decode(tens, codes, pad=enc.pad1d):
    """codes [n_q][T] -> (pcm [320 T], taps[0..5])"""
    codes = np.asarray(codes)
    n_q, T = codes.shape
    cbs = enc.codebooks(tens, n_q)

    def cv(name, x):
        return _conv1d(x, tens[name + ".weight"], tens[name + ".bias"], pad)
    z = np.zeros((T, cbs.shape[2]), np.float32)
    for q in range(n_q):
        z = z + cbs[q][codes[q]]
    x = cv("decoder.model.0.conv.conv", z.T)
    taps = [x]
    x = enc.lstm2(x, tens, "decoder.model.1.lstm") + x
    taps.append(x)
    idx = 3
    for ratio in RATIOS:
        name = f"decoder.model.{idx}.convtr.convtr"
        x = convtr1d(enc.elu(x), tens[name + ".weight"], tens[name + ".bias"], ratio)
        h = cv(f"decoder.model.{idx + 1}.block.1.conv.conv", enc.elu(x))
        h = cv(f"decoder.model.{idx + 1}.block.3.conv.conv", enc.elu(h))
        x = cv(f"decoder.model.{idx + 1}.shortcut.conv.conv", x) + h
        taps.append(x)
        idx += 3
    pcm = cv(f"decoder.model.{idx}.conv.conv", enc.elu(x))
    assert pcm.shape == (1, 320 * T)
    return pcm[0], taps
