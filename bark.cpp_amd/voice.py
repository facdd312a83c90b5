"""Voice prompts (speaker history, rule C10v of DESIGN.md section 3) for the MI355X Bark engine.

A voice prompt is three id arrays, time-major like every [T][2] / [T][8] array of the C API:
    semantic [n_sem]  ids in [0, 10000)      coarse [Tc][2]  ids in [0, 1024)      fine [Tf][8]  ids in [0, 1024)

File format (`save` / `load`; also read by bark_batch_server --voice name=file), little-endian:
    bytes 0..3   magic "BVP1"
    3 x int32    n_sem, Tc, Tf
    int32 arrays semantic [n_sem], coarse [Tc][2], fine [Tf][8], back to back
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"BVP1"


class VoicePrompt:
    def __init__(self, semantic, coarse, fine):
        self.semantic = np.ascontiguousarray(semantic, dtype=np.int32).reshape(-1)
        self.coarse = np.ascontiguousarray(coarse, dtype=np.int32).reshape(-1, 2)
        self.fine = np.ascontiguousarray(fine, dtype=np.int32).reshape(-1, 8)

    def __eq__(self, other):
        return (isinstance(other, VoicePrompt) and np.array_equal(self.semantic, other.semantic) and np.array_equal(self.coarse, other.coarse)
                and np.array_equal(self.fine, other.fine))

    def __repr__(self):
        return f"VoicePrompt(n_sem={len(self.semantic)}, Tc={len(self.coarse)}, Tf={len(self.fine)})"

    def save(self, path: str):
        save(self, path)


def from_npz(path: str) -> VoicePrompt:
    """A Suno speaker preset: `semantic_prompt` [n], `coarse_prompt` [2][T], `fine_prompt` [8][T] - codebook-major, transposed here."""
    with np.load(path) as z:
        return VoicePrompt(z["semantic_prompt"], np.asarray(z["coarse_prompt"]).T, np.asarray(z["fine_prompt"]).T)


def save(voice: VoicePrompt, path: str):
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<3i", len(voice.semantic), len(voice.coarse), len(voice.fine)))
        for a in (voice.semantic, voice.coarse, voice.fine):
            f.write(np.ascontiguousarray(a, dtype="<i4").tobytes())


def load(path: str) -> VoicePrompt:
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 16 or data[:4] != MAGIC:
        raise ValueError(f"{path}: not a voice prompt file (magic {MAGIC!r} expected)")
    n_sem, tc, tf = struct.unpack_from("<3i", data, 4)
    if min(n_sem, tc, tf) < 0 or len(data) != 16 + 4 * (n_sem + 2 * tc + 8 * tf):
        raise ValueError(f"{path}: counts {n_sem}, {tc}, {tf} do not match the file size {len(data)}")
    a = np.frombuffer(data, dtype="<i4", offset=16)
    return VoicePrompt(a[:n_sem], a[n_sem:n_sem + 2 * tc].reshape(tc, 2), a[n_sem + 2 * tc:].reshape(tf, 8))


def from_generation(ctx) -> VoicePrompt:
    """The token streams of the context's last bark_generate_audio call as the next utterance's voice prompt (long-form continuation: feed
    every utterance the one before it)."""
    v = VoicePrompt(ctx.semantic_tokens(), ctx.coarse_tokens(), ctx.fine_tokens())
    if not len(v.semantic) or not len(v.coarse):
        raise ValueError("from_generation: the context holds no generation")
    return v


def resample_24k_to_16k(pcm) -> np.ndarray:
    """24 kHz -> 16 kHz (ratio 2 / 3), polyphase, in numpy: output sample m sits at input time t = 1.5 m and is
        y[m] = sum_j x[j] h(t - j),   h(u) = c sinc(c u) w(u),   c = 0.99 * 2 / 3 (cut-off at 0.99 of the new Nyquist frequency, in cycles per input sample),
        w(u) = cos^2(pi u / (2 W)) for |u| < W, else 0 (Hann),   W = 6 / c input samples (6 zero crossings of the sinc on either side),
    over the input samples with |t - j| < W; samples outside the recording are zero.  Even m take the taps of phase 0, odd m those of phase 1/2.  The output
    has ceil(2 n / 3) samples."""
    x = np.ascontiguousarray(pcm, dtype=np.float64).reshape(-1)
    n = len(x)
    n_out = (2 * n + 2) // 3
    c = 0.99 * 2.0 / 3.0
    W = 6.0 / c
    half = int(np.ceil(W)) + 1
    out = np.zeros(n_out, np.float64)
    xp = np.concatenate([np.zeros(half), x, np.zeros(half + 2)])
    for phase in (0, 1):                                  # t = 1.5 m: integer for even m, integer + 1/2 for odd m
        m = np.arange(phase, n_out, 2)
        if not len(m):
            continue
        base = (3 * m) // 2                               # floor(t)
        frac = 0.5 * phase
        j = np.arange(-half + 1, half + 1)                # taps at floor(t) + j
        u = frac - j
        h = c * np.sinc(c * u) * np.where(np.abs(u) < W, np.cos(np.pi * u / (2.0 * W)) ** 2, 0.0)
        idx = base[:, None] + j[None, :] + half
        out[m] = xp[idx] @ h
    return out.astype(np.float32)


def from_audio(ctx, pcm, semantic=None) -> VoicePrompt:
    """A voice prompt from a recording of the speaker (24 kHz mono float samples): the coarse and fine streams are the first 2 / 8 codebooks of the
    EnCodec encoder's codes (ctx.codec_encode; the model file must carry the encoder).  The semantic ids are the caller's when given; with None the
    recording is resampled to 16 kHz (resample_24k_to_16k) and run through the context's semantic encoder (ctx.load_semantic_encoder: HuBERT and its token
    head, rule C12h) - ValueError when none is loaded."""
    if semantic is None:
        if not ctx.has_semantic_encoder():
            raise ValueError("from_audio: no semantic ids given and no semantic encoder loaded (ctx.load_semantic_encoder)")
        semantic = ctx.semantic_encode(resample_24k_to_16k(pcm))
    codes = ctx.codec_encode(pcm, 8)                  # [8][T]
    return VoicePrompt(semantic, codes[:2].T, codes[:8].T)


def from_audio_native(ctx, pcm, rate: int = 24000) -> VoicePrompt:
    """The same voice prompt made by ONE native call (ctx.voice_from_audio, bark_hip_voice_from_audio): the resampler runs on the device in f32 under rule
    C13r instead of resample_24k_to_16k above, so the semantic ids may differ from from_audio's on undecided frames; a recording longer than 20 s is used
    from its last 480 000 samples on.  rate: the recording's own rate - one of 8000, 12000, 16000, 22050, 32000, 44100, 48000 is brought to 24 kHz first by
    ctx.resample (rule C14r, bark_hip_resample).  ValueError where a call refuses."""
    if rate != 24000:
        pcm = ctx.resample(pcm, rate, 24000)
    return VoicePrompt(*ctx.voice_from_audio(pcm))
