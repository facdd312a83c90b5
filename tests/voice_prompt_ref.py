"""Rule C10v restated in Python: the three stage loops of Bark with a voice prompt (speaker history), as plain loops over the CPU
oracle's EVALUATIONS - Oracle.semantic (it takes the 513-id prompt) or Oracle.gpt_eval, Oracle.gpt_eval and Oracle.fine_eval - with the oracle's own greedy
pick rule and, for temp > 0, the MT19937 / multinomial restatement of tests/nucleus_ref.py.  Independent of the engine.  The rule follows suno-ai/bark
generation.py (generate_text_semantic / generate_coarse / generate_fine with `history_prompt`) as restated in HuggingFace modeling_bark.py:570-599, 674-716,
795-850, 1158-1232.  With an empty history the loops ARE Oracle.coarse / Oracle.fine (tests/test_voice_prompt_ref.py pins that id for id).

A voice is any object with `semantic` [n_sem], `coarse` [Tc][2] and `fine` [Tf][8] (time-major), or None."""
import math

import numpy as np

from tests import nucleus_ref

SEMANTIC_VOCAB = 10000
SEMANTIC_PAD = 10000
CODEBOOK = 1024
N_COARSE = 2
N_FINE = 8
COARSE_SEMANTIC_PAD = 12048
COARSE_INFER = 12050
SEMANTIC_RATE_HZ = np.float32(49.9)
COARSE_RATE_HZ = np.float32(75.0)


class Voice:
    def __init__(self, semantic, coarse, fine):
        self.semantic = np.asarray(semantic, np.int32).reshape(-1)
        self.coarse = np.asarray(coarse, np.int32).reshape(-1, 2)
        self.fine = np.asarray(fine, np.int32).reshape(-1, 8)


def synthetic_voice(seed, n_sem, tc, tf):
    """a voice prompt of random ids (tests: no preset can be downloaded, and the rule does not care what the ids sound like)"""
    rng = np.random.default_rng(seed)
    return Voice(rng.integers(0, SEMANTIC_VOCAB, n_sem), rng.integers(0, CODEBOOK, (tc, 2)), rng.integers(0, CODEBOOK, (tf, 8)))


def ratio():
    """r = coarse_rate_hz / semantic_rate_hz * n_coarse_codebooks in float32, as the engine and the oracle compute it"""
    return np.float32(np.float32(COARSE_RATE_HZ / SEMANTIC_RATE_HZ) * np.float32(N_COARSE))


def trim(voice, max_coarse_history=630):
    """C10v.2: (kept semantic history [n_sh], kept coarse history as offset ids [n_ch - 2]); ValueError when the trimmed history is empty"""
    if voice is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    r = ratio()
    n_sem = len(voice.semantic)
    flat = (np.asarray(voice.coarse, np.int64) + SEMANTIC_VOCAB + CODEBOOK * np.arange(N_COARSE)[None, :]).reshape(-1)      # interleaved, offset
    n_sh = min(int(math.floor(np.float32(np.float32(max_coarse_history) / r))), n_sem - n_sem % 2, int(math.floor(np.float32(np.float32(len(flat)) / r))))
    n_ch = int(np.rint(np.float32(np.float32(n_sh) * r)))
    if n_sh < 2 or n_ch <= 2:
        raise ValueError("empty trimmed history")          # python's x[-0:] would take everything
    return voice.semantic[len(voice.semantic) - n_sh:].astype(np.int32), flat[len(flat) - n_ch:][:-2].astype(np.int32)


def semantic_prompt(prompt513, voice):
    """C10v.1: ids 256..511 <- the last min(n_sem, 256) history ids, right-padded with the semantic pad token"""
    out = np.asarray(prompt513, np.int32).copy()
    if voice is not None:
        h = voice.semantic[-256:] if len(voice.semantic) else voice.semantic
        out[256:512] = SEMANTIC_PAD
        out[256:256 + len(h)] = h
    return out


# ---- picks -------------------------------------------------------------------------------------------------------------------------------------
def _exp_rows(d, exact):
    if exact:
        return np.array([math.exp(float(v)) for v in d.ravel()], np.float64).reshape(d.shape).astype(np.float32)
    return np.exp(d.astype(np.float64)).astype(np.float32)


def greedy(logits):
    """the oracle's sample_argmax (bark.cpp:223-247): l / 0.7, softmax with (float) exp((double) .) and a sequential float sum, first strict maximum of
    p.  numpy's exp can differ from the C library's in the last bit: a row whose two largest p lie within 1e-5 (relative) is redone with math.exp."""
    x = (np.asarray(logits, np.float32) / np.float32(0.7)).astype(np.float32)
    d = (x - x.max()).astype(np.float32)
    for exact in (False, True):
        e = _exp_rows(d, exact)
        p = (e / np.cumsum(e, dtype=np.float32)[-1]).astype(np.float32)
        best = int(np.argmax(p))
        rest = np.delete(p, best)
        if exact or rest.size == 0 or float(rest.max()) < float(p[best]) * (1.0 - 1e-5):
            return best
    raise AssertionError


def greedy_rows(logits):
    """greedy() for every row of [N][n]; vectorised, ambiguous rows redone one by one"""
    x = (np.asarray(logits, np.float32) / np.float32(0.7)).astype(np.float32)
    d = (x - x.max(axis=1, keepdims=True)).astype(np.float32)
    e = _exp_rows(d, False)
    fs = np.cumsum(e, axis=1, dtype=np.float32)[:, -1:]
    p = (e / fs).astype(np.float32)
    best = np.argmax(p, axis=1)
    top2 = np.partition(p, -2, axis=1)[:, -2:]
    amb = np.flatnonzero(top2[:, 0] >= top2[:, 1] * np.float32(1.0 - 1e-5))
    for i in amb:
        best[i] = greedy(logits[i])
    return best.astype(np.int32)


class Sampler:
    """temp == 0: greedy; else C8 / C8n: one uniform draw per sample from std::mt19937(seed) (nucleus_ref.MT19937), optional top-k / top-p filter"""

    def __init__(self, seed=0):
        self.rng = nucleus_ref.MT19937(seed)

    def pick(self, logits, temp, top_k=0, top_p=1.0):
        if temp == 0.0:
            return greedy(logits), None
        u = self.rng.canonical()
        keep = nucleus_ref.keep_mask(logits, top_k, top_p) if (top_k > 0 or top_p < 1.0) else None
        return nucleus_ref.multinomial(logits, temp, u, keep)


# ---- stages ------------------------------------------------------------------------------------------------------------------------------------
def semantic(orc, prompt513, voice, temp=0.0, min_eos_p=0.2, n_steps=768, sampler=None, top_k=0, top_p=1.0):
    """bark_eval_text_encoder (bark.cpp:1645-1701) on the voiced prompt: over ALL n_out logits, stop on the EOS id or eos_p >= min_eos_p"""
    prompt = semantic_prompt(prompt513, voice)
    if temp == 0.0:
        return orc.semantic(prompt, orc.params(temp=0.0, fine_temp=0.0, min_eos_p=min_eos_p, n_steps_text_encoder=n_steps))
    sampler = sampler or Sampler(0)
    out, inp, n_past = [], prompt, 0
    for _ in range(n_steps):
        logits, n_past = orc.gpt_eval(0, inp, n_past, True)
        nxt, eos_p = sampler.pick(logits, temp, top_k, top_p)
        if nxt == SEMANTIC_VOCAB or eos_p >= min_eos_p:
            break
        out.append(nxt); inp = [nxt]
    return np.asarray(out, np.int32)


def coarse(orc, sem, voice, temp=0.0, sliding_window_size=60, max_coarse_history=630, sampler=None, top_k=0, top_p=1.0, trace=None):
    """bark_eval_coarse_encoder (bark.cpp:1745-1863) with C10v.2 -> new frames [T][2]"""
    sem = np.asarray(sem, np.int32)
    sampler = sampler or Sampler(0)
    r = ratio()
    max_semantic_history = int(math.floor(np.float32(np.float32(max_coarse_history) / r)))
    n_steps = int(math.floor(np.float32(np.float32(np.float32(len(sem)) * r) / np.float32(N_COARSE))) * N_COARSE)
    assert n_steps > 0
    n_windows = int(math.ceil(np.float32(n_steps) / np.float32(sliding_window_size)))
    h_sem, h_coarse = trim(voice, max_coarse_history)
    x_sem = np.concatenate([h_sem, sem])
    x_coarse = [int(v) for v in h_coarse]               # history, then everything generated so far
    n_hist = len(x_coarse)
    step_idx = 0
    for _ in range(n_windows):
        semantic_idx = len(h_sem) + int(np.rint(np.float32(np.float32(step_idx) / r)))
        x_in = [int(v) for v in x_sem[max(semantic_idx - max_semantic_history, 0):][:256]]
        x_in += [COARSE_SEMANTIC_PAD] * (256 - len(x_in))
        x_in += [COARSE_INFER] + x_coarse[max(len(x_coarse) - max_coarse_history, 0):]
        if trace is not None:
            trace.append(list(x_in))
        n_past = 0
        for _ in range(sliding_window_size):
            if step_idx >= n_steps:
                continue
            logits, n_past = orc.gpt_eval(1, x_in, n_past, False)
            start = SEMANTIC_VOCAB + (step_idx % N_COARSE) * CODEBOOK             # codebook parity by the NEW step index
            nxt, _ = sampler.pick(logits[start:start + CODEBOOK], temp, top_k, top_p)
            nxt += start
            x_in = [nxt]; x_coarse.append(nxt)
            step_idx += 1
    new = np.asarray(x_coarse[n_hist:], np.int64)
    new = new[:len(new) - len(new) % 2].reshape(-1, 2) - SEMANTIC_VOCAB - CODEBOOK * np.arange(N_COARSE)[None, :]
    return new.astype(np.int32)


def fine_windows(n_hist, T):
    """C10v.3: [(start_idx, start_fill_idx, rel)] of the windows, and L"""
    L = max(n_hist + T, 1024)
    n_loops = max(0, int(math.ceil(np.float32(T - (1024 - n_hist)) / np.float32(512.0)))) + 1
    wins = []
    for n in range(n_loops):
        start_idx = min(512 * n, L - 1024)
        start_fill_idx = min(n_hist + 512 * n, L - 512)
        wins.append((start_idx, start_fill_idx, start_fill_idx - start_idx))
    return wins, L


def fine(orc, coarse_Tx2, voice, fine_temp=0.0, sampler=None):
    """bark_eval_fine_encoder (bark.cpp:1961-2059) with C10v.3 -> new frames [T][8].  Every one of the 1024 positions of a window is sampled (the random
    stream advances as in the reference), positions >= rel keep their pick."""
    co = np.asarray(coarse_Tx2, np.int32).reshape(-1, 2)
    sampler = sampler or Sampler(0)
    T = len(co)
    hist = np.zeros((0, 8), np.int32) if voice is None else np.asarray(voice.fine, np.int32).reshape(-1, 8)[-512:]
    if voice is not None and len(voice.fine) == 0:
        hist = np.zeros((0, 8), np.int32)
    n_hist = len(hist)
    wins, L = fine_windows(n_hist, T)
    in_arr = np.full((L, 8), CODEBOOK, np.int32)
    in_arr[:n_hist] = hist
    in_arr[n_hist:n_hist + T, :2] = co
    for start_idx, start_fill_idx, rel in wins:
        buf = in_arr[start_idx:start_idx + 1024].T.copy()              # [8][1024]
        for nn in range(N_COARSE, N_FINE):
            logits = orc.fine_eval(buf, nn)[:, :CODEBOOK]
            if fine_temp == 0.0:
                picks = greedy_rows(logits)
            else:
                picks = np.asarray([sampler.pick(logits[i], fine_temp)[0] for i in range(1024)], np.int32)
            buf[nn, rel:] = picks[rel:]
        in_arr[start_fill_idx:start_fill_idx + 1024 - rel, N_COARSE:] = buf[N_COARSE:, rel:].T
    return in_arr[n_hist:n_hist + T].copy()


def generate(orc, text, voice, temp=0.0, fine_temp=0.0, min_eos_p=0.2, n_steps=768, sliding_window_size=60, max_coarse_history=630, seed=0, top_k=0, top_p=1.0):
    """bark_generate_audio with a voice prompt: one generator through the three stages; the codec sees the new frames only"""
    s = Sampler(seed)
    sem = semantic(orc, orc.tokenize(text), voice, temp, min_eos_p, n_steps, s, top_k, top_p)
    co = coarse(orc, sem, voice, temp, sliding_window_size, max_coarse_history, s, top_k, top_p)
    fi = fine(orc, co, voice, fine_temp, s)
    return dict(semantic=sem, coarse=co, fine=fi, pcm=orc.codec_decode(fi.T.copy()))
