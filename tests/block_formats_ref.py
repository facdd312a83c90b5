"""An independent reading of ggml's weight block formats, written from ggml's definitions (block_q4_0 ... block_q8_0 and
dequantize_row_q*), not from the engine's or the oracle's code.

Every format packs 32 weights per block behind an f16 scale d (and an f16 minimum m for q4_1 / q5_1):

    q4_0  d | 16 nibble bytes               w = d * (q - 8)
    q4_1  d | m | 16 nibble bytes           w = d * q + m
    q5_0  d | u32 qh | 16 nibble bytes      w = d * ((q | h << 4) - 16)
    q5_1  d | m | u32 qh | 16 nibble bytes  w = d * (q | h << 4) + m
    q8_0  d | 32 int8                       w = d * q

Element j < 16 sits in the low nibble of byte j, element j + 16 in the high nibble of byte j; the fifth bit h of element j is bit j
of the little-endian word qh.  Products and sums are single f32 operations, as ggml's dequantisers perform them.

`write_dequantized_twin` turns a quantised model file into the f32 model file that holds the same function: every quantised matrix
replaced by its dequantised values, every other tensor widened (exactly) to f32, ftype 0 - what a model file converted without
--use-f16 looks like.  A model evaluated on the twin computes f32 weights x f32 activations; the only thing it leaves out of the
quantised model's arithmetic is ggml's q8 rounding of the activations.

`variant` selects a deliberately wrong reading (the negative controls of tests/test_block_format_reference.py):
    "swap_nibbles"   element j read from the high nibble of byte j, element j + 16 from the low one
    "qh_wrong_half"  the fifth bit of element j read from bit j + 16 (mod 32) of qh
    "drop_min"       the minimum m of q4_1 / q5_1 left out

`evaluations` lists the model evaluations that tests/test_gpu_weight_formats.py compares bit for bit between engine and oracle and
tests/test_block_format_reference.py between a quantised file and its twin.
"""
from __future__ import annotations

import os
import struct

import numpy as np

import model_patch as mp

# ggml_type -> (name, bytes per block of 32 weights)
BLOCK_TYPES = {2: ("q4_0", 18), 3: ("q4_1", 20), 6: ("q5_0", 22), 7: ("q5_1", 24), 8: ("q8_0", 34)}
TYPE_OF = {name: t for t, (name, _) in BLOCK_TYPES.items()}
VARIANTS = (None, "swap_nibbles", "qh_wrong_half", "drop_min")


def _blocks(fmt: str, raw) -> np.ndarray:
    return np.frombuffer(raw, np.uint8).reshape(-1, BLOCK_TYPES[TYPE_OF[fmt]][1])


def _f16_col(blocks: np.ndarray, off: int) -> np.ndarray:
    return np.ascontiguousarray(blocks[:, off:off + 2]).view("<f2")[:, 0].astype(np.float32)


def block_scales(fmt: str, raw) -> np.ndarray:
    """The scale d of every block, as f32."""
    return _f16_col(_blocks(fmt, raw), 0)


def levels(fmt: str, raw, variant: str | None = None) -> np.ndarray:
    """[n_blocks, 32] integer levels of the blocks in `raw` (with the offsets -8 / -16 of q4_0 / q5_0)."""
    assert variant in VARIANTS, variant
    b = _blocks(fmt, raw)
    if fmt == "q8_0":
        return np.ascontiguousarray(b[:, 2:34]).view(np.int8).astype(np.int32)
    off = 4 if fmt in ("q4_1", "q5_1") else 2
    qh = None
    if fmt in ("q5_0", "q5_1"):
        qh = np.ascontiguousarray(b[:, off:off + 4]).view("<u4")[:, 0]
        off += 4
    qs = b[:, off:off + 16].astype(np.int32)
    lo, hi = qs & 0x0F, qs >> 4
    if variant == "swap_nibbles":
        lo, hi = hi, lo
    q = np.concatenate([lo, hi], axis=1)
    if qh is not None:
        j = np.arange(32, dtype=np.uint32)
        if variant == "qh_wrong_half":
            j = (j + 16) % 32
        q |= (((qh[:, None] >> j[None, :]) & 1) << 4).astype(np.int32)
    if fmt == "q4_0":
        q -= 8
    elif fmt == "q5_0":
        q -= 16
    return q


def dequantize(fmt: str, raw, variant: str | None = None) -> np.ndarray:
    """The weights of the blocks in `raw`, flat f32 in file order."""
    b = _blocks(fmt, raw)
    w = levels(fmt, raw, variant).astype(np.float32) * _f16_col(b, 0)[:, None]
    if fmt in ("q4_1", "q5_1") and variant != "drop_min":
        w = w + _f16_col(b, 2)[:, None]
    return w.astype(np.float32).reshape(-1)


def write_dequantized_twin(src: str, dst: str, variant: str | None = None) -> dict:
    """Write the f32 twin of the quantised model file `src` (module docstring) to `dst`.  Returns how many tensors of each ggml_type
    the GPT sections of `src` hold."""
    with open(src, "rb") as f:
        buf = f.read()
    layout = mp.walk(buf)
    out = [buf[:layout["gpt"][0]["hp_off"]["n_layer"]]]               # magic and vocabulary
    seen: dict = {}

    def records(tensors):
        for info in tensors.values():
            tt = struct.unpack_from("<i", buf, info["ttype_off"])[0]
            raw = buf[info["data_off"]:info["end"]]
            if tt in BLOCK_TYPES:
                w = dequantize(BLOCK_TYPES[tt][0], raw, variant)
            else:
                w = np.frombuffer(raw, {0: "<f4", 1: "<f2"}[tt]).astype(np.float32)
            head = bytearray(buf[info["rec"]:info["data_off"]])
            struct.pack_into("<i", head, 8, 0)                            # ggml_type f32
            out.append(bytes(head))
            out.append(w.astype("<f4").tobytes())
            yield tt

    for sec in layout["gpt"]:
        hp = bytearray(buf[sec["hp_off"]["n_layer"]:sec["hp_off"]["ftype"] + 8])   # ten hparams and the tensor count
        struct.pack_into("<i", hp, 36, 0)                                 # ftype f32
        out.append(bytes(hp))
        for tt in records(sec["tensors"]):
            seen[tt] = seen.get(tt, 0) + 1
    hp = bytearray(buf[layout["codec_hp_off"] - 4:layout["codec_hp_off"] + 36])     # magic and nine hparams, ftype last
    struct.pack_into("<i", hp, 36, 0)
    out.append(bytes(hp))
    for _ in records(layout["codec"]):
        pass
    with open(dst, "wb") as f:
        for part in out:
            f.write(part)
    return seen


# ---- the evaluations compared per model file ------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hf_toy_s0.npz")
SEMANTIC_DECODE = (4242, 17)        # tokens of the two semantic decode steps behind the merged prompt
COARSE_ROWS = (1, 300, 887)         # coarse prompt lengths; 887 = 630 tokens of history + a 256-token semantic window + the infer token
COARSE_DECODE = 10777
FINE_NN = (2, 7)


def evaluation_inputs() -> dict:
    g = np.load(GOLD)
    cp = g["coarse_prompt"]
    coarse = {n: np.ascontiguousarray(cp[:n], np.int32) if n <= len(cp) else np.random.default_rng(n).integers(0, 12096, n).astype(np.int32)
              for n in COARSE_ROWS}
    fine = np.random.default_rng(11).integers(0, 1024, (8, 1024)).astype(np.int32)
    return {"semantic": np.ascontiguousarray(g["sem_prompt"], np.int32), "coarse": coarse, "fine": fine}


def evaluations(m, x: dict, rows_only: bool = False, fine_nn=FINE_NN) -> dict:
    """name -> logits of: the 257-row merged semantic prompt and two decode steps behind it; coarse prompts of COARSE_ROWS rows, each
    followed by one decode step; fine passes nn in `fine_nn`.  `m` is an engine context or an oracle (both have gpt_eval / fine_eval).
    rows_only: only the evaluations of more than one row (prompt and fine passes)."""
    out = {}
    lo, n_past = m.gpt_eval(0, x["semantic"], 0, True)
    assert n_past == 257, n_past
    out["semantic prompt (257 rows)"] = lo
    if not rows_only:
        for k, tok in enumerate(SEMANTIC_DECODE):
            lo, n_past = m.gpt_eval(0, [tok], n_past, True)
            out[f"semantic decode step {k + 1}"] = lo
    for n in COARSE_ROWS:
        if rows_only and n == 1:
            continue
        lo, n_past = m.gpt_eval(1, x["coarse"][n], 0, False)
        assert n_past == n, (n_past, n)
        out[f"coarse prompt N={n}"] = lo
        if not rows_only:
            out[f"coarse decode after N={n}"] = m.gpt_eval(1, [COARSE_DECODE], n_past, False)[0]
    for nn in fine_nn:
        out[f"fine pass nn={nn}"] = m.fine_eval(x["fine"], nn)
    return out
