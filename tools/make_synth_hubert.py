#!/usr/bin/env python3
"""Synthetic semantic-encoder files (rule C12h): seeded random weights at HuBERT's real or at toy dimensions, written through tools/convert_hubert.py from
state dicts in HuggingFace's and the token head's naming (weight-normed positional convolution included, so the converter's fold is exercised).

    hub_toy   C 128, H 384, 6 heads, F 768, 3 layers stored, output_layer 2, Kp 16, G 8, D 128, 1000 classes   (48 channels per group, as at base)
    hub_base  C 512, H 768, 12 heads, F 3072, 7 layers stored, output_layer 7, Kp 128, G 16, D 1024, 10 000 classes

Plainly initialised weights make the head pick a handful of ids whatever the signal: an LSTM with small weights averages its input and every frame lands on the
same few classes, and attention whose output is as large as the residual stream halves what varies over time in every post-norm layer.  The recipe therefore
sharpens the attention (qk), keeps its output below the residual (attn_out) and drives the LSTM by its input more than by its state (GAINS below),
chosen so that the reference's picks spread and most frames are decided by a margin far above f16 noise (tools/make_hf_golden.py asserts how far)."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convert_hubert  # noqa: E402


@dataclass
class HubPreset:
    C: int
    H: int
    n_head: int
    F: int
    n_layer_stored: int
    output_layer: int
    pos_kernel: int
    pos_groups: int
    D: int
    n_classes: int


PRESETS = {
    "hub_toy": HubPreset(128, 384, 6, 768, 3, 2, 16, 8, 128, 1000),
    "hub_base": HubPreset(512, 768, 12, 3072, 7, 7, 128, 16, 1024, 10000),
}
# gains over a variance-preserving initialisation (std = gain / sqrt(fan_in))
GAINS = dict(conv=1.4, qk=3.0, attn_out=0.15, lstm_ih=3.0, lstm_hh=0.3, out=6.0)


def state_dicts(preset: str, seed: int = 0):
    p = PRESETS[preset]
    rng = np.random.default_rng([seed, 0x68756273, sorted(PRESETS).index(preset)])

    def w(*shape, fan_in, gain=1.0):
        return (rng.standard_normal(shape) * (gain / np.sqrt(fan_in))).astype(np.float32)

    def ln(n):
        return (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)

    hub = {}
    for i, k in enumerate(convert_hubert.CONV_KERNELS):
        cin = 1 if i == 0 else p.C
        hub[f"feature_extractor.conv_layers.{i}.conv.weight"] = w(p.C, cin, k, fan_in=cin * k, gain=GAINS["conv"])
    hub["feature_extractor.conv_layers.0.layer_norm.weight"], hub["feature_extractor.conv_layers.0.layer_norm.bias"] = ln(p.C)
    hub["feature_projection.layer_norm.weight"], hub["feature_projection.layer_norm.bias"] = ln(p.C)
    hub["feature_projection.projection.weight"] = w(p.H, p.C, fan_in=p.C)
    hub["feature_projection.projection.bias"] = w(p.H, fan_in=100.0)
    Hg = p.H // p.pos_groups
    v = w(p.H, Hg, p.pos_kernel, fan_in=Hg * p.pos_kernel)
    hub["encoder.pos_conv_embed.conv.weight_v"] = v
    hub["encoder.pos_conv_embed.conv.weight_g"] = (np.sqrt((v.astype(np.float64) ** 2).sum(axis=(0, 1), keepdims=True)) *
                                                   (1.0 + 0.1 * rng.standard_normal((1, 1, p.pos_kernel)))).astype(np.float32)
    hub["encoder.pos_conv_embed.conv.bias"] = w(p.H, fan_in=100.0)
    hub["encoder.layer_norm.weight"], hub["encoder.layer_norm.bias"] = ln(p.H)
    for l in range(p.n_layer_stored):
        q = f"encoder.layers.{l}."
        for n in "qkv":
            hub[q + f"attention.{n}_proj.weight"] = w(p.H, p.H, fan_in=p.H, gain=GAINS["qk"] if n in "qk" else 1.0)
            hub[q + f"attention.{n}_proj.bias"] = w(p.H, fan_in=400.0)
        hub[q + "attention.out_proj.weight"] = w(p.H, p.H, fan_in=p.H, gain=GAINS["attn_out"])
        hub[q + "attention.out_proj.bias"] = w(p.H, fan_in=400.0)
        hub[q + "layer_norm.weight"], hub[q + "layer_norm.bias"] = ln(p.H)
        hub[q + "feed_forward.intermediate_dense.weight"] = w(p.F, p.H, fan_in=p.H)
        hub[q + "feed_forward.intermediate_dense.bias"] = w(p.F, fan_in=400.0)
        hub[q + "feed_forward.output_dense.weight"] = w(p.H, p.F, fan_in=p.F)
        hub[q + "feed_forward.output_dense.bias"] = w(p.H, fan_in=400.0)
        hub[q + "final_layer_norm.weight"], hub[q + "final_layer_norm.bias"] = ln(p.H)
    head = {}
    for l in range(2):
        kin = p.H if l == 0 else p.D
        head[f"lstm.weight_ih_l{l}"] = w(4 * p.D, kin, fan_in=kin, gain=GAINS["lstm_ih"])
        head[f"lstm.weight_hh_l{l}"] = w(4 * p.D, p.D, fan_in=p.D, gain=GAINS["lstm_hh"])
        head[f"lstm.bias_ih_l{l}"] = w(4 * p.D, fan_in=25.0)
        head[f"lstm.bias_hh_l{l}"] = w(4 * p.D, fan_in=25.0)
    head["fc.weight"] = w(p.n_classes, p.D, fan_in=p.D, gain=GAINS["out"])
    head["fc.bias"] = w(p.n_classes, fan_in=4.0)
    return p, hub, head


def write_hubert(path: str, preset: str = "hub_toy", seed: int = 0):
    p, hub, head = state_dicts(preset, seed)
    hp, tensors = convert_hubert.tensors_from_state_dicts(hub, head, p.n_layer_stored, p.n_head)
    hp["output_layer"] = p.output_layer
    assert (hp["C"], hp["H"], hp["F"], hp["pos_kernel"], hp["pos_groups"], hp["D"], hp["n_classes"]) == (p.C, p.H, p.F, p.pos_kernel, p.pos_groups, p.D, p.n_classes)
    tmp = path + f".tmp{os.getpid()}"
    convert_hubert.write_file(tmp, hp, tensors)
    os.replace(tmp, path)


def ensure_hubert(preset: str = "hub_toy", seed: int = 0, cache_dir: str | None = None) -> str:
    """Create the file once per (preset, seed) under `cache_dir` (default: $BARK_SYNTH_DIR or /tmp/bark_synth, as tools/make_synth_model.ensure_model)."""
    cache_dir = cache_dir or os.environ.get("BARK_SYNTH_DIR", "/tmp/bark_synth")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"{preset}_s{seed}.bin")
    if not os.path.exists(path):
        write_hubert(path, preset, seed)
    return path


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", default="hub_toy", choices=sorted(PRESETS))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        write_hubert(a.out, a.preset, a.seed)
        print(a.out)
    else:
        print(ensure_hubert(a.preset, a.seed))
