#!/usr/bin/env python3
"""Writes the semantic encoder's file (rule C12h) from a HuggingFace `HubertModel` state dict (feat_extract_norm="group",
do_stable_layer_norm=False, conv_bias=False) and the state dict of the token head (`lstm.*` of a two-layer nn.LSTM, `fc.weight` / `fc.bias` of the
nn.Linear behind it - the layout of the community tokenizers for Bark voice cloning).

    u32 magic 0x68756273 | 11 x i32: C, H, n_head, F, n_layer_stored, output_layer, pos_kernel, pos_groups, D, n_classes, ftype (1: f16)
    records until EOF: i32 n_dims, i32 name_len, i32 ttype, i32 dims[n_dims] (innermost first), name, data      (csrc/model_file.h)

Rank >= 2 tensors are stored as f16, the others as f32.  The positional convolution's weight norm (dim 2: w = g v / |v| with the norm over the output and
input channels of each tap) is folded into a plain weight, the q / k / v projections of a layer are stacked into one [3 H][H] matrix, and only the first
`output_layer` layers are stored - the hidden state behind that layer is what the head reads.

Usage: python tools/convert_hubert.py --hubert hubert_base.pt --head tokenizer.pth --out semantic_encoder.bin [--output-layer 7] [--heads 12]
(both inputs: torch.load-able state dicts; `--hubert` may also be a directory that HubertModel.from_pretrained accepts, if transformers is installed)."""
from __future__ import annotations

import argparse
import struct

import numpy as np

MAGIC = 0x68756273
HPARAM_NAMES = ("C", "H", "n_head", "F", "n_layer_stored", "output_layer", "pos_kernel", "pos_groups", "D", "n_classes", "ftype")
CONV_KERNELS = (10, 3, 3, 3, 3, 2, 2)      # strides 5, 2, 2, 2, 2, 2, 2: 400 samples per frame, a hop of 320


def _np(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().float().numpy()
    return np.asarray(t, dtype=np.float32)


def fold_weight_norm(g, v) -> np.ndarray:
    """torch weight_norm with dim=2 on a Conv1d weight [out][in][k]: w[..., k] = g[k] * v[..., k] / |v[..., k]|."""
    g, v = _np(g), _np(v)
    norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(0, 1), keepdims=True))
    return (g.reshape(1, 1, -1).astype(np.float64) * v / norm).astype(np.float32)


def _pos_weight(sd) -> np.ndarray:
    p = "encoder.pos_conv_embed.conv."
    if p + "weight" in sd:
        return _np(sd[p + "weight"])
    for g, v in ((p + "parametrizations.weight.original0", p + "parametrizations.weight.original1"), (p + "weight_g", p + "weight_v")):
        if g in sd:
            return fold_weight_norm(sd[g], sd[v])
    raise KeyError("no positional convolution weight in the state dict")


def tensors_from_state_dicts(hub_sd, head_sd, output_layer: int, n_head: int):
    """-> (hparams dict, [(name, array)]) in file order."""
    hub_sd = {k[len("hubert."):] if k.startswith("hubert.") else k: v for k, v in hub_sd.items()}
    out = []
    w0 = _np(hub_sd["feature_extractor.conv_layers.0.conv.weight"])
    C = w0.shape[0]
    for i, k in enumerate(CONV_KERNELS):
        w = _np(hub_sd[f"feature_extractor.conv_layers.{i}.conv.weight"])
        if w.shape != (C, 1 if i == 0 else C, k):
            raise ValueError(f"feature convolution {i} has shape {w.shape}: C12h takes kernels {CONV_KERNELS} over {C} channels")
        if f"feature_extractor.conv_layers.{i}.conv.bias" in hub_sd:
            raise ValueError("feature convolutions with a bias (conv_bias=True) are not C12h")
        out.append((f"conv{i}.weight", w))
        if i == 0:
            out.append(("conv0.norm.weight", _np(hub_sd["feature_extractor.conv_layers.0.layer_norm.weight"])))
            out.append(("conv0.norm.bias", _np(hub_sd["feature_extractor.conv_layers.0.layer_norm.bias"])))
    out.append(("proj.ln.weight", _np(hub_sd["feature_projection.layer_norm.weight"])))
    out.append(("proj.ln.bias", _np(hub_sd["feature_projection.layer_norm.bias"])))
    pw = _np(hub_sd["feature_projection.projection.weight"])
    H = pw.shape[0]
    out.append(("proj.weight", pw))
    out.append(("proj.bias", _np(hub_sd["feature_projection.projection.bias"])))
    pos = _pos_weight(hub_sd)
    G = H // pos.shape[1]
    out.append(("pos.weight", pos))
    out.append(("pos.bias", _np(hub_sd["encoder.pos_conv_embed.conv.bias"])))
    out.append(("enc.ln.weight", _np(hub_sd["encoder.layer_norm.weight"])))
    out.append(("enc.ln.bias", _np(hub_sd["encoder.layer_norm.bias"])))
    F = 0
    for l in range(output_layer):
        p = f"encoder.layers.{l}."
        q = f"layers.{l}."
        out.append((q + "attn.qkv.weight", np.concatenate([_np(hub_sd[p + f"attention.{n}_proj.weight"]) for n in "qkv"], axis=0)))
        out.append((q + "attn.qkv.bias", np.concatenate([_np(hub_sd[p + f"attention.{n}_proj.bias"]) for n in "qkv"], axis=0)))
        out.append((q + "attn.out.weight", _np(hub_sd[p + "attention.out_proj.weight"])))
        out.append((q + "attn.out.bias", _np(hub_sd[p + "attention.out_proj.bias"])))
        out.append((q + "ln1.weight", _np(hub_sd[p + "layer_norm.weight"])))
        out.append((q + "ln1.bias", _np(hub_sd[p + "layer_norm.bias"])))
        out.append((q + "fc1.weight", _np(hub_sd[p + "feed_forward.intermediate_dense.weight"])))
        out.append((q + "fc1.bias", _np(hub_sd[p + "feed_forward.intermediate_dense.bias"])))
        out.append((q + "fc2.weight", _np(hub_sd[p + "feed_forward.output_dense.weight"])))
        out.append((q + "fc2.bias", _np(hub_sd[p + "feed_forward.output_dense.bias"])))
        out.append((q + "ln2.weight", _np(hub_sd[p + "final_layer_norm.weight"])))
        out.append((q + "ln2.bias", _np(hub_sd[p + "final_layer_norm.bias"])))
        F = out[-6][1].shape[0]
    D = _np(head_sd["lstm.weight_hh_l0"]).shape[1]
    for l in range(2):
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            out.append((f"head.lstm.{n}_l{l}", _np(head_sd[f"lstm.{n}_l{l}"])))
    fc = _np(head_sd["fc.weight"])
    out.append(("head.out.weight", fc))
    out.append(("head.out.bias", _np(head_sd["fc.bias"])))
    hp = dict(C=C, H=H, n_head=n_head, F=F, n_layer_stored=output_layer, output_layer=output_layer, pos_kernel=pos.shape[2], pos_groups=G, D=D,
              n_classes=fc.shape[0], ftype=1)
    return hp, out


def write_file(path: str, hp: dict, tensors):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", MAGIC))
        f.write(struct.pack("<11i", *[int(hp[n]) for n in HPARAM_NAMES]))
        for name, a in tensors:
            a = np.ascontiguousarray(a)
            ttype = 1 if a.ndim >= 2 else 0
            nm = name.encode()
            f.write(struct.pack("<3i", a.ndim, len(nm), ttype))
            f.write(struct.pack(f"<{a.ndim}i", *reversed(a.shape)))
            f.write(nm)
            f.write(a.astype("<f2" if ttype else "<f4").tobytes())


def read_file(path: str):
    """-> (hparams dict, {name: f32 array}) - the inverse of write_file (f16 tensors widened)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 48 or struct.unpack_from("<I", data, 0)[0] != MAGIC:
        raise ValueError(f"{path}: not a semantic encoder file")
    hp = dict(zip(HPARAM_NAMES, struct.unpack_from("<11i", data, 4)))
    pos, tensors = 48, {}
    while pos < len(data):
        n_dims, name_len, ttype = struct.unpack_from("<3i", data, pos); pos += 12
        dims = struct.unpack_from(f"<{n_dims}i", data, pos); pos += 4 * n_dims
        name = data[pos:pos + name_len].decode(); pos += name_len
        count = int(np.prod(dims))
        dt = "<f2" if ttype == 1 else "<f4"
        a = np.frombuffer(data, dtype=dt, count=count, offset=pos).astype(np.float32).reshape(tuple(reversed(dims)))
        pos += count * (2 if ttype == 1 else 4)
        tensors[name] = a
    return hp, tensors


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hubert", required=True)
    ap.add_argument("--head", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--output-layer", type=int, default=7)
    ap.add_argument("--heads", type=int, default=0, help="attention heads (default: H / 64)")
    a = ap.parse_args()
    import os
    if os.path.isdir(a.hubert):
        from transformers import HubertModel
        hub_sd = HubertModel.from_pretrained(a.hubert).state_dict()
    else:
        hub_sd = torch.load(a.hubert, map_location="cpu")
    head_sd = torch.load(a.head, map_location="cpu")
    for sd_name in ("state_dict", "model"):
        if isinstance(hub_sd, dict) and sd_name in hub_sd and isinstance(hub_sd[sd_name], dict):
            hub_sd = hub_sd[sd_name]
    H = _np(hub_sd[[k for k in hub_sd if k.endswith("feature_projection.projection.weight")][0]]).shape[0]
    hp, tensors = tensors_from_state_dicts(hub_sd, head_sd, a.output_layer, a.heads or H // 64)
    write_file(a.out, hp, tensors)
    print(f"wrote {a.out}: " + ", ".join(f"{k} {v}" for k, v in hp.items()))


if __name__ == "__main__":
    main()
