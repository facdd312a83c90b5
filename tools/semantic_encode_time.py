#!/usr/bin/env python3
"""Times the semantic encoder (bark_hip_semantic_encode, rule C12h) on the synthetic `hub_base` file - HuBERT-base's dimensions with 7 layers and a token
head of width 1024: recordings of 1 s, 3 s, 10 s and 20.5 s (1024 frames, the longest input) at 16 kHz.  Per case: wall clock of the call (upload, kernels,
the copy of the ids) and the hipEvent time between its first and last kernel (bark_hip_semantic_encode_device_us), median and minimum of --iters calls after
--warmup calls.  Every case runs in a child process of its own under a time limit, and the first failure ends the run.

Usage: python tools/semantic_encode_time.py [--out profiles/semantic_encoder.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("1 s", 16000), ("3 s", 48000), ("10 s", 160000), ("20.5 s", 328079)]


def child(n_samples: int, iters: int, warmup: int):
    import numpy as np
    from bark_amd_loader import load_package
    from tools.make_synth_hubert import ensure_hubert
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    ctx.load_semantic_encoder(ensure_hubert("hub_base", 0))
    rng = np.random.default_rng(5)
    t = np.arange(n_samples) / 16000.0
    x = (0.4 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1333 * t + 1) + 0.1 * rng.standard_normal(n_samples)).astype(np.float32)
    wall, dev = [], []
    ids = None
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        ids = ctx.semantic_encode(x)
        w = 1e3 * (time.perf_counter() - t0)
        if i >= warmup:
            wall.append(w); dev.append(ctx.semantic_encode_device_us() / 1e3)
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    print(json.dumps(dict(frames=int(len(ids)), distinct=int(len(set(ids.tolist()))), wall_ms_median=med(wall), wall_ms_min=min(wall), device_ms_median=med(dev),
                          device_ms_min=min(dev))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_encoder.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.iters, a.warmup)
        return
    lines = ["Semantic encoder, synthetic `hub_base` file (C 512, H 768, 12 heads, FFN 3072, 7 layers, LSTM 2 x 1024, 10 000 classes), f16 weights; python tools/semantic_encode_time.py",
             f"median / min of {a.iters} calls after {a.warmup} warm-up calls; wall: the whole call, device: hipEvents around its kernels", ""]
    for name, n in CASES:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(n), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"{name}: FAILED (exit {r.returncode}) {r.stderr[-400:]}")
            break                                                     # nothing more is started on the GPU after a failure
        d = json.loads(r.stdout.strip().splitlines()[-1])
        lines.append(f"{name:7s} n = {n:6d} samples, T = {d['frames']:4d} frames ({d['distinct']:3d} distinct ids): wall {d['wall_ms_median']:8.2f} ms (min {d['wall_ms_min']:8.2f}), "
                     f"device {d['device_ms_median']:8.2f} ms (min {d['device_ms_min']:8.2f})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
