#!/usr/bin/env python3
"""Times the EnCodec encoder (bark_hip_codec_encode / _many) on the synthetic `small` file - EnCodec-24 kHz's real dimensions: one recording of 1 s,
5.12 s and 13.6 s, and 32 recordings of 5.12 s in one pass.  Per case: wall clock of the call (uploads, kernels, the copy of the codes) and the hipEvent
time between its first and last kernel (bark_hip_codec_encode_device_us), median and minimum of --iters calls after --warmup calls; for comparison the
decoder on the same frame counts.  Every case runs in a child process of its own under a time limit, and the first failure ends the run.

Usage: python tools/codec_encode_time.py [--out profiles/codec_encode_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("1 s", 24000, 1), ("5.12 s", 122880, 1), ("13.6 s", 326400, 1), ("32 x 5.12 s", 122880, 32)]


def child(n_samples: int, n_rec: int, iters: int, warmup: int):
    import numpy as np
    from bark_amd_loader import load_package
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("small", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    rng = np.random.default_rng(5)
    t = np.arange(n_samples) / 24000.0
    xs = [(0.4 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1333 * t + 1) + 0.1 * rng.standard_normal(n_samples)).astype(np.float32) for _ in range(n_rec)]
    wall, dev, dec = [], [], []
    codes = None
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        codes = ctx.codec_encode_many(xs, 8) if n_rec > 1 else [ctx.codec_encode(xs[0], 8)]
        w = 1e3 * (time.perf_counter() - t0)
        if i >= warmup:
            wall.append(w); dev.append(ctx.codec_encode_device_us() / 1e3)
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        ctx.codec_decode(codes[0])
        if i >= warmup:
            dec.append(1e3 * (time.perf_counter() - t0))
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    print(json.dumps(dict(frames=int(codes[0].shape[1]), wall_ms_median=med(wall), wall_ms_min=min(wall), device_ms_median=med(dev), device_ms_min=min(dev),
                          decode_one_wall_ms_median=med(dec))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_encode_time.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=2, type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup)
        return
    lines = ["EnCodec encoder, synthetic `small` file (32 filters, LSTM 2 x 512, 8 codebooks), f16 weights; python tools/codec_encode_time.py",
             f"median / min of {a.iters} calls after {a.warmup} warm-up calls; wall: the whole call, device: hipEvents around its kernels", ""]
    for name, n, b in CASES:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(n), str(b), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"{name}: FAILED (exit {r.returncode}) {r.stderr[-400:]}")
            break                                                     # nothing more is started on the GPU after a failure
        d = json.loads(r.stdout.strip().splitlines()[-1])
        lines.append(f"{name:12s} T = {d['frames']:4d} frames x {b:2d}: wall {d['wall_ms_median']:7.2f} ms (min {d['wall_ms_min']:7.2f}), device {d['device_ms_median']:7.2f} ms "
                     f"(min {d['device_ms_min']:7.2f}); decoder, one recording of T frames, wall {d['decode_one_wall_ms_median']:6.2f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
