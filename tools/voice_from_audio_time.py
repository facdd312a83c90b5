#!/usr/bin/env python3
"""Times a voice prompt from a recording on the synthetic `small` + `hub_base` files (EnCodec-24 kHz's and HuBERT-base's dimensions) for recordings of 1 s, 5 s
and 20 s: the resampler launch alone (bark_hip_time_resample, hipEvents), the hipEvent times of the two encoders inside the native call
(bark_hip_semantic_encode_device_us, bark_hip_codec_encode_device_us), the wall clock of ctx.voice_from_audio (bark_hip_voice_from_audio) and of
voice.from_audio (the numpy resampler and two native calls).  Beside the resampler's time: its byte floor, 4 n + 4 n_out bytes at --hbm-tbps, and the ratio.
Median of --iters calls after --warmup calls.  Every case runs in a child process of its own under a time limit, and the first failure ends the run.

Usage: python tools/voice_from_audio_time.py [--out profiles/voice_from_audio_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("1 s", 24000), ("5 s", 120000), ("20 s", 480000)]


def child(n: int, iters: int, warmup: int):
    import numpy as np
    from bark_amd_loader import load_package
    from tools.make_synth_hubert import ensure_hubert
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("small", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    ctx.load_semantic_encoder(ensure_hubert("hub_base", 0))
    t = np.arange(n) / 24000.0
    x = (0.4 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1333 * t + 1) + 0.1 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    resample_us = ctx.time_resample(n, 200)
    native, python, sem_us, enc_us = [], [], [], []
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        a = ctx.voice_from_audio(x)
        w = 1e3 * (time.perf_counter() - t0)
        if i >= warmup:
            native.append(w); sem_us.append(ctx.semantic_encode_device_us()); enc_us.append(ctx.codec_encode_device_us())
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        b = pkg.voice.from_audio(ctx, x)
        if i >= warmup:
            python.append(1e3 * (time.perf_counter() - t0))
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    print(json.dumps(dict(n_semantic=len(a[0]), n_frames=len(a[2]), resample_us=resample_us, semantic_device_us=med(sem_us), codec_device_us=med(enc_us),
                          native_wall_ms=med(native), python_wall_ms=med(python), semantic_ids_equal=int((a[0] == b.semantic).sum()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_from_audio_time.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-tbps", type=float, default=8.0, help="HBM rate of the byte floor (the MI355X's datasheet figure)")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.iters, a.warmup)
        return
    lines = ["voice prompt from a recording, synthetic `small` + `hub_base` files; python tools/voice_from_audio_time.py",
             f"median of {a.iters} calls after {a.warmup} warm-up calls; resampler: bark_hip_time_resample over 200 launches; floor: (4 n + 4 n_out) bytes at {a.hbm_tbps} TB/s", ""]
    for name, n in CASES:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(n), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"{name}: FAILED (exit {r.returncode}) {r.stderr[-400:]}")
            break                                                     # nothing more is started on the GPU after a failure
        d = json.loads(r.stdout.strip().splitlines()[-1])
        floor_us = (4 * n + 4 * ((2 * n + 2) // 3)) / (a.hbm_tbps * 1e12) * 1e6
        lines.append(f"{name:5s} n = {n:6d}: resampler {d['resample_us']:7.2f} us (floor {floor_us:6.3f} us, x{d['resample_us'] / floor_us:6.1f}), semantic encoder device "
                     f"{d['semantic_device_us'] / 1e3:6.2f} ms, codec encoder device {d['codec_device_us'] / 1e3:6.2f} ms, voice_from_audio wall {d['native_wall_ms']:7.2f} ms, "
                     f"voice.from_audio wall {d['python_wall_ms']:7.2f} ms; {d['n_semantic']} semantic ids ({d['semantic_ids_equal']} equal on both routes), {d['n_frames']} frames")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
