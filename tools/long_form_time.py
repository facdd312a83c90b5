#!/usr/bin/env python3
"""Times the long-form route (rules C15s / C15j).  Join: device time of one join with the default parameters (bark_hip_time_join, hipEvents, warm: the join
launch - threshold 0 runs no activity launch) for 8 and 64 segments of 5.12 s at 24000 f32, 8000 mu-law and 48000 f32; apart from it what a trim
threshold adds in front (bark_hip_time_join_activity: the table's fill and the activity launch with every frame active); and beside each join figure bark_hip_time_resample_pair of ONE recording of the
same total length in the same run - the existing kernel doing the same filter work (the identity has no such kernel: none is given there).  A recording of
bark_hip_time_resample_pair holds at most 1 310 720 samples, so the baseline is the time of ceil(total / 1 310 720) launches of equal shares.
Wall: generate_long (chain = 0, one lock-step job) of an 8-sentence text on the synthetic `small` file against 8 sequential bark_generate_audio calls of the
same chunks in the same process, and long_audio_as at 8000 mu-law.  Every case runs in a child process of its own under a time limit, and the first failure
ends the run.

Usage: python tools/long_form_time.py [--out profiles/long_form_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_EACH = 122880                 # 5.12 s
OUTPUTS = [(24000, "f32"), (8000, "mulaw"), (48000, "f32")]
TEXT = ("hello world this is bark. the water of the river is cold. we read a book and a letter! do they hear the music? the sun and the moon. "
        "a horse and a bird live here. go there and stop, then come back. the end of the story.")
MAX_RECORDING = 4096 * 320


def _load(preset, **par):
    from bark_amd_loader import load_package
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    return pkg, pkg.BarkContext.load_model(ensure_model(preset, 0), pkg.default_params(**par), seed=0)


def child_join(iters: int):
    pkg, ctx = _load("toy", temp=0.0, fine_temp=0.0)
    out = []
    for count in (8, 64):
        total = count * N_EACH + (count - 1) * 6000
        parts = -(-total // MAX_RECORDING)
        out.append(dict(count=count, total=total, activity_us=ctx.time_join_activity(count, N_EACH, iters)))
        for rate, fmt in OUTPUTS:
            join_us = ctx.time_join(count, N_EACH, rate, fmt, iters)
            base_us = parts * ctx.time_resample_pair(-(-total // parts), 24000, rate, fmt, iters) if rate != 24000 else None
            out.append(dict(count=count, total=total, rate=rate, fmt=fmt, join_us=join_us, resample_us=base_us, launches=parts))
    ctx.free()
    print(json.dumps(out))


def child_wall(iters: int):
    pkg, ctx = _load("small", temp=0.0, fine_temp=0.0)
    raw = TEXT.encode("utf-8")
    spans = ctx.split_text(TEXT, 0)
    texts = [raw[b:e].decode("utf-8") for b, e in spans]
    long_ms, seq_ms, join_ms = [], [], []
    for i in range(iters + 1):
        t0 = time.perf_counter()
        chunks = ctx.generate_long(TEXT)
        t1 = time.perf_counter()
        joined = ctx.long_audio_as(8000, "mulaw")
        t2 = time.perf_counter()
        for t in texts:
            assert ctx.generate_audio(t)
        t3 = time.perf_counter()
        if i:                                                            # the first round warms both routes
            long_ms.append(1e3 * (t1 - t0)); join_ms.append(1e3 * (t2 - t1)); seq_ms.append(1e3 * (t3 - t2))
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    print(json.dumps(dict(chunks=len(chunks), seconds=sum(len(c["pcm"]) for c in chunks) / 24000.0, joined_bytes=int(joined.size), long_ms=med(long_ms),
                          join_ms=med(join_ms), sequential_ms=med(seq_ms))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_form_time.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--wall-iters", type=int, default=3)
    ap.add_argument("--child", choices=["join", "wall"])
    a = ap.parse_args()
    if a.child == "join":
        return child_join(a.iters)
    if a.child == "wall":
        return child_wall(a.wall_iters)
    lines = ["long-form route; python tools/long_form_time.py", f"join: bark_hip_time_join, mean of {a.iters} joins after 2; segments of {N_EACH} samples (5.12 s), gap 6000", ""]
    for mode, limit in (("join", 240), ("wall", 600)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--iters", str(a.iters), "--wall-iters", str(a.wall_iters)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"{mode}: FAILED (exit {r.returncode}) {r.stderr[-400:]}")
            break                                                         # nothing more is started on the GPU after a failure
        d = json.loads(r.stdout.strip().splitlines()[-1])
        if mode == "join":
            for c in d:
                if "activity_us" in c:
                    lines.append(f"{c['count']:2d} segments, with a trim threshold only: table fill + activity launch, every frame active {c['activity_us']:8.2f} us")
                    continue
                base = "no filter runs: no baseline" if c["resample_us"] is None else \
                    f"resample_pair_kernel over the same {c['total']} samples ({c['launches']} launches) {c['resample_us']:8.2f} us, x{c['join_us'] / c['resample_us']:5.2f}"
                lines.append(f"{c['count']:2d} segments -> {c['rate']:5d} {c['fmt']:5s}: join {c['join_us']:8.2f} us; {base}")
        else:
            lines += ["", f"wall, synthetic `small`, greedy, median of {a.wall_iters} rounds after one: generate_long ({d['chunks']} chunks, {d['seconds']:.1f} s of audio, one job) "
                          f"{d['long_ms']:8.1f} ms; {d['chunks']} sequential bark_generate_audio calls {d['sequential_ms']:8.1f} ms (x{d['sequential_ms'] / d['long_ms']:.2f}); "
                          f"long_audio_as 8000 mu-law ({d['joined_bytes']} bytes) {d['join_ms']:6.2f} ms"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
