#!/usr/bin/env python3
"""Times the time-scale kernel (rule C16t, bark_hip_time_tempo: hipEvents around --iters launches, after two warm-up launches) on 1 and 64 segments of
5.12 s (122 880 samples) at speeds 0.5, 1.25 and 2.0, and beside it the long-form join (bark_hip_time_join) over the same segments at 24 kHz f32 as the
neighbour to compare with.  Every case is measured --repeats times in one process, alternating the cases, and reported as median and spread; the time per
frame is the launch time over the frames of ONE segment (the segments of a launch run side by side, one workgroup each).

Usage: python tools/tempo_time.py [--out profiles/tempo_time.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 122880
CASES = [(count, speed) for count in (1, 64) for speed in (0.5, 1.25, 2.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempo_time.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from bark_amd_loader import load_package
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    tempo = {c: [] for c in CASES}
    join = {1: [], 64: []}
    for _ in range(a.repeats):
        for count, speed in CASES:
            tempo[(count, speed)].append(ctx.time_tempo(count, N, speed, a.iters))
        for count in join:
            join[count].append(ctx.time_join(count, N, 24000, "f32", a.iters))
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    lines = ["time-scale kernel (rule C16t), segments of 122 880 samples (5.12 s at 24 kHz); python tools/tempo_time.py",
             f"device time of one launch in us (hipEvents around {a.iters} launches), median [min .. max] of {a.repeats} measurements taken in turn", ""]
    rows = []
    for count, speed in CASES:
        p = pkg.speed_permille(speed)
        frames = (-(-1000 * N // p) + 359) // 360
        v = tempo[(count, speed)]
        rows.append(dict(segments=count, speed_permille=p, frames_per_segment=frames, us_median=med(v), us_min=min(v), us_max=max(v), us_per_frame=med(v) / frames))
        lines.append(f"tempo {count:2d} x 122880 at {p:4d} per mille: {med(v):9.1f} us [{min(v):9.1f} .. {max(v):9.1f}], {frames:3d} frames a segment, {med(v) / frames:6.2f} us per frame")
    for count, v in join.items():
        rows.append(dict(segments=count, join_us_median=med(v), join_us_min=min(v), join_us_max=max(v)))
        lines.append(f"join  {count:2d} x 122880 to 24000 f32:        {med(v):9.1f} us [{min(v):9.1f} .. {max(v):9.1f}]")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    open(os.path.splitext(a.out)[0] + ".json", "w").write(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
