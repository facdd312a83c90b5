#!/usr/bin/env python3
"""Times the two loudness kernels (rule C17l, bark_hip_time_loudness: hipEvents around --iters launches, after two warm-up launches): loudness_hops and
loudness_level (gates, gain and the scaled copy) on 1 and 64 segments of 5.12 s (122 880 samples) and of 13 s (312 000 samples).  Every case is measured
--repeats times in one process, alternating the cases, and reported as median and spread.  The share of the generation is the two launches of ONE segment
against the time bark-small takes to generate such an utterance alone (--generation-ms-per-s: milliseconds of generation per second of audio, the figure
DESIGN.md section 6 derives from the recorded benchmark; the tempo section uses the same).

Usage: python tools/loudness_time.py [--out profiles/loudness_time.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [122880, 312000]
CASES = [(count, n, level) for n in LENGTHS for count in (1, 64) for level in (False, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_time.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--generation-ms-per-s", type=float, default=222.0 / 5.12)
    a = ap.parse_args()
    from bark_amd_loader import load_package
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    times = {c: [] for c in CASES}
    for _ in range(a.repeats):
        for count, n, level in CASES:
            times[(count, n, level)].append(ctx.time_loudness(count, n, level, a.iters))
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    lines = ["loudness kernels (rule C17l), segments of 122 880 samples (5.12 s) and 312 000 samples (13 s) at 24 kHz; python tools/loudness_time.py",
             f"device time of one launch in us (hipEvents around {a.iters} launches), median [min .. max] of {a.repeats} measurements taken in turn", ""]
    rows = []
    for count, n, level in CASES:
        v = times[(count, n, level)]
        name = "loudness_level" if level else "loudness_hops "
        rows.append(dict(kernel=name.strip(), segments=count, samples=n, hops_per_segment=n // 2400, us_median=med(v), us_min=min(v), us_max=max(v)))
        lines.append(f"{name} {count:2d} x {n:6d}: {med(v):9.1f} us [{min(v):9.1f} .. {max(v):9.1f}], {n // 2400:3d} hops a segment")
    lines.append("")
    for n in LENGTHS:
        both = med(times[(1, n, False)]) + med(times[(1, n, True)])
        gen_ms = a.generation_ms_per_s * n / 24000.0
        share = 100.0 * both / (1000.0 * gen_ms)
        rows.append(dict(samples=n, both_launches_us=both, generation_ms=gen_ms, share_percent=share))
        lines.append(f"both launches, 1 x {n:6d}: {both:9.1f} us = {share:5.2f} % of the {gen_ms:7.1f} ms such an utterance takes to generate ({a.generation_ms_per_s:g} ms per second of audio)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    open(os.path.splitext(a.out)[0] + ".json", "w").write(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
