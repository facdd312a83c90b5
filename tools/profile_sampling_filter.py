#!/usr/bin/env python3
"""Timing of the top-k / nucleus filter (rule C8n) through bark_hip_time_sample_filter and bark_hip_time_decode_step; writes
profiles/sampling_filter.txt.

  python tools/profile_sampling_filter.py [--out profiles/sampling_filter.txt] [--iters 50]
      one filter launch (hipEvents around the kernel alone) for n = 10 048 / 1024 logits per row, 1 / 8 / 64 slots, top_p in {0.5, 0.9, 0.99} x
      top_k in {0, 50}, on peaked rows (N(0, 1) x 4: a nucleus of a few hundred ids at n = 10 048) and flat rows (N(0, 1) x 0.01: nucleus ~ n);
      then the semantic / coarse decode step greedy, temp-only and filtered (the step the stage loops replay, 8 steps per graph).
  python tools/profile_sampling_filter.py --stage [n]
      n filtered semantic stages on the bench model (temp 0.7, top_k 50, top_p 0.9): the driver of a rocprofv3 --kernel-trace --stats run."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bark_amd_loader import load_package  # noqa: E402
from tools.make_synth_model import ensure_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_filter.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--stage", type=int, default=0, help="run this many filtered semantic stages and exit (rocprofv3 driver)")
    a = ap.parse_args()
    pkg = load_package()
    path = ensure_model("small", 0)
    ctx = pkg.BarkContext.load_model(path, pkg.default_params(temp=0.7, fine_temp=0.0, n_steps_text_encoder=256), 0)
    if a.stage:
        ctx.set_sampling_filter(50, 0.9)
        prompt = ctx.tokenize("the quick brown fox jumps over the lazy dog")
        for i in range(a.stage):
            t0 = time.time()
            ids = ctx.semantic(prompt)
            print(f"filtered semantic stage {i}: {len(ids)} ids, {1e3 * (time.time() - t0):.1f} ms host wall clock")
        ctx.free()
        return
    lines = [f"# tools/profile_sampling_filter.py: device time of ONE filter launch (us, mean of {a.iters}; hipEvents around the kernel, rows restored",
             "# outside the timed interval); 1024 threads per slot, one workgroup per slot.  peaked: N(0,1) x 4 logits, flat: N(0,1) x 0.01.",
             f"# {ctx.describe()}",
             "n      slots  rows    top_k  top_p   us"]
    worst = {}
    for n in (10048, 1024):
        for slots in (1, 8, 64):
            for peaked in (True, False):
                for top_p in (0.5, 0.9, 0.99):
                    for top_k in (0, 50):
                        us = ctx.time_sample_filter(n, slots, top_k, top_p, peaked, a.iters)
                        lines.append(f"{n:<6d} {slots:<6d} {'peaked' if peaked else 'flat':<7s} {top_k:<6d} {top_p:<7.2f} {us:8.2f}")
                        key = (n, slots, peaked)
                        worst[key] = max(worst.get(key, 0.0), us)
                # top-k alone
                us = ctx.time_sample_filter(n, slots, 50, 1.0, peaked, a.iters)
                lines.append(f"{n:<6d} {slots:<6d} {'peaked' if peaked else 'flat':<7s} {50:<6d} {1.0:<7.2f} {us:8.2f}")
    lines.append("")
    lines.append("worst case per (n, slots, rows): " + ", ".join(f"{n}/{s}/{'peaked' if p else 'flat'} {v:.2f} us" for (n, s, p), v in worst.items()))
    lines.append("")
    lines.append("decode step (us, bark_hip_time_decode_step at context 640: layers + LM head + sampling, 8 steps per graph replay)")
    for which, name in ((0, "semantic"), (1, "coarse")):
        res = {}
        for label, temp, flt in (("greedy", 0.0, (0, 1.0)), ("temp 0.7", 0.7, (0, 1.0)), ("temp 0.7 top_k 50 top_p 0.9", 0.7, (50, 0.9)),
                                 ("temp 0.7 top_p 0.9", 0.7, (0, 0.9)), ("temp 0.7 top_k 50", 0.7, (50, 1.0))):
            ctx.set_params(pkg.default_params(temp=temp, fine_temp=0.0, n_steps_text_encoder=256))
            ctx.set_sampling_filter(*flt)
            us, _ = ctx.time_decode_step(which, 640, 800)
            res[label] = us
            lines.append(f"  {name:<8s} {label:<30s} {us:8.2f}")
        base = res["temp 0.7"]
        lines.append(f"  {name:<8s} filtered (top_k 50, top_p 0.9) vs temp-only: {100.0 * (res['temp 0.7 top_k 50 top_p 0.9'] / base - 1.0):+.1f} %")
    ctx.free()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
