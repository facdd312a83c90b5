#!/usr/bin/env python3
"""Times the output rate / sample format conversion (rule C14r): the device time of ONE launch of the rational resampler (bark_hip_time_resample_pair, hipEvents)
for all 14 pairs x 3 formats at 1 s and 20 s of input, beside C13r's kernel (bark_hip_time_resample) in the same run, with the byte floor 4 n + width n_out at
--hbm-tbps; then a 64-utterance lock-step job on the synthetic `small` file and, for its 64 results, the wall clock of ONE bark_hip_resample_many call per format
(the conversion works from the host copy of the audio: upload, launch, download) as a fraction of the job's wall clock, and the share of that call that is not the
launch.  The measurement runs in a child process under a time limit.

Usage: python tools/output_format_time.py [--out profiles/output_format_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATES = (8000, 12000, 16000, 22050, 32000, 44100, 48000)
PAIRS = [(24000, r) for r in RATES] + [(r, 24000) for r in RATES]
FORMATS = ("f32", "s16", "mulaw")
WIDTH = {"f32": 4, "s16": 2, "mulaw": 1}
JOB_FORMATS = [(8000, "mulaw"), (16000, "s16"), (44100, "s16"), (48000, "f32")]


def child(iters: int, job: int):
    import numpy as np
    from bark_amd_loader import load_package
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("small", 0), pkg.default_params(temp=0.7, fine_temp=0.5, n_steps_text_encoder=128), seed=0)
    lib = ctx._lib
    rows = []
    for seconds in (1, 20):
        rows.append(dict(kind="c13r", seconds=seconds, n=24000 * seconds, n_out=(2 * 24000 * seconds + 2) // 3, us=ctx.time_resample(24000 * seconds, iters)))
        for a, b in PAIRS:
            n = a * seconds
            for f in FORMATS:
                rows.append(dict(kind="c14r", seconds=seconds, rate_in=a, rate_out=b, format=f, n=n, n_out=lib.bark_hip_resample_out_len(n, a, b),
                                 us=ctx.time_resample_pair(n, a, b, f, iters)))
    texts = [f"utterance number {i} of the job, with a few more words" for i in range(job)]
    ctx.generate_batch(texts[:4], seeds=list(range(4)))             # warm-up: graphs, scratch
    t0 = time.perf_counter()
    res = ctx.generate_batch(texts, seeds=list(range(job)))
    job_ms = 1e3 * (time.perf_counter() - t0)
    pcm = [r["pcm"] for r in res if r is not None and len(r["pcm"])]
    conv = []
    for rate, f in JOB_FORMATS:
        ctx.resample_many(pcm, 24000, rate, fmt=f)                  # warm-up: the pair's table, the buffers
        ws = []
        for _ in range(5):
            t0 = time.perf_counter()
            out = ctx.resample_many(pcm, 24000, rate, fmt=f)
            ws.append(1e3 * (time.perf_counter() - t0))
        launch_us = sum(ctx.time_resample_pair(len(x), 24000, rate, f, 20) for x in pcm[:8]) / max(len(pcm[:8]), 1) * len(pcm)      # one segment at a time: an upper bound
        conv.append(dict(rate=rate, format=f, wall_ms=sorted(ws)[2], launch_us_upper=launch_us, bytes_in=int(sum(4 * len(x) for x in pcm)), bytes_out=int(sum(o.nbytes for o in out))))
    ctx.free()
    print(json.dumps(dict(rows=rows, job=dict(utterances=len(pcm), samples=int(sum(len(x) for x in pcm)), wall_ms=job_ms), conversions=conv)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_format_time.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--job", type=int, default=64)
    ap.add_argument("--hbm-tbps", type=float, default=8.0, help="HBM rate of the byte floor (the MI355X's datasheet figure)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.iters, a.job)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--job", str(a.job)], capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        sys.exit(f"the measurement failed (rc {r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    d = json.loads(r.stdout.strip().splitlines()[-1])
    lines = [f"# tools/output_format_time.py --iters {a.iters} --job {a.job}: device us per launch (hipEvents), byte floor at {a.hbm_tbps} TB/s",
             f"{'kernel':6} {'pair':>14} {'format':>6} {'input':>5} {'n':>8} {'n_out':>8} {'us':>9} {'floor us':>9} {'x floor':>8}"]
    for w in d["rows"]:
        width = 4 if w["kind"] == "c13r" else WIDTH[w["format"]]
        floor = (4 * w["n"] + width * w["n_out"]) / (a.hbm_tbps * 1e6)
        pair = "24000->16000" if w["kind"] == "c13r" else f"{w['rate_in']}->{w['rate_out']}"
        lines.append(f"{w['kind']:6} {pair:>14} {w.get('format', 'f32'):>6} {w['seconds']:>4}s {w['n']:>8} {w['n_out']:>8} {w['us']:>9.2f} {floor:>9.3f} {w['us'] / floor:>8.1f}")
    j = d["job"]
    lines.append(f"# a lock-step job of {j['utterances']} utterances on `small` ({j['samples']} samples at 24 kHz): {j['wall_ms']:.1f} ms wall clock")
    lines.append("# one bark_hip_resample_many call over its results, from the host copy of the audio (upload + launch + download), median of 5")
    for c in d["conversions"]:
        lines.append(f"convert {c['rate']:>6} {c['format']:>6}: {c['wall_ms']:8.3f} ms wall = {100.0 * c['wall_ms'] / j['wall_ms']:5.2f} % of the job; launches <= {c['launch_us_upper'] / 1e3:.3f} ms, "
                     f"the rest is the copies ({c['bytes_in']} bytes up, {c['bytes_out']} bytes down) and the host's finite check")
    text = "\n".join(lines) + "\n"
    open(a.out, "w").write(text)
    open(os.path.splitext(a.out)[0] + ".json", "w").write(json.dumps(d, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
