#!/usr/bin/env python3
"""Times the FLAC encoder (rule C18f, bark_hip_time_flac / _flac_launch: hipEvents around --iters launches, after two warm-up launches): the two launches
together, and the frames and the pack launch alone, over 1, 8 and 64 results of 1 s, 5.12 s and 15 s at 24 kHz (a synthetic voiced signal: the codes'
lengths, and with them the time, depend on the values).  Every case is measured --repeats times in one process, alternating the cases, and reported as median
and spread.  Beside them: the resampler's launch (24000 -> 16000 s16, bark_hip_time_resample_pair) over the same samples, as launches of at most 1 310 720
samples; the share of the two launches of ONE 5.12 s result in the time bark-small takes to generate such an utterance alone (--generation-ms-per-s, the figure
DESIGN.md section 6 derives from the recorded benchmark; the loudness section uses the same); and, on the benchmark's utterance (bench.py's first prompt,
bark-small, 256 semantic steps), the FLAC bytes against the s16 bytes - what crosses to the host and goes out in the HTTP body.

Usage: python tools/flac_time.py [--out profiles/flac_time.json] [--no-utterance]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = [24000, 122880, 360000]
COUNTS = [1, 8, 64]
CASES = [(count, n, which) for n in LENGTHS for count in COUNTS for which in (0, 1, 2)]
NAMES = {0: "frames + pack", 1: "flac_frames ", 2: "flac_pack   "}
MAX_LAUNCH = 1310720


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_time.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--generation-ms-per-s", type=float, default=222.0 / 5.12)
    ap.add_argument("--no-utterance", action="store_true", help="skip the benchmark utterance (it needs the bark-small model file)")
    a = ap.parse_args()
    from bark_amd_loader import load_package
    from tools.make_synth_model import ensure_model
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    times = {c: [] for c in CASES}
    for _ in range(a.repeats):
        for count, n, which in CASES:
            times[(count, n, which)].append(ctx.time_flac(count, n, a.iters, which))
    resample = {}
    for n in LENGTHS:
        for count in COUNTS:
            parts = -(-count * n // MAX_LAUNCH)
            resample[(count, n)] = parts * ctx.time_resample_pair(-(-count * n // parts), 24000, 16000, "s16", a.iters)
    ctx.free()
    med = lambda v: float(sorted(v)[len(v) // 2])
    lines = ["FLAC encoder (rule C18f) over results of 24 000 (1 s), 122 880 (5.12 s) and 360 000 (15 s) samples at 24 kHz; python tools/flac_time.py",
             f"device time in us (hipEvents around {a.iters} launches), median [min .. max] of {a.repeats} measurements taken in turn", ""]
    rows = []
    for count, n, which in CASES:
        v = times[(count, n, which)]
        frames = count * -(-n // 4096)
        rows.append(dict(launch=NAMES[which].strip(), results=count, samples=n, frames=frames, us_median=med(v), us_min=min(v), us_max=max(v)))
        lines.append(f"{NAMES[which]} {count:2d} x {n:6d}: {med(v):9.1f} us [{min(v):9.1f} .. {max(v):9.1f}], {frames:5d} frames")
        if which == 2:
            both, rs = med(times[(count, n, 0)]), resample[(count, n)]
            rows.append(dict(results=count, samples=n, resample_24000_to_16000_s16_us=rs, both_over_resample=both / rs))
            lines.append(f"   the resampler over the same samples (24000 -> 16000 s16): {rs:9.1f} us; the two launches are {both / rs:5.2f} times that")
    lines.append("")
    n = 122880
    for count in (1, 64):
        both = med(times[(count, n, 0)])
        gen_ms = a.generation_ms_per_s * n / 24000.0
        share = 100.0 * both / (1000.0 * gen_ms)
        rows.append(dict(results=count, samples=n, both_launches_us=both, generation_ms_one_utterance=gen_ms, share_percent=share))
        lines.append(f"both launches, {count:2d} x {n}: {both:9.1f} us = {share:5.2f} % of the {gen_ms:7.1f} ms ONE such utterance takes to generate ({a.generation_ms_per_s:g} ms per second of audio)")
    # what the encoder makes of the timed signal itself (engine_time_flac's voiced tone, restated here): the synthetic weights of the benchmark give noise
    import numpy as np
    import flac_ref
    i = np.arange(n, dtype=np.float64)
    lcg, noise = 12345, np.zeros(n)
    for k in range(n):
        lcg = (lcg * 1664525 + 1013904223) & 0xFFFFFFFF
        noise[k] = (lcg >> 25) - 64
    env = 0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * i / 24000.0)
    voiced = np.round(6000.0 * env * np.sin(2.0 * np.pi * 220.0 * i / 24000.0) + 1500.0 * env * np.sin(2.0 * np.pi * 1870.0 * i / 24000.0) + noise).astype(np.int16)
    tone = pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    stream = tone.flac_encode(voiced, 24000)
    tone.free()
    assert stream == flac_ref.encode(voiced, 24000)
    rows.append(dict(signal="the timed voiced tone", samples=n, s16_bytes=2 * n, flac_bytes=len(stream), flac_over_s16=len(stream) / (2.0 * n)))
    lines += ["", f"the timed signal (a voiced tone with noise of +-64 on top), {n} samples: s16 {2 * n} bytes, FLAC {len(stream)} bytes: {len(stream) / (2.0 * n):.3f} of s16"]
    if not a.no_utterance:
        import bench
        text = bench.synth_prompts(1)[0]
        big = pkg.BarkContext.load_model(ensure_model("small", 0), pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=256), seed=0)
        assert big.generate_audio(text)
        lines.append("")
        for rate in (24000, 16000):
            s16 = big.audio_as(rate, "s16")
            flac = big.audio_as(rate, "flac").tobytes()
            assert flac == flac_ref.encode(s16, rate) and (flac_ref.decode(flac)[0] == s16).all()
            ratio = len(flac) / (2.0 * len(s16))
            rows.append(dict(utterance="bench.py prompt 0, bark-small, 256 semantic steps", rate=rate, samples=len(s16), s16_bytes=2 * len(s16), flac_bytes=len(flac), flac_over_s16=ratio))
            lines.append(f"benchmark utterance at {rate} Hz: {len(s16)} samples, s16 {2 * len(s16)} bytes, FLAC {len(flac)} bytes copied to the host: {ratio:.3f} of s16")
        big.free()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(rows, indent=1) + "\n")
    open(os.path.splitext(a.out)[0] + ".txt", "w").write(text)


if __name__ == "__main__":
    main()
