#!/usr/bin/env python3
"""Lock-step jobs on an f32 model file, measured:
  slots    bark_hip_time_slots per product and for the attention at 1 .. 64 slots (gemv_w32_slots_kernel: kind 0), one bark_hip_profile_lock_step time line
  jobs     wall time of greedy jobs of n utterances (`--steps` semantic steps each, nothing stops early) per library ARM, arms alternated, every
           arm in a fresh process per round: `--arm name=path/to/libbark.so` (repeatable).  An arm is driven through the handful of C entry points
           every library version has, so the sequential fallback of an older build can stand beside the lock-step route of this one.
usage: f32_jobs_time.py slots|jobs [--model FILE | --preset small] [--arm name=lib ...] [--jobs 8,16,64] [--steps 64] [--reps 2] [--rounds 2] [--out FILE]
Without --model the preset is written as an f32 file into a temporary directory and removed afterwards."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def slots(model, out):
    from bark_amd_loader import load_package
    pkg = load_package()
    ctx = pkg.BarkContext.load_model(model, pkg.default_params(temp=0.0, fine_temp=0.0), 0)
    ctx.reserve_batch(64)
    names = ["qkv", "proj", "fc_gelu", "mproj"]
    res = {"model": os.path.basename(model), "describe": ctx.describe(), "ctx": 640, "us_per_launch": {}}
    for B in (1, 2, 8, 16, 32, 64):
        row = {n: round(ctx.time_slots(0, op, B, 0, 640, 960), 2) for op, n in enumerate(names)}
        row["attention"] = round(ctx.time_slots(0, 5, B, 1, 640, 480), 2)
        res["us_per_launch"][f"B{B}"] = row
        print(f"B={B:2d}  " + "  ".join(f"{k} {v:7.2f}" for k, v in row.items()), flush=True)
    res["single_utterance_gemv_us"] = {n: round(ctx.time_gemv(0, op, 960)[0], 2) for op, n in enumerate(names)}
    print("one utterance (gemv_w32_kernel)  " + "  ".join(f"{k} {v:7.2f}" for k, v in res["single_utterance_gemv_us"].items()), flush=True)
    tl = ctx.profile_lock_step(1, 16, 640, 20)
    sites = {}
    for e in tl[:-1]:
        sites[e["site"]] = sites.get(e["site"], 0.0) + e["us"]
    res["lock_step_16_slots_coarse_ctx640"] = {"per_site_us": {k: round(v, 1) for k, v in sites.items()}, "eager_step_us": round(sum(sites.values()), 1),
                                                "graph_step_us": round(tl[-1]["us"], 1)}
    print("lock step, 16 slots, coarse, context 640: " + json.dumps(res["lock_step_16_slots_coarse_ctx640"]), flush=True)
    ctx.free()
    if out:
        json.dump(res, open(out, "w"), indent=1)


def job_child(model, lib_path, sizes, steps, reps):
    """one arm in this process: for every job size a warm-up job (allocations, graph captures), then `reps` timed ones"""
    import bench
    from bark_amd_loader import load_package
    api = load_package().api
    lib = C.CDLL(lib_path)
    lib.bark_context_default_params.restype = api.BarkContextParams
    lib.bark_load_model.restype = C.c_void_p
    lib.bark_load_model.argtypes = [C.c_char_p, api.BarkContextParams, C.c_uint32]
    lib.bark_hip_reserve_batch.argtypes = [C.c_void_p, C.c_int]
    lib.bark_hip_generate_batch.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int]
    lib.bark_hip_get_stats.argtypes = [C.c_void_p, C.POINTER(api.BarkHipStats)]
    lib.bark_free.argtypes = [C.c_void_p]
    p = lib.bark_context_default_params()
    p.temp = 0.0; p.fine_temp = 0.0; p.min_eos_p = 2.0; p.n_steps_text_encoder = steps
    for n in sizes:
        h = lib.bark_load_model(model.encode(), p, 0)
        assert h, "bark_load_model failed"
        assert lib.bark_hip_reserve_batch(h, max(n, 8)) == 0
        texts = bench.synth_prompts(n, seed=1)
        ts = (C.c_char_p * n)(*[t.encode() for t in texts])
        assert lib.bark_hip_generate_batch(h, ts, n) == n
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            good = lib.bark_hip_generate_batch(h, ts, n)
            walls.append(time.perf_counter() - t0)
            assert good == n
        st = api.BarkHipStats()
        lib.bark_hip_get_stats(h, C.byref(st))
        lock = None
        if hasattr(lib, "bark_hip_batch_lock_steps"):
            o = (C.c_int32 * 2)()
            lock = [int(o[0]), int(o[1])] if lib.bark_hip_batch_lock_steps(C.c_void_p(h), o) == 0 else None
        print("JOB " + json.dumps({"n": n, "wall_s": [round(w, 4) for w in walls], "lock_steps": lock,
                                   "t_semantic_ms": st.t_semantic_us / 1e3, "t_coarse_ms": st.t_coarse_us / 1e3, "t_fine_ms": st.t_fine_us / 1e3}), flush=True)
        lib.bark_free(h)


def jobs(model, arms, sizes, steps, reps, rounds, out):
    res = {"model": os.path.basename(model), "steps": steps, "arms": {name: {} for name, _ in arms}}
    for rnd in range(rounds):
        for name, lib in arms:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "job-child", "--model", model, "--arm", f"{name}={lib}", "--jobs", ",".join(map(str, sizes)),
                                "--steps", str(steps), "--reps", str(reps)], capture_output=True, text=True, timeout=1500)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-3000:])
                raise SystemExit(f"arm {name} failed (rc {r.returncode})")
            for line in r.stdout.splitlines():
                if line.startswith("JOB "):
                    j = json.loads(line[4:])
                    res["arms"][name].setdefault(str(j["n"]), []).append(j)
                    print(f"round {rnd} {name:8s} n={j['n']:3d} wall {j['wall_s']} s  lock steps {j['lock_steps']}  last job: semantic {j['t_semantic_ms']:.0f} coarse {j['t_coarse_ms']:.0f} fine {j['t_fine_ms']:.0f} ms", flush=True)
    # per size: the median and the spread (min .. max over rounds and repetitions) of every arm, and the ratio of the medians against the first arm
    base = arms[0][0]
    for n in map(str, sizes):
        row = {}
        for name, _ in arms:
            w = sorted(x for j in res["arms"][name].get(n, []) for x in j["wall_s"])
            row[name] = {"median_s": w[len(w) // 2], "min_s": w[0], "max_s": w[-1]}
        for name, _ in arms[1:]:
            row[f"{base}/{name}"] = round(row[base]["median_s"] / row[name]["median_s"], 3)
        res.setdefault("summary", {})[n] = row
        print(f"n={n}: " + json.dumps(row), flush=True)
    if out:
        json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["slots", "jobs", "job-child"])
    ap.add_argument("--model")
    ap.add_argument("--preset", default="small")
    ap.add_argument("--arm", action="append", default=[])
    ap.add_argument("--jobs", default="8,16,64")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    arms = [tuple(v.split("=", 1)) for v in a.arm] or [("this", os.path.join(ROOT, "bark.cpp_amd", "lib", "libbark.so"))]
    sizes = [int(v) for v in a.jobs.split(",")]
    if a.mode == "job-child":
        job_child(a.model, arms[0][1], sizes, a.steps, a.reps)
        return
    tmp = None
    model = a.model
    if not model:
        from tools.make_synth_model import write_model
        tmp = tempfile.mkdtemp(prefix="bark_f32_")
        model = write_model(os.path.join(tmp, f"bark_{a.preset}_f32.bin"), a.preset, 0, use_f16=False)
    try:
        if a.mode == "slots":
            slots(model, a.out)
        else:
            jobs(model, arms, sizes, a.steps, a.reps, a.rounds, a.out)
    finally:
        if tmp:
            os.remove(model)
            os.rmdir(tmp)


if __name__ == "__main__":
    main()
