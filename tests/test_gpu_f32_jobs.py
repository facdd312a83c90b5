"""Lock-step jobs on f32 model files (what the reference's convert.py writes without --use-f16): the job travels through the lock-step slots like the
jobs of every other weight format - every decode product of a step is ONE launch of gemv_w32_slots_kernel (csrc/quant_kernels.hip: each weight chunk
read once per group of eight slots) - instead of the sequential fallback of one bark_generate_audio per utterance.  Bits per utterance are the
contract: every utterance equals its own live oracle run on the same f32 file (tests/f32_jobs_ref.py), whatever the slot count, the job size or the
company it travels in.  K = 128 / 512 (toy), 256 / 1024 (mini), 768 / 3072 (bark-small); K = 4096 is covered on the host (tests/test_emulated_f32_jobs.py)."""
import os
import threading

import numpy as np
import pytest

from tests.f32_jobs_ref import check_utterance, exact, job_plan, job_reference

pytestmark = pytest.mark.gpu

N_PLAN = 23                                   # the largest job; smaller jobs take the first utterances of the plan
JOB_SIZES = (1, 2, 7, 9, 17, 23)              # sizes that leave a partial slot group, refill slots from the queue and compact the batch


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


@pytest.fixture(scope="module")
def toy_f32_oracle(toy_f32_model):
    from oracle.pyoracle import Oracle
    o = Oracle(toy_f32_model, n_threads=16)
    yield o
    o.close()


_REFS = {}


def _reference(orc, key, i, text, rq, flt, voice):
    """utterance i of the plan `key`: computed once, shared by every job that carries it"""
    if (key, i) not in _REFS:
        _REFS[(key, i)] = job_reference(orc, text, rq, flt, voice)
    return _REFS[(key, i)]


def _voices(pkg, voices):
    return [None if v is None else pkg.VoicePrompt(v.semantic, v.coarse, v.fine) for v in voices]


@pytest.mark.lock_step_job
def test_f32_job_takes_the_lock_step_route(toy_f32_model, toy_model):
    """8 greedy utterances of 20 semantic steps that nothing stops early: the prompt pass takes the first sample, 19 lock steps the others.  The accessor is
    new for every format: the f16 file reports the same kind of count.  bark_hip_time_slots runs the f32 slot product (kind 0, ops 0 - 3) and the attention."""
    import bench
    pkg = _pkg()
    texts = bench.synth_prompts(8, seed=9)
    counts = {}
    for name, path in (("f32", toy_f32_model), ("f16", toy_model)):
        ctx = pkg.BarkContext.load_model(path, pkg.default_params(temp=0.0, fine_temp=0.0, min_eos_p=2.0, n_steps_text_encoder=20), 0)
        try:
            assert ctx.batch_lock_steps() is None, "no job has run yet"
            ctx.reserve_batch(8)
            res = ctx.generate_batch(texts)
            assert all(r is not None and 0 < len(r["semantic"]) <= 20 for r in res)
            counts[name] = ctx.batch_lock_steps()
            assert counts[name] is not None and 0 < counts[name][0] <= 21 and counts[name][1] > 0, (name, counts[name])
            if name == "f32":
                for op in (0, 1, 2, 3, 5):
                    assert ctx.time_slots(0, op, 8, 0, 64, 5) >= 0
                for op, kind in ((4, 0), (0, 1), (2, 6)):                 # no f16 rows to normalise, no matrix-core kinds on an f32 file
                    with pytest.raises(RuntimeError):
                        ctx.time_slots(0, op, 8, kind, 64, 5)
                tl = ctx.profile_lock_step(0, 8, 64, 3)
                assert tl[-1]["site"] == "step (graph replay)" and all(e["us"] > 0 for e in tl)
        finally:
            ctx.free()


@pytest.mark.lock_step_job
@pytest.mark.parametrize("slots", [8, 64])
def test_ragged_f32_jobs_equal_the_oracle_per_utterance(slots, toy_f32_model, toy_f32_oracle):
    """Jobs of 1 .. 23 utterances with caps 1 .. 40 on 8 and on 64 slots (queue, refills, compaction, partial slot groups), greedy and sampled utterances
    with their own seeds, a top-k / top-p filter on some, one voiced utterance, and a second job on the same context."""
    pkg = _pkg()
    ctx = pkg.BarkContext.load_model(toy_f32_model, pkg.default_params(), seed=3)
    try:
        ctx.reserve_batch(slots)
        texts, reqs, flts, voices = job_plan(ctx, N_PLAN)
        assert {r.n_steps_text_encoder for r in reqs} >= {1, 40} and any(v is not None for v in voices)
        pv = _voices(pkg, voices)
        for n in JOB_SIZES:
            res = ctx.generate_batch(texts[:n], params=reqs[:n], filters=flts[:n], voices=pv[:n])
            steps = ctx.batch_lock_steps()
            assert steps is not None and steps[1] > 0, f"job of {n} on {slots} slots went through the sequential fallback: {steps}"
            for i in range(n):
                check_utterance(f"f32 toy job of {n} on {slots} slots, utterance {i}", res[i], _reference(toy_f32_oracle, "toy", i, texts[i], reqs[i], flts[i], voices[i]))
        # another job on the same context, other company: the last utterances of the plan in reverse order
        idx = list(range(N_PLAN - 1, N_PLAN - 6, -1))
        res = ctx.generate_batch([texts[i] for i in idx], params=[reqs[i] for i in idx], filters=[flts[i] for i in idx], voices=[pv[i] for i in idx])
        for k, i in enumerate(idx):
            check_utterance(f"second job on {slots} slots, utterance {i}", res[k], _reference(toy_f32_oracle, "toy", i, texts[i], reqs[i], flts[i], voices[i]))
    finally:
        ctx.free()


@pytest.mark.lock_step_job
def test_f32_job_at_k_256_and_1024_equals_the_oracle(tmp_path):
    """The mini preset as an f32 file: K = 256 (two rounds of the 16 chains) and K = 1024; 9 utterances on 8 slots."""
    from oracle.pyoracle import Oracle
    from tools.make_synth_model import write_model
    pkg = _pkg()
    path = write_model(str(tmp_path / "bark_mini_f32.bin"), "mini", 0, use_f16=False)
    orc = ctx = None
    try:
        orc = Oracle(path, n_threads=16)
        ctx = pkg.BarkContext.load_model(path, pkg.default_params(), seed=3)
        assert ctx.hparams(0)["ftype"] == 0 and ctx.hparams(0)["n_embd"] == 256
        ctx.reserve_batch(8)
        texts, reqs, flts, voices = job_plan(ctx, 9, max_cap=24)
        res = ctx.generate_batch(texts, params=reqs, filters=flts, voices=_voices(pkg, voices))
        assert ctx.batch_lock_steps()[1] > 0
        for i in range(9):
            check_utterance(f"f32 mini job, utterance {i}", res[i], job_reference(orc, texts[i], reqs[i], flts[i], voices[i]))
    finally:
        if ctx is not None:
            ctx.free()
        if orc is not None:
            orc.close()
        os.remove(path)


@pytest.mark.lock_step_job
def test_f32_job_at_bark_small_shapes(tmp_path):
    """K = 768 / 3072: a bark-small f32 file, 5 greedy utterances with caps <= 8.  Semantic and coarse ids per utterance equal bark_hip_semantic /
    bark_hip_coarse on a fresh context of the same library (that route is pinned to the oracle at these shapes by tests/test_gpu_weight_formats.py), the
    semantic ids also the oracle's.  Fine ids and PCM are not asserted here: the job's fine passes and codec are those of every f32 context, and the CPU
    oracle needs minutes for them at this size."""
    import bench
    from oracle.pyoracle import Oracle
    from tools.make_synth_model import write_model
    pkg = _pkg()
    path = write_model(str(tmp_path / "bark_small_f32.bin"), "small", 0, use_f16=False)
    orc = ctx = single = None
    try:
        texts = bench.synth_prompts(5, seed=7)
        caps = [8, 3, 6, 1, 7]
        ctx = pkg.BarkContext.load_model(path, pkg.default_params(temp=0.0, fine_temp=0.0), 0)
        assert ctx.hparams(0)["ftype"] == 0 and ctx.hparams(0)["n_embd"] == 768
        ctx.reserve_batch(8)
        res = ctx.generate_batch(texts, params=[ctx.request_params(n_steps_text_encoder=c) for c in caps])
        steps = ctx.batch_lock_steps()
        assert steps is not None and steps[0] > 0 and steps[1] > 0, steps
        ctx.free(); ctx = None
        single = pkg.BarkContext.load_model(path, pkg.default_params(temp=0.0, fine_temp=0.0), 0)
        orc = Oracle(path, n_threads=16)
        for i, (text, cap) in enumerate(zip(texts, caps)):
            single.set_params(pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=cap))
            sem = single.semantic(single.tokenize(text))
            assert res[i] is not None and len(sem) > 0
            exact(f"bark-small f32 job, utterance {i} semantic vs bark_hip_semantic", res[i]["semantic"], sem)
            exact(f"bark-small f32 job, utterance {i} coarse vs bark_hip_coarse", res[i]["coarse"], single.coarse(sem))
            exact(f"bark-small f32 job, utterance {i} semantic vs the oracle", res[i]["semantic"],
                  orc.semantic(orc.tokenize(text), orc.params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=cap)))
    finally:
        for c in (ctx, single):
            if c is not None:
                c.free()
        if orc is not None:
            orc.close()
        os.remove(path)


@pytest.mark.concurrency
def test_request_collector_on_an_f32_context(toy_f32_model):
    """Requests with their own parameters submitted to a bark_hip_batcher on an f32 context while the opener's job runs: whether one joins the running job
    (continuous admission) or waits for the next is a matter of timing - every result is what a fresh context with the request's parameters and seed
    generates."""
    import bench
    pkg = _pkg()
    texts = bench.synth_prompts(7, seed=11)
    c = pkg.BarkContext.load_model(toy_f32_model, pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=24), 0)
    b = pkg.Batcher(c, max_batch=8, max_wait_ms=1)
    reqs = [c.request_params(n_steps_text_encoder=300, min_eos_p=2.0)]                       # the opener: hundreds of lock steps
    reqs += [c.request_params(n_steps_text_encoder=6 + 5 * i, temp=0.7 if i % 3 == 0 else 0.0, fine_temp=0.5 if i % 3 == 0 else 0.0, seed=200 + i) for i in range(1, len(texts))]
    out = [None] * len(texts)
    errors = []

    def client(i):
        try:
            out[i] = b.wait(b.submit(texts[i], params=reqs[i]))
        except Exception as e:                                  # noqa: BLE001 - reported below with the request's index
            errors.append((i, repr(e)))

    try:
        th = [threading.Thread(target=client, args=(i,)) for i in range(len(texts))]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errors, errors
        assert b.stats()["n_requests"] == len(texts)
    finally:
        b.free()
        c.free()
    for i, (text, rq) in enumerate(zip(texts, reqs)):
        fresh = pkg.BarkContext.load_model(toy_f32_model, pkg.default_params(temp=rq.temp, fine_temp=rq.fine_temp, min_eos_p=rq.min_eos_p,
                                                                             n_steps_text_encoder=rq.n_steps_text_encoder), seed=int(rq.seed))
        try:
            assert fresh.generate_audio(text)
            exact(f"request {i} pcm vs a fresh context", out[i], fresh.audio_data())
        finally:
            fresh.free()
