"""Shared by tests/test_gpu_f32_jobs.py and tests/test_emulated_f32_jobs.py: the plan of a ragged lock-step job (per-utterance step caps, greedy and
sampled utterances with their own seeds, a top-k / top-p filter on some, one voice prompt) and the reference of one utterance - its own live oracle run
on the model file: Oracle.generate, or, for the utterances with a filter or a voice (which Oracle.generate does not know), the reference loops of
tests/voice_prompt_ref.py over the same oracle's evaluations (rules C8n and C10v)."""
import numpy as np

from tests import voice_prompt_ref as R

VOICED = 4              # the utterance of a plan that carries a voice prompt


def job_plan(ctx, n, max_cap=40):
    """-> texts, request parameters, filters (top_k, top_p), voices (tests/voice_prompt_ref.Voice or None) of utterances 0 .. n - 1; a job of m <= n
    utterances takes the first m, so one reference per utterance serves every job size and slot count"""
    import bench
    texts = bench.synth_prompts(n, seed=5)
    reqs, flts, voices = [], [], []
    for i in range(n):
        sampled = i % 3 == 1
        reqs.append(ctx.request_params(temp=0.7 if sampled else 0.0, fine_temp=0.5 if i % 4 == 2 else 0.0, min_eos_p=0.2,
                                       n_steps_text_encoder=1 + (7 * i) % max_cap, seed=500 + i))
        flts.append((50, 0.9) if i % 6 == 1 else (0, 0.95) if i == 10 else (0, 1.0))
        voices.append(R.synthetic_voice(12, 35, 41, 41) if i == VOICED else None)
    return texts, reqs, flts, voices


def job_reference(orc, text, rq, flt, voice):
    if voice is None and tuple(flt) == (0, 1.0):
        orc.seed(int(rq.seed))
        return orc.generate(text, orc.params(temp=rq.temp, fine_temp=rq.fine_temp, min_eos_p=rq.min_eos_p, n_steps_text_encoder=rq.n_steps_text_encoder))
    # the loops of voice_prompt_ref.generate, stage by stage: an utterance that stops at its first sample has no coarse stage
    smp = R.Sampler(int(rq.seed))
    sem = R.semantic(orc, orc.tokenize(text), voice, rq.temp, rq.min_eos_p, rq.n_steps_text_encoder, smp, flt[0], flt[1])
    n_steps = int(np.floor(np.float32(np.float32(np.float32(len(sem)) * R.ratio()) / np.float32(R.N_COARSE))) * R.N_COARSE)
    if n_steps == 0:
        return dict(semantic=sem, n_frames=0)
    co = R.coarse(orc, sem, voice, rq.temp, sampler=smp, top_k=flt[0], top_p=flt[1])
    fi = R.fine(orc, co, voice, rq.fine_temp, smp)
    return dict(semantic=sem, coarse=co, fine=fi, pcm=orc.codec_decode(fi.T.copy()), n_frames=len(fi))


def exact(name, got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    if not np.array_equal(got, ref):
        bad = np.flatnonzero(got.ravel() != ref.ravel())
        raise AssertionError(f"{name}: {bad.size}/{got.size} elements differ, first at {bad[0]}")


def check_utterance(tag, r, ref):
    """the pattern of tests/test_gpu_batch_ragged.py::_check_job for one utterance"""
    if len(ref["semantic"]) == 0 or ref["n_frames"] == 0:
        assert r is None or len(r["pcm"]) == 0, tag + ": the oracle produced no audio"
        return
    assert r is not None, tag + ": no audio"
    for k in ("semantic", "coarse", "fine", "pcm"):
        exact(f"{tag} {k}", r[k], ref[k])
