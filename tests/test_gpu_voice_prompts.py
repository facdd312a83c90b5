"""GPU tests of voice prompts (speaker history, rule C10v of DESIGN.md section 3): the engine against tests/voice_prompt_ref.py - the rule as three plain
Python loops over the CPU oracle's evaluations, pinned to the oracle and to HuggingFace's generate(history_prompt=...) by tests/test_voice_prompt_ref.py -
bit for bit, on live oracle runs."""
import json
import os
import socket
import subprocess
import sys
import time
import urllib.error
import urllib.request

import numpy as np
import pytest

from tests import nucleus_ref
from tests import voice_prompt_ref as R

pytestmark = pytest.mark.gpu
# Place in the suite (tests/conftest.py): the row-level tests of this file carry `boundary` - behind the per-row parity group of test_gpu_parity.py, in front
# of the lock-step jobs - as the row-level tests of the other files added since do; job tests carry `lock_step_job`, collector / server tests `concurrency`.

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "hello world , the water is cold today and the river runs fast !"
# (n_sem, Tc, Tf): short - n_sem odd, floor(2 Tc / r) = 27 the smallest term and odd, n_ch = 81: the kept coarse history starts on the second codebook;
# full - every cap active (n_sh 209, n_ch 628, 256 prompt ids, 512 fine rows); tf100 - fewer than 512 fine rows
HISTORIES = {"short": (35, 41, 41), "full": (300, 700, 700), "tf100": (120, 200, 100)}
MODES = {"greedy": dict(temp=0.0, fine_temp=0.0, top_k=0, top_p=1.0), "sampled": dict(temp=0.7, fine_temp=0.5, top_k=40, top_p=0.9)}


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _voice(name, seed=11):
    n_sem, tc, tf = HISTORIES[name]
    return R.synthetic_voice(seed + sorted(HISTORIES).index(name), n_sem, tc, tf)


def _exact(name, got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    if not np.array_equal(got, ref):
        bad = np.flatnonzero(got.ravel() != ref.ravel())
        raise AssertionError(f"{name}: {bad.size}/{got.size} elements differ, first at {bad[0]}")


def _load(path, seed=0, **over):
    pkg = _pkg()
    over.setdefault("temp", 0.0); over.setdefault("fine_temp", 0.0)
    return pkg.BarkContext.load_model(path, pkg.default_params(**over), seed=seed)


@pytest.fixture(scope="module")
def small_oracle(small_model):
    from oracle.pyoracle import Oracle
    o = Oracle(small_model, n_threads=16)
    yield o
    o.close()


@pytest.fixture(scope="module")
def ctxs(toy_model, small_model):
    made = {}

    def get(which):
        if which not in made:
            made[which] = _load(toy_model if which == "toy" else small_model)
        return made[which]
    yield get
    for c in made.values():
        c.free()


def _case(ctxs, toy_oracle, small_oracle, model, hist, mode, n_steps):
    pkg = _pkg()
    m = MODES[mode]
    base, orc = ctxs(model), (toy_oracle if model == "toy" else small_oracle)
    base.set_params(pkg.default_params(temp=m["temp"], fine_temp=m["fine_temp"], n_steps_text_encoder=n_steps))
    base.set_sampling_filter(m["top_k"], m["top_p"])
    v = _voice(hist)
    base.set_voice_prompt(v)
    return base, orc, v, m


# ---- stage calls and bark_generate_audio ---------------------------------------------------------------------------------------------------------
_REFS = {}


def _ref(orc, v, model, hist, mode, n_steps):
    """the reference loops' run of one case (one generator, seed 7, through the three stages), made once for the tests that compare against it"""
    key = (model, hist, mode, n_steps)
    if key not in _REFS:
        m = MODES[mode]
        _REFS[key] = R.generate(orc, TEXT, v, m["temp"], m["fine_temp"], n_steps=n_steps, seed=7, top_k=m["top_k"], top_p=m["top_p"])
    return _REFS[key]


def _n_steps(model):
    return 40 if model == "toy" else 24


@pytest.mark.boundary
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("hist", sorted(HISTORIES))
@pytest.mark.parametrize("model", ["toy", "small"])
def test_voiced_semantic_and_coarse_stage_calls(ctxs, toy_oracle, small_oracle, model, hist, mode):
    """bark_hip_tokenize (ids 256..511), bark_hip_semantic on that prompt, bark_hip_coarse with [history ; semantic] / [history ; generated]; called in
    order on a context seeded like the reference's generator"""
    base, orc, v, m = _case(ctxs, toy_oracle, small_oracle, model, hist, mode, _n_steps(model))
    want = _ref(orc, v, model, hist, mode, _n_steps(model))
    c = base.clone(seed=7)                                          # a clone copies parameters, filter and voice; its generator starts at the seed
    try:
        prompt = c.tokenize(TEXT)
        _exact("prompt", prompt, R.semantic_prompt(orc.tokenize(TEXT), v))
        assert not np.array_equal(prompt, orc.tokenize(TEXT))
        _exact("semantic", c.semantic(prompt), want["semantic"])
        assert len(want["semantic"]) >= 8
        _exact("coarse", c.coarse(want["semantic"]), want["coarse"])
        # the voice matters: the unvoiced stage gives other ids
        if mode == "greedy":
            assert not np.array_equal(want["coarse"], orc.coarse(want["semantic"], orc.params(temp=0.0, fine_temp=0.0)))
    finally:
        c.free()


@pytest.mark.boundary
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("hist", sorted(HISTORIES))
@pytest.mark.parametrize("model", ["toy", "small"])
def test_voiced_fine_stage_call(ctxs, toy_oracle, small_oracle, model, hist, mode):
    """bark_hip_fine: history rows in front, every window keeps its positions below rel = n_hist, the result is the new rows"""
    base, orc, v, m = _case(ctxs, toy_oracle, small_oracle, model, hist, mode, _n_steps(model))
    ref = _ref(orc, v, model, hist, mode, _n_steps(model))
    co = ref["coarse"]
    # greedy: the run's own fine stage; sampled: a generator of its own (the stage call starts from the context's seed)
    want = ref["fine"] if mode == "greedy" else R.fine(orc, co, v, m["fine_temp"], R.Sampler(6))
    c = base.clone(seed=6)
    try:
        got = c.fine(co)
        _exact("fine", got, want)
        assert np.array_equal(got[:, :2], co)
    finally:
        c.free()


@pytest.mark.boundary
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("hist", sorted(HISTORIES))
@pytest.mark.parametrize("model", ["toy", "small"])
def test_voiced_generate_audio(ctxs, toy_oracle, small_oracle, model, hist, mode):
    """bark_generate_audio end to end: ids of all stages and the PCM (the codec sees the new frames only)"""
    n_steps = _n_steps(model)
    base, orc, v, m = _case(ctxs, toy_oracle, small_oracle, model, hist, mode, n_steps)
    want = _ref(orc, v, model, hist, mode, n_steps)
    c = base.clone(seed=7)
    try:
        assert c.generate_audio(TEXT)
        _exact("semantic", c.semantic_tokens(), want["semantic"])
        _exact("coarse", c.coarse_tokens(), want["coarse"])
        _exact("fine", c.fine_tokens(), want["fine"])
        _exact("pcm", c.audio_data(), want["pcm"])
        assert len(c.audio_data()) == 320 * len(want["coarse"])
        # clearing the voice gives back the unvoiced generation
        if mode == "greedy" and model == "toy":
            c.set_voice_prompt(None)
            ref = orc.generate(TEXT, orc.params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=n_steps))
            assert c.generate_audio(TEXT)
            _exact("unvoiced fine", c.fine_tokens(), ref["fine"])
            _exact("unvoiced pcm", c.audio_data(), ref["pcm"])
    finally:
        c.free()


# ---- long inputs: rel = n_hist on the full windows, a larger value on the last one; the unvoiced route through the new kernels ------------------------
_LONG = {"tf700": ("full", 1100), "tf100": ("tf100", 1100), "unvoiced": (None, 1154)}

_GRAPH0_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from bark_amd_loader import load_package
from tests import test_gpu_voice_prompts as T
pkg = load_package()
c = pkg.BarkContext.load_model(%r, pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
out = {}
for key, (hist, n) in T._LONG.items():
    c.set_voice_prompt(None if hist is None else T._voice(hist))
    r0 = c.stats()["graph_replays"]
    out[key] = c.fine(T._long_coarse(n))
    assert c.stats()["graph_replays"] == r0, "BARK_HIP_GRAPH=0 must not replay graphs"
np.savez(%r, **out)
print("GRAPH0_OK")
"""


def _long_coarse(n):
    return np.random.default_rng(n).integers(0, 1024, (n, 2)).astype(np.int32)


@pytest.mark.boundary
def test_long_inputs_replay_the_fine_graphs_whatever_rel_holds(toy_model, toy_oracle, tmp_path):
    c = _load(toy_model)
    got = {}
    try:
        for key, (hist, n) in _LONG.items():
            v = None if hist is None else _voice(hist)
            c.set_voice_prompt(v)
            co = _long_coarse(n)
            wins, _ = R.fine_windows(0 if v is None else min(len(v.fine), 512), n)
            rels = [w[2] for w in wins]
            if v is None:
                assert rels[0] == 0 and rels[-1] > 0                       # the route that existed before: the last window of a long input
            else:
                # rel == n_hist on the full windows; with fewer than 512 history rows the short last window has a larger one, in the same run
                assert len(wins) >= 2 and rels[0] == min(len(v.fine), 512) and (rels[-1] > rels[0] if len(v.fine) < 512 else rels == [512] * 3)
            r0 = c.stats()["graph_replays"]
            got[key] = c.fine(co)
            # every window of every codebook was replayed from the captured graphs, none enqueued eagerly
            assert c.stats()["graph_replays"] - r0 == 6 * len(wins), (key, c.stats()["graph_replays"] - r0, len(wins))
            _exact(f"fine {key}", got[key], R.fine(toy_oracle, co, v))
        _exact("unvoiced == the oracle's own fine stage", got["unvoiced"], toy_oracle.fine(_long_coarse(1154), toy_oracle.params(temp=0.0, fine_temp=0.0)))
        # sampled, voiced, two windows: the uniforms are indexed as before
        c.free()
        c = _load(toy_model, seed=9, fine_temp=0.5)
        v = _voice("full")
        c.set_voice_prompt(v)
        co = _long_coarse(700)
        _exact("sampled fine", c.fine(co), R.fine(toy_oracle, co, v, 0.5, R.Sampler(9)))
    finally:
        c.free()
    out = str(tmp_path / "graph0.npz")
    r = subprocess.run([sys.executable, "-c", _GRAPH0_CHILD % (ROOT, toy_model, out)], env=dict(os.environ, BARK_HIP_GRAPH="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "GRAPH0_OK" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
    eager = np.load(out)
    for key in _LONG:
        _exact(f"graph replay vs BARK_HIP_GRAPH=0, {key}", got[key], eager[key])


_HOST_SAMPLING_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from bark_amd_loader import load_package
from tests import test_gpu_voice_prompts as T
pkg = load_package()
c = pkg.BarkContext.load_model(%r, pkg.default_params(temp=0.7, fine_temp=0.5, n_steps_text_encoder=30), seed=21)
c.set_sampling_filter(40, 0.9)
c.set_voice_prompt(T._voice("full"))
assert c.generate_audio(T.TEXT)
out = dict(semantic=c.semantic_tokens(), coarse=c.coarse_tokens(), fine=c.fine_tokens(), pcm=c.audio_data())
# the sequential fallback of a job: the context's voice for utterance 0, its own for utterance 1
res = c.generate_batch([T.TEXT, T.TEXT + " again"], params=[c.request_params(seed=31), c.request_params(seed=32)], voices=[None, T._voice("short")])
for i, r in enumerate(res):
    out["job%%d_fine" %% i] = r["fine"]; out["job%%d_pcm" %% i] = r["pcm"]
np.savez(%r, **out)
print("HOST_OK")
"""


@pytest.mark.boundary
@pytest.mark.job_order
def test_host_sampling_route_with_a_voice(toy_model, toy_oracle, tmp_path):
    """BARK_HIP_HOST_SAMPLING=1 (read at load: a child process): the host-side samplers of the three loops with a voice prompt, and the sequential
    fallback of a job with a voice per utterance"""
    from oracle import pyoracle
    out = str(tmp_path / "host.npz")
    r = subprocess.run([sys.executable, "-c", _HOST_SAMPLING_CHILD % (ROOT, toy_model, out)], env=dict(os.environ, BARK_HIP_HOST_SAMPLING="1"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "HOST_OK" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
    got = np.load(out)
    with pyoracle.job_order(False):
        want = R.generate(toy_oracle, TEXT, _voice("full"), 0.7, 0.5, n_steps=30, seed=21, top_k=40, top_p=0.9)
        for k in ("semantic", "coarse", "fine", "pcm"):
            _exact(f"host sampling {k}", got[k], want[k])
    with pyoracle.job_order(True):                                   # the fallback runs inside the job's scope: fine products in the jobs' order
        for i, (text, v, seed) in enumerate(((TEXT, _voice("full"), 31), (TEXT + " again", _voice("short"), 32))):
            want = R.generate(toy_oracle, text, v, 0.7, 0.5, n_steps=30, seed=seed, top_k=40, top_p=0.9)
            _exact(f"host sampling job {i} fine", got[f"job{i}_fine"], want["fine"])
            _exact(f"host sampling job {i} pcm", got[f"job{i}_pcm"], want["pcm"])


# ---- the pick kernels with a per-window rel against the two-step form (pick every row, keep positions >= rel) -------------------------------------
@pytest.mark.boundary
def test_pick_kernels_with_per_window_rel(toy_model):
    c = _load(toy_model)
    try:
        rng = np.random.default_rng(17)
        rel = np.array([0, 1, 511, 512, 1023, 300, 0], np.int32)
        Z, n = len(rel), 1024
        lg = (rng.standard_normal((Z * 1024, n)) * 3).astype(np.float32)
        # planted ties: exact duplicates of the maximum (the first index wins), maxima one ulp apart, and two rows of all-equal logits
        rows = rng.choice(Z * 1024, 400, replace=False)
        for k, r in enumerate(rows):
            i, j = sorted(rng.choice(n, 2, replace=False))
            top = np.float32(lg[r].max() + 1.0)
            lg[r, i] = top
            lg[r, j] = top if k % 2 == 0 else np.nextafter(top, np.float32(np.inf if k % 4 == 1 else -np.inf))
        lg[5] = 0.25; lg[1024 + 700] = -1.5
        plane = rng.integers(2000, 3000, Z * 1024).astype(np.int32)                     # ids no pick can produce
        keep = (np.arange(1024)[None, :] < rel[:, None]).reshape(-1)
        picks = R.greedy_rows(lg)
        got, ties = c.pick_rows(lg, rel, plane)
        _exact("greedy plane", got, np.where(keep, plane, picks))
        all_rows, ties0 = c.pick_rows(lg, np.zeros(Z, np.int32), plane)
        _exact("greedy, rel 0", all_rows, picks)
        assert ties == ties0 >= 200                                                       # near-tie accounting does not depend on rel
        # multinomial: uniforms indexed by row, some of them on a bin boundary (the exact path)
        u = rng.random(Z * 1024)
        temp = 0.5
        for r in rows[:60]:
            cp = nucleus_ref.bin_edges(lg[r], temp, 0, 1.0)
            u[r] = cp[int(rng.integers(0, 40))]
        want = np.array([nucleus_ref.multinomial(lg[r], temp, u[r], fast=True)[0] for r in range(Z * 1024)], np.int32)
        for r in np.flatnonzero([nucleus_ref.exact_path_forced(lg[r], temp, 0, 1.0, u[r], 2e-6) for r in range(Z * 1024)]):
            want[r] = nucleus_ref.multinomial(lg[r], temp, u[r])[0]
        got, ties = c.pick_rows(lg, rel, plane, temp=temp, u=u)
        _exact("multinomial plane", got, np.where(keep, plane, want))
        all_rows, ties0 = c.pick_rows(lg, np.zeros(Z, np.int32), plane, temp=temp, u=u)
        _exact("multinomial, rel 0", all_rows, want)
        assert ties == ties0 >= 60
    finally:
        c.free()


# ---- other weight formats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.boundary
@pytest.mark.parametrize("fmt", ["q4_0", "f32"])
def test_voiced_generation_on_other_weight_formats(fmt, toy_q4_model, toy_f32_model, toy_q4_oracle):
    from oracle.pyoracle import Oracle
    path = toy_q4_model if fmt == "q4_0" else toy_f32_model
    orc = toy_q4_oracle if fmt == "q4_0" else Oracle(path, n_threads=4)
    c = _load(path, n_steps_text_encoder=40)
    try:
        v = _voice("full")
        c.set_voice_prompt(v)
        want = R.generate(orc, TEXT, v, n_steps=40)
        assert c.generate_audio(TEXT)
        for k, got in (("semantic", c.semantic_tokens()), ("coarse", c.coarse_tokens()), ("fine", c.fine_tokens()), ("pcm", c.audio_data())):
            _exact(f"{fmt} {k}", got, want[k])
    finally:
        c.free()
        if fmt == "f32":
            orc.close()


# ---- lock-step jobs and the request collector -------------------------------------------------------------------------------------------------------
def _job_plan():
    """12 utterances for 8 slots: no voice, one shared voice, distinct voices; ragged step caps; one sampled utterance"""
    shared = _voice("full", seed=40)
    voices = [None, shared, _voice("short", 41), shared, None, _voice("tf100", 42), shared, _voice("full", 43), _voice("short", 44), None, shared, _voice("tf100", 45)]
    caps = [40, 24, 33, 16, 40, 28, 9, 36, 21, 12, 40, 30]
    texts = [f"{TEXT} number {i}" for i in range(12)]
    temps = [(0.0, 0.0)] * 12
    temps[5] = (0.7, 0.5)
    return texts, voices, caps, temps


def _job_refs(orc, texts, voices, caps, temps):
    return [R.generate(orc, t, v, tp[0], tp[1], n_steps=cap, seed=100 + i) for i, (t, v, cap, tp) in enumerate(zip(texts, voices, caps, temps))]


@pytest.mark.lock_step_job
def test_job_mixing_voices_equals_single_contexts_and_the_reference(toy_model, toy_oracle):
    pkg = _pkg()
    texts, voices, caps, temps = _job_plan()
    refs = _job_refs(toy_oracle, texts, voices, caps, temps)
    c = _load(toy_model)
    try:
        c.reserve_batch(8)
        params = [c.request_params(temp=tp[0], fine_temp=tp[1], n_steps_text_encoder=cap, seed=100 + i) for i, (cap, tp) in enumerate(zip(caps, temps))]
        pv = [None if v is None else pkg.VoicePrompt(v.semantic, v.coarse, v.fine) for v in voices]
        res = c.generate_batch(texts, params=params, voices=pv)
        for i, (r, ref) in enumerate(zip(res, refs)):
            assert r is not None, i
            for k in ("semantic", "coarse", "fine", "pcm"):
                _exact(f"utterance {i} {k} vs the reference loops", r[k], ref[k])
        # every utterance is what a fresh single context computes under an equal fine order
        for i in (1, 2, 5, 9):
            s = _load(toy_model, seed=100 + i, temp=temps[i][0], fine_temp=temps[i][1], n_steps_text_encoder=caps[i])
            try:
                s.set_fine_order(2)
                s.set_voice_prompt(voices[i])
                assert s.generate_audio(texts[i])
                _exact(f"utterance {i} fine vs a single context", res[i]["fine"], s.fine_tokens())
                _exact(f"utterance {i} pcm vs a single context", res[i]["pcm"], s.audio_data())
            finally:
                s.free()
        # the context's voice serves the utterances that carry none
        c.set_voice_prompt(voices[1])
        res2 = c.generate_batch(texts[:3], params=params[:3], voices=[None, None, pv[2]])
        want0 = R.generate(toy_oracle, texts[0], voices[1], n_steps=caps[0], seed=100)
        _exact("context voice, utterance 0", res2[0]["fine"], want0["fine"])
        _exact("context voice, utterance 1", res2[1]["pcm"], refs[1]["pcm"])
        _exact("own voice, utterance 2", res2[2]["pcm"], refs[2]["pcm"])
    finally:
        c.free()


@pytest.mark.lock_step_job
@pytest.mark.concurrency
def test_request_batcher_with_voices_and_two_job_streams(toy_model, toy_oracle):
    pkg = _pkg()
    texts, voices, caps, temps = _job_plan()
    refs = _job_refs(toy_oracle, texts, voices, caps, temps)
    c = _load(toy_model)
    try:
        with pkg.Batcher(c, max_batch=8, max_wait_ms=20, streams=2) as b:
            tickets = []
            for i, (t, v, cap, tp) in enumerate(zip(texts, voices, caps, temps)):
                rp = c.request_params(temp=tp[0], fine_temp=tp[1], n_steps_text_encoder=cap, seed=100 + i)
                tickets.append(b.submit(t, params=rp, voice=None if v is None else pkg.VoicePrompt(v.semantic, v.coarse, v.fine)))
            for i, tk in enumerate(tickets):
                _exact(f"request {i} pcm", b.wait(tk), refs[i]["pcm"])
            bad = R.synthetic_voice(1, 35, 41, 41)
            bad.coarse[3, 1] = 1024
            with pytest.raises(RuntimeError):
                b.submit("x", voice=bad)
    finally:
        c.free()


@pytest.mark.boundary
def test_from_generation_continues_an_utterance(toy_model, toy_oracle):
    pkg = _pkg()
    c = _load(toy_model, n_steps_text_encoder=60)
    try:
        assert c.generate_audio("the first sentence of a longer text .")
        a = pkg.voice.from_generation(c)
        ref_a = toy_oracle.generate("the first sentence of a longer text .", toy_oracle.params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=60))
        _exact("A semantic", a.semantic, ref_a["semantic"]); _exact("A coarse", a.coarse, ref_a["coarse"]); _exact("A fine", a.fine, ref_a["fine"])
        c.set_voice_prompt(a)
        assert c.generate_audio("and the second one , in the same voice .")
        want = R.generate(toy_oracle, "and the second one , in the same voice .", R.Voice(ref_a["semantic"], ref_a["coarse"], ref_a["fine"]), n_steps=60)
        _exact("B semantic", c.semantic_tokens(), want["semantic"])
        _exact("B coarse", c.coarse_tokens(), want["coarse"])
        _exact("B fine", c.fine_tokens(), want["fine"])
        _exact("B pcm", c.audio_data(), want["pcm"])
    finally:
        c.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.boundary
def test_refused_voice_prompts(toy_model, toy_oracle):
    pkg = _pkg()
    c = _load(toy_model, n_steps_text_encoder=20)
    try:
        good = _voice("full")
        c.set_voice_prompt(good)
        kept = c.tokenize("x")
        for field, idx, val in (("semantic", 3, 10000), ("semantic", 0, -1), ("coarse", (5, 1), 1024), ("fine", (2, 7), 1024), ("fine", (0, 0), -5)):
            bad = R.Voice(good.semantic.copy(), good.coarse.copy(), good.fine.copy())
            getattr(bad, field)[idx] = val
            with pytest.raises(ValueError):
                c.set_voice_prompt(bad)
        for n_sem, tc in ((1, 41), (35, 1), (3, 1), (0, 0)):                      # empty trimmed history
            with pytest.raises(ValueError):
                c.set_voice_prompt(R.synthetic_voice(3, n_sem, tc, 10))
        _exact("a refused voice leaves the context's voice alone", c.tokenize("x"), kept)
        # a history that cannot fit the coarse context with the context's window parameters: 257 + min(750, 626) + 160 - 1 > 1024
        c.set_voice_prompt(None)
        c.set_params(pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=20, max_coarse_history=750, sliding_window_size=160))
        assert c.hparams(1)["block_size"] == 1024
        with pytest.raises(ValueError):
            c.set_voice_prompt(good)
        c.set_voice_prompt(_voice("short"))                                       # 257 + 79 + 159 rows fit
        # ... and a job refuses a voice of its own the same way
        with pytest.raises(RuntimeError):
            c.generate_batch(["a", "b"], voices=[None, pkg.VoicePrompt(good.semantic, good.coarse, good.fine)])
    finally:
        c.free()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


@pytest.mark.concurrency
@pytest.mark.job_order
def test_native_batch_server_voices(toy_model, toy_oracle, tmp_path):
    pkg = _pkg()
    exe = os.path.join(ROOT, "bark.cpp_amd", "lib", "bark_batch_server")
    v = _voice("full")
    path = str(tmp_path / "alice.bvp")
    pkg.voice.save(pkg.VoicePrompt(v.semantic, v.coarse, v.fine), path)
    port = _free_port()
    srv = subprocess.Popen([exe, "-m", toy_model, "-p", str(port), "--temp", "0", "--fine-temp", "0", "--max-wait-ms", "10", "--voice", "alice=" + path],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        def post(body):
            req = urllib.request.Request(f"http://127.0.0.1:{port}/bark", data=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
            return urllib.request.urlopen(req, timeout=300).read()
        for _ in range(300):
            try:
                urllib.request.urlopen(f"http://127.0.0.1:{port}/", timeout=2).read(); break
            except Exception:
                assert srv.poll() is None, srv.stderr.read().decode()[-1500:]
                time.sleep(0.2)
        with pytest.raises(urllib.error.HTTPError) as e:
            post({"text": "hello", "voice": "bob"})
        assert e.value.code == 400
        with pytest.raises(urllib.error.HTTPError) as e:
            post({"text": "hello", "voice": 7})
        assert e.value.code == 400
        wav = post({"text": TEXT, "voice": "alice"})
        want = R.generate(toy_oracle, TEXT, v)                           # the server's defaults: 768 steps
        pcm = np.frombuffer(wav[44:], np.float32)
        _exact("voiced pcm from the server", pcm, want["pcm"])
        wav = post({"text": TEXT})
        ref = toy_oracle.generate(TEXT, toy_oracle.params(temp=0.0, fine_temp=0.0))
        _exact("a request without the field has no voice", np.frombuffer(wav[44:], np.float32), ref["pcm"])
    finally:
        srv.kill(); srv.wait()
    # a voice file the engine refuses stops the server at start
    bad = R.synthetic_voice(3, 1, 41, 10)
    pkg.voice.save(pkg.VoicePrompt(bad.semantic, bad.coarse, bad.fine), path)
    r = subprocess.run([exe, "-m", toy_model, "-p", str(_free_port()), "--voice", "alice=" + path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "refused" in r.stderr
