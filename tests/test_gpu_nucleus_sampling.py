"""Top-k / nucleus sampling (rule C8n) on the device: the filter kernel against the Python restatement (tests/nucleus_ref.py),
the semantic stage against the oracle's logits + the restatement, the coarse stage and whole generations against the host sampling path, lock-step
jobs, the request collector and the HTTP server against single contexts.  The tests of the C-ABI
extension - all single-context tests here - are marked `boundary` (they run after row-level parity), the job / collector / server tests
`lock_step_job` / `concurrency`."""
import json
import os
import socket
import subprocess
import sys
import tempfile
import threading
import time
import urllib.error
import urllib.request

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nucleus_ref as R  # noqa: E402
from test_nucleus_sampling_host import _rows  # noqa: E402

TEXT = "the quick brown fox jumps over the lazy dog"
PAIRS = [(0, 0.9), (50, 1.0), (5, 0.5), (1, 1.0), (200, 0.99)]


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _ctx(path, seed=0, **over):
    pkg = _pkg()
    return pkg.BarkContext.load_model(path, pkg.default_params(**over), seed=seed)


def _check_rows(ctx, rows):
    """ids bit-equal to the restatement.  eos_p: exactly 0 where the last id went, bit-equal where u lies next to an end of its bin (the sampler's
    exact path), else within n 2^-23 (C8's fast-path tree sum, as unfiltered).  Returns (mismatches, rows whose eos_p was held to the bit)."""
    bad = []
    n_bits = 0
    for n in sorted({r[0].size for r in rows}):
        sel = [r for r in rows if r[0].size == n]
        ids, eos = ctx.sample_rows_filtered(np.stack([r[0] for r in sel]), [r[1] for r in sel], [r[2] for r in sel], [r[3] for r in sel], [r[4] for r in sel])
        for (l, temp, k, p, u), i, e in zip(sel, ids, eos):
            forced = R.exact_path_forced(l, temp, k, p, u)

            def ok(ri, re):
                return i == ri and (e == re if (re == 0.0 or forced) else abs(e - re) <= n * 2.0 ** -23 * re)
            fast = R.multinomial(l, temp, u, R.keep_mask_fast(l, k, p), fast=True)
            n_bits += forced and fast[1] != 0.0
            if ok(*fast):
                continue
            ri, re = R.sample(l, temp, k, p, u)                       # the strict restatement decides (numpy's exp is not the C library's)
            if not ok(ri, re):
                bad.append((n, temp, k, p, u, ri, re, int(i), float(e)))
    return bad, n_bits


@pytest.mark.boundary
@pytest.mark.parametrize("exact", ["0", "1"])
def test_filter_kernel_matches_the_restatement_on_many_rows(toy_model, exact):
    """10^5 rows (n = 1024, 10 048 and odd sizes; peaked, flat, tied, saturated, signed zeros; a third with u within 1e-9 of a bin edge), in a
    fresh process (BARK_HIP_EXACT_SAMPLING is read once per process)"""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from bark_amd_loader import load_package; pkg = load_package()\n"
        "import test_gpu_nucleus_sampling as T, test_nucleus_sampling_host as H\n"
        "c = pkg.BarkContext.load_model(%r, pkg.default_params(temp=0.7), 0)\n"
        "rng = np.random.default_rng(7 + %s)\n"
        "bad = []; n_bits = 0\n"
        "for part in range(25):\n"
        "    rows = H._rows(rng, 3800, [1024, 1024, 2048, 1000]) + H._rows(rng, 200, [10048, 12288])\n"
        "    b, nb = T._check_rows(c, rows); bad += b; n_bits += nb\n"
        "print('BAD', len(bad), bad[:3])\n"
        "print('EOS_BITS', n_bits)\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), toy_model, exact)
    env = dict(os.environ, BARK_HIP_EXACT_SAMPLING=exact)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "BAD 0 []" in r.stdout, r.stdout[-2000:]
    assert int(r.stdout.split("EOS_BITS ")[1].split()[0]) >= 1000, r.stdout[-2000:]      # draws next to a bin edge with eos_p > 0: held to the bit


def _semantic_reference(orc, prompt, seed, temp, top_k, top_p, n_steps, min_eos_p, eos_token):
    """bark_eval_text_encoder's loop with C8n: the oracle's logits (prompt, then one row per step), the restatement, std::mt19937(seed) draws"""
    g = R.MT19937(seed)
    logits, n_past = orc.gpt_eval(0, prompt, 0, True)
    out = []
    for i in range(n_steps):
        if i > 0:
            logits, n_past = orc.gpt_eval(0, [out[-1]], n_past, False)
        nxt, eos_p = R.sample(logits, temp, top_k, top_p, g.canonical())
        if nxt == eos_token or eos_p >= min_eos_p:
            break
        out.append(nxt)
    return np.array(out, np.int32)


@pytest.mark.boundary
@pytest.mark.parametrize("which", ["toy", "mini"])
def test_semantic_stage_with_filter_matches_the_oracle_logits(which, request):
    model = request.getfixturevalue(which + "_model")
    orc = request.getfixturevalue(which + "_oracle")
    n_steps = 48
    base = _ctx(model, temp=0.7, n_steps_text_encoder=n_steps)
    p = base._params
    prompt = base.tokenize(TEXT)
    n_steps = min(n_steps, base.hparams(0)["block_size"] - 257 + 1)
    for seed in (3, 11):
        for k, tp in PAIRS:
            c = base.clone(seed)
            c.set_sampling_filter(k, tp)
            got = c.semantic(prompt)
            c.free()
            ref = _semantic_reference(orc, prompt, seed, 0.7, k, tp, n_steps, p.min_eos_p, p.semantic_vocab_size)
            assert np.array_equal(got, ref), (which, seed, k, tp, got[:20], ref[:20])
    base.free()


def _generate(model, seed, top_k, top_p, env=None, fine_order=None, filt=True):
    """ids and PCM of one bark_generate_audio in a fresh process (env: BARK_HIP_HOST_SAMPLING / BARK_HIP_GRAPH)"""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "from bark_amd_loader import load_package; pkg = load_package()\n"
        "c = pkg.BarkContext.load_model(%r, pkg.default_params(n_steps_text_encoder=40), %d)\n"
        "if %r: c.set_sampling_filter(%d, %r)\n"
        "if %r is not None: c.set_fine_order(%r)\n"
        "assert c.generate_audio(%r)\n"
        "np.savez(sys.argv[1], s=c.semantic_tokens(), c=c.coarse_tokens(), f=c.fine_tokens(), a=c.audio_data())\n"
    ) % (ROOT, model, seed, filt, top_k, top_p, fine_order, fine_order, TEXT)
    fd, out = tempfile.mkstemp(suffix=".npz")
    os.close(fd)
    r = subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = dict(np.load(out))
    os.remove(out)
    return d


def _same(a, b, keys="scfa"):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.mark.boundary
@pytest.mark.parametrize("top_k,top_p", [(0, 0.8), (20, 1.0), (8, 0.95)])
def test_filtered_generation_matches_host_sampling(toy_model, top_k, top_p):
    """default temperatures (0.7 / 0.5): device filter + sampler == filter_host + std::discrete_distribution on fetched logits, ids and PCM"""
    dev = _generate(toy_model, 5, top_k, top_p)
    host = _generate(toy_model, 5, top_k, top_p, env={"BARK_HIP_HOST_SAMPLING": "1"})
    _same(dev, host)
    plain = _generate(toy_model, 5, 0, 1.0, filt=False)
    assert not all(np.array_equal(dev[k], plain[k]) for k in "sc"), "the filter changed nothing"


@pytest.mark.boundary
def test_filtered_steps_agree_between_graph_replay_and_eager_launches(toy_model):
    _same(_generate(toy_model, 9, 10, 0.9), _generate(toy_model, 9, 10, 0.9, env={"BARK_HIP_GRAPH": "0"}))


@pytest.mark.boundary
def test_filter_off_is_bit_equal_to_a_context_that_never_set_one(toy_model):
    a = _generate(toy_model, 4, 0, 1.0, filt=True)
    b = _generate(toy_model, 4, 0, 1.0, filt=False)
    _same(a, b)
    # and switching it on and off again on one context returns to the unfiltered stream
    c = _ctx(toy_model, seed=4, n_steps_text_encoder=40)
    c.set_sampling_filter(3, 0.5)
    c.set_sampling_filter(0, 1.0)
    assert c.generate_audio(TEXT)
    assert np.array_equal(c.semantic_tokens(), b["s"]) and np.array_equal(c.audio_data(), b["a"])
    c.free()


@pytest.mark.boundary
def test_coarse_top_k_1_at_temp_07_equals_greedy(toy_model):
    greedy = _ctx(toy_model, temp=0.0, fine_temp=0.0, n_steps_text_encoder=40)
    sem = greedy.semantic(greedy.tokenize(TEXT))
    assert len(sem) > 4
    ref = greedy.coarse(sem)
    c = _ctx(toy_model, seed=2, temp=0.7, n_steps_text_encoder=40)
    c.set_sampling_filter(1, 1.0)
    got = c.coarse(sem)
    assert np.array_equal(got, ref)
    c.set_sampling_filter(0, 1.0)
    assert not np.array_equal(c.coarse(sem), ref)                     # unfiltered at 0.7 it samples
    greedy.free(); c.free()


@pytest.mark.lock_step_job
def test_lock_step_job_mixing_greedy_plain_and_filtered_slots(toy_model):
    """one job: greedy, temp-only, top-k, top-p and both; every utterance's semantic and coarse ids equal a fresh single context's"""
    pkg = _pkg()
    job = _ctx(toy_model, n_steps_text_encoder=40)
    texts = ["utterance %d of a mixed job about rivers" % i for i in range(7)]
    temps = [0.0, 0.7, 0.7, 0.7, 0.7, 0.0, 0.9]
    flts = [(0, 1.0), (0, 1.0), (30, 1.0), (0, 0.8), (12, 0.9), (5, 0.5), (1, 1.0)]
    params = [job.request_params(temp=temps[i], seed=100 + i) for i in range(len(texts))]
    res = job.generate_batch(texts, params=params, filters=flts)
    for i, t in enumerate(texts):
        c = _ctx(toy_model, seed=100 + i, temp=temps[i], n_steps_text_encoder=40)
        c.set_sampling_filter(*flts[i])
        assert c.generate_audio(t)
        assert res[i] is not None
        assert np.array_equal(res[i]["semantic"], c.semantic_tokens()), i
        assert np.array_equal(res[i]["coarse"], c.coarse_tokens()), i
        c.free()
    # the context's filter serves a job without filters of its own
    job.set_sampling_filter(12, 0.9)
    res2 = job.generate_batch(texts[4:5], params=params[4:5])
    assert np.array_equal(res2[0]["semantic"], res[4]["semantic"]) and np.array_equal(res2[0]["coarse"], res[4]["coarse"])
    job.free()


def _single_pcm(model, text, seed, top_k, top_p, **params):
    c = _ctx(model, seed=seed, **(params or {"n_steps_text_encoder": 40}))
    c.set_fine_order(2)                       # the collector's jobs run the fine products in C1m
    c.set_sampling_filter(top_k, top_p)
    assert c.generate_audio(text)
    a = c.audio_data().copy()
    c.free()
    return a


@pytest.mark.concurrency
def test_request_batcher_submit_filtered_matches_single_contexts(toy_model):
    pkg = _pkg()
    c = _ctx(toy_model, n_steps_text_encoder=40)
    c.set_sampling_filter(7, 0.95)                                   # the context's filter: what a request without one gets
    texts = ["collector request %d" % i for i in range(7)]
    flts = [(0, 0.8), (25, 1.0), None, (3, 0.6), (0, 1.0), (9, 0.7), (0, 0.85)]
    out = [None] * len(texts)
    with pkg.Batcher(c, max_batch=8, max_wait_ms=300) as b:
        def go(i):
            f = flts[i]
            if i >= 5:                                                 # no params: the context's parameters with the request's seed
                t = b.submit(texts[i], seed=60 + i, top_k=f[0], top_p=f[1])
            else:
                params = c.request_params(seed=60 + i)
                t = b.submit(texts[i], params=params) if f is None else b.submit(texts[i], params=params, top_k=f[0], top_p=f[1])
            out[i] = b.wait(t)
        th = [threading.Thread(target=go, args=(i,)) for i in range(len(texts))]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=600)
    for i, t in enumerate(texts):
        f = flts[i] or (7, 0.95)
        assert out[i] is not None and np.array_equal(out[i], _single_pcm(toy_model, t, 60 + i, *f)), i
    c.free()


def _read_float_wav(buf):
    pos = 12
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], int.from_bytes(buf[pos + 4:pos + 8], "little")
        if cid == b"data":
            return np.frombuffer(buf[pos + 8:pos + 8 + size], np.float32)
        pos += 8 + size
    raise AssertionError("no data chunk")


@pytest.mark.concurrency
def test_native_batch_server_top_k_top_p_fields(toy_model):
    exe = os.path.join(ROOT, "bark.cpp_amd", "lib", "bark_batch_server")
    assert os.path.exists(exe), "bark.cpp_amd/build.sh builds it"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    proc = subprocess.Popen([exe, "-m", toy_model, "-a", "127.0.0.1", "-p", str(port), "-s", "90", "--max-batch", "8", "--max-wait-ms", "300", "--top-p", "0.9"],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    bodies = [{"text": "server request zero", "seed": 70, "top_k": 20},
              {"text": "server request one", "seed": 71, "top_k": 4, "top_p": 0.7},
              {"text": "server request two", "seed": 72}]
    expect = [(20, 0.9), (4, 0.7), (0, 0.9)]                          # a field left out takes the server's --top-k / --top-p
    got = [None] * len(bodies)

    def post(i):
        req = urllib.request.Request(f"http://127.0.0.1:{port}/bark", data=json.dumps(bodies[i]).encode(), headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=600) as resp:
            got[i] = _read_float_wav(resp.read())

    try:
        for _ in range(600):
            try:
                socket.create_connection(("127.0.0.1", port), timeout=0.2).close(); break
            except OSError:
                assert proc.poll() is None, proc.stdout.read().decode()[-2000:]
                time.sleep(0.2)
        th = [threading.Thread(target=post, args=(i,)) for i in range(len(bodies))]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=600)
        for bad in ({"text": "x", "top_k": -1}, {"text": "x", "top_p": 0}, {"text": "x", "top_p": 1.5}, {"text": "x", "top_k": "3"}, {"text": "x", "top_p": 0.5, "top_k": 2.5}):
            req = urllib.request.Request(f"http://127.0.0.1:{port}/bark", data=json.dumps(bad).encode(), headers={"Content-Type": "application/json"})
            with pytest.raises(urllib.error.HTTPError) as e:
                urllib.request.urlopen(req, timeout=60)
            assert e.value.code == 400, bad
        # the refused requests carried no seed and drew none: the first request without a seed gets the server's --seed
        req = urllib.request.Request(f"http://127.0.0.1:{port}/bark", data=json.dumps({"text": "server request three", "top_k": 3}).encode(),
                                     headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=600) as resp:
            unseeded = _read_float_wav(resp.read())
    finally:
        proc.terminate()
        proc.wait(timeout=60)
    assert np.array_equal(unseeded, _single_pcm(toy_model, "server request three", 90, 3, 0.9, temp=0.7))
    for i, b in enumerate(bodies):
        assert got[i] is not None and np.array_equal(got[i], _single_pcm(toy_model, b["text"], b["seed"], *expect[i], temp=0.7)), i     # the server's default parameters
