"""The decode loop's samplers (rule C8) row by row on the device, through the hook bark_hip_sample_rows_state: sample_greedy_kernel
against the restatement of gpt_argmax_sample and the semantic stop rule (tests/sampler_ref.py) on rows built to sit on the edges of its fast path -
pairs around kTieCut and kNearTie (A), tie groups (B), eos_p around min_eos_p (C), the coarse slice (D), the stage state (E), launches that mix greedy,
sampled and filtered slots (F), the single-slot launch form of bark_generate_audio (G), the multinomial sampler just outside its pick margin (H) and
everything again with BARK_HIP_EXACT_SAMPLING=1 (I).  Ids, stop decisions and states equal the restatement on every row; eos_p is the restatement's
to the bit wherever the exact path ran (StepState::near_tie says so) and within n 2^-23 of it elsewhere.  tests/test_emulated_decode_sampler.py runs
a selection of this file on the host-emulated engine."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nucleus_ref as R  # noqa: E402
import sampler_ref as S  # noqa: E402

I32MAX = S.INT32_MAX
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 10048, 12288]
N_PAST, CUR, STEP, EOS_STEP, NEAR, N_OUT, LAST_EOS, FAULT = range(8)          # struct StepState
F32 = np.float32
DELTAS = [0.0] + [s * d for d in (1e-7, 1e-5, 1e-4, 6e-4, 1e-3, 1.5e-3, 1.9e-3, 2.1e-3, 2.5e-3, 3e-3, 1e-2, 0.1) for s in (1, -1)]
DEV = {}                                                                       # n -> largest relative eos_p deviation seen on fast-path greedy rows


@pytest.fixture(scope="module")
def ctx(toy_model):
    from bark_amd_loader import load_package
    pkg = load_package()
    c = pkg.BarkContext.load_model(toy_model, pkg.default_params(temp=0.0), seed=0)
    yield c
    c.free()


def _report(what):
    print("eos_p, fast path, largest relative deviation from the restatement after %s: %s"
          % (what, ", ".join("n=%d: %.3g" % (n, DEV[n]) for n in sorted(DEV)) or "no fast-path row yet"))


def _state(nr, step=0, n_out=0, n_past=0, eos_step=I32MAX, near_tie=0, cur_token=-7, last_eos_p=0.5):
    st = np.zeros((nr, 8), np.int32)
    for col, v in ((N_PAST, n_past), (CUR, cur_token), (STEP, step), (EOS_STEP, eos_step), (NEAR, near_tie), (N_OUT, n_out)):
        st[:, col] = np.broadcast_to(np.asarray(v, np.int64), (nr,))
    st[:, LAST_EOS] = np.broadcast_to(np.asarray(last_eos_p, F32), (nr,)).copy().view(np.int32)
    return st


def _bits(x):
    return np.asarray(x, F32).reshape(-1).view(np.int32)


def _check(ctx, L, prescaled=1, temp=0.0, top_k=0, top_p=1.0, u=0.5, min_eos_p=2.0, state=None, path=None, forced=False, mode=0, eos_token=-1,
           token_base=0, n_past_add=1, per_row=False, what=""):
    """One call of the hook on rows L [R, n]; every row against its restatement (greedy rows: sampler_ref, sampled rows: nucleus_ref; numpy's exp
    first, the C library's on any disagreement).  path (greedy rows): 1 the exact path must have run, 0 the fast path, -1 either; None: by rule -
    more than one logit within kNearTie of the maximum, or eos_p within 1e-3 (relative) of min_eos_p: exact; neither, and eos_p further than 3e-3
    from it: fast.  forced: BARK_HIP_EXACT_SAMPLING=1 is set, every greedy row takes the exact path.  Returns (ids, eos_p, state after)."""
    L = np.ascontiguousarray(L, F32)
    nr, n = L.shape
    bc = lambda v, t: np.ascontiguousarray(np.broadcast_to(np.asarray(v, t), (nr,)))      # noqa: E731
    temp, top_k, top_p, u, me = bc(temp, F32), bc(top_k, np.int32), bc(top_p, F32), bc(u, np.float64), bc(min_eos_p, F32)
    st0 = _state(nr) if state is None else np.ascontiguousarray(state, np.int32)
    ids, eos, st = ctx.sample_rows_state(L, temp, top_k, top_p, u, me, st0, mode=mode, eos_token=eos_token, token_base=token_base, prescaled=prescaled,
                                         n_past_add=n_past_add, per_row=per_row)
    greedy = temp == 0.0
    gid = geos = close = None
    if greedy.any():
        gid, geos = S.greedy_rows(L[greedy], prescaled, fast=True)
        close = S.near_ties(L[greedy], prescaled)
    g_of = np.cumsum(greedy) - 1
    took = st[:, NEAR].astype(np.int64) - st0[:, NEAR]
    bad = []

    def row_ok(r, ri, re, exact_eos, want_path):
        step0 = int(st0[r, STEP])
        if mode == 0:
            want_id, stop = ri, S.stop(ri, re, eos_token, me[r])
            if exact_eos:
                ok = _bits(eos[r])[0] == _bits(re)[0]
            else:
                ok = abs(float(eos[r]) - float(re)) <= n * 2.0 ** -23 * float(re)
        else:
            want_id, stop = ri + token_base + 1024 * (step0 & 1), False
            ok = _bits(eos[r])[0] == 0
        ok = ok and int(ids[r]) == want_id and int(st[r, CUR]) == want_id
        ok = ok and st[r, N_PAST] == st0[r, N_PAST] + n_past_add and st[r, STEP] == step0 + 1 and st[r, N_OUT] == st0[r, N_OUT] + 1
        ok = ok and st[r, LAST_EOS] == _bits(eos[r])[0] and st[r, FAULT] == st0[r, FAULT]
        ok = ok and st[r, EOS_STEP] == (step0 if stop and st0[r, EOS_STEP] == I32MAX else st0[r, EOS_STEP])
        ok = ok and took[r] in (0, 1) and (want_path < 0 or took[r] == want_path)
        return bool(ok)

    for r in range(nr):
        l = L[r]
        if greedy[r]:
            g = int(g_of[r])
            ri, re = int(gid[g]), F32(geos[g])
            if forced:
                wp = 1
            elif path is not None:
                wp = int(np.broadcast_to(path, (nr,))[r])
            elif close[g] > 1:
                wp = 1
            elif mode != 0:
                wp = 0
            else:
                rel = abs(float(re) - float(me[r])) / abs(float(me[r]))
                wp = 1 if rel <= 1e-3 else 0 if rel >= 3e-3 else -1
            exact_eos = took[r] == 1
            if not row_ok(r, ri, re, exact_eos, wp):
                ri, re = S.greedy(l, prescaled)                       # the strict restatement decides
                re = F32(re)
                if not row_ok(r, ri, re, exact_eos, wp):
                    bad.append((what, "greedy", r, n, "ref", ri, float(re), "got", int(ids[r]), float(eos[r]), "path", int(took[r]), wp,
                                st0[r].tolist(), st[r].tolist(), float(me[r])))
                    continue
            if mode == 0 and took[r] == 0 and float(re) > 0.0:
                DEV[n] = max(DEV.get(n, 0.0), abs(float(eos[r]) - float(re)) / float(re))
        else:
            t, k, p, uu = float(temp[r]), int(top_k[r]), float(top_p[r]), float(u[r])
            ri, re = R.multinomial(l, t, uu, R.keep_mask_fast(l, k, p), fast=True)
            exact_eos = re == 0.0 or R.exact_path_forced(l, t, k, p, uu)
            if mode != 0:
                exact_eos = True
            if not row_ok(r, ri, F32(re), exact_eos, -1):
                ri, re = R.sample(l, t, k, p, uu)
                if not row_ok(r, ri, F32(re), exact_eos, -1):
                    bad.append((what, "sampled", r, n, t, k, p, uu, "ref", ri, float(re), "got", int(ids[r]), float(eos[r]), st0[r].tolist(), st[r].tolist()))
    assert not bad, (len(bad), bad[:4])
    return ids, eos, st


# ---- A: pairs around the two thresholds ------------------------------------------------------------------------------------------------

def _below(v, k):
    v = F32(v)
    for _ in range(k):
        v = np.nextafter(v, F32(-np.inf))
    return v


def _pairs():
    """(maximum M, second candidate M + d); d is exact in float for every pair"""
    cut, near = F32(-2.0 ** -25), F32(-4.0e-7)
    out = [(F32(0.0), F32(d)) for d in (F32(0.0), F32(-2.0 ** -26), cut, _below(cut, 1), F32(-1e-7), F32(-3.9e-7), near, _below(near, 1), F32(-5e-7),
                                        F32(-1e-6))]
    out += [(F32(1.0), _below(1.0, k)) for k in (0, 1, 2, 6, 7, 8, 16)]
    for M in (0.05, 37.5, -3.25):
        out += [(F32(M), _below(M, k)) for k in (0, 1, 2, 8)]
    return out


def _positions(n):
    """index pairs (i < j < n): the same thread (i, i + 1024 k), one wave, two waves, the ends of the row, neighbours"""
    if n >= 10048:
        cand = [(0, n - 1), (5, 700), (100, 100 + 1024 * 9)]
    else:
        cand = [(0, n - 1), (n - 2, n - 1), (0, 1), (3, 40), (5, 700), (7, 7 + 1024), (n // 2, n // 2 + 1)]
    out = []
    for i, j in cand:
        if 0 <= i < j < n and (i, j) not in out:
            out.append((i, j))
    return out


def _pair_rows(n, rng):
    """family A's rows of n logits in the scaled domain: every pair at every position in both index orders over a background at least 5 below"""
    return _pair_rows_d(n, rng)[0]


def _pair_rows_d(n, rng):
    """(rows, the d = second candidate - maximum each row was built with; -inf for the single-logit rows)"""
    if n == 1:
        return np.array([[0.0], [1.0], [37.5], [-3.25]], F32), np.full(4, -np.inf, F32)
    rows, ds = [], []
    for M, s in _pairs():
        for i, j in _positions(n):
            for a, b in ((M, s), (s, M)):
                l = (float(M) - rng.uniform(5.0, 9.0, n)).astype(F32)
                l[i], l[j] = a, b
                rows.append(l); ds.append(F32(s - M))
    return np.stack(rows), np.array(ds, F32)


def _raw(L):
    """the raw copy of rows built in the scaled domain: * 0.7 rounded to float (the sampler divides it by 0.7f again)"""
    return (np.asarray(L, F32) * F32(0.7)).astype(F32)


def _family_a(ctx, variant, forced=False, sizes=SIZES, per_row=False, take=None):
    rng = np.random.default_rng(101)
    n_exact = n_fast = 0
    out = []
    for n in sizes:
        L, d = _pair_rows_d(n, rng)
        if take:
            L, d = L[::max(1, len(L) // take)][:take], d[::max(1, len(d) // take)][:take]
        pre = 1 if variant == "scaled" else 0
        if not pre:
            L = _raw(L)
        else:                                                            # in the scaled domain d is exactly what the row says
            assert np.array_equal(S.near_ties(L, 1) > 1, d >= S.NEAR_TIE), n
        # min_eos_p = 2.0: the stop band cannot fire, the path is the near-tie rule's alone (d >= kNearTie: exact; below: fast)
        ids, eos, st = _check(ctx, L, pre, min_eos_p=2.0, state=_state(len(L), near_tie=np.arange(len(L)) % 2 * 5), forced=forced, per_row=per_row,
                              what="A %s n=%d" % (variant, n))
        close = S.near_ties(L, pre)
        n_exact += int(np.count_nonzero(close > 1)); n_fast += int(np.count_nonzero(close == 1))
        out.append((ids, eos, st))
    assert n_exact > 0 and n_fast > 0
    return out


@pytest.mark.parametrize("variant", ["scaled", "raw"])
def test_a_pairs_around_the_tie_cut_and_the_near_tie_margin(ctx, variant):
    _family_a(ctx, variant)
    _report("family A, " + variant)


# ---- B: tie groups ---------------------------------------------------------------------------------------------------------------------

def _tie_rows(n, rng):
    rows = []
    for dup in sorted({d for d in (2, 3, 64, 1025, n) if d <= n}):
        for tail in (False, True):
            l = (1.5 - rng.uniform(5.0, 9.0, n)).astype(F32)
            where = np.arange(n - dup, n) if tail else rng.choice(n, dup, replace=False)
            l[where] = 1.5
            rows.append(l)
    rows.append(rng.choice(np.array([-0.0, 0.0], F32), n))
    z = np.full(n, -0.0, F32); z[-1] = 0.0
    rows.append(z)
    rows.append(np.zeros(n, F32))
    for _ in range(3):
        rows.append((np.round(rng.standard_normal(n) * 2.0) / 2.0).astype(F32))          # wide tie groups
    return np.stack(rows)


def _family_b(ctx, forced=False, sizes=SIZES, per_row=False):
    rng = np.random.default_rng(102)
    out = []
    n_exact = 0
    for n in sizes:
        L = _tie_rows(n, rng)
        for pre in (1, 0):
            X = L if pre else _raw(L)
            out.append(_check(ctx, X, pre, min_eos_p=2.0, forced=forced, per_row=per_row, what="B pre=%d n=%d" % (pre, n)))
            n_exact += int(np.count_nonzero(S.near_ties(X, pre) > 1))
    assert n_exact >= 10 * sum(1 for n in sizes if n >= 2)                 # every row but the single-logit ones holds a tie
    return out


def test_b_tie_groups(ctx):
    _family_b(ctx)
    _report("family B")


# ---- C: the stop rule ------------------------------------------------------------------------------------------------------------------

def _stop_shapes(n, rng):
    """five rows with ONE logit at the maximum (nothing else within kNearTie of it) and the last logit 0.2 .. 1.5 below: flat, two levels, normal
    rows scaled by 0.01, 1 and 4"""
    j = n // 3
    rows = [np.full(n, -0.01), np.where(rng.random(n) < 0.5, -0.5, -3.0)] + [rng.standard_normal(n) * s for s in (0.01, 1.0, 4.0)]
    out = []
    for l in rows:
        l = l.astype(F32)
        l[-1] = -np.inf
        top = F32(max(float(l.max()) + 0.01, 0.0))
        l[j] = top
        l[-1] = top - F32(rng.uniform(0.2, 1.5))
        out.append(l)
    return np.stack(out), j


def _family_c(ctx, n, forced=False, per_row=False, take=None):
    rng = np.random.default_rng(103 + n)
    shapes, j = _stop_shapes(n, rng)
    out = []
    for pre in (1, 0):
        X = shapes if pre else _raw(shapes)
        assert (S.near_ties(X, pre) == 1).all()
        ref = [S.greedy(x, pre) for x in X]                               # the C library's exp: these thresholds are the test's point
        assert all(t == j for t, _ in ref)
        L, me, path, delta = [], [], [], []
        for x, (_, eos_ref) in zip(X, ref):
            for d in DELTAS:
                L.append(x); me.append(F32(eos_ref * (1.0 + d))); delta.append(d)
                path.append(1 if abs(d) <= 1e-3 else 0 if abs(d) >= 3e-3 else -1)
        nr = len(L)
        # a fifth of the rows have stopped before (eos_step stays what it was); the others start at steps 0 .. 3
        st0 = _state(nr, step=np.arange(nr) % 4, eos_step=np.where(np.arange(nr) % 5 == 4, 0, I32MAX), n_out=np.arange(nr) % 3)
        sel = slice(None) if not take else slice(0, nr, max(1, nr // take))
        ids, eos, st = _check(ctx, np.stack(L)[sel], pre, min_eos_p=np.array(me, F32)[sel], state=st0[sel], path=np.array(path)[sel], forced=forced,
                              per_row=per_row, what="C pre=%d n=%d" % (pre, n))
        out.append((ids, eos, st))
        if not forced and not take:
            # not blind: both decisions occur on both paths (the restatement's decision is what _check demanded of each row)
            stopped = (st[:, EOS_STEP] != st0[:, EOS_STEP])
            took = st[:, NEAR] - st0[:, NEAR]
            for p in (0, 1):
                assert stopped[took == p].any() and (~stopped[(took == p) & (st0[:, EOS_STEP] == I32MAX)]).any(), (n, pre, p)
        # the presets' thresholds, a pick of the eos token far below the threshold (stops) and the same pick without an eos token (does not)
        for m in (0.2, 0.05, 1.4e-4):
            out.append(_check(ctx, X, pre, min_eos_p=m, forced=forced, per_row=per_row, what="C preset %g n=%d" % (m, n)))
        a = _check(ctx, X, pre, min_eos_p=2.0, eos_token=j, state=_state(len(X), step=3), forced=forced, per_row=per_row, what="C eos token n=%d" % n)
        b = _check(ctx, X, pre, min_eos_p=2.0, eos_token=-1, state=_state(len(X), step=3), forced=forced, per_row=per_row, what="C no eos token n=%d" % n)
        assert (a[2][:, EOS_STEP] == 3).all() and (b[2][:, EOS_STEP] == I32MAX).all() and (a[1] < 0.9).all()
        out += [a, b]
    return out


@pytest.mark.parametrize("n", [1024, 10048, 12288], ids=["n1024", "n10048", "n12288"])
def test_c_stop_rule_around_min_eos_p(ctx, n):
    _family_c(ctx, n)
    _report("family C, n = %d" % n)


# ---- D: coarse mode --------------------------------------------------------------------------------------------------------------------

def _family_d(ctx, forced=False, per_row=False, take=None):
    rng = np.random.default_rng(104)
    L = _pair_rows(1024, rng)
    if take:
        L = L[::max(1, len(L) // take)][:take]
    out = []
    for pre in (1, 0):
        X = L if pre else _raw(L)
        for step in (0, 1, 2, 3):
            nr = len(X)
            st0 = _state(nr, step=step, eos_step=np.where(np.arange(nr) % 2 == 0, I32MAX, 1), n_out=step, n_past=700 + step)
            ids, eos, st = _check(ctx, X, pre, min_eos_p=np.where(np.arange(nr) % 3 == 0, 2.0, 0.0), state=st0, forced=forced, mode=1, token_base=10000,
                                  eos_token=-1, per_row=per_row, what="D pre=%d step=%d" % (pre, step))
            assert (ids >= 10000 + 1024 * (step & 1)).all() and (ids < 10000 + 1024 * (step & 1) + 1024).all()
            assert (eos == 0.0).all() and (st[:, LAST_EOS] == 0).all() and (st[:, EOS_STEP] == st0[:, EOS_STEP]).all()
            out.append((ids, eos, st))
    return out


def test_d_coarse_slice_and_no_stop_rule(ctx):
    _family_d(ctx)


# ---- E: the stage state ----------------------------------------------------------------------------------------------------------------

def test_e_state_after_the_launch(ctx):
    rng = np.random.default_rng(105)
    for n in (65, 1025):
        L = _pair_rows(n, rng)
        nr = len(L)
        for add in (0, 1):
            for mode in (0, 1):
                st0 = _state(nr, step=rng.integers(0, 8, nr), n_out=rng.integers(0, 8, nr), n_past=rng.choice([0, 5, 1023, 2 ** 30], nr),
                             near_tie=rng.choice([0, 5], nr), cur_token=rng.integers(-5, 20000, nr), eos_step=rng.choice([I32MAX, 0, 6], nr),
                             last_eos_p=rng.random(nr))
                st0[:, FAULT] = rng.choice([0, 1], nr)                   # not the sampler's to touch
                ids, eos, st = _check(ctx, L, 1, min_eos_p=rng.choice([2.0, 1e-6], nr), state=st0, mode=mode, token_base=10000, eos_token=n - 1,
                                      n_past_add=add, what="E n=%d add=%d mode=%d" % (n, add, mode))
                took = st[:, NEAR] - st0[:, NEAR]
                assert (took[st0[:, NEAR] == 5] == 1).any() and (took[st0[:, NEAR] == 5] == 0).any()      # incremented, not set


# ---- F: mixed launches -----------------------------------------------------------------------------------------------------------------

def _mixed_rows(rng, count, n):
    L, temp, top_k, top_p, u, me = [], [], [], [], [], []
    for r in range(count):
        kind, shape = r % 3, (r // 3) % 5
        if shape == 0:
            l = rng.standard_normal(n) * 4.0
        elif shape == 1:
            l = rng.standard_normal(n) * 0.01
        elif shape == 2:
            l = np.round(rng.standard_normal(n) * 2.0) / 2.0
        elif shape == 3:
            l = np.full(n, 0.25); l[rng.integers(0, n, 3)] = 1.0
        else:
            l = rng.standard_normal(n); l[rng.integers(0, n, n // 4)] *= -0.0
        l = l.astype(F32)
        t = 0.0 if kind == 0 else float(rng.choice([0.7, 1.0]))
        k, p = (50, float(F32(0.9))) if kind == 2 else (0, 1.0)
        uu = float(rng.random())
        if kind and r % 2:                                               # next to a bin edge of the row's own draw
            cp = R.bin_edges(l, t, k, p)
            nz = np.flatnonzero(np.diff(np.concatenate([[0.0], cp])) > 0)
            uu = float(np.clip(cp[int(rng.choice(nz))] + rng.choice([-1e-9, 0.0, 1e-9]), 0.0, np.nextafter(1.0, 0.0)))
        L.append(l); temp.append(t); top_k.append(k); top_p.append(p); u.append(uu)
        me.append(float(rng.choice([0.2, 0.05, 2.0])) if kind == 0 else 2.0)
    return np.stack(L), np.array(temp, F32), np.array(top_k, np.int32), np.array(top_p, F32), np.array(u), np.array(me, F32)


@pytest.mark.parametrize("n,count", [(1024, 240), (10048, 60)], ids=["n1024", "n10048"])
def test_f_mixed_launch_leaves_every_kind_to_its_own_kernel(ctx, n, count):
    rng = np.random.default_rng(106 + n)
    L, temp, top_k, top_p, u, me = _mixed_rows(rng, count, n)
    st0 = _state(count, step=np.arange(count) % 5, n_out=np.arange(count) % 7, n_past=np.arange(count))
    ids, eos, st = _check(ctx, L, 0, temp, top_k, top_p, u, me, st0, eos_token=n - 1, what="F mixed n=%d" % n)
    for kind in (0, 1, 2):                                               # the same rows in a launch of their own kind alone: bit for bit
        s = np.arange(count) % 3 == kind
        i1, e1, s1 = _check(ctx, L[s], 0, temp[s], top_k[s], top_p[s], u[s], me[s], st0[s], eos_token=n - 1, what="F kind %d n=%d" % (kind, n))
        assert np.array_equal(i1, ids[s]) and np.array_equal(_bits(e1), _bits(eos[s])) and np.array_equal(s1, st[s]), kind
    _report("family F, n = %d" % n)


# ---- G: the single-slot launch form ----------------------------------------------------------------------------------------------------

def _same(a, b):
    assert len(a) == len(b)
    for (i0, e0, s0), (i1, e1, s1) in zip(a, b):
        assert np.array_equal(i0, i1) and np.array_equal(_bits(e0), _bits(e1)) and np.array_equal(s0, s1)


def test_g_single_slot_launches_equal_the_per_slot_form(ctx):
    """about 200 rows of A to D, one launch per row with the scalars temp / min_eos_p (bark_generate_audio's form) against the lock step's"""
    n_rows = 0
    for fam in (lambda pr: _family_a(ctx, "scaled", sizes=[65, 1025, 10048], per_row=pr, take=16),
                lambda pr: _family_a(ctx, "raw", sizes=[2, 1024], per_row=pr, take=10),
                lambda pr: _family_b(ctx, sizes=[1, 1025], per_row=pr),
                lambda pr: _family_c(ctx, 1024, per_row=pr, take=25),
                lambda pr: _family_d(ctx, per_row=pr, take=5)):
        slots, single = fam(False), fam(True)
        _same(slots, single)
        n_rows += sum(len(i) for i, _, _ in single)
    assert 150 <= n_rows <= 400, n_rows
    # a sampled and a filtered row through the same form
    rng = np.random.default_rng(107)
    L, temp, top_k, top_p, u, me = _mixed_rows(rng, 30, 1024)
    _same([_check(ctx, L, 0, temp, top_k, top_p, u, me, eos_token=1023, what="G mixed, per slot")],
          [_check(ctx, L, 0, temp, top_k, top_p, u, me, eos_token=1023, per_row=True, what="G mixed, single slot")])


# ---- H: the multinomial fast path just outside its margin ------------------------------------------------------------------------------

def _edge_rows(rng, count, n_choices):
    """tie-group and flat rows whose u sits 1.1e-6, 2e-6 or 1e-5 from an end of the bin it picks, the bin at least twice as wide"""
    out = []
    r = 0
    while len(out) < count:
        r += 1
        assert r < 20 * count
        n = int(rng.choice(n_choices))
        if r % 3 == 0:
            l = np.round(rng.standard_normal(n) * 2.0) / 2.0
        elif r % 3 == 1:
            l = np.full(n, 0.25); l[rng.integers(0, n, 3)] = 1.0
        else:
            l = rng.standard_normal(n) * 0.01
        l = l.astype(F32)
        temp = float(rng.choice([0.7, 1.0]))
        cp = R.bin_edges(l, temp, 0, 1.0)
        cp[-1] = 1.0
        lo = np.concatenate([[0.0], cp[:-1]])
        off = float(rng.choice([1.1e-6, 2e-6, 1e-5]))
        wide = np.flatnonzero(cp - lo >= 2.0 * off)
        if wide.size == 0:
            continue
        j = int(rng.choice(wide))
        u = cp[j] - off if rng.random() < 0.5 else lo[j] + off         # inside bin j, `off` from one of its ends
        if not 0.0 <= u < 1.0:
            continue
        out.append((l, temp, float(u)))
    return out


def test_h_multinomial_pick_just_outside_its_margin(ctx):
    rng = np.random.default_rng(108)
    rows = _edge_rows(rng, 1200, [1024, 1000]) + _edge_rows(rng, 200, [10048])
    n_fast = 0
    for n in sorted({l.size for l, _, _ in rows}):
        sel = [x for x in rows if x[0].size == n]
        L, temp, u = np.stack([x[0] for x in sel]), np.array([x[1] for x in sel], F32), np.array([x[2] for x in sel])
        for l, t, uu in sel:
            assert not R.exact_path_forced(l, t, 0, 1.0, uu, margin=1e-6)
        ids, eos, st = _check(ctx, L, 0, temp, 0, 1.0, u, 2.0, what="H n=%d" % n)
        n_fast += int(np.count_nonzero(st[:, NEAR] == 0))
    print("family H: %d of %d rows settled by the multinomial fast path" % (n_fast, len(rows)))
    assert n_fast >= 0.9 * len(rows), (n_fast, len(rows))


# ---- I: the exact path alone -----------------------------------------------------------------------------------------------------------

def test_i_families_a_to_d_on_the_forced_exact_path(toy_model):
    """BARK_HIP_EXACT_SAMPLING is read once per process: a fresh child runs A to D; every row must report the exact path and the restatement's eos_p bits"""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from bark_amd_loader import load_package; pkg = load_package()\n"
        "import test_gpu_decode_sampler as T\n"
        "c = pkg.BarkContext.load_model(%r, pkg.default_params(temp=0.0), 0)\n"
        "n = 0\n"
        "for v in ('scaled', 'raw'): n += sum(len(i) for i, _, _ in T._family_a(c, v, forced=True))\n"
        "n += sum(len(i) for i, _, _ in T._family_b(c, forced=True))\n"
        "for k in (1024, 10048, 12288): n += sum(len(i) for i, _, _ in T._family_c(c, k, forced=True))\n"
        "n += sum(len(i) for i, _, _ in T._family_d(c, forced=True))\n"
        "assert not T.DEV, T.DEV\n"
        "c.free()\n"
        "print('FORCED_EXACT_ROWS', n)\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), toy_model)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BARK_HIP_EXACT_SAMPLING="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split("FORCED_EXACT_ROWS ")[1].split()[0]) > 8000, r.stdout[-2000:]


# ---- the hook's own checks -------------------------------------------------------------------------------------------------------------

def test_hook_refuses_bad_arguments(ctx):
    ok = np.zeros((2, 16), F32)
    ctx.sample_rows_state(ok, 0.0, 0, 1.0, 0.5, 2.0, _state(2))
    for kw in (dict(mode=2), dict(mode=-1), dict(prescaled=2), dict(n_past_add=-1), dict(token_base=-1)):
        with pytest.raises(RuntimeError):
            ctx.sample_rows_state(ok, 0.0, 0, 1.0, 0.5, 2.0, _state(2), **kw)
    for st in (_state(2, step=8), _state(2, step=-1), _state(2, n_out=8), _state(2, n_out=-1), _state(2, n_past=-1)):
        with pytest.raises(RuntimeError):
            ctx.sample_rows_state(ok, 0.0, 0, 1.0, 0.5, 2.0, st)
    for temp, k, p, m in ((-0.5, 0, 1.0, 2.0), (float("nan"), 0, 1.0, 2.0), (0.7, -1, 1.0, 2.0), (0.7, 0, 0.0, 2.0), (0.7, 0, 1.5, 2.0), (0.0, 0, 1.0, float("nan"))):
        with pytest.raises(RuntimeError):
            ctx.sample_rows_state(ok, temp, k, p, 0.5, m, _state(2))
    with pytest.raises(RuntimeError):
        ctx.sample_rows_state(np.zeros((1, 12289), F32), 0.0, 0, 1.0, 0.5, 2.0, _state(1))
    ctx.sample_rows_state(np.zeros((1, 12288), F32), 0.0, 0, 1.0, 0.5, 2.0, _state(1))
    with pytest.raises(RuntimeError):
        ctx.sample_rows_state(np.zeros((257, 4), F32), 0.0, 0, 1.0, 0.5, 2.0, _state(257), per_row=True)
    ctx.sample_rows_state(np.zeros((256, 4), F32), 0.0, 0, 1.0, 0.5, 2.0, _state(256), per_row=True)
