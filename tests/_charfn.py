"""What the characteristic-function tests share (test_charfn_host.py, test_gpu_charfn.py, test_cli_countdist_gpu.py): the
complex weight tables of a batch, the host-compiled kernel, the reference and the comparison.

Reference: up to ten members the 3^N enumeration of test_map_host.brute_weights, each configuration's weight times
prod_p w[p][g_p] in complex128; beyond ten (and under site priors) the project's own numpy elimination (_maxproduct /
_prior_joint factors) on the complex rows lk * w, which reference() checks against the enumeration wherever it has both.
Status comes from the real rows.

Bar (include/famseq_hip.h): |cf - reference| <= 1e-12 * A, ABSOLUTE, A = Z(lk * |w|) / Z(lk) — 1 for weights of unit modulus.
Every configuration's term is a product of at most about 6 N rounded factors, the terms' moduli add up to A Z: 6 * 48 * 1.1e-16
is 3e-14 at 48 members, and the bar leaves a factor of 30 over that.  No site is left out: clear() asserts on the reference alone
that status is 0 except at planted failures and that Z >= 1e-200.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np

import _maxproduct as mp
import _prior_joint as J
import famseq_amd as fs
from test_generated_host import factor_tables, host_source
from test_map_host import brute_weights
from test_pattern_host import allowed

CF_ATOL = 1e-12     # times A
DIST_ATOL = 1e-12   # a probability of the count distribution
FLOOR = 1e-200
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4      # kCharfnVariants
LEAN_FROM = 25      # kCharfnLeanFrom (csrc/elim_codegen.cpp): this kernel's own lean threshold; begin_side()'s is forty
SELF_ATOL = 1e-13   # the elimination against the enumeration, times A: both are references


def batch_tables(ped, masks):
    """The tables of a batch, from RandomState(700 + N) -> (tables [M, N, 3] complex128, {name: slice or index}): the
    count_tables of carriers over all members; of alleles over a random 40 % of the members; two of random unit-modulus
    entries; one with moduli in (0, 1); one with a (2, 0.5i, -1) row; one real 0/1 table from the batch's masks (its dominant
    row); one of (1, 0) entries."""
    n = ped.n
    rng = np.random.RandomState(700 + n)
    parts, at, m = [], {}, 0

    def add(name, t):
        nonlocal m
        t = np.asarray(t, np.complex128).reshape(-1, n, 3)
        at[name] = slice(m, m + len(t))
        parts.append(t)
        m += len(t)

    add("carriers", fs.count_tables(fs.count_scores(n))[0])
    some = np.sort(rng.permutation(n)[:max(1, int(round(0.4 * n)))])
    at["allele_members"] = some
    add("alleles", fs.count_tables(fs.count_scores(n, some, "alleles"))[0])
    add("unit", np.exp(2j * np.pi * rng.uniform(0, 1, (2, n, 3))))
    add("inside", rng.uniform(0.05, 0.95, (n, 3)) * np.exp(2j * np.pi * rng.uniform(0, 1, (n, 3))))
    row = np.ones((n, 3), np.complex128)
    row[rng.randint(n)] = (2.0, 0.5j, -1.0)
    add("row", row)
    add("mask", allowed(masks[2:3])[0])
    add("ones", np.ones((n, 3)))
    return np.concatenate(parts), at


def as_pairs(tables):
    """complex [M, N, 3] -> float64 [M, N, 3, 2], the layout the kernel reads."""
    t = np.ascontiguousarray(tables, np.complex128)
    return t.view(np.float64).reshape(t.shape + (2,))


def _factors(ped, mrate, lk, flags, prior):
    return mp.site_factors(ped, mrate, lk, flags) if prior is None else J.site_factors(ped, mrate, lk, flags, prior)


def _eliminated(ped, mrate, rows, flags, prior):
    """The total weight (with the reference's 1e7) of the rows, real or complex, by the numpy elimination."""
    with np.errstate(invalid="ignore"):
        factors = _factors(ped, mrate, rows, flags, prior)[0]
    rest = mp.eliminate(factors, mp.elimination_order(factors, ped.n), False)[0]
    out = np.full(rows.shape[0], 1e7, rows.dtype)
    for vs, a in rest:
        assert vs == ()
        out = out * a
    return out


def reference(ped, mrate, lk, flags, tables, prior=None, brute=True):
    """-> (z[S], zm[S, M] complex, a[S, M], status[S]): the total weight of the rows as they are, of the rows times every table
    (both with the reference's 1e7), A = Z(lk |w|) / Z (1.0 where every modulus of the table is 1 to 1e-12) and the status of
    the real rows.  Up to ten members (brute, no site prior) zm is the 3^N enumeration's, and the elimination is checked
    against it here."""
    z = _eliminated(ped, mrate, lk, flags, prior)
    fail = _factors(ped, mrate, lk, flags, prior)[1]
    st = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    good = st == 0
    zm = np.stack([_eliminated(ped, mrate, lk * w, flags, prior) for w in tables], axis=1)
    a = np.ones(zm.shape)
    for j, w in enumerate(tables):
        if np.max(np.abs(np.abs(w) - 1.0)) > 1e-12:
            with np.errstate(invalid="ignore", divide="ignore"):
                a[:, j] = _eliminated(ped, mrate, lk * np.abs(w), flags, prior) / z
    if brute and ped.n <= 10 and prior is None:
        G, W, bst = brute_weights(ped, mrate, lk, flags)
        assert np.array_equal(bst != 0, ~good)
        W = np.where((bst != 0)[:, None], 0.0, np.nan_to_num(W))
        np.testing.assert_allclose(W.sum(axis=1)[good], z[good], rtol=1e-11, atol=0)
        for j, w in enumerate(tables):
            wm = W @ np.prod(w[np.arange(ped.n)[:, None], G], axis=0)
            assert np.all(np.abs(zm[good, j] - wm[good]) <= SELF_ATOL * a[good, j] * z[good])
            zm[good, j] = wm[good]
    return z, zm, a, st


def clear(ref, what="", planted=()):
    """On the reference alone: nothing is left out of a comparison."""
    z, _, a, st = ref
    ok = np.ones(len(z), bool)
    ok[list(planted)] = False
    assert np.all(st[ok] == 0) and np.all(st[~ok] != 0), what
    assert np.all(z[ok] >= FLOOR) and np.all(np.isfinite(a[ok])), what


def check(out, ref, what=""):
    """The module docstring's rules; every site and table compared.  Prints the worst error before it asserts."""
    cf, ll, st = out
    z, zm, a, ref_st = ref
    assert np.array_equal(st, ref_st), what
    ok = ref_st == 0
    assert np.all(np.isnan(ll[~ok])) and np.all(np.isnan(cf[~ok].real)) and np.all(np.isnan(cf[~ok].imag)), what
    want = zm[ok] / z[ok][:, None]
    with np.errstate(invalid="ignore", divide="ignore"):  # (A = 0: every term is exactly 0, and so must the result be)
        err = np.where(a[ok] > 0, np.abs(cf[ok] - want) / a[ok], np.where(cf[ok] == 0, 0.0, np.inf))
    ll_err = np.abs(ll[ok] - (np.log10(z[ok]) - 7.0))
    print("%s: %d sites x %d tables, worst |cf error| / A %.3g (bar %g), largest A %.3g, worst |loglik error| %.3g, smallest Z %.3g"
          % (what, ok.sum(), zm.shape[1], err.max(initial=0), CF_ATOL, a[ok].max(initial=1), ll_err.max(initial=0), z[ok].min(initial=1)))
    assert not np.any(np.isnan(err)) and np.all(err <= CF_ATOL), what
    np.testing.assert_allclose(ll[ok], np.log10(z[ok]) - 7.0, rtol=0, atol=1e-9, err_msg=what)


def brute_distribution(ped, mrate, lk, flags, scores):
    """The count's distribution [S, D + 1] binned directly from the 3^N enumeration (status-0 sites; NaN elsewhere), and D."""
    G, W, st = brute_weights(ped, mrate, lk, flags)
    sc = np.asarray(scores)
    D = int(sc.max(axis=1).sum())
    count = sc[np.arange(ped.n)[:, None], G].sum(axis=0)
    with np.errstate(invalid="ignore"):
        dist = np.stack([W[:, count == k].sum(axis=1) for k in range(D + 1)], axis=1) / W.sum(axis=1)[:, None]
    dist[st != 0] = np.nan
    return dist, D


_BUILT = {}


def build_charfn_host(model, where, variant=None, prior=False):
    """Generate famseq_charfn (prior: famseq_charfn_prior) for a one-lane workgroup on a plan-only context, compile it for the
    host (g++ -ffp-contract=off).  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("charfn_prior", "famseq_charfn_prior") if prior else ("charfn", "famseq_charfn")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option(key + "_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    src = open(plan[key + "_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and (entry + "(") in src
    assert ("founder priors per site" in src.splitlines()[0]) == prior
    assert variant is None or plan[key + "_variant"] == variant
    if src not in _BUILT:  # (the text holds no rate: one shared object per text and session)
        tag = key + ("" if variant is None else "_%d" % variant)
        cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
        open(cpp, "w").write(host_source(src))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
        fn = getattr(C.CDLL(so), entry)
        fn.restype = None
        fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_void_p, C.c_int] + ([C.c_void_p] if prior else [])
        _BUILT[src] = fn
    return _BUILT[src], plan, src


def run_charfn(fn, model, lk, flags, tables, prior=None, want=(True, True, True)):
    """-> (cf[S, M] complex128, loglik[S], status[S]); an output that is not wanted keeps its fill (-5, -5; 77)."""
    s, m = lk.shape[0], len(tables)
    a = np.ascontiguousarray(lk, dtype=np.float64)
    cf, ll, st = np.full((s, m, 2), -5.0), np.full(s, -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    cw = as_pairs(tables)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, cf.ctypes.data if want[0] else None, ll.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, cw.ctypes.data, m]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return cf.view(np.complex128)[..., 0], ll, st


def cbits(x):
    """A complex array's bits: its (re, im) pairs as uint64."""
    return np.ascontiguousarray(x, np.complex128).view(np.uint64)


def same_cf(a, b):
    return np.array_equal(cbits(a), cbits(b))
