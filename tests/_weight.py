"""What the weight tests share (test_weight_host.py, test_gpu_weight.py): the weight tables of a batch, the reference and the
comparison.

Reference: test_pattern_host._total(ped, mrate, lk * w, flags, prior) — the project's own elimination on rows premultiplied in
double — and up to ten members also the 3^N enumeration of test_map_host.brute_weights, each configuration's weight times
prod_p w[p][g_p].

Bars (test_evidence_host's derivation: a relative 1e-9 on Z is 4.3e-10 in log10): status exact, wt_loglik and loglik at an
ABSOLUTE 1e-9 on log10, -inf exactly where the reference's Z_m is exactly 0.  No site is left out: clear() asserts on the
reference alone that status is 0 except at planted failures and that Z and every non-zero Z_m are >= 1e-200.
"""
import numpy as np

import famseq_amd as fs
from test_map_host import brute_weights
from test_pattern_host import _total

LL_ATOL = 1e-9
FLOOR = 1e-200
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kWeightVariants
PENS = [(0.01, 0.8, 0.9), (0.0, 1.0, 1.0), (0.001, 0.001, 1.0), (0.05, 0.5, 0.5)]


def batch_weights(ped):
    """The ten tables of a batch, from RandomState(500 + N): four penetrance tables (PENS; at most six affected, from a random
    40 % of the members, and at most six unaffected), four that give at most six random members entries 10^U(-3, 0), one with a
    (2.0, 3.5, 0.25) row (weights above 1), one with a single 0 entry."""
    n = ped.n
    rng = np.random.RandomState(500 + n)
    tables = []
    for pen in PENS:
        order = rng.permutation(n)
        k = max(1, int(round(0.4 * n)))
        tables.append(fs.penetrance_weights(n, order[:k][:6], order[k:][:6], pen))
    for _ in range(4):
        w = np.ones((n, 3))
        who = rng.permutation(n)[:rng.randint(1, min(6, n) + 1)]
        w[who] = 10.0 ** rng.uniform(-3, 0, (len(who), 3))
        tables.append(w)
    w = np.ones((n, 3))
    w[rng.randint(n)] = (2.0, 3.5, 0.25)
    tables.append(w)
    w = np.ones((n, 3))
    w[rng.randint(n), rng.randint(3)] = 0.0
    tables.append(w)
    return np.stack(tables)


def reference(ped, mrate, lk, flags, weights, prior=None, brute=True):
    """-> (z[S], zm[S, M], status[S]): the total weight of the rows as they are, of the rows times every table (all with the
    reference's 1e7), and the status of the real rows.  Up to ten members (brute) the 3^N enumeration is checked against the
    elimination here."""
    z, fail = _total(ped, mrate, lk, flags, prior)
    cols = []
    for w in weights:
        zw, fw = _total(ped, mrate, lk * w, flags, prior)
        cols.append(np.where(fw, 0.0, zw))  # (a weighted row without any mass: the product is 0 in every configuration)
    zm = np.stack(cols, axis=1)
    if brute and ped.n <= 10 and prior is None:
        G, W, bst = brute_weights(ped, mrate, lk, flags)
        W = np.where((bst != 0)[:, None], 0.0, np.nan_to_num(W))
        for j, w in enumerate(weights):
            wm = W @ np.prod(w[np.arange(ped.n)[:, None], G], axis=0)
            good = bst == 0
            assert np.array_equal(wm[good] == 0, zm[good, j] == 0)
            np.testing.assert_allclose(zm[good, j], wm[good], rtol=1e-11, atol=0)
    st = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    return z, zm, st


def clear(ref, what="", planted=()):
    """On the reference alone: nothing is left out of a comparison."""
    z, zm, st = ref
    ok = np.ones(len(z), bool)
    ok[list(planted)] = False
    assert np.all(st[ok] == 0) and np.all(st[~ok] != 0), what
    assert np.all(z[ok] >= FLOOR) and np.all((zm[ok] == 0) | (zm[ok] >= FLOOR)), what


def check(out, ref, what="", digits=7.0):
    """The module docstring's rules; every site and table compared.  Prints the worst errors before it asserts."""
    wl, ll, st = out
    z, zm, ref_st = ref
    assert np.array_equal(st, ref_st), what
    ok = ref_st == 0
    assert np.all(np.isnan(ll[~ok])) and np.all(np.isnan(wl[~ok])), what
    zero = zm[ok] == 0
    with np.errstate(divide="ignore"):
        want = np.log10(zm[ok]) - digits
    got = wl[ok]
    err_w = np.abs(got[~zero] - want[~zero])
    err = np.abs(ll[ok] - (np.log10(z[ok]) - digits))
    print("%s: %d sites x %d tables, %d exact zeros, worst |wt_loglik error| %.3g, worst |loglik error| %.3g, smallest Z %.3g, "
          "smallest non-zero Z_m %.3g" % (what, ok.sum(), zm.shape[1], zero.sum(), err_w.max(initial=0), err.max(initial=0),
                                          z[ok].min(initial=1), zm[ok][~zero].min(initial=1)))
    assert np.array_equal(np.isneginf(got), zero), what
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=0, atol=LL_ATOL, err_msg=what)
    np.testing.assert_allclose(ll[ok], np.log10(z[ok]) - digits, rtol=0, atol=LL_ATOL, err_msg=what)
