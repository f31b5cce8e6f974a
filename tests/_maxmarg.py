"""Test helper: the max-marginals of a pedigree network, M[p][a] = max over the configurations g with g_p = a of w(g), and
the runner-up's weight.

Two references, neither of which knows the kernel generator's graph:
  elimination()  tests/_maxproduct.py's bucket elimination with max, every member but p eliminated and p last: marginals() of
                 that file in the other semiring.  Serves any size (loops too).  The runner-up comes from the rows as the
                 kernel's does (the largest entry beside the rows' arg-maxes), so its check against the brute force below is
                 a check of that argument, not of the kernel.
  brute()        over test_map_host.brute_weights, up to twelve members: the maximum of W over the configurations with
                 g_p = a, and the second largest of W.
Both return the quantities divided by Z (the sum over every configuration) where status is 0 and NaN elsewhere.
Status, as the MAP references have it: 1 the single-posterior rule, 2 the total or the maximum weight <= 0.

What check() asks, entry by entry (RTOL is tests/test_map_host.py's 1e-9, the project's bar for posteriors):
  - an entry without a supporting configuration of positive weight is exactly 0.0.  Support is decided
    on the zero pattern alone — the same reference run on the rows' indicators (lk > 0), where nothing can underflow — never on
    a product that may have underflowed;
  - a supported entry whose unnormalised value (entry x Z) is at least 1e-280 is positive and agrees at RTOL, atol 0;
  - a supported entry below 1e-280 (the rule of test_map_host.test_wide_pedigrees and tests/_prior_joint.py's TINY: what forms
    such a value passes through subnormal numbers in one order of multiplication and not in another, and a subnormal carries
    fewer than 1e-9's digits, or none) is asked to lie below 1e-279 / Z only.
"""
import collections

import numpy as np

import _maxproduct as mp
import _prior_joint as PJ

RTOL = 1e-9
TINY = 1e-280
MAX_BRUTE = 12

# maxmarg[S, N, 3], top[S, 2], status[S], z[S]; support[S, N, 3] and pair[S] (at least two configurations of positive weight) bool
Reference = collections.namedtuple("Reference", "maxmarg top status z support pair")


def runner_up(m):
    """The second-largest configuration weight from the rows m[S, N, 3]: the largest entry beside the rows' arg-maxes (first
    of equals).  Every configuration but the best differs from it at some member."""
    arg = np.argmax(m, axis=2)
    rest = np.where(np.arange(3)[None, None, :] == arg[:, :, None], -np.inf, m)
    return rest.max(axis=2).max(axis=1)


def _rows_by_elimination(factors, order, s, n):
    m = np.zeros((s, n, 3))
    for p in range(n):
        rest, _ = mp.eliminate(factors, [v for v in order if v != p], True)
        row = np.full((s, 3), 1e7)
        for vs, a in rest:
            row = row * (a if vs == (p,) else a[:, None])
        m[:, p] = row
    return m


def elimination(ped, mrate, lk, flags, prior=None):
    """-> Reference by bucket elimination (prior: the founders' rows per site, through tests/_prior_joint.py's factors)."""
    def factors_of(rows):
        return mp.site_factors(ped, mrate, rows, flags) if prior is None else PJ.site_factors(ped, mrate, rows, flags, prior)

    factors, fail = factors_of(lk)
    s, n = lk.shape[0], ped.n
    order = mp.elimination_order(factors, n)
    z = mp._constant(mp.eliminate(factors, order, False)[0], s)
    m = _rows_by_elimination(factors, order, s, n)
    ind = _rows_by_elimination(factors_of((lk > 0).astype(float))[0], order, s, n)
    wmax = m.max(axis=2).max(axis=1)
    status = np.where(fail, 1, np.where(~(z > 0) | ~(wmax > 0), 2, 0)).astype(np.uint8)
    ok = status == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        maxmarg = np.where(ok[:, None, None], m / z[:, None, None], np.nan)
        top = np.where(ok[:, None], np.stack([wmax, runner_up(m)], axis=1) / z[:, None], np.nan)
    return Reference(maxmarg, top, status, z, ind > 0, runner_up(ind) > 0)


def brute(ped, mrate, lk, flags):
    """-> Reference by the 3^N enumeration of test_map_host.brute_weights (its status: 2 where the sum or the maximum is <= 0)."""
    from test_map_host import brute_weights

    assert ped.n <= MAX_BRUTE
    G, W, status = brute_weights(ped, mrate, lk, flags)
    _, I, _ = brute_weights(ped, mrate, (lk > 0).astype(float), flags)
    s, n = lk.shape[0], ped.n
    ok = status == 0
    m = np.full((s, n, 3), np.nan)
    support = np.zeros((s, n, 3), bool)
    # (G is np.indices: configuration k has member p's genotype on axis p of the 3 x ... x 3 cube)
    Wc, Ic = W[ok].reshape((-1,) + (3,) * n), np.nan_to_num(I[ok]).reshape((-1,) + (3,) * n)
    for p in range(n):
        others = tuple(1 + q for q in range(n) if q != p)
        assert np.array_equal(G[p].reshape((3,) * n).max(axis=tuple(q for q in range(n) if q != p)), [0, 1, 2])
        m[ok, p] = Wc.max(axis=others)
        support[ok, p] = Ic.max(axis=others) > 0
    top = np.full((s, 2), np.nan)
    top[ok] = np.partition(W[ok], -2, axis=1)[:, :-3:-1]
    z = np.where(ok, W.sum(axis=1), np.nan)
    return Reference(m / z[:, None, None], top / z[:, None], status, z, support, (np.nan_to_num(I) > 0).sum(axis=1) >= 2)


def check(out, ref, what="", sites=None):
    """maxmarg and top (either may be None) against the reference by the module's three rules, status equal, failed rows NaN.
    sites: compare the numbers on these sites only (status on all).  -> the number of entries compared at RTOL."""
    maxmarg, top, st = out
    assert np.array_equal(st, ref.status), what
    ok = st == 0
    sel = ok if sites is None else ok & sites
    z = ref.z[sel]
    support_top = np.stack([np.ones(len(st), bool), ref.pair], axis=1)
    compared = 0
    for got, want, support, zz in ((maxmarg, ref.maxmarg, ref.support, z[:, None, None]), (top, ref.top, support_top, z[:, None])):
        if got is None:
            continue
        assert np.all(np.isnan(got[~ok])), what
        g, w, sup = got[sel], want[sel], support[sel]
        assert np.all(g[~sup] == 0), what + ": exact zeros"
        big = sup & (w * zz >= TINY)
        assert np.all(g[big] > 0), what
        np.testing.assert_allclose(g[big], w[big], rtol=RTOL, atol=0, err_msg=what)
        small = sup & ~big
        assert np.all((g * zz)[small] < 10 * TINY), what
        compared += int(big.sum())
    return compared
