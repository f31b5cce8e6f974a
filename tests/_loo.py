"""Test helper: leave-one-out posteriors and per-member fit of a pedigree network, by bucket elimination in numpy.

For member p the factors are tests/_maxproduct.py's (tests/_prior_joint.py's under per-site priors) with p's likelihood row
replaced by ones; every member but p is eliminated with sum, which leaves the unnormalised cavity row of p (the reference's 1e7
included, as in every weight of those helpers).  One elimination per member.  With Z_-p the row's sum and Z the total weight of
the unmasked factors:
    loo[s, p] = row / Z_-p,     fit[s, p] = Z / Z_-p.
Status: 1 from site_factors' failure flag on the real rows, 2 where any Z_-p is <= 0 or not finite, else 0.  Independent of the
kernel generator: no messages, no conditioning, and the likelihood is masked in the input, never left out of a product.

pinned() ties the helper once to the compiled per-site oracle: the oracle's posterior of a batch with row p masked to ones is
loo[:, p], at rtol 1e-9, on the sites where the oracle reports status 0 (not the shortcut's 0x80), at trio and ped10.
"""
import numpy as np

import _maxproduct as mp
import _prior_joint as J
import famseq_amd as fs

RTOL = 1e-9   # the project's bar for posteriors
FLOOR = 1e-200  # a clear batch: Z and every Z_-p at or above this


class Loo:
    """loo[S, N, 3], fit[S, N] (NaN where status != 0), status[S]; z[S] and zc[S, N] = Z_-p, what the products gave."""


def _factors(ped, mrate, lk, flags, prior):
    if prior is None:
        return mp.site_factors(ped, mrate, lk, flags)
    return J.site_factors(ped, mrate, lk, flags, prior)


def analyse(ped, mrate, lk, flags, prior=None):
    lk = np.asarray(lk, float)
    s, n = lk.shape[0], ped.n
    factors, fail = _factors(ped, mrate, lk, flags, prior)
    bare, _ = _factors(ped, mrate, np.ones_like(lk), flags, prior)  # every member's factor without its likelihood
    order = mp.elimination_order(factors, n)
    r = Loo()
    r.z = mp._constant(mp.eliminate(factors, order, False)[0], s)
    row = np.empty((s, n, 3))
    for p in range(n):
        masked = factors[:p] + [bare[p]] + factors[p + 1:]
        rest, _ = mp.eliminate(masked, [v for v in order if v != p], False)
        m = np.full((s, 3), 1e7)
        for vs, a in rest:
            assert vs in ((), (p,))
            m = m * (a if vs == (p,) else a[:, None])
        row[:, p] = m
    r.zc = row.sum(axis=2)
    bad = ~((r.zc > 0) & np.isfinite(r.zc))
    r.status = np.where(fail, 1, np.where(bad.any(axis=1), 2, 0)).astype(np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        r.loo = row / r.zc[:, :, None]
        r.fit = r.z[:, None] / r.zc
    r.loo[r.status != 0] = np.nan
    r.fit[r.status != 0] = np.nan
    return r


def is_clear(r):
    """What every test asserts of its batch, on the reference alone: no failure, Z and every Z_-p at or above 1e-200."""
    return bool(np.all(r.status == 0) and np.all(r.z >= FLOOR) and np.all(r.zc >= FLOOR))


def check(out, r, what="", clear=True):
    """loo and fit (either may be None) at RTOL with atol 0 — a reference entry of exactly 0 must be exactly 0 —, status exact,
    failed sites NaN; every site is compared.  Prints the worst relative errors before it asserts."""
    loo, fit, st = out
    if clear:
        assert is_clear(r), what
    assert np.array_equal(st, r.status), "%s: status %s, wanted %s" % (what, st, r.status)
    ok = r.status == 0
    for name, got, want in (("loo", loo, r.loo), ("fit", fit, r.fit)):
        if got is None:
            continue
        assert np.all(np.isnan(got[~ok])), what
        g, w = got[ok], want[ok]
        assert np.array_equal(g == 0, w == 0), "%s: %s: exact zeros differ" % (what, name)
        nz = w != 0
        print("%s: %s, %d values, worst relative error %.3g" % (what, name, nz.sum(), np.abs(g[nz] / w[nz] - 1.0).max(initial=0)))
        np.testing.assert_allclose(g, w, rtol=RTOL, atol=0, err_msg="%s: %s" % (what, name))


_PINNED = []


def pinned():
    """Once per session: the helper against the compiled per-site oracle, at trio and ped10 (see the module's docstring)."""
    if _PINNED:
        return
    import oracle

    for name in ("trio", "ped10"):
        ped = fs.synthetic_pedigree(name)
        ped.relations()
        rng = np.random.RandomState(17 + ped.n)
        lk = 10.0 ** (-rng.uniform(0, 30, size=(60, ped.n, 3)) / 10.0)
        flags = (np.arange(60) % 4).astype(np.uint8)
        for mrate in (1e-7, 1e-4):
            r = analyse(ped, mrate, lk, flags)
            assert is_clear(r)
            m = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=mrate)
            compared = 0
            for p in range(ped.n):
                masked = lk.copy()
                masked[:, p] = 1.0
                post, _, status = m.bn_batch(masked, flags)
                ok = status == 0
                compared += int(ok.sum())
                np.testing.assert_allclose(r.loo[ok, p], post[ok, p], rtol=RTOL, atol=0, err_msg="%s member %d" % (name, p))
            assert compared > 0.5 * 60 * ped.n, "%s: the oracle took its shortcut on most sites" % name
    _PINNED.append(True)
