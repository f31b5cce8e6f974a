"""Shared by the allele-frequency tests (tests/test_af_host.py on the CPU, tests/test_gpu_af.py and tests/test_cli_af_gpu.py on
the device): the reference, a numpy EM loop over the project's existing references.

Per step at q: the founders' rows are fs.hwe_priors(q); Z(q) is tests/_prior_joint.py's factors through tests/_maxproduct.py's
elimination (with the reference's 1e7); the founders' marginals come, up to twenty members, from tests/_prior.py's reference
(the compiled oracle, one model per site, its -LRC shortcut switched off) and beyond from the same elimination: three totals per
founder, that founder's row masked to one genotype (oracle_upto lowers the size at which the elimination takes over: the oracle
enumerates 3^N configurations per site, which above some thirteen members is no reference a test can wait for).  The update is
the ABI's:
    A = sum over founders, PED order, of (m1 + 2 m2) / (m0 + m1 + m2)   [male founder at a chrX site: m2 / (m0 + m1 + m2)]
    C = 2 founders   [chrX: 2 female founders + male founders];   q' = min(A / C, 1)
Z(0) is the elimination under rows (1, 0, 0), which is what hwe_priors(0) gives exactly.
"""
import numpy as np

import _maxproduct as mp
import _prior as P
import _prior_joint as J
import famseq_amd as fs

FLOOR = 1e-200


def total(ped, mrate, lk, flags, prior):
    """(Z[S] with the reference's 1e7, single_fail[S]) under the rows prior[S, 6]."""
    factors, fail = J.site_factors(ped, mrate, lk, flags, prior)
    return mp._constant(mp.eliminate(factors, mp.elimination_order(factors, ped.n), False)[0], lk.shape[0]), fail


def founders_of(ped):
    mo, _ = ped.relations()
    return [p for p in range(ped.n) if mo[p] < 0]


def founder_rows(ped, mrate, lk, flags, prior, oracle_upto=20):
    """{founder: m[S, 3]}: the founders' marginal rows (any positive scale) under prior[S, 6]."""
    founders = founders_of(ped)
    if ped.n <= oracle_upto:
        post, _, st = P.reference(ped, lk, flags, prior, mrate=mrate, lc=2.0)
        assert np.all(st == 0)
        return {f: post[:, f] for f in founders}
    rows = {}
    for f in founders:
        m = np.empty((lk.shape[0], 3))
        for g in range(3):
            keep = np.ones_like(lk)
            keep[:, f, :] = 0.0
            keep[:, f, g] = 1.0
            m[:, g] = total(ped, mrate, lk * keep, flags, prior)[0]
        rows[f] = m
    return rows


def step(ped, mrate, lk, flags, q, oracle_upto=20):
    """One EM step from q[S] -> q'[S]."""
    chrx = (np.asarray(flags) & fs.FLAG_CHRX) != 0
    rows = founder_rows(ped, mrate, lk, flags, fs.hwe_priors(q), oracle_upto)
    a = np.zeros(len(q))
    n_female = n_male = 0
    for f in founders_of(ped):  # PED order, left to right
        m = rows[f]
        s = (m[:, 0] + m[:, 1]) + m[:, 2]
        assert np.all((s > 0) & np.isfinite(s))
        male = ped.genders[f] == 1
        a = a + np.where(chrx & male, m[:, 2], m[:, 1] + 2 * m[:, 2]) / s
        n_male, n_female = n_male + male, n_female + (not male)
    c = np.where(chrx, 2.0 * n_female + n_male, 2.0 * (n_female + n_male))
    return np.minimum(a / c, 1.0)


class Reference:
    """Of one batch: q[T + 1, S] (q[t] after t steps), z[T + 1, S] = Z(q[t]) and z0[S] = Z(0), both with the reference's 1e7, and
    status[S] (under af0's rows).  The caller's sites are expected to be good ones: every step asserts it."""


def reference(ped, mrate, lk, flags, af0, n_iter, oracle_upto=20):
    r = Reference()
    af0 = np.asarray(af0, float)
    s = lk.shape[0]
    z, fail = total(ped, mrate, lk, flags, fs.hwe_priors(af0))
    r.status = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    assert np.all(r.status == 0) and np.all(z >= FLOOR)  # (on the reference alone: no site is left out of any comparison)
    r.q, r.z = np.empty((n_iter + 1, s)), np.empty((n_iter + 1, s))
    r.q[0], r.z[0] = af0, z
    for t in range(n_iter):
        r.q[t + 1] = step(ped, mrate, lk, flags, r.q[t], oracle_upto)
        r.z[t + 1] = total(ped, mrate, lk, flags, fs.hwe_priors(r.q[t + 1]))[0]
        assert np.all(r.z[t + 1] >= FLOOR)
    r.z0 = total(ped, mrate, lk, flags, fs.hwe_priors(np.zeros(s)))[0]
    return r


def loglik(r, t):
    """[S, 2]: what the kernel's loglik is after t steps (-inf where Z(0) is 0)."""
    with np.errstate(divide="ignore"):
        return np.stack([np.log10(r.z[t]) - 7.0, np.log10(r.z0) - 7.0], axis=1)
