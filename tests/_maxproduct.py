"""Test helper: the joint MAP configuration of a pedigree network by bucket elimination in numpy.

Independent of the kernel generator (csrc/elim_codegen.cpp passes messages over the member / nuclear-family graph and cuts loops
by conditioning; this eliminates one member at a time from a list of factor tables, in a greedy smallest-scope order, and so
serves loops without knowing about them).  Log-free: plain products of the same weights the 3^N enumeration forms,
    w(g) = 1e7 * prod_m f_m(g_m | g_mother, g_father),   f = prior * lk for a founder, T[g | gm, gf] * lk otherwise,
vectorised over sites.  max_product() eliminates with max and keeps the arg-max tables for the back-track (ties: numpy's first
maximum, which is NOT the kernel's tie rule — compare weights, not configurations); its total weight Z and the marginals come
from the same elimination with sum.
"""
import numpy as np

import famseq_amd as fs

GN, GK, GXN, GXK = (0.9985, 0.001, 0.0005), (0.45, 0.1, 0.45), (0.999, 0, 0.001), (0.5, 0, 0.5)


def site_factors(ped, mrate, lk, flags):
    """-> (factors [(vars, array[S, 3, ...])], single_fail[S]): one factor per member, axes in the order of vars."""
    mo, fa = ped.relations()
    gender = np.asarray(ped.genders)
    pcp2, xf, xm = (np.asarray(t, float).reshape(3, 3, 3) for t in fs.transmission_tables(mrate))
    flags = np.asarray(flags)
    known, chrx = (flags & 1) != 0, (flags & 2) != 0
    autos = np.where(known[:, None], np.array(GK), np.array(GN))
    male = np.where(chrx[:, None], np.where(known[:, None], np.array(GXK), np.array(GXN)), autos)
    factors, fail = [], np.zeros(lk.shape[0], bool)
    for p in range(ped.n):
        prior = male if gender[p] == 1 else autos
        fail |= (lk[:, p] * prior).sum(axis=1) <= 0  # the single-posterior failure rule (every member, founder or not)
        if mo[p] < 0:
            factors.append(((p,), prior * lk[:, p]))
        else:
            t = np.where(chrx[:, None, None, None], (xm if gender[p] == 1 else xf)[None], pcp2[None])
            factors.append(((p, int(mo[p]), int(fa[p])), t * lk[:, p][:, :, None, None]))
    return factors, fail


def _align(vars_, arr, scope):
    order = sorted(range(len(vars_)), key=lambda i: scope.index(vars_[i]))
    a = np.transpose(arr, [0] + [1 + i for i in order])
    return a.reshape([arr.shape[0]] + [3 if u in vars_ else 1 for u in scope])


def elimination_order(factors, n):
    scopes = [set(v) for v, _ in factors]
    left, order = set(range(n)), []
    while left:
        def merged(v):
            s = set()
            for sc in scopes:
                if v in sc:
                    s |= sc
            return s
        v = min(sorted(left), key=lambda u: len(merged(u)))
        s = merged(v)
        scopes = [sc for sc in scopes if v not in sc] + [s - {v}]
        left.remove(v)
        order.append(v)
    return order


def eliminate(factors, order, use_max):
    """Eliminate the members of `order` in turn.  -> (remaining factors, trace [(v, scope without v, argmax table)])."""
    factors, trace = list(factors), []
    for v in order:
        mine = [f for f in factors if v in f[0]]
        factors = [f for f in factors if v not in f[0]]
        scope = [v] + sorted({u for vs, _ in mine for u in vs} - {v})
        prod = None
        for vs, a in mine:
            a = _align(vs, a, scope)
            prod = a if prod is None else prod * a
        if prod is None:
            continue
        prod = np.broadcast_to(prod, [prod.shape[0]] + [3] * len(scope))
        if use_max:
            trace.append((v, scope[1:], prod.argmax(axis=1)))
            factors.append((tuple(scope[1:]), prod.max(axis=1)))
        else:
            factors.append((tuple(scope[1:]), prod.sum(axis=1)))
    return factors, trace


def _constant(factors, n_sites):
    out = np.full(n_sites, 1e7)
    for vs, a in factors:
        assert vs == ()
        out = out * a
    return out


def max_product(ped, mrate, lk, flags):
    """-> (map_gt[S, N] int8, w_max[S], Z[S], status[S]); map_gt is -1 where status != 0.  w_max and Z are what the products
    gave, also where status is 2 (a total at the bottom of the double range underflows in one order of products and not in
    another: the caller decides what a Z of 0 or 1e-300 is worth)."""
    factors, fail = site_factors(ped, mrate, lk, flags)
    s, n = lk.shape[0], ped.n
    order = elimination_order(factors, n)
    rest, trace = eliminate(factors, order, True)
    wmax = _constant(rest, s)
    z = _constant(eliminate(factors, order, False)[0], s)
    gt = np.zeros((s, n), np.int64)
    rows = np.arange(s)
    for v, scope, arg in reversed(trace):
        gt[:, v] = arg[(rows,) + tuple(gt[:, u] for u in scope)]
    status = np.where(fail, 1, np.where((z <= 0) | (wmax <= 0), 2, 0)).astype(np.uint8)
    bad = status != 0
    gt[bad] = -1
    return gt.astype(np.int8), wmax, z, status


def marginals(ped, mrate, lk, flags):
    """Every member's normalised marginal [S, N, 3] by the sum pass (one elimination per member, the member last)."""
    factors, _ = site_factors(ped, mrate, lk, flags)
    order = elimination_order(factors, ped.n)
    out = np.zeros((lk.shape[0], ped.n, 3))
    for p in range(ped.n):
        rest, _ = eliminate(factors, [v for v in order if v != p], False)
        m = np.ones((lk.shape[0], 3))
        for vs, a in rest:
            m = m * (a if vs == (p,) else a[:, None])
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, p] = m / m.sum(axis=1, keepdims=True)
    return out


def config_weight(ped, mrate, lk, flags, gt):
    """The weight of configuration gt[S, N] as a plain product over the members, in PED order."""
    factors, _ = site_factors(ped, mrate, lk, flags)
    rows = np.arange(lk.shape[0])
    w = np.full(lk.shape[0], 1e7)
    g = np.asarray(gt, np.int64)
    for vs, a in factors:
        w = w * a[(rows,) + tuple(g[:, u] for u in vs)]
    return w


def mendelian_consistent(ped, gt, flags):
    """[S] bool: every child's genotype has a non-zero mutation-free transmission entry given its parents'."""
    mo, fa = ped.relations()
    a0, xf0, xm0 = (np.asarray(t, float).reshape(3, 3, 3) for t in fs.transmission_tables(0.0))
    chrx = (np.asarray(flags) & 2) != 0
    g = np.asarray(gt, np.int64)
    ok = np.ones(g.shape[0], bool)
    for c in range(ped.n):
        if mo[c] < 0:
            continue
        x = xm0 if ped.genders[c] == 1 else xf0
        idx = (g[:, c], g[:, mo[c]], g[:, fa[c]])
        ok &= np.where(chrx, x[idx], a0[idx]) != 0
    return ok
