"""Shared by the tests of the trio and MAP kernels under site priors (tests/test_trio_map_prior_host.py on the CPU,
tests/test_gpu_trio_map_prior.py and tests/test_cli_prior_joint_gpu.py on the device): the reference, by the bucket elimination
of tests/_maxproduct.py over per-site-prior factors.

The factors are _maxproduct.site_factors' with the founders' prior taken from prior[S][6] instead of the model's constants:
doubles 0-2 for female founders and for every founder off chrX, doubles 3-5 for male founders at chrX sites only; the Known
bit is ignored.  From them: the MAP weight, the total weight Z, the weight of a given configuration, and the joint of (child,
mother, father) for every child by eliminating every other member with sum.  reference() pins all of that to the project's
oracle: on each batch the marginals of these joints agree with _prior.reference (the compiled oracle, one model per site, its
-LRC shortcut switched off so that every site is compared) at 1e-9.
"""
import numpy as np

import _maxproduct as mp
import _prior as P
import famseq_amd as fs

RTOL = P.RTOL
TINY = 1e-280  # a total mass below this: the MAP checks may compare status alone (tests/test_gpu_map.py)


def site_factors(ped, mrate, lk, flags, prior):
    """-> (factors [(vars, array[S, 3, ...])], single_fail[S]): one factor per member, axes in the order of vars."""
    mo, fa = ped.relations()
    gender = np.asarray(ped.genders)
    pcp2, xf, xm = (np.asarray(t, float).reshape(3, 3, 3) for t in fs.transmission_tables(mrate))
    chrx = (np.asarray(flags) & fs.FLAG_CHRX) != 0
    prior = np.asarray(prior, float)
    autos = prior[:, 0:3]
    male = np.where(chrx[:, None], prior[:, 3:6], autos)  # (the male half is not read off chrX, whatever it holds)
    factors, fail = [], np.zeros(lk.shape[0], bool)
    for p in range(ped.n):
        pr = male if gender[p] == 1 else autos
        fail |= (lk[:, p] * pr).sum(axis=1) <= 0  # the single-posterior failure rule (every member, founder or not)
        if mo[p] < 0:
            factors.append(((p,), pr * lk[:, p]))
        else:
            t = np.where(chrx[:, None, None, None], (xm if gender[p] == 1 else xf)[None], pcp2[None])
            factors.append(((p, int(mo[p]), int(fa[p])), t * lk[:, p][:, :, None, None]))
    return factors, fail


def children_of(ped):
    mo, _ = ped.relations()
    return [p for p in range(ped.n) if mo[p] >= 0]


def dnm_mask(ped, flags):
    """[S, K, 27] bool: where the mutation-free transmission table of the child is 0 (autosome; chrX: the son's or daughter's)."""
    kids = children_of(ped)
    a0, xf0, xm0 = (np.asarray(t) for t in fs.transmission_tables(0.0))
    auto = np.array([a0 == 0 for _ in kids]).reshape(-1, 27)
    x = np.array([(xm0 if ped.genders[c] == 1 else xf0) == 0 for c in kids]).reshape(-1, 27)
    return np.where(((np.asarray(flags) & fs.FLAG_CHRX) != 0)[:, None, None], x[None], auto[None])


class Reference:
    """Of one batch (lk, flags, prior): wmax, z (MAP weight and total weight, what the products gave), map_status; joint[S, K, 27]
    and dnm[S, K] (NaN where trio_status != 0), trio_status; marg[S, N, 3] (the marginals of those joints)."""
    PER_SITE = ("lk", "flags", "prior", "wmax", "z", "map_status", "joint", "dnm", "trio_status", "marg")

    def take(self, index):
        """The same of the sites index (a slice or an index array, repeats allowed)."""
        out = Reference()
        out.ped, out.mrate = self.ped, self.mrate
        for k in self.PER_SITE:
            setattr(out, k, getattr(self, k)[index])
        return out


def analyse(ped, lk, flags, prior, mrate=1e-7):
    mo, fa = ped.relations()
    s, n = lk.shape[0], ped.n
    factors, fail = site_factors(ped, mrate, lk, flags, prior)
    order = mp.elimination_order(factors, n)
    r = Reference()
    r.ped, r.mrate, r.lk, r.flags, r.prior = ped, mrate, lk, flags, prior
    r.wmax = mp._constant(mp.eliminate(factors, order, True)[0], s)
    r.z = mp._constant(mp.eliminate(factors, order, False)[0], s)
    r.map_status = np.where(fail, 1, np.where((r.z <= 0) | (r.wmax <= 0), 2, 0)).astype(np.uint8)
    kids = children_of(ped)
    raw = np.empty((s, len(kids), 27))
    for k, c in enumerate(kids):
        keep = [c, int(mo[c]), int(fa[c])]
        rest, _ = mp.eliminate(factors, [v for v in order if v not in keep], False)
        t = np.full((s, 3, 3, 3), 1e7)
        for vs, a in rest:
            t = t * mp._align(vs, a, keep)
        raw[:, k] = t.reshape(s, 27)  # 9 gc + 3 gm + gf
    tot = raw.sum(axis=2)
    r.trio_status = np.where(fail, 1, np.where((tot <= 0).any(axis=1) | (r.z <= 0), 2, 0)).astype(np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        r.joint = raw / tot[:, :, None]
    r.joint[r.trio_status != 0] = np.nan
    r.dnm = np.where(dnm_mask(ped, flags), r.joint, 0.0).sum(axis=2)
    r.dnm[r.trio_status != 0] = np.nan
    # every member's marginal: from the first joint that holds it; a member of no family by an elimination of its own
    r.marg = np.full((s, n, 3), np.nan)
    seen = set()
    for k, c in enumerate(kids):
        j = r.joint[:, k].reshape(s, 3, 3, 3)
        for p, axes in ((c, (2, 3)), (int(mo[c]), (1, 3)), (int(fa[c]), (1, 2))):
            if p not in seen:
                seen.add(p)
                r.marg[:, p] = j.sum(axis=axes)
    for p in set(range(n)) - seen:
        rest, _ = mp.eliminate(factors, [v for v in order if v != p], False)
        m = np.ones((s, 3))
        for vs, a in rest:
            m = m * (a if vs == (p,) else a[:, None])
        with np.errstate(invalid="ignore", divide="ignore"):
            r.marg[:, p] = m / m.sum(axis=1, keepdims=True)
    return r


def config_weight(r, gt):
    """The weight of configuration gt[S, N] as a plain product over the members, in PED order."""
    factors, _ = site_factors(r.ped, r.mrate, r.lk, r.flags, r.prior)
    rows = np.arange(len(r.lk))
    w = np.full(len(rows), 1e7)
    g = np.asarray(gt, np.int64)
    for vs, a in factors:
        w = w * a[(rows,) + tuple(g[:, u] for u in vs)]
    return w


def tiny_sites(r):
    """Sites whose total mass lies below 1e-280 (and that do not fail the single-posterior rule): at most 2 % of a batch."""
    tiny = (r.map_status != 1) & ~(r.z >= TINY)
    assert tiny.sum() <= 0.02 * len(tiny), "%d of %d sites below 1e-280" % (tiny.sum(), len(tiny))
    return tiny


def batch(ped, n_sites=P.N_SITES):
    """_prior.batch, its sharp sites raised where the joint needs it.  _prior.batch is conditioned for marginals; a joint has
    entries many orders below its row's total, and what holds such an entry before the division by the total can lie below the
    normal range of a double where no marginal does (joint_well_conditioned finds such sites):
      21-24 members: 1e-40 -> 1e-30.  With 1e-40, 169 entries of wide24's 200 sites (264 of its 1000) change under a rescaling.
      40 members on: 1e-18 -> 1e-12.  With 1e-18, 5 of wide48's 200 sites (2.5 %) have a total mass below 1e-280 (z down to
        1.6e-298 and one 0), more than the 2 % that may be compared on status alone, and 1323 entries change under a rescaling;
        with 1e-14 no site lies below 1e-280 (the smallest z is 8.6e-270) and 36 entries change; with 1e-12 none."""
    lk, flags, prior = P.batch(ped, n_sites)
    if 20 < ped.n <= 24:
        lk[lk == 1e-40] = 1e-30
    if ped.n >= 40:
        lk[lk == 1e-18] = 1e-12
    return lk, flags, prior


def joint_well_conditioned(r):
    """The helper's own digits can be trusted on every site and entry (_prior.assert_well_conditioned's rule, for the joint and
    the MAP weights): with every likelihood row scaled by 2^8, which scales every weight by 2^(8 N) exactly unless a product has
    left the normal range on the way, the joints have the same bits and Z and the maximum are scaled exactly."""
    again = analyse(r.ped, r.lk * 256.0, r.flags, r.prior, r.mrate)
    scale = 256.0 ** r.ped.n
    assert np.array_equal(again.trio_status, r.trio_status) and np.array_equal(again.map_status, r.map_status)
    assert np.array_equal(P.bits(again.joint), P.bits(r.joint)) and np.array_equal(P.bits(again.dnm), P.bits(r.dnm))
    assert np.array_equal(again.z, r.z * scale) and np.array_equal(again.wmax, r.wmax * scale)


_REF = {}


def reference(name, n_sites=P.N_SITES):
    """-> (ped, lk, flags, prior, Reference) of batch(pedigree(name), n_sites), computed once and pinned to the oracle."""
    key = (name, n_sites)
    if key not in _REF:
        ped = P.pedigree(name)
        lk, flags, prior = batch(ped, n_sites)
        assert set(np.unique(flags)) == {0, 1, 2, 3}
        r = analyse(ped, lk, flags, prior)
        tiny_sites(r)  # (on the helper alone, before any kernel runs)
        joint_well_conditioned(r)
        # the oracle with one model per site; lc = 2: no site takes the -LRC shortcut, whose posterior is not the network's
        ref = P.reference(ped, lk, flags, prior, lc=2.0)
        P.assert_well_conditioned(ped, lk, flags, prior, ref, lc=2.0)
        assert np.array_equal(ref[2], r.trio_status), name
        ok = ref[2] == 0
        assert ok.sum() > 0.5 * len(lk)
        np.testing.assert_allclose(r.marg[ok], ref[0][ok], rtol=RTOL, atol=0, err_msg=name)
        _REF[key] = (ped, lk, flags, prior, r)
    return _REF[key]


def check_trio(out, r, what=""):
    """joint and dnm (either may be None) at RTOL against the helper's, status equal, failed rows NaN."""
    joint, dnm, st = out
    assert np.array_equal(st, r.trio_status), what
    ok = st == 0
    if joint is not None:
        np.testing.assert_allclose(joint[ok], r.joint[ok], rtol=RTOL, atol=0, err_msg=what)
        assert np.all(np.isnan(joint[~ok])), what
    if dnm is not None:
        np.testing.assert_allclose(dnm[ok], r.dnm[ok], rtol=RTOL, atol=0, err_msg=what)
        assert np.all(np.isnan(dnm[~ok])), what


def check_map(out, r, what=""):
    """The returned configuration's weight >= (1 - 1e-9) the helper's maximum, map_post = w_returned / Z at RTOL, status equal,
    map_gt -1 exactly where status != 0.  Sites below 1e-280 of total mass: status alone (and 2 may fall on one side only).
    -> the number of sites compared in full."""
    gt, post, st = out
    bad = st != 0
    assert np.all(gt[bad] == -1) and np.all(np.isnan(post[bad])), what
    assert np.all((gt[~bad] >= 0) & (gt[~bad] <= 2)) and np.all(np.isfinite(post[~bad])), what
    tiny = (r.map_status != 1) & ~(r.z >= TINY)
    assert np.array_equal(st[~tiny], r.map_status[~tiny]) and np.array_equal(st == 1, r.map_status == 1), what
    ok = (st == 0) & (r.map_status == 0) & ~tiny
    sub = r.take(ok)
    w_ret = config_weight(sub, gt[ok])
    assert np.all(w_ret >= (1 - 1e-9) * sub.wmax), what
    np.testing.assert_allclose(post[ok], w_ret / sub.z, rtol=RTOL, atol=0, err_msg=what)
    return int(ok.sum())
