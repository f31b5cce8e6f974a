"""Shared by the tests of phase by transmission (famseq_origin: tests/test_origin_host.py on the CPU, tests/test_gpu_origin.py and
tests/test_cli_phase_gpu.py on the device): the reference in numpy.

The quantity: the pedigree network with child k's transmission factor T(gc | gm, gf) replaced by tm(a | gm) tf(b | gf) [gc ==
gamma(a, b)], a and b the alleles (0 ref, 1 alt) received from mother and father.  Given the joint posterior of (child, mother,
father) — test_trio_host.brute_joint's, a 3^N enumeration, or beyond its reach tests/_prior_joint.py's elimination — that is a
split of each joint cell by tm tf / sum_{gamma(a', b') = gc} tm tf, cells whose sum is 0 (where T is 0) skipped.  The allele rows
are formed from the rate here (allele_rows), never taken from the library; the tests assert famseq_allele_tables equal to them.
"""
import numpy as np

import famseq_amd as fs

RTOL = 1e-9  # the project's (tests/test_trio_host.py)
GN, GK, GXN, GXK = (0.9985, 0.001, 0.0005), (0.45, 0.1, 0.45), (0.999, 0, 0.001), (0.5, 0, 0.5)


def allele_rows(mu):
    """[2 chrX][2 child sex: 0 son, 1 daughter][2 parent: 0 mother, 1 father][2 allele][3 genotype]."""
    u = 1 - mu
    two = np.array([[u, 0.5, mu], [mu, 0.5, u]])
    hemi = np.array([[u, 0.0, mu], [mu, 0.0, u]])  # a father's X: never heterozygous
    none = np.array([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])  # a son gets no X from his father
    t = np.empty((2, 2, 2, 2, 3))
    t[0, :, :] = two
    t[1, :, 0] = two
    t[1, 0, 1] = none
    t[1, 1, 1] = hemi
    return t


def gamma(chrx, son, a, b):
    return 2 * a if (chrx and son) else a + b


def split_tables(mu):
    """w[2 chrX][2 sex][4 (2a+b)][27 (9 gc + 3 gm + gf)]: the share of joint cell (gc, gm, gf) that goes to (a, b)."""
    al = allele_rows(mu)
    w = np.zeros((2, 2, 4, 27))
    for x in range(2):
        for sex in range(2):
            raw = np.zeros((4, 3, 3, 3))
            for a in range(2):
                for b in range(2):
                    raw[2 * a + b, gamma(x, sex == 0, a, b)] = al[x, sex, 0, a][:, None] * al[x, sex, 1, b][None, :]
            tot = raw.sum(axis=0)
            with np.errstate(invalid="ignore", divide="ignore"):
                w[x, sex] = np.where(tot > 0, raw / tot, 0.0).reshape(4, 27)
    return w


def split(joint, ped, mu, flags):
    """joint[S, K, 27] (NaN rows stay NaN) -> (origin[S, K, 4], hettx[S, K, 4])."""
    mo, _ = ped.relations()
    kids = [p for p in range(ped.n) if mo[p] >= 0]
    w = split_tables(mu)
    chrx = ((np.asarray(flags) & 2) != 0).astype(int)
    s = joint.shape[0]
    origin, hettx = np.empty((s, len(kids), 4)), np.empty((s, len(kids), 4))
    gm = (np.arange(27) // 3) % 3
    gf = np.arange(27) % 3
    for k, c in enumerate(kids):
        wk = w[chrx, 0 if ped.genders[c] == 1 else 1]  # [S, 4, 27]
        part = wk * joint[:, k][:, None, :]
        origin[:, k] = part.sum(axis=2)
        mhet, fhet = part[:, :, gm == 1].sum(axis=2), part[:, :, gf == 1].sum(axis=2)  # [S, 4]
        hettx[:, k, 0] = mhet[:, 2] + mhet[:, 3]  # a = 1
        hettx[:, k, 1] = mhet[:, 0] + mhet[:, 1]
        hettx[:, k, 2] = fhet[:, 1] + fhet[:, 3]  # b = 1
        hettx[:, k, 3] = fhet[:, 0] + fhet[:, 2]
    return origin, hettx


def brute_joint_prior(ped, mrate, lk, flags, prior=None):
    """test_trio_host.brute_joint's statements with the founders' prior optionally the site's own rows; used for batches with
    prior rows only, and held against brute_joint itself on every batch of tests/test_origin_host.py's enumeration test (prior [S, 6]: doubles 0-2 for female
    founders and every founder off chrX, 3-5 for male founders at chrX sites; the Known bit is then not read).
    -> (joint[S, K, 27], status[S])."""
    mo, fa = ped.relations()
    n = ped.n
    gender = np.asarray(ped.genders)
    children = [p for p in range(n) if mo[p] >= 0]
    pcp2, xf, xm = fs.transmission_tables(mrate)
    G = np.indices((3,) * n).reshape(n, -1)
    joint = np.full((lk.shape[0], len(children), 27), np.nan)
    status = np.zeros(lk.shape[0], np.uint8)
    for s in range(lk.shape[0]):
        known, chrx = flags[s] & 1, flags[s] & 2
        if prior is None:
            autos = np.array(GK if known else GN)
            male = np.array(GXK if known else GXN) if chrx else autos
        else:
            autos = np.asarray(prior[s, 0:3], float)
            male = np.asarray(prior[s, 3:6], float) if chrx else autos
        pr = [male if gender[p] == 1 else autos for p in range(n)]
        if any(((lk[s, p] * pr[p]).sum() <= 0) for p in range(n)):
            status[s] = 1
            continue
        w = np.full(G.shape[1], 1e7)
        for p in range(n):
            if mo[p] < 0:
                t = pr[p][G[p]]
            else:
                T = ((xm if gender[p] == 1 else xf) if chrx else pcp2)
                t = T[9 * G[p] + 3 * G[mo[p]] + G[fa[p]]]
            w = w * (t * lk[s, p][G[p]])
        tot = w.sum()
        if tot <= 0:
            status[s] = 2
            continue
        for k, c in enumerate(children):
            joint[s, k] = np.bincount(9 * G[c] + 3 * G[mo[c]] + G[fa[c]], weights=w, minlength=27) / tot
    return joint, status


class Ref:
    """origin, hettx [S, K, 4], status [S], joint [S, K, 27] of one batch."""


def reference(ped, mrate, lk, flags, prior=None, joint=None, status=None):
    """The reference of a batch: by the 3^N enumeration (test_trio_host.brute_joint; with prior rows brute_joint_prior), or from a
    joint and status computed elsewhere."""
    from test_trio_host import brute_joint

    r = Ref()
    if joint is None:
        joint, status = brute_joint(ped, mrate, lk, flags) if prior is None else brute_joint_prior(ped, mrate, lk, flags, prior)
    r.joint, r.status, r.flags = joint, status, np.asarray(flags)
    r.origin, r.hettx = split(joint, ped, mrate, flags)
    r.ped = ped
    return r


def close(got, ref, what=""):
    """test_trio_host.check_joint's rule, per row: RTOL relative on entries >= 1e-280 x the row's maximum, <= 1e-270 x it below
    (a row of zeros — the father's pair at a chrX site — is then wanted exactly)."""
    big = np.nanmax(ref, axis=-1, keepdims=True)
    sel = ref >= 1e-280 * big
    np.testing.assert_allclose(got[sel], ref[sel], rtol=RTOL, atol=0, err_msg=what)
    assert np.all(np.abs(got - ref)[~sel] <= 1e-270 * np.broadcast_to(big, ref.shape)[~sel]), what


def check(out, r, what="", zero_exact=False):
    """status equal; failed sites NaN in both outputs; origin rows sum to 1 within 1e-12; both outputs close to the reference;
    zero_exact (mutation rate 0): every entry the reference has as 0 is exactly 0.0; origin summed to genotypes and hettx pairs
    summed equal the joint's marginals of child and parents."""
    origin, hettx, st = out
    assert np.array_equal(st, r.status), what
    ok = r.status == 0
    if origin is not None:
        assert np.all(np.isnan(origin[~ok])), what
        np.testing.assert_allclose(origin[ok].sum(axis=-1), 1.0, rtol=1e-12, atol=0, err_msg=what)
        close(origin[ok], r.origin[ok], what)
        if zero_exact:
            assert np.all(origin[ok][r.origin[ok] == 0] == 0.0), what
    if hettx is not None:
        assert np.all(np.isnan(hettx[~ok])), what
        close(hettx[ok], r.hettx[ok], what)
        if zero_exact:
            assert np.all(hettx[ok][r.hettx[ok] == 0] == 0.0), what
    if origin is not None and hettx is not None and ok.any():
        marginals(origin[ok], hettx[ok], r.joint[ok], r.ped, np.asarray(r.flags)[ok], what)


def marginals(origin, hettx, joint, ped, flags, what=""):
    """origin summed to the child's genotypes = the joint's child marginal; hettx's pairs = P(g_m = 1), P(g_f = 1)."""
    mo, _ = ped.relations()
    kids = [p for p in range(ped.n) if mo[p] >= 0]
    J = joint.reshape(joint.shape[0], len(kids), 3, 3, 3)
    for k, c in enumerate(kids):
        pairs = np.stack([hettx[:, k, 0] + hettx[:, k, 1], hettx[:, k, 2] + hettx[:, k, 3]], axis=1)
        close(pairs, np.stack([J[:, k, :, 1, :].sum(axis=(1, 2)), J[:, k, :, :, 1].sum(axis=(1, 2))], axis=1), what)
        child = J[:, k].sum(axis=(2, 3))  # [S, 3]
        son_x = ((flags & 2) != 0) & (ped.genders[c] == 1)
        o = origin[:, k]
        got = np.where(son_x[:, None], np.stack([o[:, 0] + o[:, 1], 0 * o[:, 0], o[:, 2] + o[:, 3]], axis=1),
                       np.stack([o[:, 0], o[:, 1] + o[:, 2], o[:, 3]], axis=1))
        close(got, child, what)
        assert np.all(o[son_x][:, [1, 3]] == 0.0), what
        assert np.all(hettx[:, k][(flags & 2) != 0][:, 2:] == 0.0), what


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
