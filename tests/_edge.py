"""Shared by the edge-pedigree tests (tests/test_edge_pedigrees.py on the CPU, tests/test_gpu_edge_pedigrees.py on the device):
the nine recipes of famseq_amd.prebuild_sets.EDGE_PEDIGREES, one batch per recipe, and per side product how it is run and how its
existing reference and its existing `check` are applied to that batch.  No tolerance is defined here: every comparison is the
product's own (see tests/_side_variants.py, whose Product classes serve here wherever they do not enumerate).

The batch of a recipe is tests/_side_variants.py's: 3 x 64 + 5 sites, test_map_host.clear_likelihoods' rows with the rows of
unsequenced members at 1.0, flags 0..3 in turn, one planted status-1 site and, at model rate 0, tests/_variants.py's planted
status-2 site.  Every other site is asserted, on the references alone, to have status 0, a total weight of at least 1e-200 and
partial weights that are 0 or at least that; no site is left out of a comparison.

The references are the routes the host tests take at 24 members or more, none of which enumerates 3^N:
  evidence, loo, pattern, relabel   tests/_side_variants.py's classes as they are (test_evidence_host.reference, tests/_loo.py,
                                    test_pattern_host.reference and test_relabel_host.reference take the elimination above ten)
  af                                tests/_af.py with the founders' rows from the elimination (oracle_upto)
  map, sample, trio, origin         tests/_prior_joint.py's elimination, whose factors under the model's own rows
                                    (tests/_prior.py model_rows) are tests/_maxproduct.py's: J.check_map, J.check_trio,
                                    test_sample_host's rule for a draw (samp_post = w(drawn) / Z at 1e-9, the drawn
                                    configuration Mendelian at rate 0), tests/_origin.py's split of the joint
  mutrate, weight                   test_mutrate_host.reference and tests/_weight.py's with brute=False
tests/test_edge_pedigrees.py holds the elimination against the 3^N enumeration on loop12 and loop13."""
import numpy as np

import _af as A
import _maxproduct as mp
import _origin as O
import _prior as P
import _prior_joint as J
import _side_variants as SV
import _weight as W
import famseq_amd as fs
import test_mutrate_host as M
import test_pattern_host as PT
import test_relabel_host as R
from famseq_amd import prebuild_sets as sets
from test_map_host import clear_likelihoods

PEDIGREES = tuple(sets.EDGE_PEDIGREES)
LOOPED = tuple(n for n in PEDIGREES if sets.EDGE_PEDIGREES[n][2])
BT = 64
N_SITES = 3 * BT + 5
SITE_COUNTS = (1, BT - 1, BT, BT + 1)
FLOOR = SV.FLOOR
SINGLE_FAIL, BN_FAIL = SV.SINGLE_FAIL, SV.BN_FAIL
N_DRAWS, SAMPLE_SEED = SV.N_DRAWS, SV.SAMPLE_SEED
AF_STEPS = 2


class Case:
    """name, ped, mrate, conditioned, model, lk, flags, planted (bool mask), want_status, hwe, rows (the model's own), masks,
    assign, af0, rates, weights; refs (a cache)."""


_CASES = {}


def case(name):
    if name not in _CASES:
        c = Case()
        c.name = name
        seed, n, loops, c.n_sequenced, c.conditioned, c.mrate = sets.EDGE_PEDIGREES[name]
        c.ped = ped = sets.edge_pedigree(name)
        c.model = fs.make_model(ped, mrate=c.mrate)
        c.bt = BT
        rng = np.random.RandomState(seed)
        c.lk, _ = clear_likelihoods(rng, ped, N_SITES)
        seq = np.nonzero(ped.sequenced)[0]
        c.lk[:, ped.sequenced == 0, :] = 1.0
        c.flags = (np.arange(N_SITES) % 4).astype(np.uint8)
        c.planted = np.zeros(N_SITES, bool)
        c.want_status = np.zeros(N_SITES, np.uint8)
        c.lk[SINGLE_FAIL, seq[-1]] = 0.0
        c.planted[SINGLE_FAIL], c.want_status[SINGLE_FAIL] = True, 1
        if c.mrate == 0.0:  # tests/_variants.py's construction: mother certain 0/0, child certain 1/1
            mo, _ = ped.relations()
            child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]][0]
            c.lk[BN_FAIL, mo[child]] = [1.0, 0.0, 0.0]
            c.lk[BN_FAIL, child] = [0.0, 0.0, 1.0]
            c.planted[BN_FAIL], c.want_status[BN_FAIL] = True, 2
        c.planted_sites = [int(s) for s in np.nonzero(c.planted)[0]]
        c.hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, N_SITES))
        c.rows = P.model_rows(c.model, c.flags)
        c.masks = PT.batch_masks(rng, ped)
        c.assign = R.batch_assign(rng, ped.n)
        c.af0 = rng.uniform(0.01, 0.9, N_SITES)
        c.rates = M.grid(c.mrate)
        dead = np.ones((1, ped.n, 3))
        dead[0, ped.n // 2] = 0.0  # a member without any weight: -inf at every good site
        c.weights = np.concatenate([W.batch_weights(ped), dead])
        c.refs = {}
        _CASES[name] = c
    return _CASES[name]


def joint(c, hwe):
    """tests/_prior_joint.py's analysis of the batch under the model's own rows (hwe False) or the Hardy-Weinberg rows, shared by
    map, sample, trio and origin: both statuses are the planted ones and every other site's total weight is at least 1e-200."""
    key = ("joint", hwe)
    if key not in c.refs:
        r = J.analyse(c.ped, c.lk, c.flags, c.hwe if hwe else c.rows, c.mrate)
        assert np.array_equal(r.map_status, c.want_status) and np.array_equal(r.trio_status, c.want_status), c.name
        assert np.all(r.z[~c.planted] >= FLOOR) and np.all(r.wmax[~c.planted] >= FLOOR), c.name
        c.refs[key] = r
    return c.refs[key]


class Product(SV.Product):
    """reference(c, hwe: bool), where tests/_side_variants.py's own products are handed the rows or None."""

    def cached(self, c, hwe):
        key = (self.stem, hwe)
        if key not in c.refs:
            c.refs[key] = self.reference(c, hwe)
        return c.refs[key]


class Af(SV.Af):
    def run(self, ctx, c, n, prior=None, form=1):
        return ctx.af_batch(c.af0[:n], AF_STEPS, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        good = ~c.planted  # (tests/_af.py asserts status 0 and every Z(q_t) >= 1e-200 on what it is given)
        return A.reference(c.ped, c.mrate, c.lk[good], c.flags[good], c.af0[good], AF_STEPS, oracle_upto=10)

    def check(self, c, out, ref, what):
        SV.AF.check(SV.sub(out, ~c.planted), ref, AF_STEPS, what)


class Map(Product):
    stem, fills = "map", (-1, np.nan)
    run = SV.Map.run

    def reference(self, c, hwe):
        return joint(c, hwe)

    def check(self, c, out, ref, what):
        ok = ~c.planted
        w_ret = J.config_weight(ref.take(ok), out[0][ok])
        print("%s: %d sites, worst w_returned / w_max %.17g, worst map_post relative error %.3g" % (
            what, ok.sum(), (w_ret / ref.wmax[ok]).min(), np.abs(out[1][ok] / (w_ret / ref.z[ok]) - 1.0).max()))
        assert J.check_map(out, ref, what) == int(ok.sum()), what


class Sample(Product):
    stem, fills = "sample", (-1, np.nan)
    run = SV.Sample.run

    def reference(self, c, hwe):
        return joint(c, hwe)

    def check(self, c, out, ref, what):
        """test_sample_host's rule for a draw beyond the enumeration's reach: every drawn configuration has weight, samp_post is
        that weight over Z at 1e-9, and at rate 0 it is Mendelian."""
        gt, post, st = out
        ok = ~c.planted
        assert np.array_equal(st, c.want_status), what
        assert np.all(gt[~ok] == -1) and np.all(np.isnan(post[~ok])), what
        assert np.all((gt[ok] >= 0) & (gt[ok] <= 2)) and gt.shape[1:] == (N_DRAWS, c.ped.n), what
        sub, worst = ref.take(ok), 0.0
        for d in range(N_DRAWS):
            w = J.config_weight(sub, gt[ok][:, d])
            assert np.all(w > 0), what
            worst = max(worst, float(np.abs(post[ok][:, d] / (w / sub.z) - 1.0).max()))
        print("%s: %d sites x %d draws, worst samp_post relative error %.3g" % (what, ok.sum(), N_DRAWS, worst))
        for d in range(N_DRAWS):
            np.testing.assert_allclose(post[ok][:, d], J.config_weight(sub, gt[ok][:, d]) / sub.z, rtol=J.RTOL, atol=0, err_msg=what)
            if c.mrate == 0.0:
                assert np.all(mp.mendelian_consistent(c.ped, gt[ok][:, d], c.flags[ok])), what


def _worst(got, want):
    """The largest relative error over the entries the reference has above 1e-280 x its row's maximum (information)."""
    sel = want >= 1e-280 * np.nanmax(want, axis=-1, keepdims=True)
    sel &= want > 0
    return float(np.abs(got[sel] / want[sel] - 1.0).max(initial=0))


class Trio(Product):
    stem, forms = "trio", 3
    run = SV.Trio.run

    def reference(self, c, hwe):
        return joint(c, hwe)

    def check(self, c, out, ref, what):
        jnt, dnm, st = out
        ok = ~c.planted
        print("%s: %d sites x %d children, worst joint relative error %.3g, worst dnm relative error %.3g" % (
            what, ok.sum(), ref.joint.shape[1], -1 if jnt is None else _worst(jnt[ok], ref.joint[ok]),
            -1 if dnm is None else _worst(dnm[ok], ref.dnm[ok])))
        J.check_trio(out, ref, what)
        if dnm is not None and c.mrate == 0.0:
            assert np.all(dnm[ok] == 0.0), what  # no mutation: exactly none


class Origin(Product):
    stem = "origin"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.origin_batch(lk=c.lk[:n], flags=c.flags[:n])
        return ctx.origin_prior_batch(prior[:n], lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        r = joint(c, hwe)
        return O.reference(c.ped, c.mrate, c.lk, c.flags, joint=r.joint, status=r.trio_status)

    def check(self, c, out, ref, what):
        ok = ~c.planted
        print("%s: %d sites, worst origin relative error %.3g, worst hettx relative error %.3g" % (
            what, ok.sum(), _worst(out[0][ok], ref.origin[ok]), _worst(out[1][ok], ref.hettx[ok])))
        O.check(out, ref, what, zero_exact=c.mrate == 0.0)


class Mutrate(Product):
    stem = "mutrate"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.mutrate_batch(c.rates, lk=c.lk[:n], flags=c.flags[:n])
        return ctx.mutrate_prior_batch(prior[:n], c.rates, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        ref = M.reference(c.ped, c.mrate, c.lk, c.flags, c.rates, c.hwe if hwe else None, brute=False)
        M.clear(ref, c.name, c.planted_sites)
        assert np.array_equal(ref[2], c.want_status), c.name
        return ref

    def check(self, c, out, ref, what):
        M.check(out, ref, what)


class Weight(Product):
    stem = "weight"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.weight_batch(c.weights, lk=c.lk[:n], flags=c.flags[:n])
        return ctx.weight_prior_batch(prior[:n], c.weights, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        ref = W.reference(c.ped, c.mrate, c.lk, c.flags, c.weights, c.hwe if hwe else None, brute=False)
        W.clear(ref, c.name, c.planted_sites)
        assert np.array_equal(ref[2], c.want_status), c.name
        return ref

    def check(self, c, out, ref, what):
        W.check(out, ref, what)


PRODUCTS = {p.stem: p for p in (Trio(), Map(), SV.PRODUCTS["evidence"], SV.PRODUCTS["loo"], SV.PRODUCTS["pattern"], Sample(), Af(),
                                SV.PRODUCTS["relabel"], Mutrate(), Origin(), Weight())}
assert [(p.stem, p.forms, p.has_prior) for p in PRODUCTS.values()] == [tuple(x) for x in sets.SIDE_PRODUCTS + sets.SIDE_PRODUCTS_SINCE]
# the products whose loglik output is famseq_evidence's, bit for bit, and the column of the batch that is loglik again
# (relabel: the identity assignment; mutrate: the context's own rate; pattern's all-7 row is a posterior, exactly 1.0)
LOGLIK_TWINS = {"weight": None, "relabel": 0, "mutrate": 3, "pattern": None}


def references_are_clear(name):
    """Every product's references of the recipe's batch, each asserted clear where it is made: the CPU half."""
    c = case(name)
    for p in PRODUCTS.values():
        p.cached(c, False)
        if p.has_prior:
            p.cached(c, True)
    return c


def main_reference(c, lk, flags, lc=1.0):
    """-> (post, single, status, z) of famseq_bn_batch on a looped recipe, without an enumeration: the single posterior and the
    -LRC vote by the statements of oracle/sum_product.py (prior x likelihood over (s0 + s1) + s2; a site takes the shortcut when
    no sequenced member's largest likelihood over its row sum is below lc), status 1 where a member's single posterior has no
    mass, else 0x80 where the vote says so, else 2 where the network's total weight is 0; post is tests/_maxproduct.py's
    marginals where status is 0, the single posterior where it is 0x80, NaN elsewhere."""
    ped = c.ped
    gender = np.asarray(ped.genders)
    fl = np.asarray(flags)
    known, chrx = (fl & 1) != 0, (fl & 2) != 0
    autos = np.where(known[:, None], np.array(mp.GK), np.array(mp.GN))
    male = np.where(chrx[:, None], np.where(known[:, None], np.array(mp.GXK), np.array(mp.GXN)), autos)
    prior = np.where((gender == 1)[None, :, None], male[:, None, :], autos[:, None, :])  # [S, N, 3]
    sp = lk * prior
    ssum = (sp[:, :, 0] + sp[:, :, 1]) + sp[:, :, 2]
    s_fail = (ssum <= 0).any(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        single = sp / ssum[:, :, None]
        big = lk.max(axis=2) / ((lk[:, :, 0] + lk[:, :, 1]) + lk[:, :, 2])
    full = ((big < lc) & (np.asarray(ped.sequenced) != 0)[None]).any(axis=1)
    z, fail = PT._total(ped, c.mrate, lk, flags, None)
    assert np.array_equal(fail, s_fail)
    status = np.where(s_fail, 1, np.where(~full, 0x80, np.where(~(z > 0), 2, 0))).astype(np.uint8)
    post = np.full(lk.shape, np.nan)
    ok = status == 0
    post[ok] = mp.marginals(ped, c.mrate, lk[ok], fl[ok])
    post[status == 0x80] = single[status == 0x80]
    single[s_fail] = np.nan
    return post, single, status, z


def call_batch(c):
    """tests/_soak.py's construction for the fused call path, on the recipe's sites: packed integer PLs in a shuffled column
    order, one genotype at PL 0, 5 % of the samples missing, 1 % of the entries beyond the table (a likelihood of 0), and two
    planted shortcut sites (every sample sharp: PL 0 / 200 / 250).  PLs below 100: twenty members that each contradict their
    parents keep the total weight above 1e-200, which the caller asserts.  -> (seq, pl16, lk the library's table gives)."""
    import math

    ped, n_sites = c.ped, N_SITES
    rng = np.random.RandomState(sets.EDGE_PEDIGREES[c.name][0] + 1)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)
    rng.shuffle(seq)
    k = len(seq)
    pl = rng.randint(0, 100, size=(n_sites, k, 3)).astype(np.uint16)
    pl[np.arange(n_sites)[:, None], np.arange(k)[None, :], rng.randint(0, 3, size=(n_sites, k))] = 0
    pl[rng.rand(n_sites, k) < 0.05] = fs.PL_MISSING
    pl[rng.rand(n_sites, k, 3) < 0.01] = 5000
    for s, g in ((70, 0), (133, 2)):
        pl[s] = np.roll([0, 200, 250], g)
    table = np.zeros(4097)
    table[:4096] = [math.pow(10.0, -i / 10.0) for i in range(4096)]
    lk = np.ones((n_sites, ped.n, 3))
    for j, mbr in enumerate(seq):
        v = table[np.minimum(pl[:, j].astype(np.int64), 4096)]
        v[np.all(pl[:, j] == fs.PL_MISSING, axis=1)] = 1.0
        lk[:, mbr] = v
    return seq, pl, lk
