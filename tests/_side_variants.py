"""Shared by the side products' variant matrix (tests/test_gpu_side_variants.py on the device, tests/test_side_variants_host.py
on the CPU): the three pedigrees of famseq_amd.prebuild_sets.SIDE_VARIANT_PEDIGREES, one batch per pedigree, and per side
product how it is run and how its existing reference and its existing `check` are applied to that batch.  No tolerance is
defined here: every comparison is the product's own (test_evidence_host, tests/_loo.py, test_pattern_host, test_relabel_host,
tests/_af.py with test_af_host, test_trio_host, test_gpu_map, test_sample_host; tests/_prior_joint.py under Hardy-Weinberg rows).

The batch of a pedigree: 3 BT + 5 sites (one workgroup, grid_blocks 1, makes four trips of its loop, the last partial),
test_map_host.clear_likelihoods' rows with the rows of unsequenced members at 1.0, flags 0..3 in turn, one planted status-1 site
(an all-zero row of a sequenced member) and, at mutation rate 0 (cousins), one planted status-2 site (tests/_variants.py's
construction: mother certain 0/0, child certain 1/1).  Every other site is asserted, on the references alone, to have status 0,
a total weight of at least 1e-200 and — through each product's own clear / is_clear rule — partial weights that are 0 or at
least that; no site is left out of a comparison."""
import os

import numpy as np

import _af as A
import _loo as L
import _prior as P
import _prior_joint as J
import famseq_amd as fs
import test_af_host as AF
import test_evidence_host as E
import test_pattern_host as PT
import test_relabel_host as R
import test_sample_host as S
import test_trio_host as T
from famseq_amd import prebuild_sets as sets
from test_gpu_map import check_against_enumeration
from test_map_host import brute_weights, clear_likelihoods

# name -> (mutation rate, conditioned members)
PEDIGREES = {"trio": (1e-7, 0), "cousins": (0.0, 1), "random15": (1e-4, 3)}
assert tuple(PEDIGREES) == sets.SIDE_VARIANT_PEDIGREES
N_VARIANTS = sets.SIDE_VARIANTS
FLOOR = 1e-200
SINGLE_FAIL, BN_FAIL = 6, 9  # the planted sites
N_DRAWS, SAMPLE_SEED = 3, 20261020
AF_STEPS = 3
SEEDS = {"trio": 3, "cousins": 9, "random15": 15}


class Case:
    """ped, mrate, bt, lk, flags, status (the enumeration's), planted (bool mask), hwe, masks, assign, af0; refs (a cache)."""


_CASES = {}


def case(name):
    if name not in _CASES:
        c = Case()
        c.name, (c.mrate, c.conditioned) = name, PEDIGREES[name]
        c.ped = ped = sets.side_variant_pedigree(name)
        ctx = fs.Context(fs.make_model(ped, mrate=c.mrate), device=-1)
        plan = ctx.plan()
        ctx.close()
        c.bt = plan["evidence_block_threads"]
        assert plan["loo_block_threads"] == c.bt and c.bt >= 2
        assert plan["elim_conditioned_members"] == c.conditioned
        rng = np.random.RandomState(SEEDS[name])
        n = 3 * c.bt + 5
        c.lk, _ = clear_likelihoods(rng, ped, n)
        seq = np.nonzero(ped.sequenced)[0]
        c.lk[:, ped.sequenced == 0, :] = 1.0
        c.flags = (np.arange(n) % 4).astype(np.uint8)
        c.planted = np.zeros(n, bool)
        c.lk[SINGLE_FAIL, seq[-1]] = 0.0
        c.planted[SINGLE_FAIL] = True
        c.want_status = np.zeros(n, np.uint8)
        c.want_status[SINGLE_FAIL] = 1
        if c.mrate == 0.0:
            mo, _ = ped.relations()
            child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]][0]
            c.lk[BN_FAIL, mo[child]] = [1.0, 0.0, 0.0]
            c.lk[BN_FAIL, child] = [0.0, 0.0, 1.0]
            c.planted[BN_FAIL] = True
            c.want_status[BN_FAIL] = 2
        c.hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, n))
        c.masks = PT.batch_masks(rng, ped)
        c.assign = R.batch_assign(rng, ped.n)
        c.af0 = rng.uniform(0.01, 0.9, n)  # (test_gpu_af.py's start values)
        c.model = fs.make_model(ped, mrate=c.mrate)
        c.rows = P.model_rows(c.model, c.flags)
        c.brute = brute_weights(ped, c.mrate, c.lk, c.flags)
        c.refs = {}
        # the planted sites are the only ones that fail, and every other site's total weight is at least 1e-200
        G, W, st = c.brute
        assert np.array_equal(st, c.want_status), name
        assert np.all(W[~c.planted].sum(axis=1) >= FLOOR), name
        _CASES[name] = c
    return _CASES[name]


def sub(out, index):
    return tuple(None if x is None else x[index] for x in out)


def same_bits(a, b):
    """Two outputs of one product: bit-identical (NaN patterns included), None where either is."""
    return all((x is None and y is None) or (x is not None and y is not None and x.shape == y.shape and
               np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))) for x, y in zip(a, b))


def planted_fills(c, out, fills):
    """status exact on every site, and on the planted ones the product's fill (NaN, -1)."""
    assert np.array_equal(out[-1], c.want_status), c.name
    for x, fill in zip(out[:-1], fills):
        if x is None:
            continue
        bad = x[c.planted]
        assert np.all(np.isnan(bad)) if fill != fill else np.all(bad == fill), c.name


class Product:
    """One side product: stem, forms, has_prior; run(ctx, c, n, prior, form) -> outputs with the status last; reference(c, hwe)
    -> its reference on the whole batch, asserted clear on the unplanted sites; check(c, out, ref, hwe)."""
    forms, has_prior, fills = 1, True, (np.nan, np.nan)

    def cached(self, c, hwe):
        key = (self.stem, hwe)
        if key not in c.refs:
            c.refs[key] = self.reference(c, c.hwe if hwe else None)
        return c.refs[key]


class Evidence(Product):
    stem = "evidence"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.evidence_batch(lk=c.lk[:n], flags=c.flags[:n])
        return ctx.evidence_prior_batch(prior[:n], lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        ref = E.reference(c.ped, c.mrate, c.lk, c.flags) if hwe is None else E.prior_reference(c.ped, c.mrate, c.lk, c.flags, hwe)
        z, w0, st = sub(ref, ~c.planted)
        assert np.all(st == 0) and np.all(z >= E.FLOOR) and np.all(w0 >= E.FLOOR) and np.array_equal(ref[2], c.want_status), c.name
        return ref

    def check(self, c, out, ref, what):
        E.check(sub(out, ~c.planted), sub(ref, ~c.planted), what, clear=True)
        E.check(out, ref, what + ", planted sites included", clear=False)


class Loo(Product):
    stem = "loo"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.loo_batch(lk=c.lk[:n], flags=c.flags[:n])
        return ctx.loo_prior_batch(prior[:n], lk=c.lk[:n], flags=c.flags[:n])

    @staticmethod
    def take(r, index):
        t = L.Loo()
        for k in ("loo", "fit", "status", "z", "zc"):
            setattr(t, k, getattr(r, k)[index])
        return t

    def reference(self, c, hwe):
        r = L.analyse(c.ped, c.mrate, c.lk, c.flags, hwe)
        assert L.is_clear(self.take(r, ~c.planted)) and np.array_equal(r.status, c.want_status), c.name
        return r

    def check(self, c, out, ref, what):
        L.check(sub(out, ~c.planted), self.take(ref, ~c.planted), what, clear=True)
        L.check(out, ref, what + ", planted sites included", clear=False)


class Pattern(Product):
    stem = "pattern"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.pattern_batch(c.masks, lk=c.lk[:n], flags=c.flags[:n])
        return ctx.pattern_prior_batch(prior[:n], c.masks, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        ref = PT.reference(c.ped, c.mrate, c.lk, c.flags, c.masks, hwe)
        z, zm, st = sub(ref, ~c.planted)
        assert np.all(st == 0) and np.all(z >= PT.FLOOR) and np.all((zm == 0) | (zm >= PT.FLOOR)), c.name
        assert np.array_equal(ref[2], c.want_status), c.name
        return ref

    def check(self, c, out, ref, what):
        PT.check(sub(out, ~c.planted), sub(ref, ~c.planted), c.masks, what, clear=True)
        PT.check(out, ref, c.masks, what + ", planted sites included", clear=False)


class Relabel(Product):
    stem = "relabel"

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.relabel_batch(c.assign, lk=c.lk[:n], flags=c.flags[:n])
        return ctx.relabel_prior_batch(prior[:n], c.assign, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        ref = R.reference(c.ped, c.mrate, c.lk, c.flags, c.assign, hwe)
        R.clear(sub(ref, ~c.planted), c.name)
        assert np.array_equal(ref[2], c.want_status), c.name
        return ref

    def check(self, c, out, ref, what):
        R.check(out, ref, what)


class Af(Product):
    stem, has_prior = "af", False

    def run(self, ctx, c, n, prior=None, form=1):
        return ctx.af_batch(c.af0[:n], AF_STEPS, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        good = ~c.planted  # (tests/_af.py asserts status 0 and every Z(q_t) >= 1e-200 on what it is given)
        return A.reference(c.ped, c.mrate, c.lk[good], c.flags[good], c.af0[good], AF_STEPS)

    def check(self, c, out, ref, what):
        AF.check(sub(out, ~c.planted), ref, AF_STEPS, what)


class Map(Product):
    stem, fills = "map", (-1, np.nan)

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.map_batch(lk=c.lk[:n], flags=c.flags[:n])
        return ctx.map_prior_batch(prior[:n], lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        if hwe is None:
            return None  # (the enumeration of the case, checked clear there)
        r = J.analyse(c.ped, c.lk, c.flags, hwe, c.mrate)
        assert np.array_equal(r.map_status, c.want_status) and np.all(r.z[~c.planted] >= FLOOR), c.name
        return r

    def check(self, c, out, ref, what):
        if ref is None:
            # the arg-max itself where the enumeration has no runner-up within 1e-6 (clear_likelihoods: every member sequenced);
            # a member without reads has exact ties by symmetry (random15: half its sites), and there the criterion is the one
            # that defines a MAP, the returned configuration's weight within 1e-9 of the maximum (test_map_host.py, "Ties")
            check_against_enumeration(c.ped, c.mrate, c.lk, c.flags, *out, exact=bool(np.all(c.ped.sequenced)))
        else:
            assert J.check_map(out, ref, what) == int((~c.planted).sum()), what


class Sample(Product):
    stem, fills = "sample", (-1, np.nan)

    def run(self, ctx, c, n, prior=None, form=1):
        if prior is None:
            return ctx.sample_batch(N_DRAWS, seed=SAMPLE_SEED, lk=c.lk[:n], flags=c.flags[:n])
        return ctx.sample_prior_batch(prior[:n], N_DRAWS, seed=SAMPLE_SEED, lk=c.lk[:n], flags=c.flags[:n])

    def reference(self, c, hwe):
        if hwe is None:
            return c.brute
        G, W, st = S.prior_weights(c.ped, c.mrate, c.lk, c.flags, hwe)
        assert np.array_equal(st, c.want_status) and np.all(W[~c.planted].sum(axis=1) >= FLOOR), c.name
        return G, W, st

    def check(self, c, out, ref, what):
        # every draw's samp_post against w(drawn configuration) / Z (test_sample_host.check_draws: rtol 1e-9)
        S.check_draws(c.ped, c.mrate, c.flags, out, *ref)


class Trio(Product):
    stem, forms = "trio", 3

    def run(self, ctx, c, n, prior=None, form=3):
        want = dict(want_dnm=bool(form & 1), want_joint=bool(form & 2))
        if prior is None:
            return ctx.trio_batch(lk=c.lk[:n], flags=c.flags[:n], **want)[1:]
        return ctx.trio_prior_batch(prior[:n], lk=c.lk[:n], flags=c.flags[:n], **want)[1:]

    def reference(self, c, hwe):
        if hwe is None:
            joint, st = T.brute_joint(c.ped, c.mrate, c.lk, c.flags)
            assert np.array_equal(st, c.want_status), c.name
            return joint
        r = J.analyse(c.ped, c.lk, c.flags, hwe, c.mrate)
        assert np.array_equal(r.trio_status, c.want_status) and np.all(r.z[~c.planted] >= FLOOR), c.name
        return r

    def check(self, c, out, ref, what):
        joint, dnm, st = out
        ok = ~c.planted
        if isinstance(ref, J.Reference):
            J.check_trio(out, ref, what)
        else:
            if joint is not None:
                T.check_joint(joint[ok], ref[ok])
            if dnm is not None:
                T.check_dnm(dnm[ok], ref[ok], J.children_of(c.ped), c.ped.genders, c.flags[ok])
        if dnm is not None and c.mrate == 0.0:
            assert np.all(dnm[ok] == 0.0), what  # no mutation: exactly none


PRODUCTS = {p.stem: p for p in (Trio(), Map(), Evidence(), Loo(), Pattern(), Sample(), Af(), Relabel())}
assert [(p.stem, p.forms, p.has_prior) for p in PRODUCTS.values()] == [tuple(x) for x in sets.SIDE_PRODUCTS]


def references_are_clear(name):
    """Every product's references of the pedigree's batch, each asserted clear where it is made: the CPU half of the matrix."""
    c = case(name)
    for p in PRODUCTS.values():
        p.cached(c, False)
        if p.has_prior:
            p.cached(c, True)
    return c


def forced(ctx, key, form, v, monkeypatch):
    """set_option("<key>_kernels", form) under $FAMSEQ_VARIANT_ONLY = v, the variable gone again afterwards; the plan names v."""
    monkeypatch.setenv("FAMSEQ_VARIANT_ONLY", str(v))
    try:
        ctx.set_option(key + "_kernels", form)
    finally:
        monkeypatch.delenv("FAMSEQ_VARIANT_ONLY")
    plan = ctx.plan()
    assert plan[key + "_variant"] == v and plan[key + "_code_object"].endswith(".hsaco"), (key, form, v, plan[key + "_variant"])
    return plan[key + "_code_object"]


def pick_notes(directory):
    return sorted(f for f in os.listdir(directory) if f.endswith(".pick")) if os.path.isdir(directory) else []
