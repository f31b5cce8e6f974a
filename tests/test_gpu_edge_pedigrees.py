"""The edges of the sum-product generator's decision space on the device: the nine recipes of
famseq_amd/prebuild_sets.py EDGE_PEDIGREES (tests/test_edge_pedigrees.py pins what each of them is).

  edge37 .. edge40   loop-free, around the size edges: relabel's rows leave LDS at 38 members, 39 members are the widest
                     register-resident form (where the variant contest climbs highest), every side source is lean from 40
  loop12 .. loop20   marriage loops above ten members, 1 to 3 conditioned members

Every side product (trio in its three output forms, map, evidence, loo, pattern, sample, af, relabel, mutrate, origin, weight) runs
on every recipe in the variant its contest takes (what a user runs; the plan's variant is printed next to the worst errors, no
level is forced), on tests/_edge.py's batch of 3 x 64 + 5 sites, and is held to
  - the product's own reference through the product's own check (tolerances: that module's, none defined here; tests/_edge.py
    names the route of each, none of which enumerates), status exact, NaN / -1 on the planted sites — for the plain form and
    for the site-prior form under Hardy-Weinberg rows; every site is compared;
  - the site-prior form on the model's own rows: the plain form's bits;
  - weight, relabel (the identity assignment), mutrate (the context's own rate) and pattern: evidence_batch's loglik, bit for bit;
  - 1, 63, 64 and 65 sites: the bits of the slices; trio's forms: the same bits in what they share.
The looped recipes also run the main engines: famseq_bn_batch on the sum-product engine and the fused call path (fp64 rows and
packed PLs in a shuffled column order, as numbers and as text) against tests/_edge.py main_reference — posteriors against
tests/_maxproduct.py's marginals at 1e-9 on every status-0 site, the single posterior bit for bit, the status exact with its
shortcut bit from the documented vote — and, on loop12 and loop13, the lane enumeration kernel against the enumeration oracle.
build() has compiled every code object loaded here: each test asserts that its context's objects lie in the in-tree cache."""
import os

import numpy as np
import pytest

import _edge as ED
import _prior as P
import _side_variants as SV
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets

pytestmark = pytest.mark.gpu

IN_TREE = os.path.join(os.path.dirname(fs.__file__), "lib", "kernels")


@pytest.fixture(autouse=True)
def _ordinary_cache(monkeypatch):
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN"):
        monkeypatch.delenv(key, raising=False)
    yield


def context(c, **options):
    """A device context of the recipe; a looped one (20 members at most) on the sum-product engine, which the wider ones have
    alone."""
    if c.ped.n <= fs.MAXN:
        options.setdefault("engine", fs.ENGINE_ELIM)
    return fs.Context(c.model, device=0, **options)


def in_tree(plan, keys):
    for key in keys:
        obj = plan[key + "_code_object"]
        assert obj.endswith(".hsaco") and os.path.dirname(obj) == IN_TREE, "%s: %r was not pre-built" % (key, obj)


@pytest.mark.parametrize("name", ED.PEDIGREES)
@pytest.mark.parametrize("stem", ED.PRODUCTS)
def test_side_product(stem, name):
    c, p = ED.case(name), ED.PRODUCTS[stem]
    n = len(c.lk)
    ctx = context(c)
    try:
        out = {}
        for form in (3, 1, 2) if p.forms == 3 else (1,):
            what = "%s: %s form %d" % (name, stem, form)
            plain = p.run(ctx, c, n, None, form)
            plan = ctx.plan()
            print("%s: variant %d" % (what, plan[stem + "_variant"]))
            p.check(c, plain, p.cached(c, False), what)
            SV.planted_fills(c, plain, p.fills)
            runs = [(None, plain)]
            if p.has_prior:
                assert SV.same_bits(p.run(ctx, c, n, c.rows, form), plain), what + ": the model's rows"
                hwe = p.run(ctx, c, n, c.hwe, form)
                print("%s, Hardy-Weinberg rows: variant %d" % (what, ctx.plan()[stem + "_prior_variant"]))
                p.check(c, hwe, p.cached(c, True), what + ", Hardy-Weinberg rows")
                SV.planted_fills(c, hwe, p.fills)
                runs.append((c.hwe, hwe))
            for prior, whole in runs:
                for s in ED.SITE_COUNTS:
                    assert SV.same_bits(p.run(ctx, c, s, prior, form), SV.sub(whole, slice(0, s))), (what, s, prior is not None)
            if stem in ED.LOGLIK_TWINS:
                for prior, whole in runs:
                    ev = ctx.evidence_batch(lk=c.lk, flags=c.flags) if prior is None else ctx.evidence_prior_batch(prior, lk=c.lk, flags=c.flags)
                    assert SV.same_bits((whole[1], whole[2]), (ev[0], ev[2])), what + ": loglik is not famseq_evidence's"
                    column = ED.LOGLIK_TWINS[stem]
                    if column is not None:
                        assert SV.same_bits((whole[0][:, column],), (ev[0],)), what + ": column %d is not famseq_evidence's loglik" % column
            if stem == "pattern":
                assert np.all(c.masks[0] == 7) and all(np.all(whole[0][~c.planted, 0] == 1.0) for _, whole in runs), what
            out[form] = [whole for _, whole in runs]
        if p.forms == 3:  # (joint, dnm, status): a form returns only its own outputs, and what two forms share has the same bits
            for k in range(len(out[3])):
                (j3, d3, s3), (j1, d1, s1), (j2, d2, s2) = out[3][k], out[1][k], out[2][k]
                assert j1 is None and d2 is None
                assert SV.same_bits((d1, s1), (d3, s3)) and SV.same_bits((j2, s2), (j3, s3)), (name, k)
        plan = ctx.plan()
        keys = [stem] + ([stem + "_prior"] if p.has_prior else []) + (["evidence", "evidence_prior"] if stem in ED.LOGLIK_TWINS else [])
        in_tree(plan, keys)
        assert all(0 <= plan[key + "_variant"] < sets.SIDE_VARIANTS for key in keys)
    finally:
        ctx.close()


def check_main(out, ref, what):
    """tests/_prior.py check's rules (status and single posterior bit for bit, shortcut rows bit for bit, posteriors at 1e-9 with
    exact zeros exact, failed rows NaN), the worst error printed first."""
    post, single, status = out
    ok = ref[2] == 0
    nz = ok[:, None, None] & (ref[0] > 0)
    print("%s: %d sites (%d status 0, %d shortcut, %d failed), worst relative error of a posterior %.3g" % (
        what, len(status), ok.sum(), (ref[2] == 0x80).sum(), ((ref[2] & 3) != 0).sum(), np.abs(post[nz] / ref[0][nz] - 1.0).max(initial=0)))
    P.check(out, ref[:3], what)


@pytest.mark.parametrize("name", ED.LOOPED)
def test_the_main_engines_on_looped_pedigrees(name):
    c = ED.case(name)
    ref = ED.main_reference(c, c.lk, c.flags)
    assert np.array_equal(ref[2], c.want_status) and np.all(ref[3][~c.planted] >= ED.FLOOR)
    seq, pl, lk2 = ED.call_batch(c)
    ref2 = ED.main_reference(c, lk2, c.flags)
    assert np.all(ref2[3][ref2[2] == 0] >= ED.FLOOR) and (ref2[2] == 0x80).sum() >= 2 and (ref2[2] == 0).sum() > 150
    ctx = context(c)
    try:
        whole = ctx.bn_batch(c.lk, c.flags)
        check_main(whole, ref, "%s: sum-product engine" % name)
        post2, single2, st2 = ctx.bn_batch(lk2, c.flags)
        check_main((post2, single2, st2), ref2, "%s: sum-product engine, the call path's rows" % name)
        # the fused call path (tests/_soak.py's checks): fp64 rows and packed PLs give the same numbers, the status is
        # bn_batch's, FGT is call_genotypes of bn_batch's posteriors, FPP fabs(-10 log10) of them (__graft_entry__.smoke's bar)
        a = ctx.bn_call_batch(seq, lk=lk2, flags=c.flags)
        b = ctx.bn_call_batch(seq, pl16=pl, flags=c.flags)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), name
        assert np.array_equal(a[3], st2), name
        okc = (st2 & 3) == 0
        assert np.array_equal(a[2][okc], fs.call_genotypes(post2[okc][:, seq]).reshape(-1, len(seq))), name
        with np.errstate(divide="ignore"):
            want = np.abs(-10 * np.log10(post2[okc][:, seq]))
        want[np.isinf(want)] = 99999.0
        np.testing.assert_allclose(a[1][okc], want, rtol=1e-9, atol=1e-9, err_msg=name)
        # ... and as text: Python's '%g' of the numbers, every computed site and column
        text, st3 = ctx.bn_call_text_batch(seq, pl16=pl, flags=c.flags)
        assert np.array_equal(st3, st2), name
        for s in np.nonzero(okc)[0]:
            for j in range(len(seq)):
                rec = text[s, j]
                want = "%g,%g,%g:%g,%g,%g:%s\t" % (tuple(a[0][s, j]) + tuple(a[1][s, j]) + ({0: "0/0", 1: "0/1"}.get(int(a[2][s, j]), "1/1"),))
                assert bytes(rec[:rec[-1]]) == want.encode(), (name, s, j)
        plan = ctx.plan()
        objects = {k: v for k, v in plan.items() if k.endswith("_code_object") and v}
        assert any(k.startswith("elim") for k in objects), sorted(objects)
        for k, v in objects.items():
            assert v.endswith(".hsaco") and os.path.dirname(v) == IN_TREE, "%s: %r was not pre-built" % (k, v)
        print("%s: %s" % (name, ", ".join("%s %s" % (k, plan[k]) for k in sorted(plan) if k.endswith("_variant") and plan[k] not in (-1, ""))))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", [n for n in ED.LOOPED if sets.EDGE_PEDIGREES[n][1] <= sets.EDGE_LANE_MAX])
def test_the_lane_kernel_against_the_enumeration_oracle(name):
    import oracle

    c = ED.case(name)
    ped = c.ped
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=c.mrate).bn_batch(c.lk, c.flags, threads=8)
    assert np.array_equal(ref[2], c.want_status)
    ctx = fs.Context(c.model, device=0, enum_impl=1)
    try:
        whole = ctx.bn_batch(c.lk, c.flags)
        check_main(whole, ref, "%s: lane kernel" % name)
        plan = ctx.plan()
        in_tree(plan, ["enum_lane"])
        print("%s: lane variant %d, %s" % (name, plan["enum_lane_variant"], plan["enum_lane_shape"]))
    finally:
        ctx.close()
