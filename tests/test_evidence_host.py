"""The evidence kernel's arithmetic (famseq_evidence / famseq_evidence_prior: log10 of the site's likelihood under the pedigree
and the posterior probability that every member is hom-ref), checked without a GPU.

As in test_map_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++.  References: the 3^N enumeration of test_map_host.brute_weights up to ten members, tests/_maxproduct.py beyond, and
tests/_prior_joint.py under per-site priors.  Wanted: loglik = log10(z) - 7 and pref = w0 / z, with z the total weight and
w0 = w(0, ..., 0), both with the reference's 1e7.

Tolerances (derived, not measured): pref at the project's rtol 1e-9; loglik at an ABSOLUTE 1e-9 — a relative 1e-9 on z is
4.3e-10 in log10, and the logarithm's own few ulp on values of magnitude <= 130 add about 1e-13; status exact; the site-prior
form fed the model's rows bit-identical to the plain form.  No site is left out of a comparison: on the clear batches used here
(every member sequenced, PLs uniform in [0, 30)) every reference has status 0 and z, w0 >= 1e-200, which each test asserts.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _maxproduct as mp
import _prior as P
import _prior_joint as J
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from test_generated_host import factor_tables, host_source, misaligned
from test_map_host import brute_weights, clear_likelihoods

RTOL = 1e-9    # pref: the project's bar for posteriors
LL_ATOL = 1e-9  # loglik: absolute (see the module's docstring)
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kEvidenceVariants
FLOOR = 1e-200


def build_evidence_host(model, where, variant=None, prior=False):
    """Generate famseq_evidence (prior: famseq_evidence_prior) for a one-lane workgroup on a plan-only context, compile it for
    the host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("evidence_prior", "famseq_evidence_prior") if prior else ("evidence", "famseq_evidence")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option(key + "_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    src = open(plan[key + "_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and (entry + "(") in src
    assert ("founder priors per site" in src.splitlines()[0]) == prior
    assert variant is None or plan[key + "_variant"] == variant
    tag = key + ("" if variant is None else "_%d" % variant)
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), entry)
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def run_evidence(fn, model, lk, flags, prior=None, want=(True, True, True), misalign_prior=False):
    s = lk.shape[0]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    ll, p0, st = np.full(s, -5.0), np.full(s, -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, ll.ctypes.data if want[0] else None, p0.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0]
    if prior is not None:
        if misalign_prior:
            pr = misaligned(prior.shape)
        else:
            raw = np.zeros(prior.size + 2)
            pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
            assert pr.ctypes.data % 16 == 0
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return ll, p0, st


def cycled(lk):
    """Flags 0..3 in turn."""
    return (np.arange(len(lk)) % 4).astype(np.uint8)


def reference(ped, mrate, lk, flags):
    """-> (z, w0, status) of the model's own priors: the enumeration up to ten members, the bucket elimination beyond."""
    if ped.n <= 10:
        _, W, st = brute_weights(ped, mrate, lk, flags)
        return W.sum(axis=1), W[:, 0], st  # (configuration 0 is every member at genotype 0)
    _, _, z, _ = mp.max_product(ped, mrate, lk, flags)
    _, fail = mp.site_factors(ped, mrate, lk, flags)
    st = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    return z, mp.config_weight(ped, mrate, lk, flags, np.zeros((len(lk), ped.n), np.int64)), st


def prior_reference(ped, mrate, lk, flags, prior):
    r = J.analyse(ped, lk, flags, prior, mrate)
    st = np.where(r.map_status == 1, 1, np.where(~((r.z > 0) & np.isfinite(r.z)), 2, 0)).astype(np.uint8)
    return r.z, J.config_weight(r, np.zeros((len(lk), ped.n), np.int64)), st


def check(out, ref, what="", clear=True):
    """status exact, loglik at LL_ATOL absolute, pref at RTOL, failed sites NaN.  clear: the reference has status 0 and z, w0 >=
    1e-200 on every site, and every site is compared."""
    ll, p0, st = out
    z, w0, ref_st = ref
    if clear:
        assert np.all(ref_st == 0) and np.all(z >= FLOOR) and np.all(w0 >= FLOOR), what
    assert np.array_equal(st, ref_st), what
    ok = ref_st == 0
    assert np.all(np.isnan(ll[~ok])) and np.all(np.isnan(p0[~ok])), what
    err = np.abs(ll[ok] - (np.log10(z[ok]) - 7.0))
    rel = np.abs(p0[ok] / (w0[ok] / z[ok]) - 1.0) if clear else np.zeros(1)
    print("%s: %d sites, worst |loglik error| %.3g, worst pref relative error %.3g" % (what, ok.sum(), err.max(initial=0), rel.max()))
    np.testing.assert_allclose(ll[ok], np.log10(z[ok]) - 7.0, rtol=0, atol=LL_ATOL, err_msg=what)
    np.testing.assert_allclose(p0[ok], w0[ok] / z[ok], rtol=RTOL, atol=0, err_msg=what)


def bits(out):
    return [np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint8) for x in out]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def conditioned(ped):
    ctx = fs.Context(fs.make_model(ped), device=-1)
    k = ctx.plan()["elim_conditioned_members"]
    ctx.close()
    return k


def random_of(loops):
    """The first random pedigree of 5 to 10 members that has (loops) / has not a conditioned member."""
    for seed in range(30):
        rng, ped = random_pedigree(seed)
        ped.relations()
        if 5 <= ped.n <= 10 and (conditioned(ped) > 0) == loops:
            return rng, ped
    raise AssertionError("no such pedigree")


def pedigrees():
    out = {name: fs.synthetic_pedigree(name) for name in ("trio", "quad")}
    out["tree"], out["loop"] = random_of(False)[1], random_of(True)[1]
    out["wide48"] = wide_pedigree(48)
    for ped in out.values():
        ped.relations()
    return out


PED_NAMES = ("trio", "quad", "tree", "loop", "wide48", "lone")
_PEDS = {}


def pedigree(name):
    if not _PEDS:
        _PEDS.update(pedigrees())
        # two components: a trio and an unrelated founder (each component of a loop-free pedigree carries the 1e7 of its own)
        _PEDS["lone"] = fs.Pedigree([1, 2, 3, 4], [0, 0, 2, 0], [0, 0, 1, 0], [1, 2, 2, 1], ["a", "b", "c", "d"])
        _PEDS["lone"].relations()
    return _PEDS[name]


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", PED_NAMES)
def test_every_variant_matches_the_reference(name, variant, tmp_path):
    ped = pedigree(name)
    model0 = fs.make_model(ped)
    fn, plan, src = build_evidence_host(model0, tmp_path, variant)
    assert ("conditioned on" in src.splitlines()[0]) == (name == "loop")
    assert ("#define l0_0 lgv[0]" in src) == (name == "wide48")  # the lean form
    rng = np.random.RandomState(40 + ped.n)
    lk, _ = clear_likelihoods(rng, ped, 200)
    flags = cycled(lk)
    outs = []
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        out = run_evidence(fn, model, lk, flags)
        check(out, reference(ped, mrate, lk, flags), "%s variant %d mrate %g" % (name, variant, mrate))
        outs.append(out)
    assert not same_bits(outs[0][:2], outs[1][:2])  # (the mutation rate reaches the kernel)


@pytest.mark.parametrize("name", ["loop", "tree"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped = pedigree(name)
    model = fs.make_model(ped, mrate=1e-4)
    lk, _ = clear_likelihoods(np.random.RandomState(5), ped, 128)
    flags = cycled(lk)
    outs = [run_evidence(build_evidence_host(model, tmp_path, v)[0], model, lk, flags) for v in range(N_VARIANTS)]
    for out in outs[1:]:
        assert same_bits(out, outs[0])


@pytest.mark.parametrize("mrate", [1e-7, 0.0])
@pytest.mark.parametrize("n", [24, 48, 64])
def test_wide_pedigrees(n, mrate, tmp_path):
    ped = wide_pedigree(n)
    ped.relations()
    lk, _ = clear_likelihoods(np.random.RandomState(n), ped, 200)
    flags = cycled(lk)
    model = fs.make_model(ped, mrate=mrate)
    fn, _, _ = build_evidence_host(model, tmp_path)
    check(run_evidence(fn, model, lk, flags), reference(ped, mrate, lk, flags), "wide%d mrate %g" % (n, mrate))


@pytest.mark.parametrize("name", PED_NAMES)
def test_site_prior_form(name, tmp_path):
    """Under the model's rows the plain form's bits; under Hardy-Weinberg rows tests/_prior_joint.py's numbers; the same bits from
    a prior array that is only 8-byte aligned."""
    ped = pedigree(name)
    rng = np.random.RandomState(7 + ped.n)
    lk, _ = clear_likelihoods(rng, ped, 200)
    flags = cycled(lk)
    hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, len(lk)))
    for variant in (0, 2):
        plain = build_evidence_host(fs.make_model(ped), tmp_path / "plain", variant)[0]
        fn, _, src = build_evidence_host(fs.make_model(ped), tmp_path / "prior", variant, prior=True)
        assert "PRIOR_LOAD(site);" in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src
        for mrate in MRATES:
            model = fs.make_model(ped, mrate=mrate)
            want = run_evidence(plain, model, lk, flags)
            assert np.all(want[2] == 0)
            assert same_bits(run_evidence(fn, model, lk, flags, P.model_rows(model, flags)), want)
            got = run_evidence(fn, model, lk, flags, hwe)
            # (a male founder's Hardy-Weinberg row has no heterozygotes at chrX sites: w0 stays positive, genotype 0 has weight)
            check(got, prior_reference(ped, mrate, lk, flags, hwe), "%s variant %d mrate %g, HWE rows" % (name, variant, mrate))
            assert same_bits(run_evidence(fn, model, lk, flags, hwe, misalign_prior=True), got)


def test_each_output_may_be_null(tmp_path):
    ped = pedigree("tree")
    model = fs.make_model(ped)
    lk, _ = clear_likelihoods(np.random.RandomState(1), ped, 64)
    flags = cycled(lk)
    for prior in (None, P.model_rows(model, flags)):
        fn = build_evidence_host(model, tmp_path, prior=prior is not None)[0]
        full = run_evidence(fn, model, lk, flags, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = run_evidence(fn, model, lk, flags, prior, want=want)
            untouched = (np.full(64, -5.0), np.full(64, -5.0), np.full(64, 77, np.uint8))
            for k in range(3):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


def test_failure_statuses(tmp_path):
    """An all-zero likelihood row: status 1.  A transmission-impossible trio at mutation rate 0 (the quad_mu0 shape: both parents
    hom-ref for certain, a child hom-alt for certain): status 2.  A hom-ref configuration without weight is no failure: pref 0.0."""
    ped = pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 32)
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    lk[9] = (1.0, 0.0, 0.0)
    lk[9, child] = (0.0, 0.0, 1.0)
    lk[13, child, 0] = 0.0  # the child cannot be hom-ref: w0 = 0, the site stands
    model = fs.make_model(ped, mrate=0.0)
    ref = reference(ped, 0.0, lk, flags)
    assert ref[2][5] == 1 and ref[2][9] == 2 and ref[1][13] == 0 and np.all(np.delete(ref[2], [5, 9]) == 0)
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = build_evidence_host(model, tmp_path, variant, prior=prior is not None)[0]
            ll, p0, st = out = run_evidence(fn, model, lk, flags, prior)
            check(out, ref, "planted failures", clear=False)
            assert st[5] == 1 and st[9] == 2 and st[13] == 0 and p0[13] == 0.0 and np.isfinite(ll[13])
    # a total weight that is not finite fails the site too
    big = np.full((2, ped.n, 3), 1e160)
    fn = build_evidence_host(model, tmp_path, 0)[0]
    ll, p0, st = run_evidence(fn, model, big, np.zeros(2, np.uint8))
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(p0))


def test_the_likelihood_may_exceed_one(tmp_path):
    """Rows scaled by 2^8 (as the LK driver's scales may be): loglik moves by N * 8 * log10(2) exactly to rounding and is positive,
    pref keeps its bits."""
    ped = pedigree("trio")
    model = fs.make_model(ped)
    lk, _ = clear_likelihoods(np.random.RandomState(2), ped, 64)
    flags = cycled(lk)
    fn = build_evidence_host(model, tmp_path)[0]
    a, b = run_evidence(fn, model, lk, flags), run_evidence(fn, model, lk * 256.0, flags)
    assert np.all(b[2] == 0) and same_bits([a[1]], [b[1]])
    np.testing.assert_allclose(b[0], a[0] + ped.n * 8 * np.log10(2.0), rtol=0, atol=1e-12)
    check(b, reference(ped, 1e-7, lk * 256.0, flags), "scaled rows")
    assert (b[0] > 0).any()


@pytest.mark.parametrize("gender", [1, 2])
def test_a_single_founder(gender, tmp_path):
    """One member, no family: pref is famseq's single posterior P(g = 0) = prior_0 lk_0 / sum_g prior_g lk_g, loglik the log10 of
    that sum."""
    ped = fs.Pedigree([1], [0], [0], [gender], ["a"])
    ped.relations()
    model = fs.make_model(ped)
    lk, _ = clear_likelihoods(np.random.RandomState(gender), ped, 64)
    flags = cycled(lk)
    fn = build_evidence_host(model, tmp_path)[0]
    ll, p0, st = run_evidence(fn, model, lk, flags)
    known, chrx = (flags & 1) != 0, (flags & 2) != 0
    autos = np.where(known[:, None], np.array(mp.GK), np.array(mp.GN))
    prior = np.where(chrx[:, None], np.where(known[:, None], np.array(mp.GXK), np.array(mp.GXN)), autos) if gender == 1 else autos
    p = prior * lk[:, 0]
    assert np.all(st == 0)
    np.testing.assert_allclose(p0, p[:, 0] / p.sum(axis=1), rtol=RTOL, atol=0)
    np.testing.assert_allclose(ll, np.log10(p.sum(axis=1)), rtol=0, atol=LL_ATOL)


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("evidence_kernels", "evidence_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = pedigree("tree")
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["evidence_code_object"] == "" and plan["evidence_variant"] == -1
        assert plan["evidence_prior_code_object"] == "" and plan["evidence_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("evidence_kernels", 2)
        ctx.set_option("evidence_kernels", 1)
        ctx.set_option("evidence_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["evidence_code_object"].endswith(".hsaco") and 0 <= plan["evidence_variant"] < N_VARIANTS
        assert plan["evidence_prior_code_object"].endswith(".hsaco") and plan["evidence_prior_variant"] == plan["evidence_variant"]
        assert plan["evidence_prior_code_object"] != plan["evidence_code_object"] and plan["map_code_object"] == ""
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.evidence_batch(lk=np.ones((1, ped.n, 3)))
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.evidence_prior_batch(np.ones((1, 6)), lk=np.ones((1, ped.n, 3)))
        with pytest.raises(fs.FamseqError, match="exactly one of"):
            lib_call_without_input(ctx)
        ctx.close()


def lib_call_without_input(ctx):
    rc = fs.lib().famseq_evidence_batch(ctx._h, 1, None, None, None, 0, None, None, None, None)
    ctx._check(rc, "famseq_evidence_batch")


def test_generating_the_evidence_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new body must not reach the text of the existing kernels (their code objects are cached by content hash)."""
    ped = pedigree("loop")
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    keys = ("elim_code_object", "trio_code_object", "map_code_object", "map_prior_code_object")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        ctx.set_option("map_kernels", 1)
        ctx.set_option("map_prior_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        ctx.set_option("evidence_kernels", 1)
        ctx.set_option("evidence_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["evidence_code_object"] not in [before[k] for k in keys]


def famseq_binary():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "FamSeq")


def test_cli_refuses_siteq_with_aftag(tmp_path):
    """-siteQ with -afTag: one output line must not mix two models (the message -dnm / -map get); said before any device is
    touched."""
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testdata")
    r = subprocess.run([famseq_binary(), "vcf", "-vcfFile", os.path.join(data, "test_subset.vcf"), "-pedFile", os.path.join(data, "fam01.ped"),
                        "-output", str(tmp_path / "o.vcf"), "-siteQ", "-afTag", "AF"], capture_output=True, text=True)
    assert r.returncode == 255
    assert "-afTag cannot be combined with -dnm or -map" in r.stdout
    assert not (tmp_path / "o.vcf").exists()
