"""The pattern kernel's arithmetic (famseq_pattern / famseq_pattern_prior: per site and pattern m the posterior probability
Z_m / Z that every member's genotype is one its mask allows, and the site's log10 likelihood), checked without a GPU.

As in test_evidence_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled
with g++.  References: up to ten members the 3^N enumeration of test_map_host.brute_weights, whose G and W give Z_m as the sum
of W over the configurations every mask admits; beyond, tests/_maxproduct.py's Z (max_product(...)[2]) on masked rows over the
same on the real rows; under per-site priors tests/_prior_joint.py's factors through the same elimination.

Wanted: status exact; ppost == 0.0 exactly where the reference's Z_m is exactly 0 (male heterozygotes on chrX, Mendelian-
impossible patterns at mutation rate 0, a mask of 0); elsewhere ppost at the project's rtol 1e-9; ppost == 1.0 exactly for a
row of 7s and ppost <= 1.0 everywhere; loglik at an ABSOLUTE 1e-9 (test_evidence_host's derivation: a relative 1e-9 on Z is
4.3e-10 in log10, the logarithm's own few ulp on magnitudes <= 130 add about 1e-13).  The kernel keeps famseq_evidence's
statements for the unmasked pass, so its loglik is BIT-EQUAL to the host-compiled famseq_evidence of the same variant (the
stronger of the two claims the issue allows; asserted below), and the all-1 row equals that kernel's pref at 1e-9.

No site is left out of a comparison: every batch asserts, on the reference alone, status 0 everywhere and Z and every
non-zero Z_m >= 1e-200 (the references alone on these inputs: Z >= 6e-75, non-zero Z_m >= 2e-142, the 48-member case the smallest).
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
from test_evidence_host import build_evidence_host, run_evidence
from test_generated_host import factor_tables, host_source
from test_map_host import brute_weights, clear_likelihoods

RTOL = 1e-9     # ppost: the project's bar for posteriors
LL_ATOL = 1e-9  # loglik: absolute (see the module's docstring)
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kPatternVariants
FLOOR = 1e-200
TWO_CUT_SEED = 99  # tools/source_digests.py: the first random_pedigree seed whose loops need two conditioned members
N_SITES = 64


def build_pattern_host(model, where, variant=None, prior=False):
    """Generate famseq_pattern (prior: famseq_pattern_prior) for a one-lane workgroup on a plan-only context, compile it for
    the host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("pattern_prior", "famseq_pattern_prior") if prior else ("pattern", "famseq_pattern")
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
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_void_p, C.c_int] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def run_pattern(fn, model, lk, flags, masks, prior=None, want=(True, True, True)):
    s, m = lk.shape[0], masks.shape[0]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    pp, ll, st = np.full((s, m), -5.0), np.full(s, -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    mk = np.ascontiguousarray(masks, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, pp.ctypes.data if want[0] else None, ll.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, mk.ctypes.data, m]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return pp, ll, st


def cycled(lk):
    """Flags 0..3 in turn."""
    return (np.arange(len(lk)) % 4).astype(np.uint8)


def allowed(masks):
    """masks[M, N] -> [M, N, 3] of 0.0 / 1.0: what a pattern multiplies a likelihood row by (exactly)."""
    return ((np.asarray(masks, np.uint8)[:, :, None] >> np.arange(3)) & 1).astype(np.float64)


def _total(ped, mrate, lk, flags, prior):
    """(Z[S], single_fail[S]) of the rows lk: max_product's Z (its own statements) or, under site priors, _prior_joint's factors
    through the same elimination."""
    if prior is None:
        _, _, z, _ = mp.max_product(ped, mrate, lk, flags)
        return z, mp.site_factors(ped, mrate, lk, flags)[1]
    factors, fail = J.site_factors(ped, mrate, lk, flags, prior)
    return mp._constant(mp.eliminate(factors, mp.elimination_order(factors, ped.n), False)[0], lk.shape[0]), fail


def reference(ped, mrate, lk, flags, masks, prior=None):
    """-> (z[S], zm[S, M], status[S]): the total weight, every pattern's weight (both with the reference's 1e7), and the status
    of the real rows."""
    keep = allowed(masks)
    if ped.n <= 10 and prior is None:
        G, W, st = brute_weights(ped, mrate, lk, flags)
        admit = np.all(keep[:, np.arange(ped.n)[:, None], G] == 1.0, axis=1)  # [M, 3^N]
        with np.errstate(invalid="ignore"):
            return W.sum(axis=1), np.stack([W[:, a].sum(axis=1) for a in admit], axis=1), st
    z, fail = _total(ped, mrate, lk, flags, prior)
    zm = np.stack([_total(ped, mrate, lk * k, flags, prior)[0] for k in keep], axis=1)
    st = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    return z, zm, st


def batch_masks(rng, ped):
    """The masks of one batch: all 7, all 1, a dominant and a recessive row for a random 40 % affected (of the others every
    second one unaffected, the rest unconstrained), four rows that constrain at most six random members to a random non-empty
    set, one row that holds a 0."""
    n = ped.n
    order = rng.permutation(n)
    k = max(1, int(round(0.4 * n)))
    aff, unaff = order[:k], order[k::2]
    rows = [np.full(n, 7, np.uint8), np.full(n, 1, np.uint8), fs.segregation_masks(n, aff, unaff, "dominant"),
            fs.segregation_masks(n, aff, unaff, "recessive")]
    for _ in range(4):
        row = np.full(n, 7, np.uint8)
        who = rng.permutation(n)[:rng.randint(1, min(6, n) + 1)]
        row[who] = rng.randint(1, 8, len(who))
        rows.append(row)
    zero = np.full(n, 7, np.uint8)
    zero[rng.randint(n)] = 0
    rows.append(zero)
    return np.stack(rows)


def check(out, ref, masks, what="", clear=True):
    """The module docstring's rules; every site and pattern compared.  Prints the worst errors before it asserts."""
    pp, ll, st = out
    z, zm, ref_st = ref
    if clear:
        assert np.all(ref_st == 0) and np.all(z >= FLOOR) and np.all((zm == 0) | (zm >= FLOOR)), what
    assert np.array_equal(st, ref_st), what
    ok = ref_st == 0
    assert np.all(np.isnan(ll[~ok])) and np.all(np.isnan(pp[~ok])), what
    want = zm[ok] / z[ok][:, None]
    got = pp[ok]
    zero = zm[ok] == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(zero, 0.0, np.abs(got / want - 1.0))
    err = np.abs(ll[ok] - (np.log10(z[ok]) - 7.0))
    print("%s: %d sites x %d patterns, %d exact zeros, worst ppost relative error %.3g, worst |loglik error| %.3g, smallest Z %.3g, "
          "smallest non-zero Z_m %.3g" % (what, ok.sum(), masks.shape[0], zero.sum(), rel.max(initial=0), err.max(initial=0),
                                          z[ok].min(initial=1), zm[ok][~zero].min(initial=1)))
    assert np.all(got[zero] == 0.0), what
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=RTOL, atol=0, err_msg=what)
    assert np.all(got <= 1.0), what
    free = np.all(masks == 7, axis=1)
    assert np.all(got[:, free] == 1.0), what
    np.testing.assert_allclose(ll[ok], np.log10(z[ok]) - 7.0, rtol=0, atol=LL_ATOL, err_msg=what)


def bits(out):
    return [np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint8) for x in out]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


_PEDS = {}


def pedigree(name):
    """random<seed> (random_pedigree), wide<n>, trio, quad."""
    if name not in _PEDS:
        if name.startswith("random"):
            ped = random_pedigree(int(name[6:]))[1]
        elif name.startswith("wide"):
            ped = wide_pedigree(int(name[4:]))
        else:
            ped = fs.synthetic_pedigree(name)
        ped.relations()
        _PEDS[name] = ped
    return _PEDS[name]


def batch(name, seed=0):
    ped = pedigree(name)
    rng = np.random.RandomState(100 + 7 * ped.n + seed)
    lk, flags = clear_likelihoods(rng, ped, N_SITES)  # flags 0..3 mixed
    return ped, lk, flags, batch_masks(rng, ped)


PED_NAMES = ["random0", "random1", "random2", "random3", "random%d" % TWO_CUT_SEED, "wide24", "wide48"]


@pytest.mark.parametrize("name", PED_NAMES)
def test_the_kernel_matches_the_reference(name, tmp_path):
    ped, lk, flags, masks = batch(name)
    fn, plan, src = build_pattern_host(fs.make_model(ped), tmp_path)
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= 40)  # the lean form from forty members on
    assert src.count("for (int pt_ = 0;") == 1 and src.count("const double Zp_") == 1  # the pass's text stands once
    assert {0, 1, 2, 3} <= set(flags.tolist())
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", plan["pattern_variant"])[0]
    zeros = 0
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        ref = reference(ped, mrate, lk, flags, masks)
        out = run_pattern(fn, model, lk, flags, masks)
        check(out, ref, masks, "%s mrate %g" % (name, mrate))
        zeros += int((ref[1] == 0).sum())
        # the unmasked pass keeps famseq_evidence's statements: its loglik, bit for bit; the all-1 row is that kernel's pref
        ll, p0, st = run_evidence(ev, model, lk, flags)
        assert np.all(st == 0) and same_bits([out[1]], [ll])
        np.testing.assert_allclose(out[0][:, 1], p0, rtol=RTOL, atol=0)
    assert zeros > N_SITES  # (the row with a 0 alone gives that many; chrX males and mutation rate 0 add theirs)


def test_exact_zeros_come_from_the_model_too():
    """The references hold exact zeros that no mask of 0 put there: a male heterozygote on chrX, and at mutation rate 0 a
    pattern Mendel forbids."""
    ped = pedigree("trio")
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(1), ped, 8)
    male = [p for p in range(ped.n) if ped.genders[p] == 1][0]
    het = np.full((1, ped.n), 7, np.uint8)
    het[0, male] = 2
    z, zm, st = reference(ped, 1e-7, lk, np.full(8, 2, np.uint8), het)
    assert np.all(st == 0) and np.all(zm == 0)
    imp = np.full((1, ped.n), 1, np.uint8)
    imp[0, child] = 4
    z, zm, st = reference(ped, 0.0, lk, np.zeros(8, np.uint8), imp)
    assert np.all(st == 0) and np.all(zm == 0) and np.all(z > 0)


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped, lk, flags, masks = batch(name, 1)
    model = fs.make_model(ped, mrate=1e-4)
    outs = [run_pattern(build_pattern_host(model, tmp_path, v)[0], model, lk, flags, masks) for v in range(N_VARIANTS)]
    assert np.all(outs[0][2] == 0)
    for out in outs[1:]:
        assert same_bits(out, outs[0])


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_site_prior_form(name, tmp_path):
    """Fed the model's rows: the plain form's bits.  Under Hardy-Weinberg rows: tests/_prior_joint.py's factors on masked rows."""
    ped, lk, flags, masks = batch(name, 2)
    hwe = fs.hwe_priors(np.random.RandomState(3).uniform(0.01, 0.5, len(lk)))
    plain = build_pattern_host(fs.make_model(ped), tmp_path / "plain", 1)[0]
    fn, _, src = build_pattern_host(fs.make_model(ped), tmp_path / "prior", 1, prior=True)
    assert "PRIOR_LOAD(site);" in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src
    assert "int n_patterns, const double *__restrict__ prior_g) {" in src  # the masks stand in front of the prior rows
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        want = run_pattern(plain, model, lk, flags, masks)
        assert np.all(want[2] == 0)
        assert same_bits(run_pattern(fn, model, lk, flags, masks, P.model_rows(model, flags)), want)
        check(run_pattern(fn, model, lk, flags, masks, hwe), reference(ped, mrate, lk, flags, masks, hwe), masks,
              "%s mrate %g, HWE rows" % (name, mrate))


@pytest.mark.parametrize("name", ["random0", "random1"])
def test_one_members_three_rows_are_its_marginal(name, tmp_path):
    """The three patterns {g_i = a}: sum to 1 within 1e-12 and equal the oracle's marginal of member i at 1e-9."""
    import oracle

    ped, lk, flags, _ = batch(name, 3)
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_pattern_host(model, tmp_path)[0]
    post, _, status = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=1e-4).bn_batch(lk, flags)
    assert np.all(status == 0)
    for i in range(ped.n):
        masks = np.full((3, ped.n), 7, np.uint8)
        masks[:, i] = (1, 2, 4)
        pp, _, st = run_pattern(fn, model, lk, flags, masks)
        assert np.all(st == 0)
        np.testing.assert_allclose(pp.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pp, post[:, i], rtol=RTOL, atol=1e-300)


def test_failure_statuses(tmp_path):
    """An all-zero likelihood row: status 1.  The quad_mu0 shape (both parents hom-ref for certain, a child hom-alt for certain,
    mutation rate 0): status 2.  Every output of such a site is NaN; a pattern without weight on a good site is 0.0."""
    ped = pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 32)
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    lk[9] = (1.0, 0.0, 0.0)
    lk[9, child] = (0.0, 0.0, 1.0)
    masks = batch_masks(np.random.RandomState(4), ped)
    model = fs.make_model(ped, mrate=0.0)
    ref = reference(ped, 0.0, lk, flags, masks)
    assert ref[2][5] == 1 and ref[2][9] == 2 and np.all(np.delete(ref[2], [5, 9]) == 0)
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = build_pattern_host(model, tmp_path, variant, prior=prior is not None)[0]
            pp, ll, st = out = run_pattern(fn, model, lk, flags, masks, prior)
            check(out, ref, masks, "planted failures", clear=False)
            assert st[5] == 1 and st[9] == 2 and np.all(np.isnan(pp[[5, 9]])) and np.all(np.isnan(ll[[5, 9]]))
            assert np.all(pp[np.delete(np.arange(32), [5, 9]), -1] == 0.0)
    # a total weight that is not finite fails the site too
    big = np.full((2, ped.n, 3), 1e160)
    pp, ll, st = run_pattern(build_pattern_host(model, tmp_path, 0)[0], model, big, np.zeros(2, np.uint8), masks)
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(pp))


def test_each_output_may_be_null(tmp_path):
    ped, lk, flags, masks = batch("random1", 4)
    model = fs.make_model(ped)
    for prior in (None, P.model_rows(model, flags)):
        fn = build_pattern_host(model, tmp_path, prior=prior is not None)[0]
        full = run_pattern(fn, model, lk, flags, masks, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = run_pattern(fn, model, lk, flags, masks, prior, want=want)
            untouched = (np.full(full[0].shape, -5.0), np.full(N_SITES, -5.0), np.full(N_SITES, 77, np.uint8))
            for k in range(3):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


@pytest.mark.parametrize("name", ["random0", "wide48"])
def test_one_pattern_and_thirty_two(name, tmp_path):
    """n_patterns = 1 and FAMSEQ_MAX_PATTERNS: a pattern's value does not depend on how many others the call holds."""
    ped, lk, flags, masks = batch(name, 5)
    rng = np.random.RandomState(6)
    many = np.concatenate([masks, rng.randint(1, 8, size=(32 - len(masks), ped.n)).astype(np.uint8)])
    assert many.shape[0] == 32
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_pattern_host(model, tmp_path)[0]
    out = run_pattern(fn, model, lk, flags, many)
    check(out, reference(ped, 1e-4, lk, flags, many), many, "%s, 32 patterns" % name)
    for m in (0, 2, 31):
        one = run_pattern(fn, model, lk, flags, many[m:m + 1])
        assert same_bits([one[0][:, 0], one[1], one[2]], [out[0][:, m], out[1], out[2]])


def test_generating_the_pattern_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new body must not reach the text of the existing kernels (their code objects are cached by content hash)."""
    ped = pedigree("random0")
    assert fs.Context(fs.make_model(ped), device=-1).plan()["elim_conditioned_members"] > 0  # (a pedigree with a loop)
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    keys = ("elim_code_object", "trio_code_object", "map_code_object", "map_prior_code_object", "evidence_code_object",
            "evidence_prior_code_object", "loo_code_object", "loo_prior_code_object", "prior_code_object")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        for stem in ("map", "map_prior", "evidence", "evidence_prior", "loo", "loo_prior", "prior"):
            ctx.set_option(stem + "_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        ctx.set_option("pattern_kernels", 1)
        ctx.set_option("pattern_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["pattern_code_object"] not in [before[k] for k in keys]
    assert after["pattern_prior_code_object"] not in [before[k] for k in keys] + [after["pattern_code_object"]]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("pattern_kernels", "pattern_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = pedigree("random0")
    ones = np.ones((1, ped.n, 3))
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["pattern_code_object"] == "" and plan["pattern_variant"] == -1
        assert plan["pattern_prior_code_object"] == "" and plan["pattern_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("pattern_kernels", 2)
        ctx.set_option("pattern_kernels", 1)
        ctx.set_option("pattern_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["pattern_code_object"].endswith(".hsaco") and 0 <= plan["pattern_variant"] < N_VARIANTS
        assert plan["pattern_prior_code_object"].endswith(".hsaco") and plan["pattern_prior_variant"] == plan["pattern_variant"]
        assert plan["pattern_prior_code_object"] != plan["pattern_code_object"] and plan["evidence_code_object"] == ""
        # the ABI's refusals of the masks come before anything else, so a context without a device gives them too
        good = np.full((1, ped.n), 7, np.uint8)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_patterns must be 1\.\.32"):
            ctx.pattern_batch(np.full((33, ped.n), 7, np.uint8), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_patterns must be 1\.\.32"):
            ctx.pattern_batch(np.zeros((0, ped.n), np.uint8), lk=ones)
        bad = good.copy()
        bad[0, ped.n - 1] = 8
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*pattern 0, member %d is 8" % (ped.n - 1)):
            ctx.pattern_batch(bad, lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*pattern 0, member %d is 8" % (ped.n - 1)):
            ctx.pattern_prior_batch(np.ones((1, 6)), bad, lk=ones)
        for fn, more in (("famseq_pattern_batch", ()), ("famseq_pattern_prior_batch", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 1, None, None, None)
            assert rc == -1 and "masks must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        for fn, more in (("famseq_pattern_batch_device", ()), ("famseq_pattern_prior_batch_device", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 0, None, None, None, None)
            assert rc == -1 and "n_patterns must be 1..32" in fs.lib().famseq_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match="shape"):
            ctx.pattern_batch(np.full((1, ped.n + 1), 7, np.uint8), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.pattern_batch(good, lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.pattern_prior_batch(np.ones((1, 6)), good, lk=ones)
        ctx.close()


def test_segregation_masks():
    assert fs.segregation_masks(5, [0, 3], [1], "dominant").tolist() == [6, 1, 7, 6, 7]
    assert fs.segregation_masks(5, [0, 3], [1], "recessive").tolist() == [4, 3, 7, 4, 7]
    assert fs.segregation_masks(3, [2]).tolist() == [7, 7, 6] and fs.segregation_masks(2, []).dtype == np.uint8
    for args in ((3, [3], [], "dominant"), (3, [0], [0], "dominant"), (3, [0], [], "additive")):
        with pytest.raises(ValueError):
            fs.segregation_masks(*args)
