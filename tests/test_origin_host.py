"""The origin kernel's arithmetic (famseq_origin / famseq_origin_prior: per child the posterior of the alleles received from
mother and father, and the expected transmissions from heterozygous parents), checked without a GPU.

As in test_trio_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++ -ffp-contract=off.  The reference is tests/_origin.py's: the 3^N enumeration of test_trio_host.brute_joint, each joint cell
split by the allele-level factor, the allele rows formed from the rate in numpy (and asserted equal, bit for bit, to
famseq_allele_tables').  On the wide pedigrees, which the enumeration cannot reach, the genotype sums of origin and the pair sums
of hettx are compared with the sum-product oracle's marginals.

Wanted (tests/_origin.check): status equal to the reference's; origin rows sum to 1 within 1e-12; both outputs at RTOL = 1e-9
relative on entries >= 1e-280 x the row's maximum and <= 1e-270 x it below; at rate 0 every entry the reference has as 0 exactly
0.0; origin summed to genotypes and hettx's pairs equal to the enumeration's marginals; failed sites NaN in both outputs.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _origin as O
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_generated_host import factor_tables, host_source
from test_trio_host import wide_likelihoods

RTOL = O.RTOL
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kOriginVariants


def build_origin_host(model, where, variant=None, prior=False):
    """Generate famseq_origin (prior: famseq_origin_prior) for a one-lane workgroup on a plan-only context, compile it for the
    host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("origin_prior", "famseq_origin_prior") if prior else ("origin", "famseq_origin")
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
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_void_p] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def allele_tables_of(model):
    ctx = fs.Context(model, device=-1)
    t = ctx.allele_tables()
    ctx.close()
    return t


def n_children(model):
    return int(sum(1 for p in range(model.n_members) if model.mother[p] >= 0))


def run_origin(fn, model, lk, flags, prior=None, want=(True, True, True), tables=None):
    s, k = lk.shape[0], n_children(model)
    a = np.ascontiguousarray(lk, dtype=np.float64)
    og, hg, st = np.full((s, k, 4), -5.0), np.full((s, k, 4), -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    al = np.ascontiguousarray(allele_tables_of(model) if tables is None else tables)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, og.ctypes.data if want[0] else None, hg.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, al.ctypes.data]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return og, hg, st


_KERNELS = {}


def kernel(seed, tmp_path_factory, variant=None, prior=False):
    key = (seed, variant, prior)
    if key not in _KERNELS:
        rng, ped = random_pedigree(seed)
        ped.relations()
        _KERNELS[key] = build_origin_host(fs.make_model(ped), tmp_path_factory.mktemp("origin_%d" % seed), variant, prior)
    return _KERNELS[key]


@pytest.mark.parametrize("mu", [0.0, 1e-9, 1e-7, 1e-4, 1e-3, 0.3, 0.5, 1.0])
def test_the_allele_rows_multiply_out_to_the_models_tables(mu):
    """sum over gamma(a, b) = gc of tm tf is T: the same zero pattern, 2.2e-16 relative at the worst (one unit in the last place;
    the son's table exactly), and famseq_allele_tables gives numpy's rows bit for bit."""
    rng, ped = random_pedigree(0)
    model = fs.make_model(ped, mrate=mu)
    al = O.allele_rows(mu)
    assert O.same_bits(allele_tables_of(model), al)
    pcp2, xf, xm = (np.asarray(t).reshape(3, 3, 3) for t in fs.transmission_tables(mu))
    for x, sex, T in ((0, 0, pcp2), (0, 1, pcp2), (1, 1, xf), (1, 0, xm)):
        P = np.zeros((3, 3, 3))
        for a in range(2):
            for b in range(2):
                P[O.gamma(x, sex == 0, a, b)] += al[x, sex, 0, a][:, None] * al[x, sex, 1, b][None, :]
        assert np.array_equal(P == 0, T == 0)
        np.testing.assert_allclose(P, T, rtol=2.3e-16, atol=0)
        if (x, sex) == (1, 0):
            assert np.array_equal(P, T)
    ctx = fs.Context(model, device=-1)
    assert ctx.plan()["origin_mrate"] == mu
    ctx.close()


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_origin_matches_the_enumeration(seed, mrate, tmp_path_factory):
    rng, ped = random_pedigree(seed)  # 3 to 9 members, loops on every third seed
    ped.relations()
    model = fs.make_model(ped, mrate=mrate)
    fn, plan, src = kernel(seed, tmp_path_factory)
    lk, flags = random_likelihoods(rng, ped, 200)
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    ref = O.reference(ped, mrate, lk, flags)
    # (without prior rows the reference is test_trio_host.brute_joint itself; the form that takes prior rows is its statements)
    j, st = O.brute_joint_prior(ped, mrate, lk, flags)
    assert np.array_equal(st, ref.status) and np.array_equal(j[st == 0], ref.joint[st == 0])
    assert (ref.status == 0).sum() > 100
    out = run_origin(fn, model, lk, flags)
    O.check(out, ref, "seed %d rate %g" % (seed, mrate), zero_exact=mrate == 0.0)
    if mrate == 0.0 and n_children(model):
        assert (ref.origin[ref.status == 0] == 0).any()
    # a NULL output leaves the other's bits unchanged
    o2, _, s2 = run_origin(fn, model, lk, flags, want=(True, False, True))
    _, h3, s3 = run_origin(fn, model, lk, flags, want=(False, True, False))
    assert O.same_bits(o2, out[0]) and O.same_bits(h3, out[1]) and np.array_equal(s2, out[2]) and np.all(s3 == 77)


@pytest.mark.parametrize("seed", [0, 1, 3, 6])
def test_the_four_variants_agree(seed, tmp_path_factory):
    rng, ped = random_pedigree(seed)
    model = fs.make_model(ped, mrate=1e-4)
    lk, flags = random_likelihoods(rng, ped, 64)
    outs, srcs = [], []
    for v in range(N_VARIANTS):
        fn, plan, src = kernel(seed, tmp_path_factory, variant=v)
        outs.append(run_origin(fn, model, lk, flags))
        srcs.append(src)
    ok = outs[0][2] == 0
    # (the message passing and the outputs: from the allele rows' pointer on; a fence is an empty asm statement.  The single
    # posterior in front decides status 1 alone and is written differently where it is fenced)
    fence = lambda s: "\n".join(l for l in s[s.index("const double *alx"):].splitlines() if "asm volatile" not in l)
    for v in range(1, N_VARIANTS):
        assert np.array_equal(outs[v][2], outs[0][2])
        for a, b in zip(outs[v][:2], outs[0][:2]):
            np.testing.assert_allclose(a[ok], b[ok], rtol=RTOL, atol=1e-300)
            assert np.all(np.isnan(a[~ok]))
    # variants 1, 2 and 3 differ in their compiler fences alone: the same statements, the same bits
    assert fence(srcs[1]) == fence(srcs[2]) == fence(srcs[3])
    for v in (2, 3):
        assert O.same_bits(outs[v][0], outs[1][0]) and O.same_bits(outs[v][1], outs[1][1])


@pytest.mark.parametrize("seed", [0, 3, 5])
def test_the_site_prior_form(seed, tmp_path_factory):
    """On the model's own rows the plain form's bits; on Hardy-Weinberg rows the enumeration under those rows."""
    import _prior as P

    rng, ped = random_pedigree(seed)
    ped.relations()
    model = fs.make_model(ped, mrate=1e-4)
    lk, flags = random_likelihoods(rng, ped, 120)
    fn, _, _ = kernel(seed, tmp_path_factory)
    fnp, _, _ = kernel(seed, tmp_path_factory, prior=True)
    plain = run_origin(fn, model, lk, flags)
    rows = P.model_rows(model, flags)
    mine = run_origin(fnp, model, lk, flags, prior=rows)
    assert O.same_bits(mine[0], plain[0]) and O.same_bits(mine[1], plain[1]) and np.array_equal(mine[2], plain[2])
    hwe = fs.hwe_priors(np.random.RandomState(seed).uniform(0.01, 0.6, lk.shape[0]))
    ref = O.reference(ped, 1e-4, lk, flags, prior=hwe)
    assert (ref.status == 0).sum() > 60
    O.check(run_origin(fnp, model, lk, flags, prior=hwe), ref, "HWE rows, seed %d" % seed)


def test_the_text_holds_no_rate(tmp_path):
    """Kernels are cached per pedigree, not per rate: models made at two rates generate the same text."""
    rng, ped = random_pedigree(3)
    srcs = [build_origin_host(fs.make_model(ped, mrate=m), tmp_path / str(i))[2] for i, m in enumerate((1e-7, 3e-4))]
    assert srcs[0] == srcs[1] and "al_g" in srcs[0]


def test_failed_sites_are_nan(tmp_path_factory):
    rng, ped = random_pedigree(1)
    model = fs.make_model(ped)
    fn, _, _ = kernel(1, tmp_path_factory)
    lk, flags = random_likelihoods(rng, ped, 8)
    lk[:] = np.where(lk > 0, lk, 0.5)
    lk[3, 0, :] = 0.0  # an all-zero likelihood row
    og, hg, st = run_origin(fn, model, lk, flags)
    assert st[3] == 1 and np.all(np.isnan(og[3])) and np.all(np.isnan(hg[3]))
    assert np.all(st[[0, 1, 2, 4, 5, 6, 7]] == 0) and not np.isnan(og[st == 0]).any() and not np.isnan(hg[st == 0]).any()


def test_models_without_an_allele_level_form_are_refused():
    """One table entry perturbed, or tables of two different rates: FAMSEQ_E_ARG, from every way in, without a device."""
    rng, ped = random_pedigree(0)
    for spoil in ("entry", "rates"):
        model = fs.make_model(ped, mrate=1e-4)
        if spoil == "entry":
            model.pcp2[4] = np.nextafter(model.pcp2[4], 1.0)
        else:
            other = fs.make_model(ped, mrate=1e-5)
            for i in range(27):
                model.pcp2Xf[i] = other.pcp2Xf[i]
        ctx = fs.Context(model, device=-1)
        assert ctx.plan()["origin_mrate"] is None
        for call in (lambda: ctx.set_option("origin_kernels", 1), lambda: ctx.set_option("origin_prior_kernels", 1), ctx.allele_tables,
                     lambda: ctx.origin_batch(lk=np.ones((1, ped.n, 3)))):
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*no allele-level model for custom"):
                call()
        ctx.close()


def test_a_pedigree_the_engine_refuses():
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("origin_kernels", "origin_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*phase by transmission \(sum-product engine\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()


def test_option_values_and_plan_keys(tmp_path):
    rng, ped = random_pedigree(2)
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        for bad in (0, 2):
            with pytest.raises(fs.FamseqError, match="origin_kernels takes 1"):
                ctx.set_option("origin_kernels", bad)
        assert ctx.plan()["origin_code_object"] == "" and ctx.plan()["origin_variant"] == -1
        ctx.set_option("origin_kernels", 1)
        ctx.set_option("origin_prior_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    assert plan["origin_code_object"].endswith(".hsaco") and 0 <= plan["origin_variant"] < N_VARIANTS
    assert plan["origin_prior_code_object"].endswith(".hsaco") and plan["origin_prior_variant"] == plan["origin_variant"]
    assert plan["origin_mrate"] == 1e-7


def test_phased_calls():
    o = np.array([[0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25], [np.nan] * 4, [0.0, 0.5, 0.5, 0.0], [1.0, 0.0, 0.0, 0.0]])
    idx, p = fs.phased_calls(o)
    assert idx.dtype == np.int8 and list(idx) == [3, 0, -1, 1, 0]
    assert np.array_equal(p[[0, 1, 3, 4]], [0.4, 0.25, 0.5, 1.0]) and np.isnan(p[2])
    idx2, p2 = fs.phased_calls(o.reshape(5, 1, 4))
    assert idx2.shape == (5, 1) and np.array_equal(idx2[:, 0], idx)


@pytest.mark.parametrize("n", [24, 48])
def test_wide_pedigrees_marginals(n, tmp_path):
    """Beyond the enumeration's reach (48: the lean form): origin summed to genotypes and hettx's pairs against the sum-product
    oracle's marginals.  No site is left out: the oracle alone says every site is clear, then the kernel's status must agree."""
    import oracle.sum_product as sp

    ped = wide_pedigree(n)
    mo, fa = ped.relations()
    lk, flags = wide_likelihoods(ped, n)
    # (the floor raised under the rows' hard zeros as well: at 48 members three sites of this draw give a male at a chrX site a
    # row that is 0 wherever his prior is not, which fails the single posterior in the oracle and the kernel alike)
    lk[lk < 1e-2] = 1e-2
    post, _, ref_st = sp.pedigree_posterior(ped, lk, flags, lc=2.0)  # lc > 1: no shortcut, every site the full network
    assert np.all(ref_st == 0)
    model = fs.make_model(ped)
    fn, plan, src = build_origin_host(model, tmp_path / "k")
    assert ("lgv[" in src) == (n >= 40)
    og, hg, st = run_origin(fn, model, lk, flags)
    assert np.array_equal(st, ref_st)
    np.testing.assert_allclose(og.sum(axis=-1), 1.0, rtol=1e-12, atol=0)
    kids = [p for p in range(ped.n) if mo[p] >= 0]
    for k, c in enumerate(kids):
        o = og[:, k]
        son_x = ((flags & 2) != 0) & (ped.genders[c] == 1)
        child = np.where(son_x[:, None], np.stack([o[:, 0] + o[:, 1], 0 * o[:, 0], o[:, 2] + o[:, 3]], axis=1),
                         np.stack([o[:, 0], o[:, 1] + o[:, 2], o[:, 3]], axis=1))
        O.close(child, post[:, c], "child %d" % c)
        pairs = np.stack([hg[:, k, 0] + hg[:, k, 1], hg[:, k, 2] + hg[:, k, 3]], axis=1)
        want = np.stack([post[:, mo[c], 1], post[:, fa[c], 1]], axis=1)
        sel = want >= 1e-280
        np.testing.assert_allclose(pairs[sel], want[sel], rtol=RTOL, atol=0)
        assert np.all(np.abs(pairs - want)[~sel] <= 1e-270)
