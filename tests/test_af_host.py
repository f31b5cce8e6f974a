"""The allele-frequency kernel's arithmetic (famseq_af: per site n_iter EM steps on the allele frequency q of the founders'
Hardy-Weinberg prior, the site's log10 likelihood at the result and at q = 0), checked without a GPU.

As in test_pattern_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled
with g++ (-ffp-contract=off).  The reference is tests/_af.py's numpy EM loop over the project's existing references.

Wanted: status exact; af at the project's rtol 1e-9 (atol 1e-300); both loglik entries at an ABSOLUTE 1e-9
(test_evidence_host's derivation: a relative 1e-9 on Z is 4.3e-10 in log10, the logarithm's own few ulp on magnitudes <= 130
add about 1e-13); loglik[1] == -inf exactly where the reference's Z(0) is exactly 0.  A pass keeps famseq_evidence_prior's
statements for its total weight, so at n_iter = 0 loglik[0] is BIT-EQUAL to the host-compiled famseq_evidence_prior of the same
variant on hwe_priors(af0) (the stronger of the two claims the issue allows; asserted below), and status equals its status.

No site is left out of a comparison: every batch asserts, on the reference alone, status 0 everywhere and every Z(q_t) >= 1e-200
(tests/_af.py reference()).
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _af as A
import famseq_amd as fs
from test_evidence_host import build_evidence_host, run_evidence
from test_generated_host import factor_tables, host_source
from test_map_host import clear_likelihoods
from test_pattern_host import TWO_CUT_SEED, pedigree, same_bits

RTOL, ATOL = 1e-9, 1e-300  # af: the project's bar for posteriors
LL_ATOL = 1e-9             # loglik: absolute (see the module's docstring)
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kAfVariants
N_SITES = 64


def build_af_host(model, where, variant=None):
    """Generate famseq_af for a one-lane workgroup on a plan-only context, compile it for the host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option("af_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    src = open(plan["af_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and "famseq_af(" in src
    first = src.splitlines()[0]
    assert "founder allele frequency by maximum likelihood" in first and "founder priors per site" not in first
    assert "q' = min(sum_f count_f / C, 1)" in src  # the leading comment states the update rule
    assert "PRIOR_LOAD" not in src and "prior_g" not in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src
    assert "const double *__restrict__ af0_g, int n_iter) {" in src
    # the pass's text stands once whatever n_iter is
    assert src.count("for (int it_ = -1; it_ <= n_it_; ++it_)") == 1 and src.count("const double Zp_") == 1
    assert src.count("#pragma unroll 1\n      for (int it_") == 1 and src.count("q_ = qn_ < 1.0") == 1
    assert variant is None or plan["af_variant"] == variant
    tag = "af" + ("" if variant is None else "_%d" % variant)
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = C.CDLL(so).famseq_af
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_void_p, C.c_int]
    return fn, plan, src


def run_af(fn, model, lk, flags, af0, n_iter, want=(True, True, True)):
    s = lk.shape[0]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    q0 = np.ascontiguousarray(np.broadcast_to(af0, (s,)), dtype=np.float64)
    af, ll, st = np.full(s, -5.0), np.full((s, 2), -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    fn(a.ctypes.data, fl.ctypes.data, af.ctypes.data if want[0] else None, ll.ctypes.data if want[1] else None,
       st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, q0.ctypes.data, n_iter)
    return af, ll, st


def check(out, r, t, what=""):
    """The module docstring's rules against step t of the reference r; every site compared.  Prints the worst errors first."""
    af, ll, st = out
    want_ll = A.loglik(r, t)
    dead = np.isinf(want_ll[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(af / r.q[t] - 1.0)
    err = np.abs(ll[:, 0] - want_ll[:, 0]).max()
    err0 = np.abs(ll[~dead, 1] - want_ll[~dead, 1]).max(initial=0)
    print("%s, %d steps: %d sites, worst af relative error %.3g (af %.3g .. %.3g), worst |loglik error| %.3g / %.3g, %d sites exclude "
          "q = 0, smallest Z %.3g" % (what, t, len(af), np.nanmax(rel), af.min(), af.max(), err, err0, dead.sum(), r.z[:t + 1].min()))
    assert np.all(st == 0) and np.all(r.status == 0), what
    np.testing.assert_allclose(af, r.q[t], rtol=RTOL, atol=ATOL, err_msg=what)
    np.testing.assert_allclose(ll[:, 0], want_ll[:, 0], rtol=0, atol=LL_ATOL, err_msg=what)
    np.testing.assert_allclose(ll[~dead, 1], want_ll[~dead, 1], rtol=0, atol=LL_ATOL, err_msg=what)
    assert np.all(ll[dead, 1] == -np.inf), what


def batch(name, seed=0):
    ped = pedigree(name)
    rng = np.random.RandomState(300 + 7 * ped.n + seed)
    lk, flags = clear_likelihoods(rng, ped, N_SITES)  # flags 0..3 mixed
    assert {0, 1, 2, 3} <= set(flags.tolist())
    return ped, lk, flags, rng.uniform(0.01, 0.9, N_SITES)


PED_STEPS = [("random0", 8), ("random1", 8), ("random2", 8), ("random%d" % TWO_CUT_SEED, 8), ("wide24", 3), ("wide48", 3)]


@pytest.mark.parametrize("name,steps", PED_STEPS)
def test_the_kernel_matches_the_reference(name, steps, tmp_path):
    ped, lk, flags, af0 = batch(name)
    fn, plan, src = build_af_host(fs.make_model(ped), tmp_path)
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= 40)  # the lean form from forty members on
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", plan["af_variant"], prior=True)[0]
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        r = A.reference(ped, mrate, lk, flags, af0, steps)
        outs = {}
        for t in (0, 1, steps):
            outs[t] = run_af(fn, model, lk, flags, af0, t)
            check(outs[t], r, t, "%s mrate %g" % (name, mrate))
        # no steps: the start value's bits, and famseq_evidence_prior's loglik and status on hwe_priors(af0), bit for bit
        assert same_bits([outs[0][0]], [af0])
        e_ll, _, e_st = run_evidence(ev, model, lk, flags, fs.hwe_priors(af0))
        assert np.array_equal(outs[0][2], e_st)
        np.testing.assert_allclose(outs[0][1][:, 0], e_ll, rtol=0, atol=LL_ATOL)
        assert same_bits([np.ascontiguousarray(outs[0][1][:, 0])], [e_ll])


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_the_likelihood_never_decreases_and_calls_chain(name, tmp_path):
    """On the kernel's own outputs: loglik[0] after t + 1 steps >= after t steps (EM's guarantee, within the comparison's own
    tolerance).  Three steps, then five from their result, are the bits of eight; no steps return af0's bits."""
    ped, lk, flags, af0 = batch(name, 1)
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_af_host(model, tmp_path)[0]
    outs = [run_af(fn, model, lk, flags, af0, t) for t in range(9)]
    assert all(np.all(o[2] == 0) for o in outs)
    for t in range(8):
        gain = outs[t + 1][1][:, 0] - outs[t][1][:, 0]
        assert np.all(gain >= -1e-9), (t, gain.min())
        assert same_bits([outs[t + 1][1][:, 1]], [outs[t][1][:, 1]])  # (log10 Z(0) does not depend on the steps)
    print("%s: smallest gain of a step %.3g, total gain %.3g .. %.3g" % (
        name, min((outs[t + 1][1][:, 0] - outs[t][1][:, 0]).min() for t in range(8)),
        (outs[8][1][:, 0] - outs[0][1][:, 0]).min(), (outs[8][1][:, 0] - outs[0][1][:, 0]).max()))
    assert same_bits([outs[0][0]], [af0])
    three = outs[3]
    assert same_bits(run_af(fn, model, lk, flags, three[0], 5), outs[8])
    assert same_bits(run_af(fn, model, lk, flags, outs[8][0], 0), outs[8])


@pytest.mark.parametrize("name", ["random1", "random0", "wide48"])  # loop-free, looped, lean
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped, lk, flags, af0 = batch(name, 2)
    assert (fs.Context(fs.make_model(ped), device=-1).plan()["elim_conditioned_members"] > 0) == (name == "random0")
    model = fs.make_model(ped, mrate=1e-4)
    outs = [run_af(build_af_host(model, tmp_path, v)[0], model, lk, flags, af0, 4) for v in range(N_VARIANTS)]
    assert np.all(outs[0][2] == 0)
    for out in outs[1:]:
        assert same_bits(out, outs[0])


def males_and_mother():
    """Three male founders and one mother: (f1 x m) -> a son and a daughter, who marry the other two founders' line: every
    founder but one is male, so a chrX site counts 2 + 3 chromosomes where an autosomal one counts 8."""
    ids, mids, fids = [1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 0, 2, 2, 6], [0, 0, 0, 0, 1, 1, 3]
    ped = fs.Pedigree(ids, mids, fids, [1, 2, 1, 1, 1, 2, 1], ["s%d" % i for i in ids])
    ped.relations()
    return ped


def test_chrx_counts_one_chromosome_per_male_founder(tmp_path):
    ped = males_and_mother()
    assert [ped.genders[f] for f in A.founders_of(ped)] == [1, 2, 1, 1]
    rng = np.random.RandomState(5)
    lk, _ = clear_likelihoods(rng, ped, N_SITES)
    flags = np.where(np.arange(N_SITES) % 2 == 0, 2, 0).astype(np.uint8)
    af0 = rng.uniform(0.01, 0.9, N_SITES)
    model = fs.make_model(ped)
    fn = build_af_host(model, tmp_path)[0]
    r = A.reference(ped, 1e-7, lk, flags, af0, 4)
    for t in (0, 1, 4):
        check(run_af(fn, model, lk, flags, af0, t), r, t, "males and mother")
    # a lone trio by hand: father (male founder), mother, son, one step from q on chrX.  The founders are independent given the
    # son's row summed out: m_fa(g) = pm(g) l_fa(g) sum_{gm, gc} pa(gm) l_mo(gm) T(gc | gm, g) l_c(gc), likewise the mother's
    trio = pedigree("trio")
    mo, fa = trio.relations()
    c = [p for p in range(3) if mo[p] >= 0][0]
    m_, f_ = int(mo[c]), int(fa[c])
    assert trio.genders[f_] == 1 and trio.genders[m_] == 2
    tlk, _ = clear_likelihoods(np.random.RandomState(6), trio, 8)
    q = np.linspace(0.05, 0.8, 8)
    table = np.asarray(fs.transmission_tables(1e-7)[2 if trio.genders[c] == 1 else 1], float).reshape(3, 3, 3)  # [gc, gm, gf] on chrX
    pa, pm = np.stack([(1 - q) ** 2, 2 * q * (1 - q), q * q], 1), np.stack([1 - q, 0 * q, q], 1)
    w = np.einsum("sm,sf,cmf,sc->smf", pa * tlk[:, m_], pm * tlk[:, f_], table, tlk[:, c])
    m_mo, m_fa = w.sum(axis=2), w.sum(axis=1)
    want = np.minimum(((m_mo[:, 1] + 2 * m_mo[:, 2]) / m_mo.sum(1) + m_fa[:, 2] / m_fa.sum(1)) / 3.0, 1.0)
    tmodel = fs.make_model(trio)
    got = run_af(build_af_host(tmodel, tmp_path / "trio")[0], tmodel, tlk, np.full(8, 2, np.uint8), q, 1)
    assert np.all(got[2] == 0)
    np.testing.assert_allclose(got[0], want, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[0], A.step(trio, 1e-7, tlk, np.full(8, 2, np.uint8), q), rtol=RTOL, atol=0)


def test_planted_sites(tmp_path):
    """On the quad.  An all-zero likelihood row: status 1.  The quad_mu0 shape (both parents hom-ref for certain, a child hom-alt
    for certain, mutation rate 0): status 2.  Every output of a failed site is NaN.  A founder whose row is (0, x, y) on an
    otherwise good site: the data exclude q = 0, loglik[1] is -inf, everything else is finite and the status 0.  A start value of
    1.5 given straight to the kernel: status 2."""
    ped = pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    founder = A.founders_of(ped)[0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 32)
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    lk[9] = (1.0, 0.0, 0.0)
    lk[9, child] = (0.0, 0.0, 1.0)
    lk[13, founder, 0] = 0.0
    af0 = np.full(32, 0.3)
    af0[20] = 1.5
    af0[21] = np.nan
    af0[22] = -0.25
    model = fs.make_model(ped, mrate=0.0)
    bad = [5, 9, 20, 21, 22]
    good = np.delete(np.arange(32), bad)
    for variant in (0, 3):
        fn = build_af_host(model, tmp_path, variant)[0]
        for t in (0, 3):
            af, ll, st = run_af(fn, model, lk, flags, af0, t)
            assert st[5] == 1 and st[9] == 2 and st[20] == 2 and st[21] == 2 and st[22] == 2 and np.all(st[good] == 0)
            assert np.all(np.isnan(af[bad])) and np.all(np.isnan(ll[bad]))
            assert np.all(np.isfinite(af[good])) and np.all(np.isfinite(ll[good, 0]))
            assert ll[13, 1] == -np.inf and np.all(np.isfinite(np.delete(ll[good, 1], list(good).index(13))))
    # the good sites against the reference, the planted -inf among them
    r = A.reference(ped, 0.0, lk[good], flags[good], af0[good], 3)
    assert r.z0[list(good).index(13)] == 0.0
    check(run_af(fn, model, lk[good], flags[good], af0[good], 3), r, 3, "quad, planted sites")
    # a total weight that is not finite fails the site too
    big = np.full((2, ped.n, 3), 1e160)
    af, ll, st = run_af(fn, model, big, np.zeros(2, np.uint8), 0.3, 2)
    assert np.all(st == 2) and np.all(np.isnan(af)) and np.all(np.isnan(ll))


def test_each_output_may_be_null(tmp_path):
    ped, lk, flags, af0 = batch("random1", 4)
    model = fs.make_model(ped)
    fn = build_af_host(model, tmp_path)[0]
    full = run_af(fn, model, lk, flags, af0, 2)
    for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
        got = run_af(fn, model, lk, flags, af0, 2, want=want)
        untouched = (np.full(N_SITES, -5.0), np.full((N_SITES, 2), -5.0), np.full(N_SITES, 77, np.uint8))
        for k in range(3):
            assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


def test_boundary_start_values(tmp_path):
    """af0 exactly 0 and exactly 1 are legal and are fixed points of the step: every founder is hom-ref (hom-alt) for certain."""
    ped, lk, flags, _ = batch("random1", 5)
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_af_host(model, tmp_path)[0]
    for q in (0.0, 1.0):
        r = A.reference(ped, 1e-4, lk, flags, np.full(N_SITES, q), 0)
        for t in (0, 1, 5):
            af, ll, st = run_af(fn, model, lk, flags, q, t)
            assert np.all(st == 0) and np.all(af == q)
            np.testing.assert_allclose(ll, A.loglik(r, 0), rtol=0, atol=LL_ATOL)
        if q == 0.0:
            assert same_bits([np.ascontiguousarray(ll[:, 0])], [np.ascontiguousarray(ll[:, 1])])


def test_generating_the_af_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new body and the shell's new field must not reach the text of the existing kernels (cached by content hash)."""
    ped = pedigree("random0")
    assert fs.Context(fs.make_model(ped), device=-1).plan()["elim_conditioned_members"] > 0  # (a pedigree with a loop)
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    stems = ("map", "map_prior", "evidence", "evidence_prior", "loo", "loo_prior", "pattern", "pattern_prior", "sample", "sample_prior", "prior")
    keys = ("elim_code_object", "trio_code_object") + tuple(s + "_code_object" for s in stems)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        for stem in stems:
            ctx.set_option(stem + "_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        ctx.set_option("af_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["af_code_object"].endswith(".hsaco") and after["af_code_object"] not in [before[k] for k in keys]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*founder allele frequency \(sum-product engine\).*more than three"):
        ctx.set_option("af_kernels", 1)
    ctx.close()
    ped = pedigree("random0")
    ones = np.ones((3, ped.n, 3))
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["af_code_object"] == "" and plan["af_variant"] == -1
        assert not [k for k in plan if k.startswith("af_prior")]  # the prior is the unknown: no such form, no such name
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("af_kernels", 2)
        with pytest.raises(fs.FamseqError, match="unknown option af_prior_kernels"):
            ctx.set_option("af_prior_kernels", 1)
        assert not hasattr(fs.lib(), "famseq_af_prior_batch")
        ctx.set_option("af_kernels", 1)
        plan = ctx.plan()
        assert plan["af_code_object"].endswith(".hsaco") and 0 <= plan["af_variant"] < N_VARIANTS
        assert plan["evidence_code_object"] == "" and plan["evidence_prior_code_object"] == ""
        # the ABI's refusals come before the device is asked for, so a context without one gives them too
        for n_iter in (-1, 65):
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_iter must be 0\.\.64, got %d" % n_iter):
                ctx.af_batch(0.5, n_iter, lk=ones)
            rc = fs.lib().famseq_af_batch_device(ctx._h, 3, None, None, None, 0, None, None, n_iter, None, None, None, None)
            assert rc == -1 and "n_iter must be 0..64" in fs.lib().famseq_last_error(ctx._h).decode()
        for fn, tail in (("famseq_af_batch", ()), ("famseq_af_batch_device", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 3, None, None, None, 0, None, None, 4, None, None, None, *tail)
            assert rc == -1 and "af0 must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        for bad in (np.nan, 1.5, -0.1, np.inf):
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*af0 entries must be finite numbers in \[0, 1\] \(site 1\)"):
                ctx.af_batch([0.5, bad, 2.0], 4, lk=ones)
        with pytest.raises(ValueError, match="one value per site"):
            ctx.af_batch([0.5, 0.5], 4, lk=ones)
        for af0 in (0.5, [0.0, 1.0, 0.5]):
            with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
                ctx.af_batch(af0, 4, lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.af_batch_device(3, 1 << 20, 4, d_lk=1 << 21)
        ctx.close()
