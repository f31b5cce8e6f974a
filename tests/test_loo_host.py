"""The leave-one-out kernel's arithmetic (famseq_loo / famseq_loo_prior: every member's genotype distribution given every row
but its own, and the predictive likelihood fit = Z / Z_-p of its own row), checked without a GPU.

As in test_evidence_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled
with g++.  Reference: tests/_loo.py, a numpy bucket elimination over factors in which member p's likelihood is masked to ones
(one elimination per member), pinned once to the compiled per-site oracle.

Tolerances (the project's, not measured): loo and fit at rtol 1e-9 with atol 0, so that a reference entry of exactly 0 (a male
founder's het prior at a chrX site, a mutation-free transmission zero at mutation rate 0) must be exactly 0; status exact; failed
sites NaN; bits wherever two routes have to agree.  No site is left out of a comparison: on the clear batches used here (every
member sequenced, PLs uniform in [0, 30)) the reference has status 0 and Z and every Z_-p >= 1e-200, which each test asserts on
the reference alone (_loo.check).  That floor holds at 48 and at 64 members with the same PL range (asserted there as well).
"""
import ctypes as C
import hashlib
import os
import re
import subprocess
from unittest import mock

import numpy as np
import pytest

import _loo as L
import _prior as P
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from test_generated_host import build_host_kernel, factor_tables, host_source, misaligned, run_host
from test_map_host import clear_likelihoods

RTOL = L.RTOL
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kLooVariants
SENTINEL, ST_SENTINEL = -5.0, 77


def build_loo_host(model, where, variant=None, prior=False):
    """Generate famseq_loo (prior: famseq_loo_prior) for a one-lane workgroup on a plan-only context, compile it for the host.
    -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("loo_prior", "famseq_loo_prior") if prior else ("loo", "famseq_loo")
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


def run_loo(fn, model, lk, flags, prior=None, want=(True, True, True), misalign_prior=False):
    """-> (loo, fit, status); an output that is not wanted is passed as NULL and comes back as its sentinels."""
    s, n = lk.shape[0], lk.shape[1]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    loo, fit, st = np.full((s, n, 3), SENTINEL), np.full((s, n), SENTINEL), np.full(s, ST_SENTINEL, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, loo.ctypes.data if want[0] else None, fit.ctypes.data if want[1] else None,
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
    return loo, fit, st


def cycled(lk):
    """Flags 0..3 in turn."""
    return (np.arange(len(lk)) % 4).astype(np.uint8)


def bits(out):
    return [np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint8) for x in out]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def cut_members(src):
    """The members the generated source conditions on (the assignments of its cut loop)."""
    return [int(x) for x in re.findall(r"const int a(\d+) = \(as_ / ", src)]


# random_pedigree seeds: 0 has one loop (a conditioned founder), 36 one loop (a conditioned child), 15 three conditioned members
# (two founders and a child); each is asserted where its kernel is generated
LOOP_SEEDS = {"loop": 0, "loopchild": 36, "loop3": 15}
PED_NAMES = ("trio", "quad", "ped10", "loop", "loopchild", "loop3", "two", "lone", "wide32", "wide48", "wide64")
_PEDS = {}


def pedigree(name):
    if name not in _PEDS:
        if name in LOOP_SEEDS:
            ped = random_pedigree(LOOP_SEEDS[name])[1]
        elif name == "two":  # two components with a family each: each carries the 1e7 of its own
            ped = fs.Pedigree([1, 2, 3, 4, 5, 6, 7], [0, 0, 2, 0, 0, 5, 5], [0, 0, 1, 0, 0, 4, 4], [1, 2, 2, 1, 2, 1, 2], list("abcdefg"))
        elif name == "lone":  # a trio and a founder of no family: its cavity is its prior
            ped = fs.Pedigree([1, 2, 3, 4], [0, 0, 2, 0], [0, 0, 1, 0], [1, 2, 2, 1], list("abcd"))
        elif name.startswith("wide"):
            ped = wide_pedigree(int(name[4:]))
        else:
            ped = fs.synthetic_pedigree(name)
        ped.relations()
        _PEDS[name] = ped
    return _PEDS[name]


_REFS = {}


def reference(name, mrate, n_sites=60):
    """-> (lk, flags, _loo.analyse of them): one clear batch per pedigree, its reference computed once per mutation rate."""
    key = (name, mrate, n_sites)
    if key not in _REFS:
        ped = pedigree(name)
        lk, _ = clear_likelihoods(np.random.RandomState(40 + ped.n), ped, n_sites)
        flags = cycled(lk)
        _REFS[key] = (lk, flags, L.analyse(ped, mrate, lk, flags))
    return _REFS[key]


def check_source_shape(name, src):
    ped = pedigree(name)
    mo, _ = ped.relations()
    cut = cut_members(src)
    assert ("conditioned on" in src.splitlines()[0]) == (name in LOOP_SEEDS)
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= 40)  # the lean form
    assert "s_l[" not in src and "__shared__ double s_tc[432];" in src  # no LDS beyond the factor tables
    if name == "loop":
        assert len(cut) == 1 and mo[cut[0]] < 0
    if name == "loopchild":
        assert len(cut) == 1 and mo[cut[0]] >= 0
    if name == "loop3":
        assert len(cut) == 3 and any(mo[k] < 0 for k in cut) and any(mo[k] >= 0 for k in cut)


def test_the_helper_is_pinned_to_the_oracle():
    L.pinned()


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", PED_NAMES)
def test_every_variant_matches_the_reference(name, variant, tmp_path):
    L.pinned()
    ped = pedigree(name)
    fn, plan, src = build_loo_host(fs.make_model(ped), tmp_path, variant)
    check_source_shape(name, src)
    outs = []
    for mrate in MRATES:
        lk, flags, ref = reference(name, mrate)
        out = run_loo(fn, fs.make_model(ped, mrate=mrate), lk, flags)
        L.check(out, ref, "%s variant %d mrate %g" % (name, variant, mrate))
        assert np.abs(out[0].sum(axis=2) - 1.0).max() < 1e-12
        outs.append(out)
    assert not same_bits(outs[0][:2], outs[1][:2])  # (the mutation rate reaches the kernel)
    if name in ("trio", "quad", "lone"):  # mutation-free transmission zeros and the male founders' chrX het prior: exact zeros
        assert (outs[2][0] == 0).any()


@pytest.mark.parametrize("name", ["loop3", "ped10"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped = pedigree(name)
    model = fs.make_model(ped, mrate=1e-4)
    lk, flags, _ = reference(name, 1e-4)
    outs = [run_loo(build_loo_host(model, tmp_path, v)[0], model, lk, flags) for v in range(N_VARIANTS)]
    for out in outs[1:]:
        assert same_bits(out, outs[0])


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "loop3", "lone", "wide32"])
def test_the_posterior_is_loo_times_likelihood_over_fit(name, tmp_path, monkeypatch):
    """post = loo * lk / fit against famseq_elim's own host build (lc = 2: no site takes the -LRC shortcut), at 1e-9."""
    ped = pedigree(name)
    model = fs.make_model(ped)
    lk, flags, ref = reference(name, 1e-7)
    assert L.is_clear(ref)
    loo, fit, st = run_loo(build_loo_host(model, tmp_path / "loo")[0], model, lk, flags)
    post, _, pst = run_host(build_host_kernel(model, "elim", tmp_path, monkeypatch), model, lk, flags, lc=2.0)
    assert np.all(st == 0) and np.all(pst == 0)
    np.testing.assert_allclose(loo * lk / fit[:, :, None], post, rtol=RTOL, atol=0)
    np.testing.assert_allclose((loo * lk).sum(axis=2), fit, rtol=1e-12, atol=0)  # fit is the row's product with the likelihood


@pytest.mark.parametrize("name", ["quad", "loop3"])
def test_a_member_without_reads_has_its_marginal(name, tmp_path, monkeypatch):
    """A row of all ones: loo is that member's posterior and fit is 1."""
    ped = pedigree(name)
    model = fs.make_model(ped)
    lk, flags, _ = reference(name, 1e-7)
    lk = lk.copy()
    who = np.arange(len(lk)) % ped.n
    lk[np.arange(len(lk)), who] = 1.0
    loo, fit, st = run_loo(build_loo_host(model, tmp_path / "loo")[0], model, lk, flags)
    post, _, pst = run_host(build_host_kernel(model, "elim", tmp_path, monkeypatch), model, lk, flags, lc=2.0)
    assert np.all(st == 0) and np.all(pst == 0)
    rows = np.arange(len(lk))
    np.testing.assert_allclose(loo[rows, who], post[rows, who], rtol=RTOL, atol=0)
    np.testing.assert_allclose(fit[rows, who], 1.0, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "loop3", "lone", "wide48"])
def test_site_prior_form(name, tmp_path):
    """Under the model's rows the plain form's bits; under Hardy-Weinberg rows the reference's numbers (tests/_prior_joint.py's
    factors); the same bits from a prior array that is 16-byte aligned and from one that is only 8-byte aligned."""
    ped = pedigree(name)
    lk, flags, _ = reference(name, 1e-7)
    hwe = fs.hwe_priors(np.random.RandomState(7 + ped.n).uniform(0.01, 0.5, len(lk)))
    for variant in (0, 2):
        plain = build_loo_host(fs.make_model(ped), tmp_path / "plain", variant)[0]
        fn, _, src = build_loo_host(fs.make_model(ped), tmp_path / "prior", variant, prior=True)
        assert "PRIOR_LOAD(site);" in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src and "= tcf[0]" not in src
        for mrate in MRATES:
            model = fs.make_model(ped, mrate=mrate)
            want = run_loo(plain, model, lk, flags)
            assert np.all(want[2] == 0)
            assert same_bits(run_loo(fn, model, lk, flags, P.model_rows(model, flags)), want)
            got = run_loo(fn, model, lk, flags, hwe)
            L.check(got, L.analyse(ped, mrate, lk, flags, hwe), "%s variant %d mrate %g, HWE rows" % (name, variant, mrate))
            assert same_bits(run_loo(fn, model, lk, flags, hwe, misalign_prior=True), got)
            assert not same_bits(got[:2], want[:2])


def test_each_output_may_be_null(tmp_path):
    ped = pedigree("ped10")
    model = fs.make_model(ped)
    lk, flags, _ = reference("ped10", 1e-7)
    n = len(lk)
    for prior in (None, P.model_rows(model, flags)):
        fn = build_loo_host(model, tmp_path, prior=prior is not None)[0]
        full = run_loo(fn, model, lk, flags, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = run_loo(fn, model, lk, flags, prior, want=want)
            untouched = (np.full((n, ped.n, 3), SENTINEL), np.full((n, ped.n), SENTINEL), np.full(n, ST_SENTINEL, np.uint8))
            for k in range(3):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


@pytest.mark.parametrize("name", ["trio", "quad"])
def test_planted_cases(name, tmp_path):
    """At mutation rate 0, rows that are certain (one 1, two exact 0):
      site 3: parents 0/0 and 0/0, a child 0/1: the total weight is 0, yet every cavity row is positive: status 0, every fit
              exactly 0.0 (each member's reads are impossible given the others), the loo rows finite and summing to 1.  That is
              the trio's answer; in a quad the second child is left with three relatives who contradict one another, its
              cavity row has no weight and the site has status 2;
      site 5: parents 0/0, a child 1/1: the mother's cavity row has no weight at all: status 2, all outputs NaN;
      site 7: a member's row all zero: status 1;
      site 9: a single exact 0 in an otherwise clear site, where the cavity is positive: status 0 and a positive loo entry at
              that genotype (a kernel that divided the marginal by the likelihood would give NaN or 0 there)."""
    ped = pedigree(name)
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 12)
    flags = np.zeros(12, np.uint8)
    for site, row in ((3, (0.0, 1.0, 0.0)), (5, (0.0, 0.0, 1.0))):
        lk[site] = 1.0  # (a quad's other child has no reads there)
        lk[site, [mo[child], fa[child]]] = (1.0, 0.0, 0.0)
        lk[site, child] = row
    lk[7, 1, :] = 0.0
    lk[9, child, 1] = 0.0
    lk[9, mo[child], 0] = 0.0
    ref = L.analyse(ped, 0.0, lk, flags)
    planted = [0 if ped.n == 3 else 2, 2, 1, 0]
    assert list(ref.status[[3, 5, 7, 9]]) == planted and np.all(np.delete(ref.status, [3, 5, 7]) == 0)
    assert ref.z[3] == 0 and ref.loo[9, child, 1] > 0 and ref.loo[9, mo[child], 0] > 0
    assert ped.n > 3 or np.all(ref.fit[3] == 0)
    model = fs.make_model(ped, mrate=0.0)
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = build_loo_host(model, tmp_path, variant, prior=prior is not None)[0]
            loo, fit, st = out = run_loo(fn, model, lk, flags, prior)
            L.check(out, ref, "planted cases", clear=False)
            assert list(st[[3, 5, 7, 9]]) == planted
            if ped.n == 3:
                assert np.all(fit[3] == 0.0) and np.all(np.isfinite(loo[3])) and np.abs(loo[3].sum(axis=1) - 1.0).max() < 1e-12
            assert np.all(np.isnan(loo[[5, 7]])) and np.all(np.isnan(fit[[5, 7]]))
            assert loo[9, child, 1] > 0 and loo[9, mo[child], 0] > 0 and np.all(fit[9] > 0)
    # a cavity row that is not finite fails the site too
    big = np.full((2, ped.n, 3), 1e160)
    loo, fit, st = run_loo(build_loo_host(model, tmp_path, 0)[0], model, big, np.zeros(2, np.uint8))
    assert np.all(st == 2) and np.all(np.isnan(loo)) and np.all(np.isnan(fit))


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("loo_kernels", "loo_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*leave-one-out posteriors \(sum-product engine\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = pedigree("ped10")
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["loo_code_object"] == "" and plan["loo_variant"] == -1
        assert plan["loo_prior_code_object"] == "" and plan["loo_prior_variant"] == -1
        assert plan["loo_block_threads"] == plan["evidence_block_threads"] >= 2
        with pytest.raises(fs.FamseqError, match="loo_kernels takes 1"):
            ctx.set_option("loo_kernels", 2)
        ctx.set_option("loo_kernels", 1)
        ctx.set_option("loo_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["loo_code_object"].endswith(".hsaco") and 0 <= plan["loo_variant"] < N_VARIANTS
        assert plan["loo_prior_code_object"].endswith(".hsaco") and plan["loo_prior_variant"] == plan["loo_variant"]
        assert plan["loo_prior_code_object"] != plan["loo_code_object"] and plan["evidence_code_object"] == ""
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.loo_batch(lk=np.ones((1, ped.n, 3)))
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.loo_prior_batch(np.ones((1, 6)), lk=np.ones((1, ped.n, 3)))
        ctx.close()


# ped10's variant-0 sources on the commit before famseq_loo came (SHA-256 of the text)
PARENT_SOURCES = {
    "elim_code_object": "2815921a548f058f0bfbfb537cc663c118e2d5e03cfa9835fd17a298c6fe791c",
    "prior_code_object": "4c416a620340f98297aaa26b054cf506cc8a80913f5e560b6f8d19c2058cd35f",
    "trio_code_object": "1b3a896ace6d5fcad0e48daab53d3519f2717057c5fb9966f12b7fc870d86937",
    "map_code_object": "03782464451372a4dce145731bc6a61c2cc2bd47a268835eee4e25fe05a8b582",
    "evidence_code_object": "a79fadc2fb1e11b6ede7202f7fd14054972b70959b346c5c65d2b7d18997a7f4",
}


def test_the_other_kernels_sources_are_the_parents(tmp_path):
    """With loo_source unused and used, every existing kernel's text is what it was: elim, prior, trio (dnm + joint), map and
    evidence of ped10 in variant 0, by hash; generating the new kernel moves none of them."""
    ped = pedigree("ped10")
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1", FAMSEQ_VARIANT_ONLY="0")
    digest = lambda path: hashlib.sha256(open(path[:-6] + ".hip", "rb").read()).hexdigest()
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        for opt, v in (("engine", fs.ENGINE_ELIM), ("prior_kernels", 1), ("trio_kernels", 3), ("map_kernels", 1), ("evidence_kernels", 1)):
            ctx.set_option(opt, v)
        before = ctx.plan()
        assert {k: digest(before[k]) for k in PARENT_SOURCES} == PARENT_SOURCES
        ctx.set_option("loo_kernels", 1)
        ctx.set_option("loo_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    assert {k: digest(after[k]) for k in PARENT_SOURCES} == PARENT_SOURCES
    assert all(before[k] == after[k] for k in PARENT_SOURCES)
    assert after["loo_code_object"] not in [after[k] for k in PARENT_SOURCES]


# ---- the four entries' argument checks, on plan-only contexts (in the manner of test_side_entries_host.py) ---------------------

E_ARG, E_NODEVICE = -1, -2
ONE_OF = b"exactly one of lk / pl16 must be given"
D_PRIOR = b"d_prior must be given (six doubles per site)"
NO_DEVICE = b"context was created without a device; there is no CPU path"
ENTRIES = [(prior, device) for prior in (False, True) for device in (False, True)]


def call(ctx, entry, n_sites=1, lk=True, pl16=False, prior=True):
    """-> (return code, famseq_last_error) of one entry on arrays for one site; lk / pl16 / prior False: that pointer NULL."""
    site_prior, device = entry
    fn = getattr(fs.lib(), "famseq_loo%s_batch%s" % ("_prior" if site_prior else "", "_device" if device else ""))
    n = ctx.n
    args = [np.ones((1, n, 3)) if lk else None, np.zeros((1, n, 3), np.uint16) if pl16 else None, np.arange(n, dtype=np.int32), n,
            np.zeros(1, np.uint8)]
    if site_prior:
        args.append(np.full((1, 6), 0.25) if prior else None)
    args += [np.zeros(3 * n), np.zeros(n), np.zeros(1, np.uint8)]
    args = [ctx._h, n_sites] + args + ([None] if device else [])
    assert len(args) == len(fn.argtypes)
    keep = [a for a in args if isinstance(a, np.ndarray)]  # (alive over the call)
    rc = fn(*[a.ctypes.data_as(t) if isinstance(a, np.ndarray) else a for a, t in zip(args, fn.argtypes)])
    del keep
    return rc, fs.lib().famseq_last_error(ctx._h)


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: "loo%s%s" % ("_prior" if e[0] else "", "_device" if e[1] else ""))
def test_argument_checks_in_their_order(entry):
    site_prior, device = entry
    ctx = fs.Context(fs.make_model(fs.synthetic_pedigree("trio")), device=-1)
    first = D_PRIOR if device else ONE_OF
    assert call(ctx, entry, lk=False, pl16=False) == (E_ARG, ONE_OF)
    assert call(ctx, entry, lk=True, pl16=True) == (E_ARG, ONE_OF)
    if site_prior:
        assert call(ctx, entry, lk=False, pl16=False, prior=False) == (E_ARG, first)
        no_prior = (E_ARG, D_PRIOR) if device else (E_NODEVICE, NO_DEVICE)
        assert call(ctx, entry, prior=False) == no_prior
        assert call(ctx, entry, lk=False, pl16=True, prior=False) == no_prior
    assert call(ctx, entry) == (E_NODEVICE, NO_DEVICE)
    assert call(ctx, entry, lk=False, pl16=True) == (E_NODEVICE, NO_DEVICE)
    assert call(ctx, entry, n_sites=0) == (E_NODEVICE, NO_DEVICE)
    assert call(ctx, entry, n_sites=-1) == (E_ARG, ONE_OF)
    ctx.close()
    fn = getattr(fs.lib(), "famseq_loo%s_batch%s" % ("_prior" if site_prior else "", "_device" if device else ""))
    assert fn(None, 1, *[None if t is not C.c_int32 else 0 for t in fn.argtypes[2:]]) == E_ARG


def famseq_binary():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "FamSeq")


def test_cli_refuses_loo_with_aftag(tmp_path):
    """-loo with -afTag: one output line must not mix two models (the message -dnm / -map get); said before any device is
    touched.  -h lists the flag."""
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testdata")
    r = subprocess.run([famseq_binary(), "vcf", "-vcfFile", os.path.join(data, "test_subset.vcf"), "-pedFile", os.path.join(data, "fam01.ped"),
                        "-output", str(tmp_path / "o.vcf"), "-loo", "-afTag", "AF"], capture_output=True, text=True)
    assert r.returncode == 255
    assert "-afTag cannot be combined with -dnm or -map" in r.stdout
    assert not (tmp_path / "o.vcf").exists()
    r = subprocess.run([famseq_binary(), "-h"], capture_output=True, text=True)
    assert "-loo\t" in r.stdout + r.stderr
