"""The mutation-rate kernel's arithmetic (famseq_mutrate / famseq_mutrate_prior: per site and rate r the log10 of the network's
total weight Z_r with the children's transmission entries taken from the factor table of rate r, and the site's own log10
likelihood), checked without a GPU.

As in test_relabel_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled
with g++ -ffp-contract=off.  References: test_pattern_host._total(ped, rate_r, lk, flags, prior) — tests/_maxproduct.py's Z, under
per-site priors tests/_prior_joint.py's factors through the same elimination — and up to ten members also the 3^N enumeration
of test_map_host.brute_weights.

Wanted: status exact (the rows as given and the context's own Z decide it); rate_loglik and loglik at an ABSOLUTE 1e-9
(test_evidence_host's derivation: a relative 1e-9 on Z is 4.3e-10 in log10); -inf exactly where the reference's Z_r is exactly 0;
and the bit contracts of include/famseq_hip.h against the host-compiled famseq_evidence of the same variant fed the factor
tables of a model made at rates[r]: rate_loglik[s][r] is that kernel's loglik wherever it has status 0, the model's own rate
gives loglik's bits, loglik is famseq_evidence's under the model's tables, a column depends neither on n_rates nor on the other
rates, equal rates give equal bits, the prior form on the model's rows gives the plain form's bits.

No site is left out of a comparison: every batch asserts, on the reference alone and before the kernel runs, status 0 everywhere
except the planted failures and Z and every non-zero Z_r >= 1e-200.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from test_evidence_host import build_evidence_host, run_evidence
from test_generated_host import factor_tables, host_source
from test_map_host import brute_weights, clear_likelihoods
from test_pattern_host import _total, pedigree, same_bits

LL_ATOL = 1e-9  # absolute, on log10 Z (see the module's docstring)
MRATES = [1e-7, 1e-4, 0.0]  # the rates the model is made with
N_VARIANTS = 4  # kMutrateVariants
FLOOR = 1e-200
N_SITES = 64
PED_NAMES = ["random0", "random1", "random2", "random3", "random99", "wide24", "wide48"]  # random99: two conditioned members


def grid(mrate):
    return np.array([0.0, 1e-9, 1e-7, mrate, 1e-3, 0.5, 1.0])


def build_mutrate_host(model, where, variant=None, prior=False):
    """Generate famseq_mutrate (prior: famseq_mutrate_prior) for a one-lane workgroup on a plan-only context, compile it for the
    host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("mutrate_prior", "famseq_mutrate_prior") if prior else ("mutrate", "famseq_mutrate")
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


def tables_of(model, rates):
    """famseq_rate_tables on a plan-only context of the model: [R, 432]."""
    ctx = fs.Context(model, device=-1)
    t = ctx.rate_tables(rates)
    ctx.close()
    return t


def run_mutrate(fn, model, lk, flags, rates, prior=None, want=(True, True, True), tables=None):
    s, r = lk.shape[0], len(rates)
    a = np.ascontiguousarray(lk, dtype=np.float64)
    rl, ll, st = np.full((s, r), -5.0), np.full(s, -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    rt = np.ascontiguousarray(tables_of(model, rates) if tables is None else tables)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, rl.ctypes.data if want[0] else None, ll.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, rt.ctypes.data, r]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return rl, ll, st


def reference(ped, mrate, lk, flags, rates, prior=None, brute=True):
    """-> (z[S], zr[S, R], status[S]): the total weight at the model's rate, at every rate of the grid (all with the reference's
    1e7), and the status.  Up to ten members (brute) the 3^N enumeration is checked against the elimination here."""
    z, fail = _total(ped, mrate, lk, flags, prior)
    zr = np.stack([_total(ped, r, lk, flags, prior)[0] for r in rates], axis=1)
    if brute and ped.n <= 10 and prior is None:
        for j, r in enumerate(rates):
            _, W, bst = brute_weights(ped, float(r), lk, flags)
            W = np.where(bst != 0, 0.0, np.nansum(W, axis=1))  # (its NaN rows: a row times its prior all zeros, or a total of 0)
            assert np.array_equal(W == 0, zr[:, j] == 0)
            np.testing.assert_allclose(zr[:, j], W, rtol=1e-12, atol=0)
    st = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    return z, zr, st


def clear(ref, what="", planted=()):
    """On the reference alone: nothing is left out of a comparison."""
    z, zr, st = ref
    ok = np.ones(len(z), bool)
    ok[list(planted)] = False
    assert np.all(st[ok] == 0) and np.all(st[~ok] != 0), what
    assert np.all(z[ok] >= FLOOR) and np.all((zr[ok] == 0) | (zr[ok] >= FLOOR)), what


def check(out, ref, what=""):
    """The module docstring's rules; every site and rate compared.  Prints the worst errors before it asserts."""
    rl, ll, st = out
    z, zr, ref_st = ref
    assert np.array_equal(st, ref_st), what
    ok = ref_st == 0
    assert np.all(np.isnan(ll[~ok])) and np.all(np.isnan(rl[~ok])), what
    zero = zr[ok] == 0
    with np.errstate(divide="ignore"):
        want = np.log10(zr[ok]) - 7.0
    got = rl[ok]
    err_r = np.abs(got[~zero] - want[~zero])
    err = np.abs(ll[ok] - (np.log10(z[ok]) - 7.0))
    print("%s: %d sites x %d rates, %d exact zeros, worst |rate_loglik error| %.3g, worst |loglik error| %.3g, smallest Z %.3g, "
          "smallest non-zero Z_r %.3g" % (what, ok.sum(), zr.shape[1], zero.sum(), err_r.max(initial=0), err.max(initial=0),
                                          z[ok].min(initial=1), zr[ok][~zero].min(initial=1)))
    assert np.array_equal(np.isneginf(got), zero), what
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=0, atol=LL_ATOL, err_msg=what)
    np.testing.assert_allclose(ll[ok], np.log10(z[ok]) - 7.0, rtol=0, atol=LL_ATOL, err_msg=what)


def evidence_bits(ev, ped, mrate, lk, flags, rates, out, prior=None):
    """The bit contracts against the host-compiled famseq_evidence: loglik under the model's own tables, every column under the
    tables of a model made at that rate wherever that call has status 0 (where it has status 2 on a good site, Z_r is 0 and the
    column holds -inf).  -> the number of column entries compared bit for bit."""
    rl, ll, st = out
    e_ll, _, e_st = run_evidence(ev, fs.make_model(ped, mrate=mrate), lk, flags, prior)
    assert np.array_equal(st, e_st) and same_bits([ll], [e_ll])
    compared = 0
    for j, r in enumerate(rates):
        r_ll, _, r_st = run_evidence(ev, fs.make_model(ped, mrate=float(r)), lk, flags, prior)
        good = (r_st == 0) & (st == 0)
        assert same_bits([rl[good, j]], [r_ll[good]])
        assert np.all(np.isneginf(rl[(r_st == 2) & (st == 0), j]))
        compared += int(good.sum())
        if r == mrate:
            assert same_bits([rl[:, j]], [ll])
    return compared


def batch(name, seed=0):
    ped = pedigree(name)
    rng = np.random.RandomState(300 + 7 * ped.n + seed)  # (the relabel tests' rows)
    lk, flags = clear_likelihoods(rng, ped, N_SITES)  # flags 0..3 mixed
    return ped, lk, flags


@pytest.mark.parametrize("name", PED_NAMES)
def test_the_kernel_matches_the_reference(name, tmp_path):
    ped, lk, flags = batch(name)
    assert {0, 1, 2, 3} <= set(flags.tolist())
    refs = {mrate: reference(ped, mrate, lk, flags, grid(mrate)) for mrate in MRATES}
    for mrate in MRATES:
        clear(refs[mrate], "%s mrate %g" % (name, mrate))
    fn, plan, src = build_mutrate_host(fs.make_model(ped), tmp_path)
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= 40)  # the rows in registers below forty members, lean from there
    assert src.count("for (int ps_ = 0;") == 1 and src.count("const double Zp_") == 1  # the pass's text stands once
    assert "#pragma unroll 1\n      for (int ps_ = 0; ps_ <= last_; ++ps_)" in src
    assert "__shared__" in src and src.count("__shared__") == 1  # no LDS beyond famseq_evidence's factor tables
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", plan["mutrate_variant"])[0]
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        out = run_mutrate(fn, model, lk, flags, grid(mrate))
        check(out, refs[mrate], "%s mrate %g" % (name, mrate))
        assert evidence_bits(ev, ped, mrate, lk, flags, grid(mrate), out) > N_SITES  # (the model's own column alone gives that many)


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped, lk, flags = batch(name, 1)
    model = fs.make_model(ped, mrate=1e-4)
    outs, srcs = [], []
    for v in range(N_VARIANTS):
        fn, _, src = build_mutrate_host(model, tmp_path, v)
        outs.append(run_mutrate(fn, model, lk, flags, grid(1e-4)))
        srcs.append(src)
    # every variant reads a pass's entries through a wave-uniform pointer inside the chrX loop (variant 0 takes the loop as well)
    assert all("(pu_ - 1) * RTD) + x_ * 216;" in s and "tcx[" not in s for s in srcs)
    assert all("trt[" in s and "const int pu_ = __builtin_amdgcn_readfirstlane(ps_);" in s for s in srcs)
    assert np.all(outs[0][2] == 0)
    for out in outs[1:]:
        assert same_bits(out, outs[0])
    ev = build_evidence_host(model, tmp_path / "ev", 2)[0]
    assert evidence_bits(ev, ped, 1e-4, lk, flags, grid(1e-4), outs[2]) > N_SITES


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_site_prior_form(name, tmp_path):
    """Fed the model's rows: the plain form's bits.  Under Hardy-Weinberg rows: tests/_prior_joint.py's factors at every rate,
    and famseq_evidence_prior's bits."""
    ped, lk, flags = batch(name, 2)
    hwe = fs.hwe_priors(np.random.RandomState(3).uniform(0.01, 0.5, len(lk)))
    refs = {mrate: reference(ped, mrate, lk, flags, grid(mrate), hwe) for mrate in MRATES}
    for mrate in MRATES:
        clear(refs[mrate], "%s mrate %g, HWE rows" % (name, mrate))
    plain = build_mutrate_host(fs.make_model(ped), tmp_path / "plain", 1)[0]
    fn, _, src = build_mutrate_host(fs.make_model(ped), tmp_path / "prior", 1, prior=True)
    assert "PRIOR_LOAD(site);" in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src
    assert "int n_rates, const double *__restrict__ prior_g) {" in src  # the tables stand in front of the prior rows
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", 1, prior=True)[0]
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        want = run_mutrate(plain, model, lk, flags, grid(mrate))
        assert np.all(want[2] == 0)
        assert same_bits(run_mutrate(fn, model, lk, flags, grid(mrate), P.model_rows(model, flags)), want)
        out = run_mutrate(fn, model, lk, flags, grid(mrate), hwe)
        check(out, refs[mrate], "%s mrate %g, HWE rows" % (name, mrate))
        assert evidence_bits(ev, ped, mrate, lk, flags, grid(mrate), out, hwe) > 0


def test_a_mendel_impossible_trio_site(tmp_path):
    """Parents (1, 0, 0), child (0, 1, 0): rate 0 gives -inf, every positive rate a finite value, status 0 — also where the model
    itself is made at a positive rate (at a model rate of 0 the site's own Z is 0: status 2, everything NaN)."""
    ped = pedigree("trio")
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk = np.zeros((3, ped.n, 3))
    lk[:, :, 0] = 1.0
    lk[:2, child] = (0.0, 1.0, 0.0)  # sites 0, 1 impossible without a mutation; site 2 hom-ref throughout
    flags = np.zeros(3, np.uint8)
    rates = np.array([0.0, 1e-9, 1e-7, 1e-3, 0.5])  # (at rate 1 every allele mutates and a het child of hom-ref parents is impossible again)
    ref = reference(ped, 1e-7, lk, flags, rates)
    clear(ref)
    assert np.all(ref[1][:2, 0] == 0) and np.all(ref[1][:2, 1:] > 0) and np.all(ref[1][2] > 0)
    model = fs.make_model(ped, mrate=1e-7)
    for variant in range(N_VARIANTS):
        out = run_mutrate(build_mutrate_host(model, tmp_path, variant)[0], model, lk, flags, rates)
        check(out, ref, "Mendel-impossible trio, variant %d" % variant)
        assert np.all(np.isneginf(out[0][:2, 0])) and np.all(np.isfinite(out[0][:2, 1:])) and np.all(out[2] == 0)
        # the Bayes factor "the site needs a mutation" is +inf there and about 0 at the hom-ref site
        assert np.all(out[0][:2, 2] - out[0][:2, 0] == np.inf) and abs(out[0][2, 2] - out[0][2, 0]) < 1e-6
    zero = fs.make_model(ped, mrate=0.0)
    ref0 = reference(ped, 0.0, lk, flags, rates)
    clear(ref0, planted=(0, 1))
    out = run_mutrate(build_mutrate_host(zero, tmp_path)[0], zero, lk, flags, rates)
    check(out, ref0, "the same rows on a model made at rate 0")
    assert out[2].tolist() == [2, 2, 0] and np.all(np.isnan(out[0][:2])) and np.all(np.isnan(out[1][:2]))


def test_failure_statuses(tmp_path):
    """An all-zero likelihood row: status 1.  1e160 rows: status 2.  Every output of such a site is NaN."""
    ped = pedigree("quad")
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 32)
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    rates = grid(1e-4)
    model = fs.make_model(ped, mrate=1e-4)
    ref = reference(ped, 1e-4, lk, flags, rates)
    clear(ref, planted=(5,))
    assert ref[2][5] == 1
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = build_mutrate_host(model, tmp_path, variant, prior=prior is not None)[0]
            rl, ll, st = out = run_mutrate(fn, model, lk, flags, rates, prior)
            check(out, ref, "planted failure")
            assert st[5] == 1 and np.all(np.isnan(rl[5])) and np.isnan(ll[5])
            assert not np.any(np.isnan(np.delete(rl, 5, axis=0)))
    big = np.full((2, ped.n, 3), 1e160)
    rl, ll, st = run_mutrate(build_mutrate_host(model, tmp_path, 0)[0], model, big, np.zeros(2, np.uint8), rates)
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(rl))


def test_each_output_may_be_null(tmp_path):
    ped, lk, flags = batch("random1", 4)
    model = fs.make_model(ped)
    rates = grid(1e-7)
    for prior in (None, P.model_rows(model, flags)):
        fn = build_mutrate_host(model, tmp_path, prior=prior is not None)[0]
        full = run_mutrate(fn, model, lk, flags, rates, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = run_mutrate(fn, model, lk, flags, rates, prior, want=want)
            untouched = (np.full(full[0].shape, -5.0), np.full(N_SITES, -5.0), np.full(N_SITES, 77, np.uint8))
            for k in range(3):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


@pytest.mark.parametrize("name", ["random0", "wide48"])
def test_a_column_depends_on_its_own_rate_alone(name, tmp_path):
    """n_rates = 1, 2, 7 and FAMSEQ_MAX_RATES: a column's bits depend neither on how many others the call holds nor on what
    they are; equal rates give equal bits."""
    ped, lk, flags = batch(name, 5)
    rng = np.random.RandomState(6)
    seven = grid(1e-4)
    many = np.concatenate([seven, 10.0 ** rng.uniform(-10, 0, fs.MAX_RATES - len(seven) - 2), [1e-3, 1e-3]])
    assert len(many) == 32 == fs.MAX_RATES
    ref = reference(ped, 1e-4, lk, flags, many, brute=False)
    clear(ref)
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_mutrate_host(model, tmp_path)[0]
    out = run_mutrate(fn, model, lk, flags, many)
    check(out, ref, "%s, 32 rates" % name)
    assert same_bits([out[0][:, 4]], [out[0][:, 30]]) and same_bits([out[0][:, 30]], [out[0][:, 31]])  # 1e-3 three times
    assert same_bits([out[0][:, 3]], [out[1]])  # the model's own rate
    for r in (0, 2, 17, 31):
        one = run_mutrate(fn, model, lk, flags, many[r:r + 1])
        assert same_bits([one[0][:, 0], one[1], one[2]], [out[0][:, r], out[1], out[2]])
    two = run_mutrate(fn, model, lk, flags, many[[9, 0]])
    assert same_bits([two[0]], [out[0][:, [9, 0]]])
    assert same_bits([run_mutrate(fn, model, lk, flags, seven)[0]], [out[0][:, :7]])
    assert same_bits([run_mutrate(fn, model, lk, flags, many[::-1])[0][:, ::-1]], [out[0]])
    # n_rates beyond the maximum is clamped by the kernel itself (what a device entry's caller cannot reach: the host refuses it)
    more = np.concatenate([tables_of(model, many), np.full((1, fs.RATE_TABLE_DOUBLES), np.nan)])
    s = len(lk)
    rl = np.full((s, 33), -5.0)
    tc = np.ascontiguousarray(factor_tables(model))
    a, fl = np.ascontiguousarray(lk), np.ascontiguousarray(flags, np.uint8)
    fn(a.ctypes.data, fl.ctypes.data, rl.ctypes.data, None, None, s, tc.ctypes.data, 1.0, more.ctypes.data, 33)
    flat = rl.reshape(-1)
    assert same_bits([flat[:s * 32].reshape(s, 32)], [out[0]]) and np.all(flat[s * 32:] == -5.0)


def test_only_the_transmission_entries_of_a_block_are_read(tmp_path):
    """The founders' prior entries of a block (and everything else outside the two child tables of each chrX half) may hold
    anything: the priors are the context's."""
    ped, lk, flags = batch("random1", 7)
    model = fs.make_model(ped, mrate=1e-7)
    rates = grid(1e-7)
    t = tables_of(model, rates)
    want = run_mutrate(build_mutrate_host(model, tmp_path)[0], model, lk, flags, rates, tables=t)
    junk = t.reshape(len(rates), 4, 4, 27).copy()
    junk[:, :, :2, :] = np.nan  # the founder kinds' tables
    junk[:, 1::2, :, :] = np.nan  # the Known halves: the transmission entries are read from the chrX half's first block
    for variant in range(N_VARIANTS):
        fn = build_mutrate_host(model, tmp_path, variant)[0]
        assert same_bits(run_mutrate(fn, model, lk, flags, rates, tables=junk.reshape(len(rates), -1)), want)


def test_rate_tables(tmp_path):
    """Block r equals factor_tables of the model rebuilt at that rate, bit for bit; the refusals."""
    for name in ("trio", "random1", "wide48"):
        ped = pedigree(name)
        rates = np.concatenate([grid(1e-4), [0.25, 3e-8]])
        kw = dict(genoProbN=[0.9, 0.07, 0.03], genoProbXK=[0.4, 0.0, 0.6]) if name == "random1" else {}
        got = tables_of(fs.make_model(ped, mrate=1e-7, **kw), rates)
        assert got.shape == (len(rates), fs.RATE_TABLE_DOUBLES)
        for r, rate in enumerate(rates):
            want = np.ascontiguousarray(factor_tables(fs.make_model(ped, mrate=float(rate), **kw))).reshape(-1)
            assert same_bits([got[r]], [want])
    ctx = fs.Context(fs.make_model(pedigree("trio")), device=-1)
    assert ctx.rate_tables(0.5).shape == (1, 432)  # a scalar is one rate
    for bad, at in (([1e-7, -1e-9], 1), ([np.nan], 0), ([0.0, 0.5, 1.0000001, 2.0], 2), ([np.inf], 0)):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*rates\[%d\] must be a finite number in \[0, 1\]" % at):
            ctx.rate_tables(bad)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_rates must be 1\.\.32, got 33"):
        ctx.rate_tables(np.zeros(33))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_rates must be 1\.\.32, got 0"):
        ctx.rate_tables([])
    one = np.zeros(1)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    assert fs.lib().famseq_rate_tables(ctx._h, None, 1, p) == -1 and "rates must be given" in fs.lib().famseq_last_error(ctx._h).decode()
    assert fs.lib().famseq_rate_tables(ctx._h, p, 1, None) == -1 and "tables must be given" in fs.lib().famseq_last_error(ctx._h).decode()
    ctx.close()


def test_generating_the_mutrate_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new body, the shared sum pass and the emitter's new option must not reach the text of the existing kernels (their
    code objects are cached by content hash)."""
    ped = pedigree("random0")
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    stems = ("map", "map_prior", "evidence", "evidence_prior", "loo", "loo_prior", "prior", "pattern", "pattern_prior", "sample",
             "sample_prior", "af", "relabel", "relabel_prior")
    keys = ("elim_code_object", "trio_code_object") + tuple(s + "_code_object" for s in stems)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        for stem in stems:
            ctx.set_option(stem + "_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        assert before["mutrate_code_object"] == "" and before["mutrate_variant"] == -1
        ctx.set_option("mutrate_kernels", 1)
        ctx.set_option("mutrate_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["mutrate_code_object"] not in [before[k] for k in keys]
    assert after["mutrate_prior_code_object"] not in [before[k] for k in keys] + [after["mutrate_code_object"]]
    # the plan's older keys keep their order, the new ones come last
    names = list(after)
    assert names[-4:] == ["mutrate_code_object", "mutrate_variant", "mutrate_prior_code_object", "mutrate_prior_variant"]
    assert [k for k in names if k in before and not k.startswith("mutrate")] == [k for k in before if not k.startswith("mutrate")]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("mutrate_kernels", "mutrate_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = pedigree("random0")
    ones = np.ones((1, ped.n, 3))
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["mutrate_code_object"] == "" and plan["mutrate_variant"] == -1
        assert plan["mutrate_prior_code_object"] == "" and plan["mutrate_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("mutrate_kernels", 2)
        ctx.set_option("mutrate_kernels", 1)
        ctx.set_option("mutrate_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["mutrate_code_object"].endswith(".hsaco") and 0 <= plan["mutrate_variant"] < N_VARIANTS
        assert plan["mutrate_prior_code_object"].endswith(".hsaco") and plan["mutrate_prior_variant"] == plan["mutrate_variant"]
        assert plan["mutrate_prior_code_object"] != plan["mutrate_code_object"] and plan["evidence_code_object"] == ""
        # the ABI's refusals of the rates come before anything else, so a context without a device gives them too
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_rates must be 1\.\.32, got 33"):
            ctx.mutrate_batch(np.full(33, 1e-7), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_rates must be 1\.\.32, got 0"):
            ctx.mutrate_batch([], lk=ones)
        for bad in (-1e-12, 1.5, np.nan, np.inf):
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*rates\[1\] must be a finite number in \[0, 1\]"):
                ctx.mutrate_batch([0.0, bad, bad], lk=ones)
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*rates\[1\] must be a finite number in \[0, 1\]"):
                ctx.mutrate_prior_batch(np.ones((1, 6)), [0.0, bad, bad], lk=ones)
        for fn, more in (("famseq_mutrate_batch", ()), ("famseq_mutrate_prior_batch", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 1, None, None, None)
            assert rc == -1 and "rates must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        for fn, more in (("famseq_mutrate_batch_device", ()), ("famseq_mutrate_prior_batch_device", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 0, None, None, None, None)
            assert rc == -1 and "n_rates must be 1..32" in fs.lib().famseq_last_error(ctx._h).decode()
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 2, None, None, None, None)
            assert rc == -1 and "d_tables must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match="list of mutation rates"):
            ctx.mutrate_batch(np.zeros((2, 2)), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.mutrate_batch([1e-7], lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.mutrate_prior_batch(np.ones((1, 6)), [1e-7], lk=ones)
        ctx.close()
