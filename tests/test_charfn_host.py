"""The characteristic-function kernel's arithmetic (famseq_charfn / famseq_charfn_prior: per site and table of complex
per-member weights cf = Z(lk * w) / Z(lk), and the site's own log10 likelihood) and the count distribution built on it, checked
without a GPU.

As in test_weight_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++ -ffp-contract=off.  Tables, reference, bar (|cf - reference| <= 1e-12 A, absolute) and the floor every batch asserts on the
reference alone: tests/_charfn.py.

The bit contracts of include/famseq_hip.h, against the host-compiled famseq_evidence and famseq_pattern of the same variant:
loglik is famseq_evidence's; a column depends on neither n_tables nor the other tables; equal tables give equal bits; the
conjugate table gives the conjugate; imaginary parts of +0.0 (real parts >= 0) stay +0.0; a 0/1 table gives famseq_pattern's
pat_post in cf.re; a table of (1, 0) gives (1.0, +0.0); every variant gives the same bits; the prior form on the model's rows
gives the plain form's bits.

The distribution: count_tables -> the kernel -> count_from_cf against the directly binned 3^N enumeration at 1e-12 absolute.
"""
import os
from unittest import mock

import numpy as np
import pytest

import _charfn as X
import _prior as P
import famseq_amd as fs
from test_evidence_host import build_evidence_host, run_evidence
from test_generated_host import factor_tables
from test_pattern_host import PED_NAMES, allowed, batch, build_pattern_host, pedigree, run_pattern, same_bits
from test_weight_host import build_weight_host, run_weight

N_SITES = 64
PLUS_ZERO = np.zeros(1).view(np.uint64)[0]


def imag_bits(cf):
    return np.ascontiguousarray(cf.imag).view(np.uint64)


@pytest.mark.parametrize("name", PED_NAMES)
def test_the_kernel_matches_the_reference(name, tmp_path):
    ped, lk, flags, masks = batch(name)
    assert {0, 1, 2, 3} <= set(flags.tolist())
    tables, at = X.batch_tables(ped, masks)
    refs = {mrate: X.reference(ped, mrate, lk, flags, tables) for mrate in X.MRATES}
    for mrate in X.MRATES:
        X.clear(refs[mrate], "%s mrate %g" % (name, mrate))
    fn, plan, src = X.build_charfn_host(fs.make_model(ped), tmp_path)
    # emitted-text pins: the rows in registers below the kernel's lean threshold, lean from there; each pass's text stands once;
    # the table through a wave-uniform pointer; no LDS beyond famseq_evidence's factor tables
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= X.LEAN_FROM) == ("#define zc0_0r " in src)
    assert src.count("for (int ps_ = 1;") == 1 and src.count("const double Zp_r") == 1 and src.count("const double Zp_ ") == 1
    assert "#pragma unroll 1\n      for (int ps_ = 1; ps_ <= last_; ++ps_)" in src
    assert "const int pu_ = __builtin_amdgcn_readfirstlane(ps_);" in src and "cw_g + (long)(pu_ - 1) * CW6;" in src
    assert "#define CW6 %d\n" % (6 * ped.n) in src and "#define MAXCW 64\n" in src
    assert src.count("__shared__") == 1
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", plan["charfn_variant"])[0]
    pt = build_pattern_host(fs.make_model(ped), tmp_path / "pt", plan["charfn_variant"])[0]
    for mrate in X.MRATES:
        model = fs.make_model(ped, mrate=mrate)
        cf, ll, st = out = X.run_charfn(fn, model, lk, flags, tables)
        X.check(out, refs[mrate], "%s mrate %g" % (name, mrate))
        e_ll, _, e_st = run_evidence(ev, model, lk, flags)
        assert np.array_equal(st, e_st) and same_bits([ll], [e_ll])
        # conjugate tables: the conjugate result, exactly (a zero imaginary part compares equal whatever its sign)
        cj = X.run_charfn(fn, model, lk, flags, np.conj(tables))[0]
        assert same_bits([cj.real], [cf.real]) and np.array_equal(cj.imag, -cf.imag)
        # a table of (1, 0): exactly (1.0, +0.0); frequency 0 of both counts is such a table
        for col in (at["ones"].start, at["carriers"].start, at["alleles"].start):
            assert np.all(cf[:, col].real == 1.0) and np.all(imag_bits(cf[:, col]) == PLUS_ZERO)
        # 0/1 tables with +0.0 imaginary parts: famseq_pattern's posteriors bit for bit, imaginary parts +0.0
        pp, p_ll, p_st = run_pattern(pt, model, lk, flags, masks)
        got = X.run_charfn(fn, model, lk, flags, allowed(masks))[0]
        assert np.all(p_st == 0) and same_bits([got.real], [pp]) and np.all(imag_bits(got) == PLUS_ZERO)
        assert X.same_cf(got[:, 2], cf[:, at["mask"].start])


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped, lk, flags, masks = batch(name, 1)
    model = fs.make_model(ped, mrate=1e-4)
    tables = X.batch_tables(ped, masks)[0]
    outs = [X.run_charfn(X.build_charfn_host(model, tmp_path / str(v), v)[0], model, lk, flags, tables) for v in range(X.N_VARIANTS)]
    assert np.all(outs[0][2] == 0)
    for out in outs[1:]:
        assert X.same_cf(out[0], outs[0][0]) and same_bits(out[1:], outs[0][1:])
    X.check(outs[2], X.reference(ped, 1e-4, lk, flags, tables), "%s variant 2" % name)


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_site_prior_form(name, tmp_path):
    """Fed the model's rows: the plain form's bits.  Under Hardy-Weinberg rows: tests/_prior_joint.py's factors on the complex
    rows, and famseq_evidence_prior's loglik bits."""
    ped, lk, flags, masks = batch(name, 2)
    tables = X.batch_tables(ped, masks)[0]
    hwe = fs.hwe_priors(np.random.RandomState(3).uniform(0.01, 0.5, len(lk)))
    plain = X.build_charfn_host(fs.make_model(ped), tmp_path / "plain", 1)[0]
    fn, _, src = X.build_charfn_host(fs.make_model(ped), tmp_path / "prior", 1, prior=True)
    assert "PRIOR_LOAD(site);" in src and "tcf[0] * (l" not in src and "tcf[27] * (l" not in src
    assert "int n_tables, const double *__restrict__ prior_g) {" in src  # the tables stand in front of the prior rows
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", 1, prior=True)[0]
    for mrate in X.MRATES:
        model = fs.make_model(ped, mrate=mrate)
        want = X.run_charfn(plain, model, lk, flags, tables)
        assert np.all(want[2] == 0)
        got = X.run_charfn(fn, model, lk, flags, tables, P.model_rows(model, flags))
        assert X.same_cf(got[0], want[0]) and same_bits(got[1:], want[1:])
        ref = X.reference(ped, mrate, lk, flags, tables, hwe)
        X.clear(ref, "%s mrate %g, HWE rows" % (name, mrate))
        out = X.run_charfn(fn, model, lk, flags, tables, hwe)
        X.check(out, ref, "%s mrate %g, HWE rows" % (name, mrate))
        e_ll, _, e_st = run_evidence(ev, model, lk, flags, hwe)
        assert np.array_equal(out[2], e_st) and same_bits([out[1]], [e_ll])


@pytest.mark.parametrize("name", ["random0", "wide48"])
def test_one_table_and_sixty_four(name, tmp_path):
    """n_tables = 1, 2 and FAMSEQ_MAX_CWEIGHTS: a column's bits depend neither on how many others the call holds nor on what
    they are; equal tables give equal bits; beyond the maximum the kernel clamps."""
    ped, lk, flags, masks = batch(name, 5)
    rng = np.random.RandomState(6)
    some = X.batch_tables(ped, masks)[0][-6:]
    more = np.exp(2j * np.pi * rng.uniform(0, 1, (fs.MAX_CWEIGHTS - 8, ped.n, 3)))
    many = np.concatenate([some, more, some[0:1], some[0:1]])
    assert len(many) == 64 == fs.MAX_CWEIGHTS
    ref = X.reference(ped, 1e-4, lk, flags, many, brute=False)
    X.clear(ref)
    model = fs.make_model(ped, mrate=1e-4)
    fn = X.build_charfn_host(model, tmp_path)[0]
    out = X.run_charfn(fn, model, lk, flags, many)
    X.check(out, ref, "%s, 64 tables" % name)
    assert X.same_cf(out[0][:, 0], out[0][:, 62]) and X.same_cf(out[0][:, 62], out[0][:, 63])
    for m in (0, 2, 17, 63):
        one = X.run_charfn(fn, model, lk, flags, many[m:m + 1])
        assert X.same_cf(one[0][:, 0], out[0][:, m]) and same_bits(one[1:], out[1:])
    assert X.same_cf(X.run_charfn(fn, model, lk, flags, many[[9, 0]])[0], out[0][:, [9, 0]])
    assert X.same_cf(X.run_charfn(fn, model, lk, flags, many[::-1])[0][:, ::-1], out[0])
    # n_tables beyond the maximum is clamped by the kernel itself (what a device entry's caller cannot reach: the host refuses it)
    over = X.as_pairs(np.concatenate([many, np.full((1, ped.n, 3), np.nan)]))
    s = len(lk)
    cf = np.full((s, 65, 2), -5.0)
    tc = np.ascontiguousarray(factor_tables(model))
    a, fl = np.ascontiguousarray(lk), np.ascontiguousarray(flags, np.uint8)
    fn(a.ctypes.data, fl.ctypes.data, cf.ctypes.data, None, None, s, tc.ctypes.data, 1.0, over.ctypes.data, 65)
    flat = cf.reshape(-1)
    assert X.same_cf(flat[:s * 128].view(np.complex128).reshape(s, 64), out[0]) and np.all(flat[s * 128:] == -5.0)


def test_each_output_may_be_null(tmp_path):
    ped, lk, flags, masks = batch("random1", 4)
    model = fs.make_model(ped)
    tables = X.batch_tables(ped, masks)[0]
    for prior in (None, P.model_rows(model, flags)):
        fn = X.build_charfn_host(model, tmp_path, prior=prior is not None)[0]
        full = X.run_charfn(fn, model, lk, flags, tables, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = X.run_charfn(fn, model, lk, flags, tables, prior, want=want)
            untouched = (np.full(full[0].shape, -5.0 - 5.0j), np.full(N_SITES, -5.0), np.full(N_SITES, 77, np.uint8))
            assert X.same_cf(got[0], full[0] if want[0] else untouched[0])
            for k in (1, 2):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])
        # without cf only the real pass runs, and the table is not read: no table at all will do
        a, fl = np.ascontiguousarray(lk), np.ascontiguousarray(flags, np.uint8)
        tc = np.ascontiguousarray(factor_tables(model))
        ll = np.full(N_SITES, -5.0)
        more = [] if prior is None else [np.ascontiguousarray(prior).ctypes.data]
        fn(a.ctypes.data, fl.ctypes.data, None, ll.ctypes.data, None, N_SITES, tc.ctypes.data, 1.0, None, 10, *more)
        assert same_bits([ll], [full[1]])


def test_failure_statuses_and_exact_zeros(tmp_path):
    """An all-zero likelihood row: status 1.  1e160 rows: status 2.  Both parts of every cf entry and loglik of such a site are
    NaN.  A table that gives one member three zeros: (0.0, 0.0) at every good site, a result."""
    ped = pedigree("quad")
    _, lk, _, masks = batch("quad")
    lk = lk[:32].copy()
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    tables = X.batch_tables(ped, masks)[0]
    dead = np.exp(1j * np.ones((1, ped.n, 3)))
    dead[0, 2] = 0.0
    tables = np.concatenate([tables, dead])
    model = fs.make_model(ped, mrate=1e-4)
    ref = X.reference(ped, 1e-4, lk, flags, tables)
    X.clear(ref, planted=(5,))
    assert ref[3][5] == 1
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = X.build_charfn_host(model, tmp_path / str(variant), variant, prior=prior is not None)[0]
            cf, ll, st = out = X.run_charfn(fn, model, lk, flags, tables, prior)
            X.check(out, ref, "planted failure")
            assert st[5] == 1 and np.all(np.isnan(cf[5].real)) and np.all(np.isnan(cf[5].imag)) and np.isnan(ll[5])
            rest = np.delete(cf, 5, axis=0)
            assert not np.any(np.isnan(rest)) and np.all(rest[:, -1] == 0)
    fn = X.build_charfn_host(model, tmp_path / "0", 0)[0]
    big = np.full((2, ped.n, 3), 1e160)
    cf, ll, st = X.run_charfn(fn, model, big, np.zeros(2, np.uint8), tables)
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(cf.real)) and np.all(np.isnan(cf.imag))


def test_generating_the_charfn_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new arithmetic must not reach the text of the existing kernels (their code objects are cached by content hash); the
    plan's keys: behind the max-marginal kernel's, in front of the mutation-rate profile's four."""
    ped = pedigree("random0")
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    stems = ("map", "map_prior", "evidence", "evidence_prior", "loo", "loo_prior", "prior", "pattern", "pattern_prior", "sample",
             "sample_prior", "af", "relabel", "relabel_prior", "mutrate", "mutrate_prior", "origin", "origin_prior", "weight",
             "weight_prior", "maxmarg", "maxmarg_prior")
    keys = ("elim_code_object", "trio_code_object") + tuple(s + "_code_object" for s in stems)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        for stem in stems:
            ctx.set_option(stem + "_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        assert before["charfn_code_object"] == "" and before["charfn_variant"] == -1
        ctx.set_option("charfn_kernels", 1)
        ctx.set_option("charfn_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["charfn_code_object"] not in [before[k] for k in keys]
    assert after["charfn_prior_code_object"] not in [before[k] for k in keys] + [after["charfn_code_object"]]
    names = list(after)
    assert names == list(before)
    assert names[-4:] == ["mutrate_code_object", "mutrate_variant", "mutrate_prior_code_object", "mutrate_prior_variant"]
    at = names.index("charfn_code_object")
    assert names[at:at + 4] == ["charfn_code_object", "charfn_variant", "charfn_prior_code_object", "charfn_prior_variant"]
    assert names[at - 1] == "maxmarg_prior_variant" and at + 4 < len(names) - 4


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("charfn_kernels", "charfn_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            ctx.set_option(key, 1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.charfn_batch(np.ones((1, ctx.n, 3), np.complex128), lk=np.ones((1, ctx.n, 3)))
    ctx.close()
    ped = pedigree("random0")
    ones = np.ones((1, ped.n, 3))
    table = np.ones((3, ped.n, 3), np.complex128)
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["charfn_code_object"] == "" and plan["charfn_variant"] == -1
        assert plan["charfn_prior_code_object"] == "" and plan["charfn_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("charfn_kernels", 2)
        ctx.set_option("charfn_kernels", 1)
        ctx.set_option("charfn_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["charfn_code_object"].endswith(".hsaco") and 0 <= plan["charfn_variant"] < X.N_VARIANTS
        assert plan["charfn_prior_code_object"].endswith(".hsaco") and plan["charfn_prior_variant"] == plan["charfn_variant"]
        assert plan["charfn_prior_code_object"] != plan["charfn_code_object"] and plan["evidence_code_object"] == ""
        # the ABI's refusals of the tables come before anything else, so a context without a device gives them too
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_tables must be 1\.\.64, got 65"):
            ctx.charfn_batch(np.ones((65, ped.n, 3), np.complex128), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_tables must be 1\.\.64, got 0"):
            ctx.charfn_batch(np.ones((0, ped.n, 3), np.complex128), lk=ones)
        for bad, part, text in ((complex(np.nan, 0.0), "real", "nan"), (complex(1.0, np.inf), "imaginary", "inf"),
                                (complex(1.0, -np.inf), "imaginary", "-inf")):
            t = table.copy()
            t[2, 1, 0] = bad
            t[2, 4, 2] = bad
            for call in (lambda: ctx.charfn_batch(t, lk=ones), lambda: ctx.charfn_prior_batch(np.ones((1, 6)), t, lk=ones)):
                with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0, %s part is %s$" % (part, text)):
                    call()
        for fn, more in (("famseq_charfn_batch", ()), ("famseq_charfn_prior_batch", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 1, None, None, None)
            assert rc == -1 and "cweights must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        for fn, more in (("famseq_charfn_batch_device", ()), ("famseq_charfn_prior_batch_device", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 0, None, None, None, None)
            assert rc == -1 and "n_tables must be 1..64" in fs.lib().famseq_last_error(ctx._h).decode()
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 2, None, None, None, None)
            assert rc == -1 and "d_cweights must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match=r"cweights must be complex \[M, %d, 3\]" % ped.n):
            ctx.charfn_batch(np.ones((2, ped.n + 1, 3), np.complex128), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.charfn_batch(table[0], lk=ones)  # (a single [N, 3] table is accepted)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.charfn_prior_batch(np.ones((1, 6)), X.as_pairs(table), lk=ones)  # (and the real [M, N, 3, 2] layout)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.count_batch(fs.count_scores(ped.n), lk=ones)
        ctx.close()


@pytest.mark.parametrize("n", [24, 25, 39, 40])
def test_the_lean_threshold_is_the_kernels_own(n, tmp_path):
    """Lean from 25 members (profiles/charfn/resources.txt: the register-resident complex pass spills before forty), where its
    sibling famseq_weight turns lean at forty: the emitted text on both sides of both edges, and FAMSEQ_CHARFN_LEAN_FROM, the
    tuning aid the survey was made with."""
    from famseq_amd.prebuild_sets import CHARFN_LEAN_FROM, wide_pedigree

    assert CHARFN_LEAN_FROM == X.LEAN_FROM
    ped = wide_pedigree(n)
    ped.relations()
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")

    def texts(more):
        with mock.patch.dict(os.environ, dict(env, **more)):
            ctx = fs.Context(model, device=-1)
            ctx.set_option("charfn_kernels", 1)
            ctx.set_option("weight_kernels", 1)
            plan = ctx.plan()
            ctx.close()
        return [open(plan[k + "_code_object"][:-6] + ".hip").read() for k in ("charfn", "weight")]

    charfn, weight = texts({})
    assert ("#define l0_0 lgv[0]" in charfn) == (n >= 25) and ("#define l0_0 lgv[0]" in weight) == (n >= 40)
    assert ("#define zc0_0r " in charfn) == (n >= 25) and ("const double zc0_0r = " in charfn) == (n < 25)
    moved, same = texts({"FAMSEQ_CHARFN_LEAN_FROM": "40"})
    assert same == weight and ("#define l0_0 lgv[0]" in moved) == (n >= 40)


def test_count_scores_tables_and_inverse():
    s = fs.count_scores(5, [0, 3], "alleles")
    assert s.shape == (5, 3) and s.dtype.kind == "i" and s[0].tolist() == s[3].tolist() == [0, 1, 2] and not s[[1, 2, 4]].any()
    assert fs.count_scores(3).tolist() == [[0, 1, 1]] * 3 and fs.count_scores(2, kind="homalt").tolist() == [[0, 0, 1]] * 2
    with pytest.raises(ValueError, match="kind must be"):
        fs.count_scores(3, kind="hets")
    with pytest.raises(ValueError, match="outside 0..4"):
        fs.count_scores(5, [5])
    with pytest.raises(ValueError, match="listed twice"):
        fs.count_scores(5, [1, 1])
    t, D = fs.count_tables(s)
    assert D == 4 and t.shape == (3, 5, 3) and t.dtype == np.complex128 and np.all(t[0] == 1.0) and np.all(t[:, [1, 2, 4]] == 1.0)
    np.testing.assert_allclose(t[1, 0], np.exp(2j * np.pi * np.arange(3) / 5), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.abs(t), 1.0, rtol=0, atol=2e-16)
    assert fs.count_tables(fs.count_scores(63, kind="alleles"))[0].shape[0] == 64  # D = 126: 64 tables, the most a call takes
    with pytest.raises(ValueError, match="D = 127 needs 65 tables"):
        fs.count_tables(fs.count_scores(64, list(range(63)), "alleles") + fs.count_scores(64, [63]))
    with pytest.raises(ValueError, match="non-negative integers"):
        fs.count_tables(np.ones((3, 3)))
    # the inverse: a known distribution's characteristic function at the frequencies of count_tables gives it back
    rng = np.random.RandomState(0)
    for D in (1, 2, 7, 10):
        p = rng.dirichlet(np.ones(D + 1), 4)
        p[0, 1] = 0.0
        p[0] /= p[0].sum()
        M = D + 1
        phi = p @ np.exp(2j * np.pi * np.outer(np.arange(M), np.arange(M // 2 + 1)) / M)
        got = fs.count_from_cf(phi, D)
        np.testing.assert_allclose(got, p, rtol=0, atol=1e-15)
        assert np.all(got >= 0)
        assert np.array_equal(fs.count_from_cf(np.stack([phi.real, phi.imag], axis=-1), D), got)
    nan = fs.count_from_cf(np.full((1, 3), np.nan + 1j * np.nan), 4)
    assert nan.shape == (1, 5) and np.all(np.isnan(nan))
    assert fs.count_from_cf(np.array([[1.0 + 0j, 1.0 + 5e-13]]), 1)[0].tolist() == [1.0 + 2.5e-13, 0.0]  # [-1e-12, 0): rounding below 0
    assert fs.count_from_cf(np.array([[1.0 + 0j, -1.0 - 1e-9]]), 1)[0, 0] < 0  # beyond the clip nothing is hidden
    with pytest.raises(ValueError, match="3 frequencies"):
        fs.count_from_cf(np.ones((2, 4), np.complex128), 4)


def host_count(fn, model, lk, flags, scores, prior=None):
    """Context.count_batch with the host-compiled kernel between count_tables and count_from_cf."""
    tables, D = fs.count_tables(scores)
    cf, ll, st = X.run_charfn(fn, model, lk, flags, tables, prior)
    return fs.count_from_cf(cf, D), ll, st


@pytest.mark.parametrize("name", ["random0", "random1", "random%d" % 99, "ped10"])
def test_the_count_distribution(name, tmp_path):
    """dist against the directly binned 3^N enumeration at 1e-12 absolute: carriers, alleles and homalt, over all members and
    over a subset; every row sums to 1; P(nobody carries it) is famseq_evidence's pref, P(everybody does) the pattern of 6s;
    sum_k dist[k] 0.5^k is famseq_weight's 10^(wt_loglik - loglik) on the table 0.5^scores."""
    ped, lk, flags, _ = batch(name, 7)
    n = ped.n
    assert n <= 10
    some = np.sort(np.random.RandomState(n).permutation(n)[:max(2, n // 2)])
    worst = 0.0
    for mrate in (1e-7, 0.0):
        model = fs.make_model(ped, mrate=mrate)
        fn, plan, _ = X.build_charfn_host(model, tmp_path)
        for kind in ("carriers", "alleles", "homalt"):
            for members in (None, some):
                scores = fs.count_scores(n, members, kind)
                want, D = X.brute_distribution(ped, mrate, lk, flags, scores)
                dist, ll, st = host_count(fn, model, lk, flags, scores)
                assert dist.shape == want.shape == (N_SITES, D + 1) and np.all(st == 0) and not np.any(np.isnan(want))
                worst = max(worst, np.abs(dist - want).max(), np.abs(dist.sum(axis=1) - 1.0).max())
                assert np.all(np.abs(dist - want) <= X.DIST_ATOL) and np.all(dist >= 0)
                assert np.all(np.abs(dist.sum(axis=1) - 1.0) <= X.DIST_ATOL)
        v = plan["charfn_variant"]
        scores = fs.count_scores(n)
        dist, ll, st = host_count(fn, model, lk, flags, scores)
        e_ll, pref, _ = run_evidence(build_evidence_host(model, tmp_path / "ev", v)[0], model, lk, flags)
        assert same_bits([ll], [e_ll]) and np.all(np.abs(dist[:, 0] - pref) <= X.DIST_ATOL)
        pp = run_pattern(build_pattern_host(model, tmp_path / "pt", v)[0], model, lk, flags, np.full((1, n), 6, np.uint8))[0]
        assert np.all(np.abs(dist[:, n] - pp[:, 0]) <= X.DIST_ATOL)
        for scores in (scores, fs.count_scores(n, some, "alleles")):
            dist = host_count(fn, model, lk, flags, scores)[0]
            wl, w_ll, _ = run_weight(build_weight_host(model, tmp_path / "wt", v)[0], model, lk, flags, 0.5 ** scores[None].astype(float))
            mgf = 10.0 ** (wl[:, 0] - w_ll)
            np.testing.assert_allclose(dist @ 0.5 ** np.arange(dist.shape[1]), mgf, rtol=1e-9, atol=1e-12)
    print("%s: worst |dist - enumeration| and |sum - 1| %.3g (bar %g)" % (name, worst, X.DIST_ATOL))


def test_the_count_distribution_under_site_priors(tmp_path):
    """The prior form between count_tables and count_from_cf: on the model's rows the plain form's distribution bit for bit; on
    Hardy-Weinberg rows a distribution (rows sum to 1) whose zero bin is famseq_evidence_prior's pref."""
    ped, lk, flags, _ = batch("random1", 8)
    model = fs.make_model(ped)
    plain = X.build_charfn_host(model, tmp_path / "plain", 1)[0]
    fn = X.build_charfn_host(model, tmp_path / "prior", 1, prior=True)[0]
    scores = fs.count_scores(ped.n, kind="alleles")
    want = host_count(plain, model, lk, flags, scores)
    got = host_count(fn, model, lk, flags, scores, P.model_rows(model, flags))
    assert same_bits(got, want)
    hwe = fs.hwe_priors(np.random.RandomState(4).uniform(0.01, 0.5, len(lk)))
    dist, ll, st = host_count(fn, model, lk, flags, scores, hwe)
    e_ll, pref, _ = run_evidence(build_evidence_host(model, tmp_path / "ev", 1, prior=True)[0], model, lk, flags, hwe)
    assert np.all(st == 0) and same_bits([ll], [e_ll])
    assert np.all(np.abs(dist.sum(axis=1) - 1.0) <= X.DIST_ATOL) and np.all(np.abs(dist[:, 0] - pref) <= X.DIST_ATOL)
