"""The weight kernel's arithmetic (famseq_weight / famseq_weight_prior: per site and weight table m the log10 of the network's
total weight Z_m on the rows lk * w_m, and the site's own log10 likelihood), checked without a GPU.

As in test_mutrate_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled
with g++ -ffp-contract=off.  References, bars and the floor every batch asserts on the reference alone: tests/_weight.py.

The bit contracts of include/famseq_hip.h, against the host-compiled famseq_evidence of the same variant on rows premultiplied in
double: wt_loglik[s][m] is that kernel's loglik wherever it has status 0 (-inf where it has not on a good site); loglik is
famseq_evidence's on the rows as they are; a column depends on neither n_weights nor the other tables; a table of ones gives
loglik's bits; equal tables give equal bits; the prior form on the model's rows gives the plain form's bits.  Against the
host-compiled famseq_pattern on 0/1 tables: 10**(wt_loglik - loglik) is its ppost to 1e-9 relative, -inf exactly where ppost
is 0.0.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _prior as P
import _weight as W
import famseq_amd as fs
from test_evidence_host import build_evidence_host, run_evidence
from test_generated_host import factor_tables, host_source
from test_pattern_host import PED_NAMES, allowed, batch, build_pattern_host, pedigree, run_pattern, same_bits

N_SITES = 64


def build_weight_host(model, where, variant=None, prior=False):
    """Generate famseq_weight (prior: famseq_weight_prior) for a one-lane workgroup on a plan-only context, compile it for the
    host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("weight_prior", "famseq_weight_prior") if prior else ("weight", "famseq_weight")
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


def run_weight(fn, model, lk, flags, weights, prior=None, want=(True, True, True)):
    s, m = lk.shape[0], len(weights)
    a = np.ascontiguousarray(lk, dtype=np.float64)
    wl, ll, st = np.full((s, m), -5.0), np.full(s, -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    wt = np.ascontiguousarray(weights, dtype=np.float64)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, wl.ctypes.data if want[0] else None, ll.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, wt.ctypes.data, m]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return wl, ll, st


def evidence_bits(ev, model, lk, flags, weights, out, prior=None):
    """The bit contracts against the host-compiled famseq_evidence: loglik on the rows as they are, every column on the rows
    premultiplied in double wherever that call has status 0 (where it has not on a good site, Z_m is 0 and the column holds
    -inf).  -> the number of column entries compared bit for bit."""
    wl, ll, st = out
    e_ll, _, e_st = run_evidence(ev, model, lk, flags, prior)
    assert np.array_equal(st, e_st) and same_bits([ll], [e_ll])
    compared = 0
    for j, w in enumerate(weights):
        m_ll, _, m_st = run_evidence(ev, model, lk * w, flags, prior)
        good = (m_st == 0) & (st == 0)
        assert same_bits([wl[good, j]], [m_ll[good]])
        assert np.all(np.isneginf(wl[(m_st != 0) & (st == 0), j]))
        compared += int(good.sum())
    return compared


@pytest.mark.parametrize("name", PED_NAMES)
def test_the_kernel_matches_the_reference(name, tmp_path):
    ped, lk, flags, masks = batch(name)
    assert {0, 1, 2, 3} <= set(flags.tolist())
    weights = W.batch_weights(ped)
    refs = {mrate: W.reference(ped, mrate, lk, flags, weights) for mrate in W.MRATES}
    for mrate in W.MRATES:
        W.clear(refs[mrate], "%s mrate %g" % (name, mrate))
    fn, plan, src = build_weight_host(fs.make_model(ped), tmp_path)
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= 40)  # the rows in registers below forty members, lean from there
    assert src.count("for (int ps_ = 0;") == 1 and src.count("const double Zp_") == 1  # the pass's text stands once
    assert "#pragma unroll 1\n      for (int ps_ = 0; ps_ <= last_; ++ps_)" in src
    assert "const int pu_ = __builtin_amdgcn_readfirstlane(ps_);" in src and "(long)(pu_ - 1) * W3;" in src
    assert src.count("__shared__") == 1  # no LDS beyond famseq_evidence's factor tables
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", plan["weight_variant"])[0]
    pt = build_pattern_host(fs.make_model(ped), tmp_path / "pt", plan["weight_variant"])[0]
    for mrate in W.MRATES:
        model = fs.make_model(ped, mrate=mrate)
        out = run_weight(fn, model, lk, flags, weights)
        W.check(out, refs[mrate], "%s mrate %g" % (name, mrate))
        assert evidence_bits(ev, model, lk, flags, weights, out) > N_SITES
        # 0/1 tables: the pattern kernel's posteriors
        keep = allowed(masks)
        wl, ll, st = run_weight(fn, model, lk, flags, keep)
        pp, p_ll, p_st = run_pattern(pt, model, lk, flags, masks)
        assert np.array_equal(st, p_st) and np.all(st == 0) and same_bits([ll], [p_ll])
        assert np.array_equal(np.isneginf(wl), pp == 0.0)
        some = pp != 0.0
        np.testing.assert_allclose((10.0 ** (wl - ll[:, None]))[some], pp[some], rtol=1e-9, atol=0)
        assert same_bits([wl[:, 0]], [ll])  # (masks[0] allows everything: a table of ones)


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped, lk, flags, _ = batch(name, 1)
    model = fs.make_model(ped, mrate=1e-4)
    weights = W.batch_weights(ped)
    outs = [run_weight(build_weight_host(model, tmp_path, v)[0], model, lk, flags, weights) for v in range(W.N_VARIANTS)]
    assert np.all(outs[0][2] == 0)
    for out in outs[1:]:
        assert same_bits(out, outs[0])
    ev = build_evidence_host(model, tmp_path / "ev", 2)[0]
    assert evidence_bits(ev, model, lk, flags, weights, outs[2]) > N_SITES


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_site_prior_form(name, tmp_path):
    """Fed the model's rows: the plain form's bits.  Under Hardy-Weinberg rows: tests/_prior_joint.py's factors on the weighted
    rows, and famseq_evidence_prior's bits."""
    ped, lk, flags, _ = batch(name, 2)
    weights = W.batch_weights(ped)
    hwe = fs.hwe_priors(np.random.RandomState(3).uniform(0.01, 0.5, len(lk)))
    refs = {mrate: W.reference(ped, mrate, lk, flags, weights, hwe) for mrate in W.MRATES}
    for mrate in W.MRATES:
        W.clear(refs[mrate], "%s mrate %g, HWE rows" % (name, mrate))
    plain = build_weight_host(fs.make_model(ped), tmp_path / "plain", 1)[0]
    fn, _, src = build_weight_host(fs.make_model(ped), tmp_path / "prior", 1, prior=True)
    assert "PRIOR_LOAD(site);" in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src
    assert "int n_weights, const double *__restrict__ prior_g) {" in src  # the tables stand in front of the prior rows
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", 1, prior=True)[0]
    for mrate in W.MRATES:
        model = fs.make_model(ped, mrate=mrate)
        want = run_weight(plain, model, lk, flags, weights)
        assert np.all(want[2] == 0)
        assert same_bits(run_weight(fn, model, lk, flags, weights, P.model_rows(model, flags)), want)
        out = run_weight(fn, model, lk, flags, weights, hwe)
        W.check(out, refs[mrate], "%s mrate %g, HWE rows" % (name, mrate))
        assert evidence_bits(ev, model, lk, flags, weights, out, hwe) > N_SITES


@pytest.mark.parametrize("name", ["random0", "wide48"])
def test_one_table_and_thirty_two(name, tmp_path):
    """n_weights = 1, 2, 10 and FAMSEQ_MAX_WEIGHTS: a column's bits depend neither on how many others the call holds nor on
    what they are; equal tables give equal bits; a table of ones gives loglik's bits."""
    ped, lk, flags, _ = batch(name, 5)
    rng = np.random.RandomState(6)
    ten = W.batch_weights(ped)
    more = 10.0 ** rng.uniform(-1, 0.3, (fs.MAX_WEIGHTS - len(ten) - 3, ped.n, 3))
    many = np.concatenate([ten, more, np.ones((1, ped.n, 3)), ten[4:5], ten[4:5]])
    assert len(many) == 32 == fs.MAX_WEIGHTS
    ref = W.reference(ped, 1e-4, lk, flags, many, brute=False)
    W.clear(ref)
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_weight_host(model, tmp_path)[0]
    out = run_weight(fn, model, lk, flags, many)
    W.check(out, ref, "%s, 32 tables" % name)
    assert same_bits([out[0][:, 4]], [out[0][:, 30]]) and same_bits([out[0][:, 30]], [out[0][:, 31]])
    assert same_bits([out[0][:, 29]], [out[1]])  # the table of ones
    for m in (0, 2, 17, 31):
        one = run_weight(fn, model, lk, flags, many[m:m + 1])
        assert same_bits([one[0][:, 0], one[1], one[2]], [out[0][:, m], out[1], out[2]])
    assert same_bits([run_weight(fn, model, lk, flags, many[[9, 0]])[0]], [out[0][:, [9, 0]]])
    assert same_bits([run_weight(fn, model, lk, flags, ten)[0]], [out[0][:, :10]])
    assert same_bits([run_weight(fn, model, lk, flags, many[::-1])[0][:, ::-1]], [out[0]])
    # n_weights beyond the maximum is clamped by the kernel itself (what a device entry's caller cannot reach: the host refuses it)
    over = np.concatenate([many, np.full((1, ped.n, 3), np.nan)])
    s = len(lk)
    wl = np.full((s, 33), -5.0)
    tc = np.ascontiguousarray(factor_tables(model))
    a, fl = np.ascontiguousarray(lk), np.ascontiguousarray(flags, np.uint8)
    fn(a.ctypes.data, fl.ctypes.data, wl.ctypes.data, None, None, s, tc.ctypes.data, 1.0, over.ctypes.data, 33)
    flat = wl.reshape(-1)
    assert same_bits([flat[:s * 32].reshape(s, 32)], [out[0]]) and np.all(flat[s * 32:] == -5.0)


def test_each_output_may_be_null(tmp_path):
    ped, lk, flags, _ = batch("random1", 4)
    model = fs.make_model(ped)
    weights = W.batch_weights(ped)
    for prior in (None, P.model_rows(model, flags)):
        fn = build_weight_host(model, tmp_path, prior=prior is not None)[0]
        full = run_weight(fn, model, lk, flags, weights, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = run_weight(fn, model, lk, flags, weights, prior, want=want)
            untouched = (np.full(full[0].shape, -5.0), np.full(N_SITES, -5.0), np.full(N_SITES, 77, np.uint8))
            for k in range(3):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])
        # without wt_loglik only the unweighted pass runs, and the table is not read: no table at all will do
        a, fl = np.ascontiguousarray(lk), np.ascontiguousarray(flags, np.uint8)
        tc = np.ascontiguousarray(factor_tables(model))
        ll = np.full(N_SITES, -5.0)
        more = [] if prior is None else [np.ascontiguousarray(prior).ctypes.data]
        fn(a.ctypes.data, fl.ctypes.data, None, ll.ctypes.data, None, N_SITES, tc.ctypes.data, 1.0, None, 10, *more)
        assert same_bits([ll], [full[1]])


def test_failure_statuses_and_a_member_without_weight(tmp_path):
    """An all-zero likelihood row: status 1.  1e160 rows: status 2.  Every output of such a site is NaN.  A table whose three
    weights of one member are 0: -inf at every good site.  Weights above 1 that overflow Z_m: +inf, a result."""
    ped = pedigree("quad")
    lk = batch("quad")[1][:32].copy()
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    weights = W.batch_weights(ped)
    dead = np.ones((1, ped.n, 3))
    dead[0, 2] = 0.0
    weights = np.concatenate([weights, dead])
    model = fs.make_model(ped, mrate=1e-4)
    ref = W.reference(ped, 1e-4, lk, flags, weights)
    W.clear(ref, planted=(5,))
    assert ref[2][5] == 1 and np.all(ref[1][np.arange(32) != 5, -1] == 0)
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = build_weight_host(model, tmp_path, variant, prior=prior is not None)[0]
            wl, ll, st = out = run_weight(fn, model, lk, flags, weights, prior)
            W.check(out, ref, "planted failure")
            assert st[5] == 1 and np.all(np.isnan(wl[5])) and np.isnan(ll[5])
            assert not np.any(np.isnan(np.delete(wl, 5, axis=0))) and np.all(np.isneginf(np.delete(wl, 5, axis=0)[:, -1]))
    fn = build_weight_host(model, tmp_path, 0)[0]
    big = np.full((2, ped.n, 3), 1e160)
    wl, ll, st = run_weight(fn, model, big, np.zeros(2, np.uint8), weights)
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(wl))
    huge = np.full((1, ped.n, 3), 1e100)
    wl, ll, st = run_weight(fn, model, lk, flags, huge)
    assert np.all(np.delete(st, 5) == 0) and np.all(np.delete(wl[:, 0], 5) == np.inf) and np.all(np.isfinite(np.delete(ll, 5)))


def test_generating_the_weight_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new body must not reach the text of the existing kernels (their code objects are cached by content hash); the plan's
    keys: behind every older one, in front of the mutation-rate profile's four."""
    ped = pedigree("random0")
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    stems = ("map", "map_prior", "evidence", "evidence_prior", "loo", "loo_prior", "prior", "pattern", "pattern_prior", "sample",
             "sample_prior", "af", "relabel", "relabel_prior", "mutrate", "mutrate_prior", "origin", "origin_prior")
    keys = ("elim_code_object", "trio_code_object") + tuple(s + "_code_object" for s in stems)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        for stem in stems:
            ctx.set_option(stem + "_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        assert before["weight_code_object"] == "" and before["weight_variant"] == -1
        ctx.set_option("weight_kernels", 1)
        ctx.set_option("weight_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["weight_code_object"] not in [before[k] for k in keys]
    assert after["weight_prior_code_object"] not in [before[k] for k in keys] + [after["weight_code_object"]]
    names = list(after)
    assert names == list(before)
    assert names[-4:] == ["mutrate_code_object", "mutrate_variant", "mutrate_prior_code_object", "mutrate_prior_variant"]
    at = names.index("weight_code_object")
    assert names[at:at + 4] == ["weight_code_object", "weight_variant", "weight_prior_code_object", "weight_prior_variant"]
    assert names[at - 1] == "origin_prior_variant" and at + 4 < len(names) - 4


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("weight_kernels", "weight_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = pedigree("random0")
    ones = np.ones((1, ped.n, 3))
    table = np.ones((3, ped.n, 3))
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["weight_code_object"] == "" and plan["weight_variant"] == -1
        assert plan["weight_prior_code_object"] == "" and plan["weight_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("weight_kernels", 2)
        ctx.set_option("weight_kernels", 1)
        ctx.set_option("weight_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["weight_code_object"].endswith(".hsaco") and 0 <= plan["weight_variant"] < W.N_VARIANTS
        assert plan["weight_prior_code_object"].endswith(".hsaco") and plan["weight_prior_variant"] == plan["weight_variant"]
        assert plan["weight_prior_code_object"] != plan["weight_code_object"] and plan["evidence_code_object"] == ""
        # the ABI's refusals of the tables come before anything else, so a context without a device gives them too
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_weights must be 1\.\.32, got 33"):
            ctx.weight_batch(np.ones((33, ped.n, 3)), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_weights must be 1\.\.32, got 0"):
            ctx.weight_batch(np.ones((0, ped.n, 3)), lk=ones)
        for bad, text in ((-0.5, "-0.5"), (np.nan, "nan"), (np.inf, "inf")):
            t = table.copy()
            t[2, 1, 0] = bad
            t[2, 4, 2] = bad
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0 is %s$" % text):
                ctx.weight_batch(t, lk=ones)
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0 is %s$" % text):
                ctx.weight_prior_batch(np.ones((1, 6)), t, lk=ones)
        for fn, more in (("famseq_weight_batch", ()), ("famseq_weight_prior_batch", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 1, None, None, None)
            assert rc == -1 and "weights must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        for fn, more in (("famseq_weight_batch_device", ()), ("famseq_weight_prior_batch_device", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 0, None, None, None, None)
            assert rc == -1 and "n_weights must be 1..32" in fs.lib().famseq_last_error(ctx._h).decode()
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 2, None, None, None, None)
            assert rc == -1 and "d_weights must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match=r"weights must be \[M, %d, 3\]" % ped.n):
            ctx.weight_batch(np.ones((2, ped.n + 1, 3)), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.weight_batch(table[0], lk=ones)  # (a single [N, 3] table is accepted)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.weight_prior_batch(np.ones((1, 6)), table, lk=ones)
        ctx.close()


def test_penetrance_weights():
    w = fs.penetrance_weights(5, [0, 3], [1], (0.01, 0.8, 0.9))
    assert w.shape == (5, 3) and w.dtype == np.float64
    assert w[0].tolist() == w[3].tolist() == [0.01, 0.8, 0.9] and w[1].tolist() == [1 - 0.01, 1 - 0.8, 1 - 0.9]
    assert np.all(w[[2, 4]] == 1.0)
    assert np.array_equal(fs.penetrance_weights(3, [2]), [[1, 1, 1], [1, 1, 1], [0, 1, 1]])
    assert np.all(fs.penetrance_weights(2, []) == 1.0)
    # the dominant corner is segregation_masks' dominant pattern
    keep = allowed(fs.segregation_masks(6, [1, 2], [4], "dominant")[None])[0]
    assert np.array_equal(fs.penetrance_weights(6, [1, 2], [4], (0, 1, 1)), keep)
    with pytest.raises(ValueError, match="outside 0..4"):
        fs.penetrance_weights(5, [5])
    with pytest.raises(ValueError, match="outside 0..4"):
        fs.penetrance_weights(5, [0], [-1])
    with pytest.raises(ValueError, match="affected and as unaffected"):
        fs.penetrance_weights(5, [0, 1], [1])
    for pen in ((0, 1), (0, 1, 1.5), (-0.1, 1, 1), (0, np.nan, 1)):
        with pytest.raises(ValueError, match="three probabilities"):
            fs.penetrance_weights(5, [0], pen=pen)
