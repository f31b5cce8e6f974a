"""The max-marginal kernel's arithmetic (famseq_maxmarg / famseq_maxmarg_prior: per member and genotype the posterior of the
best configuration with that genotype, and the runner-up's posterior), checked without a GPU.

As in test_map_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++.  References: tests/_maxmarg.py — the 3^N enumeration of test_map_host.brute_weights up to nine members, the bucket
elimination of tests/_maxproduct.py in the max semiring beyond — and what each comparison asks is written there (check()).
Bits wherever two routes have to agree: top[0] against the host-compiled MAP kernel, the four variants, the site-prior form on
the model's rows.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _maxmarg as M
import _prior as P
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, side_variant_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_generated_host import factor_tables, host_source
from test_map_host import build_map_host, clear_likelihoods, run_map_host

RTOL = M.RTOL
MRATES = [1e-7, 0.0]
N_VARIANTS = 4  # kMaxmargVariants
SENTINEL, ST_SENTINEL = -5.0, 77


def build_maxmarg_host(model, where, variant=None, prior=False):
    """Generate famseq_maxmarg (prior: famseq_maxmarg_prior) for a one-lane workgroup on a plan-only context, compile it for the
    host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("maxmarg_prior", "famseq_maxmarg_prior") if prior else ("maxmarg", "famseq_maxmarg")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option(key + "_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    src = open(plan[key + "_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and (entry + "(") in src
    assert ("founder priors per site" in src.splitlines()[0]) == prior
    assert variant is None or plan[key + "_variant"] == variant
    assert "unsigned xf" not in src and "unsigned xa" not in src  # no back-pointer words
    tag = key + ("" if variant is None else "_%d" % variant)
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), entry)
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def run_maxmarg(fn, model, lk, flags, prior=None, want=(True, True, True)):
    """-> (maxmarg, top, status); an output that is not wanted is passed as NULL and comes back as its sentinels."""
    s, n = lk.shape[0], lk.shape[1]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    mm, top, st = np.full((s, n, 3), SENTINEL), np.full((s, 2), SENTINEL), np.full(s, ST_SENTINEL, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, mm.ctypes.data if want[0] else None, top.ctypes.data if want[1] else None,
            st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return mm, top, st


def bits(out):
    return [np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint8) for x in out]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


_KERNELS = {}


def kernel(seed, tmp_path_factory, variant=None, prior=False):
    key = (seed, variant, prior)
    if key not in _KERNELS:
        ped = random_pedigree(seed)[1]
        ped.relations()
        _KERNELS[key] = build_maxmarg_host(fs.make_model(ped), tmp_path_factory.mktemp("maxmarg_%d" % seed), variant, prior)[0]
    return _KERNELS[key]


def batches(seed):
    """-> (ped, [(name, lk, flags)]): test_map_host's clear batch and its adversarial one (integer PLs, hard zeros, unsequenced
    members), drawn as that file draws them."""
    rng, ped = random_pedigree(seed)
    ped.relations()
    clear = clear_likelihoods(rng, ped, 200)
    rng, _ = random_pedigree(seed)
    return ped, [("clear",) + clear, ("adversarial",) + random_likelihoods(rng, ped, 200)]


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_against_the_enumeration(seed, mrate, tmp_path_factory):
    ped, both = batches(seed)  # loops on every third seed
    model = fs.make_model(ped, mrate=mrate)
    fn = kernel(seed, tmp_path_factory)
    for name, lk, flags in both:
        assert set(np.unique(flags)) == {0, 1, 2, 3}
        ref = M.brute(ped, mrate, lk, flags)
        out = run_maxmarg(fn, model, lk, flags)
        what = "seed %d mrate %g %s" % (seed, mrate, name)
        compared = M.check(out, ref, what)
        ok = out[2] == 0
        assert ok.sum() > 100
        zeros = int((ref.maxmarg[ok] == 0).sum())
        print("%s: %d sites, %d entries at RTOL, %d exact zeros" % (what, ok.sum(), compared, zeros))
        assert compared > 0.5 * (3 * ped.n + 2) * ok.sum()
        if mrate == 0.0:
            assert zeros > 0 and np.all(out[0][ok][ref.maxmarg[ok] == 0] == 0.0)
        # every row's maximum is the best configuration's posterior, and the runner-up is not above it
        np.testing.assert_allclose(out[0][ok].max(axis=2), np.broadcast_to(out[1][ok][:, :1], (ok.sum(), ped.n)), rtol=RTOL, atol=0)
        assert np.all(out[1][ok][:, 1] <= out[1][ok][:, 0] * (1 + RTOL))


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_top0_has_the_map_kernels_bits(seed, mrate, tmp_path_factory):
    ped, both = batches(seed)
    model = fs.make_model(ped, mrate=mrate)
    fn = kernel(seed, tmp_path_factory)
    fmap = build_map_host(fs.make_model(ped), tmp_path_factory.mktemp("map_for_maxmarg_%d" % seed))[0]
    for name, lk, flags in both:
        _, top, st = run_maxmarg(fn, model, lk, flags)
        _, post, mst = run_map_host(fmap, model, lk, flags)
        assert np.array_equal(st, mst)
        assert np.array_equal(top[:, 0].view(np.uint64), post.view(np.uint64)), name


@pytest.mark.parametrize("seed", [1, 0, 15])  # random_pedigree: loop-free, one loop, three conditioned members
def test_the_four_variants_give_the_same_bits(seed, tmp_path_factory):
    ped, both = batches(seed)
    model = fs.make_model(ped, mrate=1e-4)
    ctx = fs.Context(model, device=-1)
    assert ctx.plan()["elim_conditioned_members"] == {1: 0, 0: 1, 15: 3}[seed]
    ctx.close()
    for name, lk, flags in both:
        outs = [run_maxmarg(kernel(seed, tmp_path_factory, variant=v), model, lk, flags) for v in range(N_VARIANTS)]
        for out in outs[1:]:
            assert same_bits(out, outs[0]), name


@pytest.mark.parametrize("seed", [1, 0, 15])
def test_site_prior_form(seed, tmp_path_factory):
    """Under the model's rows the plain form's bits; under Hardy-Weinberg rows the reference with that prior."""
    ped, both = batches(seed)
    for variant in (0, 2):
        plain = kernel(seed, tmp_path_factory, variant)
        fn = kernel(seed, tmp_path_factory, variant, prior=True)
        for mrate in MRATES:
            model = fs.make_model(ped, mrate=mrate)
            for name, lk, flags in both:
                want = run_maxmarg(plain, model, lk, flags)
                assert same_bits(run_maxmarg(fn, model, lk, flags, P.model_rows(model, flags)), want)
                hwe = fs.hwe_priors(np.random.RandomState(7 + ped.n).uniform(0.01, 0.5, len(lk)))
                got = run_maxmarg(fn, model, lk, flags, hwe)
                M.check(got, M.elimination(ped, mrate, lk, flags, hwe), "seed %d variant %d mrate %g %s, HWE rows" % (seed, variant, mrate, name))
                assert not same_bits(got[:2], want[:2])


def test_each_output_may_be_null(tmp_path_factory):
    ped, both = batches(1)
    model = fs.make_model(ped)
    _, lk, flags = both[1]
    n = len(lk)
    fn = kernel(1, tmp_path_factory)
    full = run_maxmarg(fn, model, lk, flags)
    assert (full[2] != 0).any() and (full[2] == 0).any()
    for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
        got = run_maxmarg(fn, model, lk, flags, want=want)
        untouched = (np.full((n, ped.n, 3), SENTINEL), np.full((n, 2), SENTINEL), np.full(n, ST_SENTINEL, np.uint8))
        for k in range(3):
            assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_the_helper_matches_the_enumeration(seed, mrate):
    """tests/_maxmarg.py's elimination against its brute force, on the seeds above (loops included)."""
    ped, both = batches(seed)
    for name, lk, flags in both:
        ref, got = M.brute(ped, mrate, lk, flags), M.elimination(ped, mrate, lk, flags)
        assert np.array_equal(ref.support[ref.status == 0], got.support[ref.status == 0])
        assert np.array_equal(ref.pair[ref.status == 0], got.pair[ref.status == 0])
        M.check((got.maxmarg, got.top, got.status), ref, "helper, seed %d mrate %g %s" % (seed, mrate, name))


@pytest.mark.parametrize("name", ["random15", "wide24", "wide48"])
def test_beyond_the_enumeration(name, tmp_path):
    """A three-cut pedigree, 24 members and 48 (the lean form: the messages towards the roots are formed twice), against the
    elimination helper.  Sites whose total lies below 1e-280: status only
    (test_map_host.test_wide_pedigrees' rule; 2 may fall on one side only there)."""
    ped = wide_pedigree(int(name[4:])) if name.startswith("wide") else side_variant_pedigree(name)
    ped.relations()
    lk, flags = random_likelihoods(np.random.RandomState(ped.n), ped, 300, max_pl=40)
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        fn, plan, src = build_maxmarg_host(model, tmp_path / ("k%g" % mrate))
        assert ("conditioned on 3 member(s)" in src.splitlines()[0]) == (name == "random15")
        assert ("#define l0_0 lgv[0]" in src) == ("      double Xc0;\n" in src) == (name == "wide48")
        ref = M.elimination(ped, mrate, lk, flags)
        out = run_maxmarg(fn, model, lk, flags)
        tiny = (ref.status != 1) & ~(ref.z >= M.TINY)
        differ = (out[2] == 0) != (ref.status == 0)
        assert np.all(tiny[differ]) and np.array_equal(out[2][ref.status == 1], ref.status[ref.status == 1])
        ok = (out[2] == 0) & (ref.status == 0) & ~tiny
        assert ok.sum() > 20
        pinned = ref._replace(status=np.where(tiny, out[2], ref.status).astype(np.uint8))
        compared = M.check(out, pinned, "%s mrate %g" % (name, mrate), sites=ok)
        print("%s mrate %g: %d sites compared, %d tiny, %d entries at RTOL" % (name, mrate, ok.sum(), tiny.sum(), compared))


def test_generating_the_maxmarg_kernel_leaves_the_other_sources_alone(tmp_path):
    """The back-pointer switch must not reach the text of the existing kernels (the MAP kernel's above all)."""
    ped = random_pedigree(3)[1]  # a loop pedigree
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    keys = ("elim_code_object", "trio_code_object", "map_code_object", "map_prior_code_object", "loo_code_object", "evidence_code_object")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        for opt, v in (("trio_kernels", 3), ("map_kernels", 1), ("map_prior_kernels", 1), ("loo_kernels", 1), ("evidence_kernels", 1)):
            ctx.set_option(opt, v)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        ctx.set_option("maxmarg_kernels", 1)
        ctx.set_option("maxmarg_prior_kernels", 1)
        after = ctx.plan()
        assert after["maxmarg_code_object"] and after["maxmarg_code_object"] not in [before[k] for k in keys]
        ctx.close()
        # a fresh context that generates the new kernel FIRST names the same objects
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("maxmarg_prior_kernels", 1)
        ctx.set_option("maxmarg_kernels", 1)
        for opt, v in (("trio_kernels", 3), ("map_kernels", 1), ("map_prior_kernels", 1), ("loo_kernels", 1), ("evidence_kernels", 1)):
            ctx.set_option(opt, v)
        again = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] == again[k]
        assert open(after[k][:-6] + ".hip").read() == texts[k]
    assert again["maxmarg_code_object"] == after["maxmarg_code_object"]
    assert again["maxmarg_prior_code_object"] == after["maxmarg_prior_code_object"]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("maxmarg_kernels", "maxmarg_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*max-marginals \(sum-product engine\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = fs.synthetic_pedigree("ped10")
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["maxmarg_code_object"] == "" and plan["maxmarg_variant"] == -1
        assert plan["maxmarg_prior_code_object"] == "" and plan["maxmarg_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="maxmarg_kernels takes 1"):
            ctx.set_option("maxmarg_kernels", 2)
        ctx.set_option("maxmarg_kernels", 1)
        ctx.set_option("maxmarg_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["maxmarg_code_object"].endswith(".hsaco") and 0 <= plan["maxmarg_variant"] < N_VARIANTS
        assert plan["maxmarg_prior_code_object"].endswith(".hsaco") and plan["maxmarg_prior_variant"] == plan["maxmarg_variant"]
        assert plan["maxmarg_prior_code_object"] != plan["maxmarg_code_object"] and plan["map_code_object"] == ""
        with pytest.raises(fs.FamseqError, match=r"\(-2\)|without a device"):
            ctx.maxmarg_batch(lk=np.ones((1, ped.n, 3)))
        with pytest.raises(fs.FamseqError, match=r"\(-2\)|without a device"):
            ctx.maxmarg_prior_batch(np.ones((1, 6)), lk=np.ones((1, ped.n, 3)))
        ctx.close()


def test_joint_call_quality():
    rows = np.array([[[0.5, 0.25, 0.0], [0.2, 0.2, 0.1], [0.0, 0.0, 0.7], [np.nan, 0.1, 0.2]],
                     [[0.1, 0.1, 0.1], [0.0, 0.3, 0.003], [1e-300, 0.0, 1e-310], [0.0, 0.5, 0.0]]])
    jgt, jgq = fs.joint_call_quality(rows)
    assert jgt.dtype == np.int8 and jgq.dtype == np.float64 and jgt.shape == (2, 4) and jgq.shape == (2, 4)
    assert jgt.tolist() == [[0, 0, 2, -1], [0, 1, 0, 1]]  # ties go to the lowest genotype; a NaN row is -1
    want = np.array([[-10 * np.log10(0.5), 0.0, np.inf, np.nan], [0.0, 20.0, -10 * np.log10(1e-310 / 1e-300), np.inf]])
    assert np.isnan(jgq[0, 3]) and np.isposinf(jgq[0, 2]) and np.isposinf(jgq[1, 3])
    fin = np.isfinite(want)
    np.testing.assert_allclose(jgq[fin], want[fin], rtol=1e-12, atol=0)
    assert jgq[0, 1] == 0.0 and jgq[1, 0] == 0.0  # an exact tie: quality 0
    # whole NaN batches and a single row pass through
    jgt, jgq = fs.joint_call_quality(np.full((3, 2, 3), np.nan))
    assert np.all(jgt == -1) and np.all(np.isnan(jgq))
    jgt, jgq = fs.joint_call_quality([0.1, 0.6, 0.3])
    assert jgt == 1 and jgq == pytest.approx(-10 * np.log10(0.5))
