"""The MAP kernel's arithmetic (famseq_map: the most probable joint genotype configuration and its posterior), checked without
a GPU.

As in test_trio_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++.  References: a 3^N enumeration written here (the weights of test_trio_host.brute_joint) and, beyond its reach, the numpy
bucket elimination of tests/_maxproduct.py, itself checked here against the enumeration and against oracle/sum_product.py.

Ties.  The kernel's arg-max is deterministic (lowest genotype first, strictly greater replaces) but two configurations whose
weights differ by rounding only may compare differently under the enumeration's order of multiplication.  So on the inputs that
have ties (integer PLs: about a quarter of the sites) the criterion is the one that defines a MAP — the enumeration's weight of
the RETURNED configuration is within 1e-9 of the enumeration's maximum — and only on continuous PLs, where the enumeration
itself finds no runner-up within 1e-6, must the configuration be the enumeration's arg-max exactly.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _maxproduct as mp
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_generated_host import factor_tables, host_source

RTOL = 1e-9      # the project's bar for posteriors
NEAR_TIE = 1e-6  # a runner-up this close (relative) to the maximum: the exact comparison may leave the site out
MRATES = [1e-7, 1e-4, 0.0]


def build_map_host(model, where, variant=None):
    """Generate the MAP kernel for a one-lane workgroup on a plan-only context, compile it for the host.  -> (fn, plan)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option("map_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    src = open(plan["map_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and "famseq_map" in src
    tag = "t" if variant is None else "t%d" % variant
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), "famseq_map")
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double]
    return fn, plan


def run_map_host(fn, model, lk, flags):
    s, n = lk.shape[0], lk.shape[1]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    gt = np.full((s, n), 77, np.int8)
    post = np.full(s, -5.0)
    st = np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    fn(a.ctypes.data, fl.ctypes.data, gt.ctypes.data, post.ctypes.data, st.ctypes.data, s, tc.ctypes.data, 1.0)
    return gt, post, st


def brute_weights(ped, mrate, lk, flags):
    """-> (G[N, 3^N] the configurations, w[S, 3^N] their weights (NaN rows where status != 0), status[S])."""
    mo, fa = ped.relations()
    n = ped.n
    gender = np.asarray(ped.genders)
    pcp2, xf, xm = fs.transmission_tables(mrate)
    G = np.indices((3,) * n).reshape(n, -1)
    W = np.full((lk.shape[0], G.shape[1]), np.nan)
    status = np.zeros(lk.shape[0], np.uint8)
    for s in range(lk.shape[0]):
        known, chrx = flags[s] & 1, flags[s] & 2
        autos = np.array(mp.GK if known else mp.GN)
        male = np.array(mp.GXK if known else mp.GXN) if chrx else autos
        prior = [male if gender[p] == 1 else autos for p in range(n)]
        if any(((lk[s, p] * prior[p]).sum() <= 0) for p in range(n)):
            status[s] = 1
            continue
        w = np.full(G.shape[1], 1e7)
        for p in range(n):
            if mo[p] < 0:
                t = prior[p][G[p]]
            else:
                T = ((xm if gender[p] == 1 else xf) if chrx else pcp2)
                t = T[9 * G[p] + 3 * G[mo[p]] + G[fa[p]]]
            w = w * (t * lk[s, p][G[p]])
        if w.sum() <= 0 or w.max() <= 0:
            status[s] = 2
            continue
        W[s] = w
    return G, W, status


def config_index(gt):
    n = gt.shape[1]
    return (gt.astype(np.int64) * 3 ** np.arange(n - 1, -1, -1)).sum(axis=1)


def clear_likelihoods(rng, ped, n_sites):
    """Every member sequenced, PLs continuous and uniform in [0, 30): no exact ties."""
    return 10.0 ** (-rng.uniform(0, 30, size=(n_sites, ped.n, 3)) / 10.0), rng.randint(0, 4, n_sites).astype(np.uint8)


_KERNELS = {}


def kernel(seed, tmp_path_factory, variant=None):
    key = (seed, variant)
    if key not in _KERNELS:
        rng, ped = random_pedigree(seed)
        ped.relations()
        _KERNELS[key] = build_map_host(fs.make_model(ped), tmp_path_factory.mktemp("map_%d" % seed), variant)[0]
    return _KERNELS[key]


def check_failed_sites(gt, post, st):
    bad = st != 0
    assert np.all(gt[bad] == -1) and np.all(np.isnan(post[bad]))
    assert np.all((gt[~bad] >= 0) & (gt[~bad] <= 2)) and np.all(np.isfinite(post[~bad]))


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_clear_sites_give_the_enumerations_argmax(seed, mrate, tmp_path_factory):
    rng, ped = random_pedigree(seed)  # loops on every third seed
    ped.relations()
    model = fs.make_model(ped, mrate=mrate)
    fn = kernel(seed, tmp_path_factory)
    lk, flags = clear_likelihoods(rng, ped, 200)
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    gt, post, st = run_map_host(fn, model, lk, flags)
    G, W, ref_st = brute_weights(ped, mrate, lk, flags)
    assert np.array_equal(st, ref_st)
    check_failed_sites(gt, post, st)
    ok = st == 0
    assert ok.sum() > 100
    top2 = np.sort(W[ok], axis=1)[:, -2:]
    near = top2[:, 0] >= (1 - NEAR_TIE) * top2[:, 1]  # the enumeration's own runner-up within 1e-6 of its maximum
    print("seed %d mrate %g: %d sites, %d near ties left out" % (seed, mrate, ok.sum(), near.sum()))
    assert near.sum() <= 0.01 * ok.sum()
    ref_gt = G[:, np.argmax(W[ok], axis=1)].T
    assert np.array_equal(gt[ok][~near], ref_gt[~near])
    np.testing.assert_allclose(post[ok], W[ok].max(axis=1) / W[ok].sum(axis=1), rtol=RTOL, atol=0)


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_adversarial_sites_give_a_maximal_configuration(seed, mrate, tmp_path_factory):
    """Integer PLs, hard zeros, sharp sites, unsequenced members: exact and near ties on about a quarter of the sites.  The
    returned configuration's weight under the enumeration is its maximum (to 1e-9) on every site, none left out."""
    rng, ped = random_pedigree(seed)
    ped.relations()
    model = fs.make_model(ped, mrate=mrate)
    fn = kernel(seed, tmp_path_factory)
    lk, flags = random_likelihoods(rng, ped, 200)
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    gt, post, st = run_map_host(fn, model, lk, flags)
    G, W, ref_st = brute_weights(ped, mrate, lk, flags)
    assert np.array_equal(st, ref_st)
    check_failed_sites(gt, post, st)
    ok = st == 0
    assert ok.sum() > 100
    idx = config_index(gt[ok])
    assert np.array_equal(G[:, idx].T, gt[ok])
    w_ret, w_max = W[ok][np.arange(ok.sum()), idx], W[ok].max(axis=1)
    print("seed %d mrate %g: worst w_returned / w_max = %.17g" % (seed, mrate, (w_ret / w_max).min()))
    assert np.all(w_ret >= (1 - 1e-9) * w_max)
    np.testing.assert_allclose(post[ok], w_max / W[ok].sum(axis=1), rtol=RTOL, atol=0)


def test_map_is_consistent_where_the_marginal_call_is_not(tmp_path_factory):
    """Mutation rate 0: every MAP configuration is Mendelian-consistent; the member-wise arg-max of the marginals (what FGT
    is) is not, on some sites of the same inputs — the case the joint call exists for."""
    map_bad = marg_bad = sites = 0
    for seed in range(10):
        rng, ped = random_pedigree(seed)
        ped.relations()
        model = fs.make_model(ped, mrate=0.0)
        fn = kernel(seed, tmp_path_factory)
        lk, flags = random_likelihoods(rng, ped, 200)
        gt, post, st = run_map_host(fn, model, lk, flags)
        G, W, ref_st = brute_weights(ped, 0.0, lk, flags)
        assert np.array_equal(st, ref_st)
        ok = st == 0
        marg_gt = np.zeros((ok.sum(), ped.n), np.int8)
        for p in range(ped.n):  # the enumeration's marginals, member by member
            m = np.stack([np.where(G[p] == g, W[ok], 0.0).sum(axis=1) for g in range(3)], axis=1)
            marg_gt[:, p] = np.argmax(m, axis=1)
        sites += ok.sum()
        map_bad += (~mp.mendelian_consistent(ped, gt[ok], flags[ok])).sum()
        marg_bad += (~mp.mendelian_consistent(ped, marg_gt, flags[ok])).sum()
    print("%d sites: %d inconsistent MAP configurations, %d inconsistent marginal calls" % (sites, map_bad, marg_bad))
    assert map_bad == 0
    assert marg_bad >= 1


@pytest.mark.parametrize("mrate", [1e-7, 0.0])
@pytest.mark.parametrize("seed", range(10))
def test_the_helper_matches_the_enumeration(seed, mrate):
    """tests/_maxproduct.py against the brute force, on the seeds above (loops included): status, maximum, total, marginals."""
    rng, ped = random_pedigree(seed)
    ped.relations()
    lk, flags = random_likelihoods(rng, ped, 200)
    G, W, ref_st = brute_weights(ped, mrate, lk, flags)
    gt, wmax, z, st = mp.max_product(ped, mrate, lk, flags)
    assert np.array_equal(st, ref_st)
    ok = st == 0
    np.testing.assert_allclose(wmax[ok], W[ok].max(axis=1), rtol=RTOL, atol=0)
    np.testing.assert_allclose(z[ok], W[ok].sum(axis=1), rtol=RTOL, atol=0)
    w_ret = W[ok][np.arange(ok.sum()), config_index(gt[ok])]
    assert np.all(w_ret >= (1 - 1e-9) * W[ok].max(axis=1))
    np.testing.assert_allclose(mp.config_weight(ped, mrate, lk[ok], flags[ok], gt[ok]), w_ret, rtol=1e-12, atol=0)
    marg = mp.marginals(ped, mrate, lk[ok], flags[ok])
    for p in range(ped.n):
        ref = np.stack([np.where(G[p] == g, W[ok], 0.0).sum(axis=1) for g in range(3)], axis=1) / W[ok].sum(axis=1)[:, None]
        np.testing.assert_allclose(marg[:, p], ref, rtol=RTOL, atol=1e-300)


@pytest.mark.parametrize("n", [24, 32, 48, 64, 128])
def test_wide_pedigrees(n, tmp_path):
    """Beyond the enumeration's reach: against the helper's max-product, whose marginals are checked against the sum-product
    oracle's here."""
    import oracle.sum_product as sp

    ped = wide_pedigree(n)
    ped.relations()
    lk, flags = random_likelihoods(np.random.RandomState(n), ped, 300, max_pl=40)
    model = fs.make_model(ped)
    fn, _ = build_map_host(model, tmp_path / "k")
    gt, post, st = run_map_host(fn, model, lk, flags)
    ref_gt, wmax, z, ref_st = mp.max_product(ped, 1e-7, lk, flags)
    check_failed_sites(gt, post, st)
    # the helper's sum pass against the oracle (lc > 1: no shortcut, every site the full network)
    o_post, _, o_st = sp.pedigree_posterior(ped, lk, flags, lc=2.0)
    # sites whose total mass is below 1e-280 (where every implementation's digits are what gradual underflow leaves): status only
    # (status 2 on one side only happens there and nowhere else: a total at the bottom of the double range underflows in one
    # order of products and not in another)
    tiny = (ref_st != 1) & ~(z >= 1e-280)
    both = (ref_st == 0) & (o_st == 0) & ~tiny
    marg = mp.marginals(ped, 1e-7, lk[both], flags[both])
    # (an entry is compared where its unnormalised value, marginal x total mass, is itself above 1e-280: below that the sum pass
    # works in subnormal numbers, which carry fewer than 1e-9's digits)
    sel = o_post[both] * z[both][:, None, None] >= 1e-280
    assert sel.mean() > 0.5
    np.testing.assert_allclose(marg[sel], o_post[both][sel], rtol=RTOL, atol=0)
    differ = (st == 0) != (ref_st == 0)
    assert np.all(tiny[differ]) and np.array_equal(st[ref_st == 1], ref_st[ref_st == 1])
    ok = (st == 0) & (ref_st == 0) & ~tiny
    assert ok.sum() > 20
    w_ret = mp.config_weight(ped, 1e-7, lk[ok], flags[ok], gt[ok])
    print("n %d: %d sites compared, %d tiny; worst w_returned / w_max = %.17g" % (n, ok.sum(), tiny.sum(), (w_ret / wmax[ok]).min()))
    assert np.all(w_ret >= (1 - 1e-9) * wmax[ok])
    np.testing.assert_allclose(post[ok], w_ret / z[ok], rtol=RTOL, atol=0)


def loop_and_tree_seeds():
    return [1, 0]  # random_pedigree: loop-free, with a loop


@pytest.mark.parametrize("seed", loop_and_tree_seeds())
def test_the_four_variants_give_the_same_bits(seed, tmp_path_factory):
    rng, ped = random_pedigree(seed)
    ped.relations()
    model = fs.make_model(ped, mrate=1e-4)
    ctx = fs.Context(model, device=-1)
    assert (ctx.plan()["elim_conditioned_members"] > 0) == (seed == 0)
    ctx.close()
    lk, flags = random_likelihoods(rng, ped, 128)
    outs = [run_map_host(kernel(seed, tmp_path_factory, variant=v), model, lk, flags) for v in range(4)]
    for gt, post, st in outs[1:]:
        assert np.array_equal(gt, outs[0][0]) and np.array_equal(st, outs[0][2])
        assert np.array_equal(post.view(np.uint64), outs[0][1].view(np.uint64))


def test_generating_the_map_kernel_leaves_the_other_sources_alone(tmp_path):
    """The semiring switch must not reach the text of the existing kernels (their code objects are cached by content hash)."""
    rng, ped = random_pedigree(3)  # a loop pedigree
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    keys = ("elim_code_object", "trio_code_object", "elim_call_code_object")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys if before.get(k)}
        assert "elim_code_object" in texts and "trio_code_object" in texts
        ctx.set_option("map_kernels", 1)
        after = ctx.plan()
        assert after["map_code_object"] and after["map_code_object"] not in [before[k] for k in texts]
        ctx.close()
        # a fresh context that generates the MAP kernel FIRST names the same objects
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("map_kernels", 1)
        ctx.set_option("trio_kernels", 3)
        again = ctx.plan()
        ctx.close()
    for k in texts:
        assert before[k] == after[k] == again[k]
        assert open(after[k][:-6] + ".hip").read() == texts[k]
    assert again["map_code_object"] == after["map_code_object"]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.set_option("map_kernels", 1)
    ctx.close()
    rng, ped = random_pedigree(1)
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["map_code_object"] == "" and plan["map_variant"] == -1
        ctx.set_option("map_kernels", 1)
        plan = ctx.plan()
        assert plan["map_code_object"].endswith(".hsaco") and 0 <= plan["map_variant"] < 4
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.map_batch(lk=np.ones((1, ped.n, 3)))
        ctx.close()
