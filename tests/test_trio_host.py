"""The trio kernel's arithmetic (famseq_trio: joint posteriors of child and parents, de novo posteriors), checked without a GPU.

As in test_generated_host.py, the kernel is generated for a one-lane workgroup and its source compiled with g++; here it is
compared with a brute-force enumeration of the pedigree network written below (the weight of a configuration as
oracle/bn_oracle.c forms it: 1e7 times, per member, prior * lk for a founder and T[g | g_mother, g_father] * lk otherwise),
and, on the wide pedigrees the enumeration cannot reach, with the sum-product oracle's marginals.
"""
import ctypes as C
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_generated_host import factor_tables, host_source

GN, GK, GXN, GXK = (0.9985, 0.001, 0.0005), (0.45, 0.1, 0.45), (0.999, 0, 0.001), (0.5, 0, 0.5)
RTOL = 1e-9


def build_trio_host(model, form, where, variant=None):
    """Generate the trio kernel of output form `form` (1 dnm, 2 joint, 3 both) for a one-lane workgroup, compile it for the
    host.  -> (fn, children)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option("trio_kernels", form)
        obj = ctx.plan()["trio_code_object"]
        children = ctx.trio_children()
        ctx.close()
    src = open(obj[:-6] + ".hip").read()
    assert "#define BT 1\n" in src and "famseq_trio" in src
    cpp, so = str(where / "t.cpp"), str(where / "t.so")
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), "famseq_trio")
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double]
    return fn, children


def run_trio_host(fn, model, k, lk, flags, joint=True, dnm=True):
    s = lk.shape[0]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    j = np.full((s, k, 27), -1.0) if joint else None
    d = np.full((s, k), -1.0) if dnm else None
    st = np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    fn(a.ctypes.data, fl.ctypes.data, None if j is None else j.ctypes.data, None if d is None else d.ctypes.data, st.ctypes.data, s,
       tc.ctypes.data, 1.0)
    return j, d, st


def dnm_masks(children, genders):
    """[2][K][27] bool: where the mutation-free transmission table is 0 (autosome; chrX: the son's or the daughter's)."""
    a0, xf0, xm0 = fs.transmission_tables(0.0)
    auto = np.array([a0 == 0 for _ in children]).reshape(-1, 27)
    x = np.array([(xm0 if genders[c] == 1 else xf0) == 0 for c in children]).reshape(-1, 27)
    return auto, x


def brute_joint(ped, mrate, lk, flags):
    """-> (joint[S,K,27], status[S]) by enumerating all 3^N configurations."""
    mo, fa = ped.relations()
    n = ped.n
    gender = np.asarray(ped.genders)
    children = [p for p in range(n) if mo[p] >= 0]
    pcp2, xf, xm = fs.transmission_tables(mrate)
    G = np.indices((3,) * n).reshape(n, -1)
    joint = np.full((lk.shape[0], len(children), 27), np.nan)
    status = np.zeros(lk.shape[0], np.uint8)
    for s in range(lk.shape[0]):
        known, chrx = flags[s] & 1, flags[s] & 2
        autos = np.array(GK if known else GN)
        male = np.array(GXK if known else GXN) if chrx else autos
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
        tot = w.sum()
        if tot <= 0:
            status[s] = 2
            continue
        for k, c in enumerate(children):
            joint[s, k] = np.bincount(9 * G[c] + 3 * G[mo[c]] + G[fa[c]], weights=w, minlength=27) / tot
    return joint, status


def check_joint(joint, ref):
    big = np.nanmax(ref, axis=-1, keepdims=True)
    sel = ref >= 1e-280 * big
    np.testing.assert_allclose(joint[sel], ref[sel], rtol=RTOL, atol=0)
    assert np.all(np.abs(joint - ref)[~sel] <= 1e-270 * np.broadcast_to(big, ref.shape)[~sel])


def check_dnm(dnm, ref_joint, children, genders, flags):
    auto, x = dnm_masks(children, genders)
    m = np.where((flags & 2)[:, None, None] != 0, x[None], auto[None])
    ref = np.where(m, ref_joint, 0.0).sum(axis=-1)
    sel = ref >= 1e-280
    np.testing.assert_allclose(dnm[sel], ref[sel], rtol=RTOL, atol=0)
    assert np.all(np.abs(dnm[~sel]) <= 1e-270)
    return ref


_KERNELS = {}


def kernel(seed, form, tmp_path_factory, variant=None):
    key = (seed, form, variant)
    if key not in _KERNELS:
        rng, ped = random_pedigree(seed)
        ped.relations()
        model = fs.make_model(ped)
        _KERNELS[key] = build_trio_host(model, form, tmp_path_factory.mktemp("trio_%d_%d" % (seed, form)), variant)
    return _KERNELS[key]


@pytest.mark.parametrize("mrate", [1e-7, 1e-4, 0.0])
@pytest.mark.parametrize("seed", range(10))
def test_trio_matches_the_enumeration(seed, mrate, tmp_path_factory):
    rng, ped = random_pedigree(seed)  # loops on every third seed
    ped.relations()
    model = fs.make_model(ped, mrate=mrate)
    fn, children = kernel(seed, 3, tmp_path_factory)
    assert list(children) == [p for p in range(ped.n) if ped.relations()[0][p] >= 0]
    lk, flags = random_likelihoods(rng, ped, 200)
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    joint, dnm, st = run_trio_host(fn, model, len(children), lk, flags)
    ref, ref_st = brute_joint(ped, mrate, lk, flags)
    assert np.array_equal(st, ref_st)
    ok = st == 0
    assert ok.sum() > 100
    np.testing.assert_allclose(joint[ok].sum(axis=-1), 1.0, rtol=1e-12)
    check_joint(joint[ok], ref[ok])
    ref_dnm = check_dnm(dnm[ok], ref[ok], children, ped.genders, flags[ok])
    if mrate == 0:
        assert np.all(dnm[ok] == 0.0)
    elif len(children):
        assert ref_dnm.max() > 0
    assert np.all(np.isnan(joint[~ok])) and np.all(np.isnan(dnm[~ok]))


@pytest.mark.parametrize("seed", [0, 4])
def test_output_forms_give_the_same_bits(seed, tmp_path_factory):
    """dnm-only, joint-only and both: the same values to the bit; a NULL output leaves the other alone.  Also the chrX-loop
    variant (transmission entries through a wave-uniform pointer) against the plain one."""
    rng, ped = random_pedigree(seed)
    model = fs.make_model(ped, mrate=1e-4)
    lk, flags = random_likelihoods(rng, ped, 64)
    fn3, children = kernel(seed, 3, tmp_path_factory)
    k = len(children)
    j3, d3, s3 = run_trio_host(fn3, model, k, lk, flags)
    j3n, _, s3n = run_trio_host(fn3, model, k, lk, flags, dnm=False)
    _, d3n, _ = run_trio_host(fn3, model, k, lk, flags, joint=False)
    fn1, _ = kernel(seed, 1, tmp_path_factory)
    _, d1, s1 = run_trio_host(fn1, model, k, lk, flags, joint=False)
    fn2, _ = kernel(seed, 2, tmp_path_factory)
    j2, _, s2 = run_trio_host(fn2, model, k, lk, flags, dnm=False)
    fnv, _ = kernel(seed, 3, tmp_path_factory, variant=2)
    jv, dv, sv = run_trio_host(fnv, model, k, lk, flags)
    for st in (s3n, s1, s2, sv):
        assert np.array_equal(st, s3)
    for d in (d3n, d1):
        assert np.array_equal(d.view(np.uint64), d3.view(np.uint64))
    for j in (j3n, j2):
        assert np.array_equal(j.view(np.uint64), j3.view(np.uint64))
    np.testing.assert_allclose(jv[s3 == 0], j3[s3 == 0], rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(dv[s3 == 0], d3[s3 == 0], rtol=RTOL, atol=1e-300)


def test_failed_sites_are_nan(tmp_path_factory):
    rng, ped = random_pedigree(1)
    model = fs.make_model(ped)
    fn, children = kernel(1, 3, tmp_path_factory)
    lk, flags = random_likelihoods(rng, ped, 8)
    lk[:] = np.where(lk > 0, lk, 0.5)
    lk[3, 0, :] = 0.0  # an all-zero likelihood row
    joint, dnm, st = run_trio_host(fn, model, len(children), lk, flags)
    assert st[3] in (1, 2)
    assert np.all(np.isnan(joint[3])) and np.all(np.isnan(dnm[3]))
    assert np.all(st[[0, 1, 2, 4, 5, 6, 7]] == 0)


def marginals_from_joint(joint, children, mo, fa, n):
    """Each child's marginal from its joint (summed over the parents), each parent's from the joint of each of its children."""
    J = joint.reshape(joint.shape[0], len(children), 3, 3, 3)
    out = {}
    for k, c in enumerate(children):
        out.setdefault(c, []).append(J[:, k].sum(axis=(2, 3)))
        out.setdefault(int(mo[c]), []).append(J[:, k].sum(axis=(1, 3)))
        out.setdefault(int(fa[c]), []).append(J[:, k].sum(axis=(1, 2)))
    return out


def wide_likelihoods(ped, seed, n_sites=300):
    """random_likelihoods without its sharp rows' 1e-40 (many members that contradict their parents that sharply put a
    site's whole mass below the double range, where every implementation's digits are what gradual underflow leaves)."""
    lk, flags = random_likelihoods(np.random.RandomState(seed), ped, n_sites, max_pl=20)
    lk[(lk > 0) & (lk < 1e-2)] = 1e-2
    return lk, flags


@pytest.mark.parametrize("n", [24, 32, 48, 128])
def test_wide_pedigrees_marginals(n, tmp_path):
    """Beyond the enumeration's reach: every child's and parent's marginal from the trio joints equals the sum-product
    oracle's marginal (pinned to the reference's -method 2)."""
    import oracle.sum_product as sp

    ped = wide_pedigree(n)
    mo, fa = ped.relations()
    lk, flags = wide_likelihoods(ped, n)
    model = fs.make_model(ped)
    fn, children = build_trio_host(model, 3, tmp_path / "k")
    joint, dnm, st = run_trio_host(fn, model, len(children), lk, flags)
    post, _, ref_st = sp.pedigree_posterior(ped, lk, flags, lc=2.0)  # lc > 1: no shortcut, every site the full network
    # (a site whose total weight sits at the bottom of the double range — fifty members that each contradict their parents
    # a little — underflows in one order of products and not in another: status 2 on one side only, rare)
    differ = (st == 0) != (ref_st == 0)
    assert differ.sum() <= 0.02 * len(st) and np.all(st[differ & (st != 0)] == 2)
    ok = (ref_st == 0) & (st == 0)
    assert ok.sum() > 20
    margs = marginals_from_joint(joint[ok], children, mo, fa, ped.n)
    for p, rows in margs.items():
        for r in rows:
            sel = post[ok, p] >= 1e-280
            np.testing.assert_allclose(r[sel], post[ok, p][sel], rtol=RTOL, atol=0)


def test_a_pedigree_the_engine_refuses():
    """Four disjoint cousin marriages need four conditioned members: FAMSEQ_E_ARG with the engine's message."""
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.trio_children()
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.set_option("trio_kernels", 1)
    ctx.close()
