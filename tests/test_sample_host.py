"""The sampling kernel's arithmetic and law (famseq_sample / famseq_sample_prior: per site and draw a joint genotype
configuration drawn with probability w(g) / Z, and that probability), checked without a GPU.

As in test_map_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++.  References: up to nine members the 3^N enumeration of test_map_host.brute_weights (under per-site priors the same product
over tests/_prior_joint.py's factors), beyond that tests/_maxproduct.py.

The law is tested with a fixed seed against the enumeration's probabilities: a cell whose expected count n p is at least 10 must
lie within 6 sqrt(n p (1 - p)) of it — over the few thousand cells compared a false-alarm chance below 1e-5, and with the seed
fixed the test is deterministic: a failure is a wrong law.  Cells of smaller expectation are pooled into one per table, which is
held to the same rule where its own expectation reaches 10; below that its count is at most 10 + 6 sqrt(10) < 29, the rule's
upper limit for a cell of expectation 10, which such a cell's count lies below in distribution.  A cell of probability 0 has
count 0 exactly.
"""
import ctypes as C
import os
import re
import subprocess
from unittest import mock

import numpy as np
import pytest

import _maxproduct as mp
import _prior as P
import _prior_joint as J
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_generated_host import factor_tables, host_source
from test_map_host import brute_weights, clear_likelihoods, config_index

RTOL = 1e-9
MRATES = [1e-7, 1e-4, 0.0]
CSRC = os.path.join(os.path.dirname(fs.__file__), "csrc")
# the kernel's helpers are device functions: qualifiers the existing shim does not define away
SHIM_SAMPLE = "#define __device__\n#define __forceinline__ inline\n"


def build_sample_host(model, where, variant=None, prior=False):
    """Generate famseq_sample (prior: famseq_sample_prior) for a one-lane workgroup on a plan-only context, compile it for the
    host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    key, entry = ("sample_prior", "famseq_sample_prior") if prior else ("sample", "famseq_sample")
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
    open(cpp, "w").write(SHIM_SAMPLE + host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), entry)
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_ulong, C.c_long, C.c_int] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def run_sample(fn, model, lk, flags, n_draws, seed=0, site_base=0, prior=None):
    s, n = lk.shape[0], lk.shape[1]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    gt = np.full((s, n_draws, n), 77, np.int8)
    post = np.full((s, n_draws), -5.0)
    st = np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, gt.ctypes.data, post.ctypes.data, st.ctypes.data, s, tc.ctypes.data, 1.0, seed, site_base, n_draws]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return gt, post, st


_KERNELS = {}


def kernel(ped_key, ped, tmp_path_factory, variant=None, prior=False):
    key = (ped_key, variant, prior)
    if key not in _KERNELS:
        ped.relations()
        _KERNELS[key] = build_sample_host(fs.make_model(ped), tmp_path_factory.mktemp("sample"), variant, prior)[0]
    return _KERNELS[key]


def prior_weights(ped, mrate, lk, flags, prior):
    """brute_weights under per-site founder priors: the product of _prior_joint's factors over the 3^N configurations."""
    factors, fail = J.site_factors(ped, mrate, lk, flags, prior)
    G = np.indices((3,) * ped.n).reshape(ped.n, -1)
    W = np.full((lk.shape[0], G.shape[1]), 1e7)
    for vs, a in factors:
        W = W * a[(slice(None),) + tuple(G[u] for u in vs)]
    status = np.where(fail, 1, np.where(W.sum(axis=1) <= 0, 2, 0)).astype(np.uint8)
    W[status != 0] = np.nan
    return G, W, status


def check_draws(ped, mrate, flags, out, G, W, ref_st):
    """Check 2 of the module: status, failed sites, genotype range, samp_post and the drawn configurations' weights."""
    gt, post, st = out
    assert np.array_equal(st, ref_st)
    bad = st != 0
    assert np.all(gt[bad] == -1) and np.all(np.isnan(post[bad]))
    ok = ~bad
    assert ok.sum() > 100
    assert np.all((gt[ok] >= 0) & (gt[ok] <= 2))
    k = gt.shape[1]
    z = W[ok].sum(axis=1)
    for d in range(k):
        idx = config_index(gt[ok][:, d])
        assert np.array_equal(G[:, idx].T, gt[ok][:, d])
        w = W[ok][np.arange(ok.sum()), idx]
        assert np.all(w > 0)
        np.testing.assert_allclose(post[ok][:, d], w / z, rtol=RTOL, atol=0)
        if mrate == 0.0:
            assert np.all(mp.mendelian_consistent(ped, gt[ok][:, d], flags[ok]))


# ---- 1. Philox ----------------------------------------------------------------------------------------------------------

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr, key, want", KNOWN_ANSWERS)
def test_philox_reproduces_the_known_answers(ctr, key, want):
    assert [int(x) for x in fs.philox4x32(ctr, key)] == list(want)


def test_the_generated_source_carries_the_shared_philox_text(tmp_path):
    """philox_src.h is stringified into the kernel: its tokens, in order, stand in the generated source."""
    rng, ped = random_pedigree(1)
    ped.relations()
    _, _, src = build_sample_host(fs.make_model(ped), tmp_path / "k")
    text = open(os.path.join(CSRC, "philox_src.h")).read()
    body = text[text.index("FS_PHILOX_DEF(") + len("FS_PHILOX_DEF("):text.rindex(")")]
    squeeze = lambda t: re.sub(r"\s+", "", t)
    assert "0xD2511F53ull" in body and squeeze(body) in squeeze(src)


# ---- 2. every draw is what it says ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("mrate", MRATES)
@pytest.mark.parametrize("seed", range(10))
def test_every_draw_is_what_it_says(seed, mrate, tmp_path_factory):
    rng, ped = random_pedigree(seed)  # loops on every third seed
    ped.relations()
    model = fs.make_model(ped, mrate=mrate)
    fn = kernel(seed, ped, tmp_path_factory)
    lk, flags = random_likelihoods(rng, ped, 200)
    out = run_sample(fn, model, lk, flags, 5, seed=1234 + seed)
    G, W, ref_st = brute_weights(ped, mrate, lk, flags)
    check_draws(ped, mrate, flags, out, G, W, ref_st)


# ---- 3. the law -----------------------------------------------------------------------------------------------------------

LAW_CASES = ["trio", "quad"] + list(range(6))
ROWS, REPEAT, DRAWS = 8, 2048, 32


def law_pedigree(case):
    ped = fs.synthetic_pedigree(case) if isinstance(case, str) else random_pedigree(case)[1]
    ped.relations()
    return ped


def check_cells(obs, p, n, what):
    """The module docstring's rule on one table: obs[c] counts out of n against probabilities p[c]."""
    obs, p = np.asarray(obs, float).ravel(), np.asarray(p, float).ravel()
    e = n * p
    big = e >= 10
    dev = np.abs(obs[big] - e[big])
    lim = 6 * np.sqrt(e[big] * (1 - p[big]))
    assert np.all(dev <= lim), "%s: worst %.2f sd" % (what, (dev / np.maximum(lim / 6, 1e-300)).max())
    assert np.all(obs[p == 0] == 0), what
    po, pp = obs[~big].sum(), p[~big].sum()
    if n * pp >= 10:
        assert abs(po - n * pp) <= 6 * np.sqrt(n * pp * (1 - pp)), what
    else:
        assert po <= 10 + 6 * np.sqrt(10), what
    return int(big.sum())


def law_checks(ped, gt, G, W, rows, repeat, full_joint):
    """gt[rows * repeat, K, N]: row r of the inputs at sites [r repeat, (r + 1) repeat).  -> cells compared."""
    mo, fa = ped.relations()
    n_cfg, k = G.shape[1], gt.shape[1]
    cells = 0
    for r in range(rows):
        p = W[r] / W[r].sum()
        g = gt[r * repeat:(r + 1) * repeat]
        n = repeat * k
        flat = g.reshape(n, ped.n)
        if full_joint:
            cells += check_cells(np.bincount(config_index(flat), minlength=n_cfg), p, n, "joint, row %d" % r)
        marg = np.stack([[p[G[m] == a].sum() for a in range(3)] for m in range(ped.n)])
        for m in range(ped.n):
            cells += check_cells(np.bincount(flat[:, m], minlength=3), marg[m], n, "marginal of member %d, row %d" % (m, r))
        for c in range(ped.n):
            if mo[c] < 0:
                continue
            code = 9 * G[c] + 3 * G[mo[c]] + G[fa[c]]
            pt = np.bincount(code, weights=p, minlength=27)
            seen = 9 * flat[:, c].astype(int) + 3 * flat[:, mo[c]] + flat[:, fa[c]]
            cells += check_cells(np.bincount(seen, minlength=27), pt, n, "triple of child %d, row %d" % (c, r))
        # independence of member 0 between draws k, k + 1 of a site and between draw 0 of sites i, i + 1 (disjoint pairs, so that
        # the pairs themselves are independent and the cell's count is binomial)
        pp = np.outer(marg[0], marg[0])
        a, b = g[:, 0:k - 1:2, 0].astype(int).ravel(), g[:, 1:k:2, 0].astype(int).ravel()
        cells += check_cells(np.bincount(3 * a + b, minlength=9), pp, len(a), "draws k, k + 1, row %d" % r)
        a, b = g[0:repeat - 1:2, 0, 0].astype(int), g[1:repeat:2, 0, 0].astype(int)
        cells += check_cells(np.bincount(3 * a + b, minlength=9), pp, len(a), "sites i, i + 1, row %d" % r)
    return cells


def law_inputs(ped, rows, repeat, seed=5):
    lk8, fl8 = clear_likelihoods(np.random.RandomState(seed), ped, rows)
    assert len(np.unique(lk8.reshape(rows, -1), axis=0)) == rows
    return lk8, fl8, np.repeat(lk8, repeat, axis=0), np.repeat(fl8, repeat)


@pytest.mark.parametrize("case", LAW_CASES)
def test_the_law(case, tmp_path_factory):
    ped = law_pedigree(case)
    mrate = 1e-4
    model = fs.make_model(ped, mrate=mrate)
    fn = kernel(("law", case), ped, tmp_path_factory)
    lk8, fl8, lk, flags = law_inputs(ped, ROWS, REPEAT)
    gt, post, st = run_sample(fn, model, lk, flags, DRAWS, seed=20261019)
    G, W, ref_st = brute_weights(ped, mrate, lk8, fl8)
    assert np.all(ref_st == 0) and np.all(st == 0)
    cells = law_checks(ped, gt, G, W, ROWS, REPEAT, isinstance(case, str))
    print("%s: %d cells of expectation >= 10 compared" % (case, cells))
    assert cells > 100


# ---- 4. what a draw depends on --------------------------------------------------------------------------------------------


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


@pytest.mark.parametrize("seed", [1, 0])  # random_pedigree: loop-free, with a loop
def test_a_draw_depends_on_seed_site_and_draw_only(seed, tmp_path_factory):
    rng, ped = random_pedigree(seed)
    ped.relations()
    model = fs.make_model(ped, mrate=1e-4)
    fn = kernel(seed, ped, tmp_path_factory)
    lk, flags = random_likelihoods(rng, ped, 96)
    whole = run_sample(fn, model, lk, flags, 32, seed=77, site_base=1000)
    assert (whole[2] == 0).sum() > 48
    a, b = 17, 61
    part = run_sample(fn, model, lk[a:b], flags[a:b], 32, seed=77, site_base=1000 + a)
    assert same_bits(part, tuple(x[a:b] for x in whole))
    few = run_sample(fn, model, lk, flags, 3, seed=77, site_base=1000)
    assert same_bits(few, (whole[0][:, :3], whole[1][:, :3], whole[2]))
    ok = whole[2] == 0
    other_seed = run_sample(fn, model, lk, flags, 32, seed=78, site_base=1000)
    other_base = run_sample(fn, model, lk, flags, 32, seed=77, site_base=1001)
    high_seed = run_sample(fn, model, lk, flags, 32, seed=77 + (1 << 32), site_base=1000)
    high_base = run_sample(fn, model, lk, flags, 32, seed=77, site_base=1000 + (1 << 32))
    for other in (other_seed, other_base, high_seed, high_base):
        assert np.array_equal(other[2], whole[2])
        assert (other[0][ok] != whole[0][ok]).any(axis=(1, 2)).mean() > 0.5


@pytest.mark.parametrize("seed", [1, 0])
def test_the_four_variants_give_the_same_bits(seed, tmp_path_factory):
    rng, ped = random_pedigree(seed)
    ped.relations()
    model = fs.make_model(ped, mrate=1e-4)
    ctx = fs.Context(model, device=-1)
    assert (ctx.plan()["elim_conditioned_members"] > 0) == (seed == 0)
    ctx.close()
    lk, flags = random_likelihoods(rng, ped, 128)
    outs = [run_sample(kernel(seed, ped, tmp_path_factory, variant=v), model, lk, flags, 4, seed=3) for v in range(4)]
    for o in outs[1:]:
        assert same_bits(o, outs[0])


@pytest.mark.parametrize("seed", [1, 0, 2])
def test_the_site_prior_form(seed, tmp_path_factory):
    rng, ped = random_pedigree(seed)
    ped.relations()
    mrate = 1e-4
    model = fs.make_model(ped, mrate=mrate)
    plain, prior_fn = kernel(seed, ped, tmp_path_factory), kernel(seed, ped, tmp_path_factory, prior=True)
    lk, flags = random_likelihoods(rng, ped, 200)
    # the model's own rows: the plain form's bits
    own = run_sample(prior_fn, model, lk, flags, 5, seed=9, prior=P.model_rows(model, flags))
    assert same_bits(own, run_sample(plain, model, lk, flags, 5, seed=9))
    # Hardy-Weinberg rows: check 2 against the enumeration under per-site priors
    af = 10.0 ** rng.uniform(-6, np.log10(0.999), len(lk))
    prior = fs.hwe_priors(af)
    out = run_sample(prior_fn, model, lk, flags, 5, seed=9, prior=prior)
    G, W, ref_st = prior_weights(ped, mrate, lk, flags, prior)
    check_draws(ped, mrate, flags, out, G, W, ref_st)


# ---- 5. wide pedigrees ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [24, 32, 48, 64])
def test_wide_pedigrees(n, tmp_path):
    ped = wide_pedigree(n)
    ped.relations()
    lk, flags = random_likelihoods(np.random.RandomState(n), ped, 300, max_pl=40)
    model = fs.make_model(ped)
    fn, _, src = build_sample_host(model, tmp_path / "k")
    assert ("lgv[" in src) == (n >= 40)  # the lean form from forty members on
    gt, post, st = run_sample(fn, model, lk, flags, 4, seed=n)
    _, _, z, ref_st = mp.max_product(ped, 1e-7, lk, flags)
    bad = st != 0
    assert np.all(gt[bad] == -1) and np.all(np.isnan(post[bad]))
    assert np.all((gt[~bad] >= 0) & (gt[~bad] <= 2))
    tiny = (ref_st != 1) & ~(z >= 1e-280)
    differ = (st == 0) != (ref_st == 0)
    assert np.all(tiny[differ]) and np.array_equal(st[ref_st == 1], ref_st[ref_st == 1])
    ok = (st == 0) & (ref_st == 0) & ~tiny
    assert ok.sum() >= 20
    for d in range(4):
        w = mp.config_weight(ped, 1e-7, lk[ok], flags[ok], gt[ok][:, d])
        assert np.all(w > 0)
        np.testing.assert_allclose(post[ok][:, d], w / z[ok], rtol=RTOL, atol=0)
    print("n %d: %d sites compared, %d tiny" % (n, ok.sum(), tiny.sum()))


# ---- 6. nothing else moved ------------------------------------------------------------------------------------------------

OTHERS = ("trio", "map", "evidence", "loo", "pattern")


def test_generating_the_sample_kernel_leaves_the_other_sources_alone(tmp_path):
    rng, ped = random_pedigree(3)  # a loop pedigree
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    keys = ["elim_code_object"] + [k + "_code_object" for k in OTHERS]

    def others(ctx):
        ctx.set_option("trio_kernels", 3)
        for k in OTHERS[1:]:
            ctx.set_option(k + "_kernels", 1)

    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        others(ctx)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        ctx.set_option("sample_kernels", 1)
        ctx.set_option("sample_prior_kernels", 1)
        after = ctx.plan()
        assert after["sample_code_object"] and after["sample_code_object"] not in [before[k] for k in keys]
        assert after["sample_prior_code_object"] not in [after["sample_code_object"]] + [before[k] for k in keys]
        ctx.close()
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)  # ... and with the sampling kernels generated FIRST
        ctx.set_option("sample_kernels", 1)
        ctx.set_option("sample_prior_kernels", 1)
        others(ctx)
        again = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] == again[k]
        assert open(after[k][:-6] + ".hip").read() == texts[k]
    assert again["sample_code_object"] == after["sample_code_object"]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.set_option("sample_kernels", 1)
    ctx.close()
    rng, ped = random_pedigree(1)
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["sample_code_object"] == "" and plan["sample_variant"] == -1
        assert plan["sample_prior_code_object"] == "" and plan["sample_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*sample_kernels takes 1"):
            ctx.set_option("sample_kernels", 2)
        ctx.set_option("sample_kernels", 1)
        plan = ctx.plan()
        assert plan["sample_code_object"].endswith(".hsaco") and 0 <= plan["sample_variant"] < 4
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.sample_batch(2, lk=np.ones((1, ped.n, 3)))
        ctx.close()


def test_the_argument_refusals_need_no_device():
    rng, ped = random_pedigree(1)
    ctx = fs.Context(fs.make_model(ped), device=-1)
    lk = np.ones((2, ped.n, 3))
    for k in (0, -1, 257):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_draws must be 1\.\.256"):
            ctx.sample_batch(k, lk=lk)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*site_base must be >= 0"):
        ctx.sample_batch(2, site_base=-1, lk=lk)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_draws"):
        ctx.sample_prior_batch(np.ones((2, 6)), 300, lk=lk)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_draws"):
        ctx.sample_batch_device(2, 0, d_lk=0)
    ctx.close()
