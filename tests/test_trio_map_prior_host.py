"""The trio and MAP kernels under site priors (famseq_trio_prior, famseq_map_prior: famseq_trio and famseq_map with the
founders' genotype prior read per site), checked without a GPU.

As in test_prior_host.py and test_trio_host.py, the kernels are generated for a one-lane workgroup on a plan-only context and
their source compiled with g++.  The reference is tests/_prior_joint.py (bucket elimination over per-site-prior factors, pinned
there to the compiled oracle); the plain kernels built the same way are the reference for bit identity under the model's rows.
"""
import ctypes as C
import hashlib
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _prior as P
import _prior_joint as J
import famseq_amd as fs
from _cases import load_cases
from test_generated_host import factor_tables, host_source, misaligned
from test_map_host import build_map_host, run_map_host
from test_prior_host import PARENT_SOURCES
from test_trio_host import build_trio_host, run_trio_host

PEDIGREES = ("trio", "quad", "ped10", "cousins", "wide24", "wide48")  # conditioned body: cousins; lean shell: 48
N_VARIANTS = 4  # kTrioVariants = kMapVariants
KINDS = {"trio1": ("trio_prior_kernels", 1), "trio2": ("trio_prior_kernels", 2), "trio3": ("trio_prior_kernels", 3),
         "map": ("map_prior_kernels", 1)}


def build_host(model, where, kind, variant=None):
    """Generate famseq_trio_prior (kind trio<form>) or famseq_map_prior (map) for a one-lane workgroup on a plan-only context,
    compile it for the host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option(*KINDS[kind])
        plan = ctx.plan()
        ctx.close()
    key, entry = ("map_prior", "famseq_map_prior") if kind == "map" else ("trio_prior", "famseq_trio_prior")
    src = open(plan[key + "_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and (entry + "(") in src and "founder priors per site" in src.splitlines()[0]
    assert variant is None or plan[key + "_variant"] == variant
    tag = kind + ("" if variant is None else "_%d" % variant)
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), entry)
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_void_p]
    return fn, plan, src


def prior_array(prior, misalign):
    if misalign:
        pr = misaligned(prior.shape)
    else:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        assert pr.ctypes.data % 16 == 0
    pr[...] = prior
    return pr


def run_trio(fn, model, k, lk, flags, prior, form=3, misalign_prior=False):
    s = lk.shape[0]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    j = np.full((s, k, 27), -1.0) if form & 2 else None
    d = np.full((s, k), -1.0) if form & 1 else None
    st = np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    pr = prior_array(prior, misalign_prior)
    fn(a.ctypes.data, fl.ctypes.data, None if j is None else j.ctypes.data, None if d is None else d.ctypes.data, st.ctypes.data, s,
       tc.ctypes.data, 1.0, pr.ctypes.data)
    return j, d, st


def run_map(fn, model, lk, flags, prior, misalign_prior=False):
    s, n = lk.shape[0], lk.shape[1]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    gt = np.full((s, n), 77, np.int8)
    post = np.full(s, -5.0)
    st = np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    pr = prior_array(prior, misalign_prior)
    fn(a.ctypes.data, fl.ctypes.data, gt.ctypes.data, post.ctypes.data, st.ctypes.data, s, tc.ctypes.data, 1.0, pr.ctypes.data)
    return gt, post, st


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", PEDIGREES)
def test_every_variant_matches_the_helper(name, variant, tmp_path):
    ped, lk, flags, prior, ref = J.reference(name)
    assert len(lk) == 200 and set(np.unique(flags & 2)) == {0, 2}
    model = fs.make_model(ped)
    k = len(J.children_of(ped))
    out = {}
    for form in (1, 2, 3):
        fn, plan, src = build_host(model, tmp_path, "trio%d" % form, variant)
        assert "conditioned on" in src.splitlines()[0] if name == "cousins" else "conditioned on" not in src.splitlines()[0]
        assert ("#define l0_0 lgv[0]" in src) == (name == "wide48")  # the lean shell
        out[form] = run_trio(fn, model, k, lk, flags, prior, form)
        J.check_trio(out[form], ref, "%s variant %d form %d" % (name, variant, form))
    # the de novo mass of the joint under the mask, and the three forms give one another's bits
    ok = out[3][2] == 0
    np.testing.assert_allclose(out[3][1][ok], np.where(J.dnm_mask(ped, flags), out[3][0], 0.0).sum(axis=2)[ok], rtol=J.RTOL, atol=0)
    assert same_bits((out[1][1], out[1][2]), (out[3][1], out[3][2])) and same_bits((out[2][0], out[2][2]), (out[3][0], out[3][2]))
    fn_map, plan, src = build_host(model, tmp_path, "map", variant)
    got = run_map(fn_map, model, lk, flags, prior)
    assert J.check_map(got, ref, "%s variant %d MAP" % (name, variant)) > 150
    if variant == 0:  # ... and the same bits from a prior array that is only 8-byte aligned
        assert same_bits(run_trio(fn, model, k, lk, flags, prior, 3, misalign_prior=True), out[3])
        assert same_bits(run_map(fn_map, model, lk, flags, prior, misalign_prior=True), got)


SYNTH = [c for c in load_cases(("bn_synth.npz",))]


@pytest.mark.parametrize("case", SYNTH, ids=[c.name for c in SYNTH])
def test_model_constant_rows_give_the_plain_kernels_bits(case, tmp_path):
    """Every synthetic fixture (custom priors, chrX, mutation rate 0 among them): fed the rows the model would have used, chosen by
    each site's Known flag, famseq_trio_prior and famseq_map_prior return famseq_trio's and famseq_map's bytes."""
    model = fs.make_model(case.pedigree(), **case.consts)
    rows = P.model_rows(model, case.flags)
    plain, children = build_trio_host(model, 3, tmp_path / "trio")
    fn, _, src = build_host(model, tmp_path / "trio_prior", "trio3")
    assert "tcf[0] * l" not in src and "tcf[27] * l" not in src and "pa_0 * l" in src + "pm_0 * l"
    want = run_trio_host(plain, model, len(children), case.lk, case.flags)
    assert (want[2] == 0).any()
    assert same_bits(run_trio(fn, model, len(children), case.lk, case.flags, rows), want)
    plain = build_map_host(model, tmp_path / "map")[0]
    fn, _, src = build_host(model, tmp_path / "map_prior", "map")
    assert "tcf[0] * l" not in src and "tcf[27] * l" not in src
    assert same_bits(run_map(fn, model, case.lk, case.flags, rows), run_map_host(plain, model, case.lk, case.flags))


def test_edge_rows(tmp_path):
    ped = P.pedigree("trio")
    mo, fa = ped.relations()
    child = int(np.nonzero(np.asarray(mo) >= 0)[0][0])
    male = int(np.nonzero(np.asarray(ped.genders) == 1)[0][0])
    model = fs.make_model(ped, mrate=0.0)
    lk = np.full((4, ped.n, 3), 0.25)
    lk[:, :, 0] = 0.5
    flags = np.array([0, 2, 0, 1], np.uint8)
    prior = fs.hwe_priors(np.full(4, 0.1))
    prior[0, 0:3] = 0.0                    # an all-zero autosomal row
    prior[1, 3:6] = [1.0, 0.0, 0.0]        # chrX: the male row allows hom-ref only, a male's likelihood hom-alt only
    lk[1, male] = [0.0, 0.0, 1.0]
    prior[2, 0:3] = [0.5, 0.0, 0.5]        # no heterozygous founder; the parents' rows make the child one at mutation rate 0,
    lk[2, mo[child]] = [1.0, 0.0, 0.0]     # which its own likelihood rules out: every configuration has weight 0
    lk[2, fa[child]] = [0.0, 0.0, 1.0]
    lk[2, child] = [1.0, 0.0, 1.0]
    prior[3, 3:6] = np.nan                 # not a chrX site: the male row is not read, whatever it holds
    ref = J.analyse(ped, lk, flags, prior, mrate=0.0)
    assert ref.trio_status.tolist() == [1, 1, 2, 0] and ref.map_status.tolist() == [1, 1, 2, 0]
    joint, dnm, st = run_trio(build_host(model, tmp_path, "trio3")[0], model, 1, lk, flags, prior)
    assert st.tolist() == [1, 1, 2, 0]
    J.check_trio((joint, dnm, st), ref)
    assert np.all(np.isnan(joint[:3])) and np.all(np.isnan(dnm[:3])) and np.all(np.isfinite(joint[3])) and dnm[3, 0] == 0.0
    gt, post, st = run_map(build_host(model, tmp_path, "map")[0], model, lk, flags, prior)
    assert st.tolist() == [1, 1, 2, 0] and np.all(gt[:3] == -1) and np.all(np.isnan(post[:3]))
    J.check_map((gt, post, st), ref)  # (the Known bit of the last site is not read either)


# sha256 (first 16 hex digits) of the generated source of the ten-member benchmark pedigree's kernels on the parent commit:
# test_prior_host's three kinds, and the site-prior sum-product kernel as the parent generates it
PARENT_PRIOR = ["4c416a620340f982", "7f8458af7fa119db", "8cecd0f96d5faee6", "6eda4165a9e5e4a5", "43784c6cf94ac8e2", "a0f6f1951884b399",
                "0698493034ef0b2d", "24c33998c5357da0", "2846ad28468f11e3", "8a033b45ddb8199f", "4545345ea146f8e2", "aaa41eca204cc535"]


def test_the_existing_kernels_sources_are_the_parents(tmp_path):
    """With the switches off the generators' text is what it was — and generating the new kernels in the same context does not
    change that."""
    model = fs.make_model(fs.synthetic_pedigree("ped10"))
    options = {"elim": ("engine", fs.ENGINE_ELIM), "map": ("map_kernels", 1), "trio": ("trio_kernels", 3), "prior": ("prior_kernels", 1)}
    assert [len(PARENT_SOURCES[k]) for k in ("elim", "map", "trio")] == [12, 4, 4]
    for kind, want in dict(PARENT_SOURCES, prior=PARENT_PRIOR).items():
        for v, digest in enumerate(want):
            env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path / ("%s%d" % (kind, v))), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
            os.makedirs(env["FAMSEQ_KERNEL_CACHE"])
            with mock.patch.dict(os.environ, env):
                ctx = fs.Context(model, device=-1)
                with mock.patch.dict(os.environ, dict(FAMSEQ_VARIANT_ONLY=str(v & 3))):  # (the new kernels have four variants)
                    ctx.set_option("trio_prior_kernels", 3)
                    ctx.set_option("map_prior_kernels", 1)
                with mock.patch.dict(os.environ, dict(FAMSEQ_VARIANT_ONLY=str(v))):
                    ctx.set_option(*options[kind])
                plan = ctx.plan()
                ctx.close()
            new = {plan["trio_prior_code_object"], plan["map_prior_code_object"]}
            assert len(new) == 2 and "" not in new and plan[kind + "_code_object"] not in new
            src = open(plan[kind + "_code_object"][:-6] + ".hip", "rb").read()
            assert hashlib.sha256(src).hexdigest()[:16] == digest, (kind, v)


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key, value in (("trio_prior_kernels", 1), ("map_prior_kernels", 1)):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*site priors.*more than three"):
            ctx.set_option(key, value)
    ctx.close()
    ped = P.pedigree("quad")
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["trio_prior_code_object"] == "" and plan["trio_prior_variant"] == -1
        assert plan["map_prior_code_object"] == "" and plan["map_prior_variant"] == -1
        for key, value, msg in (("trio_prior_kernels", 0, "takes 1 .dnm., 2 .joint. or 3 .both."), ("trio_prior_kernels", 4, "takes 1"),
                                ("map_prior_kernels", 0, "map_prior_kernels takes 1"), ("map_prior_kernels", 2, "map_prior_kernels takes 1")):
            with pytest.raises(fs.FamseqError, match=msg):
                ctx.set_option(key, value)
        for form in (1, 2, 3):
            ctx.set_option("trio_prior_kernels", form)
            ctx.set_option("trio_kernels", form)
            plan = ctx.plan()
            assert plan["trio_prior_code_object"].endswith(".hsaco") and plan["trio_prior_code_object"] != plan["trio_code_object"]
            assert 0 <= plan["trio_prior_variant"] == plan["trio_variant"] < N_VARIANTS
        ctx.set_option("map_kernels", 1)  # the sibling first this time: the order must not matter
        ctx.set_option("map_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["map_prior_code_object"].endswith(".hsaco") and 0 <= plan["map_prior_variant"] == plan["map_variant"] < N_VARIANTS
        assert plan["prior_code_object"] == ""  # (nothing else was generated on the way)
        lk = np.ones((1, ped.n, 3))
        for call in (ctx.trio_prior_batch, ctx.map_prior_batch):
            with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
                call(fs.hwe_priors([0.1]), lk=lk)
            with pytest.raises(ValueError):
                call(np.ones((1, 3)), lk=lk)
            with pytest.raises(ValueError):
                call(np.ones((2, 6)), lk=lk)
        ctx.close()


def test_the_variant_is_the_plain_siblings_whatever_the_new_kernel_spills(tmp_path):
    """As test_prior_host's for famseq_elim_prior: the resource notes of a scratch cache stand in for the compiler.  The plain
    kernels' variant 0 spills and 1 does not; the site-prior kernels' own notes say the opposite, and are not asked."""
    model = fs.make_model(P.pedigree("trio"))
    base = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")
    option = {"trio": ("trio_kernels", 1), "map": ("map_kernels", 1), "trio_prior": ("trio_prior_kernels", 1), "map_prior": ("map_prior_kernels", 1)}
    for kind in option:
        for v, scratch in ((0, 8), (1, 100)) if kind.endswith("prior") else ((0, 100), (1, 8)):
            with mock.patch.dict(os.environ, dict(base, FAMSEQ_VARIANT_ONLY=str(v))):
                ctx = fs.Context(model, device=-1)
                ctx.set_option(*option[kind])
                note = ctx.plan()[kind + "_code_object"][:-6] + ".res"
                ctx.close()
            assert open(note).read() == "0\n"
            open(note, "w").write("%d\n" % scratch)
    with mock.patch.dict(os.environ, base):
        ctx = fs.Context(model, device=-1)
        ctx.set_option("trio_prior_kernels", 1)  # before the plain kernels are there
        ctx.set_option("map_prior_kernels", 1)
        assert ctx.plan()["trio_prior_variant"] == 1 and ctx.plan()["map_prior_variant"] == 1
        ctx.set_option("trio_kernels", 1)
        ctx.set_option("map_kernels", 1)
        assert ctx.plan()["trio_variant"] == 1 and ctx.plan()["map_variant"] == 1
        ctx.close()
