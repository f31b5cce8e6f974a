"""The site-prior kernel's arithmetic (famseq_elim_prior: the sum-product kernel with the founders' genotype prior read per
site), checked without a GPU.

As in test_map_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled with
g++.  The reference is the existing oracle with one model per site (tests/_prior.py); the plain kernel built the same way is
the reference for bit identity under the model's own rows.
"""
import ctypes as C
import hashlib
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from _cases import load_cases
from test_generated_host import factor_tables, host_source, misaligned

PEDIGREES = ("trio", "quad", "ped10", "cousins", "wide24", "wide48")  # conditioned body: cousins; staged / unstaged shell: 24 / 48
N_VARIANTS = 12  # kElimVariants: every index is a variant of every pedigree's plain kernel


def build_host(model, where, prior, variant=None):
    """Generate famseq_elim_prior (prior) or famseq_elim for a one-lane workgroup on a plan-only context, compile it for the
    host.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        if prior:
            ctx.set_option("prior_kernels", 1)
        else:
            ctx.set_option("engine", fs.ENGINE_ELIM)
        plan = ctx.plan()
        ctx.close()
    entry, key = ("famseq_elim_prior", "prior") if prior else ("famseq_elim", "elim")
    src = open(plan[key + "_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and (entry + "(") in src
    assert variant is None or plan[key + "_variant"] == variant
    tag = key + ("" if variant is None else str(variant))
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), entry)
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def run(fn, model, lk, flags, prior=None, lc=None, misalign_prior=False):
    """One call of the host-compiled kernel; arrays at 8 mod 16, so the one-lane block takes its 8-byte staging (the prior
    array at either alignment: the kernel loads 16-byte pieces from one that allows them)."""
    a, post, single = misaligned(lk.shape), misaligned(lk.shape), misaligned(lk.shape)
    a[...] = lk
    post[...] = -1
    single[...] = -1
    st = np.full(len(lk), 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [a.ctypes.data, fl.ctypes.data, post.ctypes.data, single.ctypes.data, st.ctypes.data, len(lk), tc.ctypes.data,
            float(model.lc if lc is None else lc)]
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
    return post, single, st


_REF = {}


def reference(name):
    """The pedigree's batch and its per-site oracle, computed once and asserted to be well-conditioned."""
    if name not in _REF:
        ped = P.pedigree(name)
        lk, flags, prior = P.batch(ped)
        assert len(lk) == 200 and set(np.unique(flags & 2)) == {0, 2}
        ref = P.reference(ped, lk, flags, prior)
        P.assert_well_conditioned(ped, lk, flags, prior, ref)
        assert ((ref[2] & 3) == 0).sum() > 100 and (ref[2] == 0).sum() > 50
        _REF[name] = (ped, lk, flags, prior, ref)
    return _REF[name]


@pytest.mark.parametrize("variant", range(N_VARIANTS))
@pytest.mark.parametrize("name", PEDIGREES)
def test_every_variant_matches_the_per_site_oracle(name, variant, tmp_path):
    ped, lk, flags, prior, ref = reference(name)
    model = fs.make_model(ped)
    fn, plan, src = build_host(model, tmp_path, True, variant)
    assert ("rows straight from and to global memory" in src.splitlines()[0]) == (variant >= 8)
    assert "conditioned on" in src.splitlines()[0] if name == "cousins" else "conditioned on" not in src.splitlines()[0]
    out = run(fn, model, lk, flags, prior)
    P.check(out, ref, "%s variant %d" % (name, variant))
    if variant in (0, 4, 8):  # ... and the same bits from a prior array that is only 8-byte aligned
        again = run(fn, model, lk, flags, prior, misalign_prior=True)
        for a, b in zip(out, again):
            assert np.array_equal(a, b, equal_nan=True)


def test_the_default_variant_is_the_plain_kernels(tmp_path):
    for name in ("trio", "ped10", "wide48"):
        model = fs.make_model(P.pedigree(name))
        want = build_host(model, tmp_path / name / "plain", False)[1]["elim_variant"]
        assert build_host(model, tmp_path / name / "prior", True)[1]["prior_variant"] == want


SYNTH = [c for c in load_cases(("bn_synth.npz",))]


@pytest.mark.parametrize("case", SYNTH, ids=[c.name for c in SYNTH])
def test_model_constant_rows_give_the_plain_kernels_bits(case, tmp_path):
    """Every synthetic fixture (custom priors, chrX, mutation rate 0, the -LRC boundary among them): fed the rows the model
    would have used, chosen by each site's Known flag, famseq_elim_prior returns famseq_elim's post, single and status."""
    model = fs.make_model(case.pedigree(), **case.consts)
    plain, _, plain_src = build_host(model, tmp_path / "plain", False)
    prior, _, prior_src = build_host(model, tmp_path / "prior", True)
    assert "tcf[0] * l" in plain_src or "tcf[27] * l" in plain_src  # a founder's prior as the plain kernel reads it ...
    assert "tcf[0] * l" not in prior_src and "tcf[27] * l" not in prior_src and "pa_0 * l" in prior_src + "pm_0 * l"
    want = run(plain, model, case.lk, case.flags)
    assert np.array_equal(want[2], case.status)  # (the plain kernel against the fixture: what test_generated_host checks)
    got = run(prior, model, case.lk, case.flags, P.model_rows(model, case.flags))
    for a, b in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_the_shortcut_boundary_is_the_oracles(tmp_path):
    """The -LRC fixture's rows under allele-frequency priors: 0x80 exactly where the per-site oracle says, both sides seen."""
    case = [c for c in SYNTH if c.name.endswith("trio_lrc")][0]
    ped = case.pedigree()
    ped.relations()
    model = fs.make_model(ped, **case.consts)
    prior = fs.hwe_priors(10.0 ** np.random.RandomState(5).uniform(-6, -0.001, len(case.lk)))
    ref = P.reference(ped, case.lk, case.flags, prior, **{k: v for k, v in case.consts.items() if k in ("mrate", "lc")})
    assert (ref[2] == 0x80).any() and (ref[2] == 0).any()
    fn = build_host(model, tmp_path, True)[0]
    P.check(run(fn, model, case.lk, case.flags, prior), ref)


def test_edge_rows(tmp_path):
    ped = P.pedigree("trio")
    mo, fa = ped.relations()
    child = int(np.nonzero(np.asarray(mo) >= 0)[0][0])
    male = int(np.nonzero(np.asarray(ped.genders) == 1)[0][0])
    model = fs.make_model(ped, mrate=0.0)
    fn = build_host(model, tmp_path, True)[0]
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
    post, single, st = run(fn, model, lk, flags, prior)
    assert st.tolist() == [1, 1, 2, 0]
    assert np.all(np.isnan(post[:3])) and np.all(np.isnan(single[:2])) and np.all(np.isfinite(single[2:])) and np.all(np.isfinite(post[3]))
    ref = P.reference(ped, lk[2:], flags[2:], np.nan_to_num(prior[2:]), mrate=0.0)
    P.check((post[2:], single[2:], st[2:]), ref)  # (the Known bit of the last site is not read either)


# sha256 (first 16 hex digits) of the generated source of the ten-member benchmark pedigree's kernels on the parent commit
PARENT_SOURCES = {
    "elim": ["2815921a548f058f", "06a5be119d0b3460", "0fee743667c79782", "2a40cdca7642d8f6", "abe0fba83f378a7f", "edabef4b904686b8",
             "791fbe626d8bfa8b", "0c41366c4bea3768", "576baf42900e656b", "80eb18d7c8508e2a", "f547af9a58db556b", "f8dcfcb3b6feb2b4"],
    "map": ["03782464451372a4", "4fee940437ce76f9", "15bf06e12efe1602", "82dd142f91e52f14"],
    "trio": ["1b3a896ace6d5fca", "46c3783cd221beac", "fc57a8f8b8cd571e", "df3d3b8a92827d47"],
}


def test_the_existing_kernels_sources_are_the_parents(tmp_path):
    """With the switch off the generators' text is what it was (code objects are cached by content hash; the shipped table of
    measured picks is keyed by it) — and generating the site-prior kernel in the same context does not change that."""
    model = fs.make_model(fs.synthetic_pedigree("ped10"))
    options = {"elim": ("engine", fs.ENGINE_ELIM), "map": ("map_kernels", 1), "trio": ("trio_kernels", 3)}
    for kind, want in PARENT_SOURCES.items():
        for v, digest in enumerate(want):
            env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path / ("%s%d" % (kind, v))), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1",
                       FAMSEQ_VARIANT_ONLY=str(v))
            os.makedirs(env["FAMSEQ_KERNEL_CACHE"])
            with mock.patch.dict(os.environ, env):
                ctx = fs.Context(model, device=-1)
                ctx.set_option("prior_kernels", 1)
                ctx.set_option(*options[kind])
                plan = ctx.plan()
                ctx.close()
            assert plan["prior_code_object"] and plan["prior_code_object"] != plan[kind + "_code_object"]
            src = open(plan[kind + "_code_object"][:-6] + ".hip", "rb").read()
            assert hashlib.sha256(src).hexdigest()[:16] == digest, (kind, v)


def test_hwe_priors():
    q = np.concatenate([[0.0, 1.0, 0.5, 1e-6, 0.999], np.random.RandomState(2).rand(1000)])
    want = np.stack([(1 - q) * (1 - q), 2 * q * (1 - q), q * q, 1 - q, np.zeros_like(q), q], axis=1)
    got = fs.hwe_priors(q)
    assert got.shape == (len(q), 6) and np.array_equal(P.bits(got), P.bits(want))


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*site priors.*more than three"):
        ctx.set_option("prior_kernels", 1)
    ctx.close()
    ped = P.pedigree("quad")
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["prior_code_object"] == "" and plan["prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="prior_kernels takes 1"):
            ctx.set_option("prior_kernels", 2)
        ctx.set_option("prior_kernels", 1)
        plan = ctx.plan()
        assert plan["prior_code_object"].endswith(".hsaco") and 0 <= plan["prior_variant"] < N_VARIANTS
        lk = np.ones((1, ped.n, 3))
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.bn_prior_batch(lk, fs.hwe_priors([0.1]))
        with pytest.raises(ValueError):
            ctx.bn_prior_batch(lk, np.ones((1, 3)))
        ctx.close()


def test_the_wide_context_names_the_kernel_too(tmp_path):
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(P.pedigree("wide24")), device=-1)
        ctx.set_option("prior_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    assert plan["prior_code_object"].endswith(".hsaco") and plan["prior_variant"] == plan["elim_variant"]


def test_the_variant_is_the_plain_kernels_whatever_the_prior_kernel_spills(tmp_path):
    """famseq_elim_prior runs in the variant famseq_elim's contest takes, not in the winner of a contest over its own scratch
    (at 48 members the compiler spills less of the site-prior kernel in variant 9 and less of the plain one in variant 8).
    The resource notes of a scratch cache stand in for the compiler: plain variant 0 spills, plain variant 1 does not; the
    site-prior kernel's own notes say the opposite."""
    model = fs.make_model(P.pedigree("trio"))
    base = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")
    notes = {("elim", 0): 100, ("elim", 1): 8, ("prior", 0): 8, ("prior", 1): 100}
    for (kind, v), scratch in notes.items():
        with mock.patch.dict(os.environ, dict(base, FAMSEQ_VARIANT_ONLY=str(v))):
            ctx = fs.Context(model, device=-1)
            ctx.set_option(*(("prior_kernels", 1) if kind == "prior" else ("engine", fs.ENGINE_ELIM)))
            note = ctx.plan()[kind + "_code_object"][:-6] + ".res"
            ctx.close()
        assert open(note).read() == "0\n"
        open(note, "w").write("%d\n" % scratch)
    with mock.patch.dict(os.environ, base):
        ctx = fs.Context(model, device=-1)
        ctx.set_option("prior_kernels", 1)  # before the plain kernel is there: the order must not matter
        assert ctx.plan()["prior_variant"] == 1
        ctx.set_option("engine", fs.ENGINE_ELIM)
        assert ctx.plan()["elim_variant"] == 1
        ctx.close()
