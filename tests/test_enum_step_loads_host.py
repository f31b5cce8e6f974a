"""The once-per-site form's loads one step ahead (csrc/enum_codegen.cpp, FAMSEQ_LANE_PRE) without a GPU.

With the default (2) the innermost loop's transmission entries are loop-carried scalars loaded a step ahead, the likelihoods its
table statements multiply them with are read ahead of that loop, and every loop level reads its marginal slot where its step
begins.  No arithmetic statement changes, so the text generated with FAMSEQ_LANE_PRE=0 — the text before this change, byte for
byte — and the default text must produce the same bits.  Both are compiled for the host (the helpers of test_generated_host.py).
"""
import os

import numpy as np
import pytest

import famseq_amd as fs
import _variants as V
from _cases import load_cases
from test_generated_host import build_host_kernel, run_host

RTOL = 1e-9  # the project's tolerance on posteriors (atol 0)
ONCE = "prefix tables and marginals once per site"
PARENT_OBJECT = "9a2b09063e603740"  # ten members, lane variant 4, before this change
SHAPE10 = "looped members [5 0 1], unrolled block [4 2 6 7 3 8 9] = 2187 configurations per step, " + ONCE
CASES = {c.name: c for c in load_cases()}


def both_kernels(model, tmp_path, monkeypatch):
    """(host function, source) of the default text and of the FAMSEQ_LANE_PRE=0 text."""
    out = []
    for pre in (None, "0"):
        if pre is None:
            monkeypatch.delenv("FAMSEQ_LANE_PRE", raising=False)
        else:
            monkeypatch.setenv("FAMSEQ_LANE_PRE", pre)
        d = tmp_path / ("pre_" + (pre or "default"))
        d.mkdir()
        fn = build_host_kernel(model, "lane", d, monkeypatch)
        out.append((fn, open(d / "cache_lane" / "k.cpp").read()))
    monkeypatch.delenv("FAMSEQ_LANE_PRE", raising=False)
    (fn_new, src_new), (fn_old, src_old) = out
    assert ONCE in src_new.splitlines()[0] and ONCE in src_old.splitlines()[0]
    assert src_new != src_old and "tq0" in src_new and "tq0" not in src_old
    return fn_new, fn_old


def check(fn_new, fn_old, model, lk, flags, ref, what):
    new, old = run_host(fn_new, model, lk, flags), run_host(fn_old, model, lk, flags)
    for a, b, name in zip(new, old, ("post", "single", "status")):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        same = np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)
        assert same, "%s: %s differs between the two texts" % (what, name)
    post, single, st = new
    want_post, want_single, want_status = ref
    assert np.array_equal(st, want_status), what
    ok, s_ok = (want_status & 3) == 0, (want_status & 3) != 1
    assert np.array_equal(single[s_ok].view(np.uint64), np.ascontiguousarray(want_single[s_ok]).view(np.uint64)), what
    nz = want_post[ok] > 0
    dev = np.max(np.abs(post[ok][nz] - want_post[ok][nz]) / want_post[ok][nz]) if nz.any() else 0.0
    print("%s: %d sites (%d full), bit-identical texts, largest relative deviation from the oracle %.3e" % (what, len(st), int(ok.sum()), dev))
    np.testing.assert_allclose(post[ok], want_post[ok], rtol=RTOL, atol=0)
    assert np.all(np.isnan(post[~ok]))


def object_and_shape(monkeypatch, cache):
    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(cache), FAMSEQ_JIT_SOURCE_ONLY="1").items():
        monkeypatch.setenv(k, v)
    ctx = fs.Context(fs.make_model(fs.synthetic_pedigree("ped10")), device=-1)
    try:
        ctx.set_option("pick_lane", 4)
        ctx.set_option("enum_impl", 1)
        plan = ctx.plan()
    finally:
        ctx.close()
    return os.path.basename(plan["enum_lane_code_object"]), plan["enum_lane_shape"]


def test_the_switch_restores_the_parents_text(tmp_path, monkeypatch):
    monkeypatch.setenv("FAMSEQ_LANE_PRE", "0")
    obj, shape = object_and_shape(monkeypatch, tmp_path)
    assert obj == PARENT_OBJECT + ".hsaco" and shape.startswith(SHAPE10)
    monkeypatch.delenv("FAMSEQ_LANE_PRE")
    obj2, shape2 = object_and_shape(monkeypatch, tmp_path)
    assert obj2 != obj and shape2.startswith(SHAPE10)
    assert shape2 == shape  # the cost model counts the same fp64 statements: no arithmetic was added


@pytest.mark.parametrize("name", ["bn_synth:ped10", "bn_synth:ped10_x"])
def test_ten_member_fixtures(name, tmp_path, monkeypatch):
    """Every fixture of the ten-member pedigree, autosome and chrX (the carried entries are re-primed per pass)."""
    case = CASES[name]
    model = fs.make_model(case.pedigree(), **case.consts)
    fn_new, fn_old = both_kernels(model, tmp_path, monkeypatch)
    ref = (case.post, case.single, case.status)  # the oracle's record (test_oracle_golden.py holds the oracle to it)
    check(fn_new, fn_old, model, case.lk, case.flags, ref, name)


def test_ten_members_every_flag_and_planted_site(tmp_path, monkeypatch):
    """All four (Known, chrX) combinations, a shortcut site, failed single posteriors, a BN failure (the variant matrices' batch)."""
    ped = V.pedigree("ped10")
    model = fs.make_model(ped, mrate=V.MRATE)
    fn_new, fn_old = both_kernels(model, tmp_path, monkeypatch)
    lk, flags, has_bn_fail = V.variant_batch(ped, 128)
    ref = V.reference(ped, lk, flags)
    assert has_bn_fail and 2 in ref[2] and 1 in ref[2] and 0x80 in ref[2]
    check(fn_new, fn_old, model, lk, flags, ref, "ped10 planted sites")


@pytest.mark.parametrize("seed", [2, 10, 24, 26, 33])
def test_soak_pedigrees_that_take_the_form(seed, tmp_path, monkeypatch):
    import oracle
    from famseq_amd.prebuild_sets import soak_pedigree
    from famseq_amd.synth import random_likelihoods

    rng, ped, mu = soak_pedigree(seed)
    model = fs.make_model(ped, mrate=mu)
    fn_new, fn_old = both_kernels(model, tmp_path, monkeypatch)
    lk, flags = random_likelihoods(rng, ped, 64)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=mu).bn_batch(lk, flags, threads=4)
    check(fn_new, fn_old, model, lk, flags, ref, "soak %d" % seed)
