"""The lane kernel's outer-leaf plan (csrc/enum_codegen.cpp, outer_leaf_shape; lane variants 8-11) without a GPU.

Where a founder and its one or two children, all leaves by one other parent, can be the block's super-leaf, that other
parent becomes the outermost loop and the super-leaf table is built three times per site instead of once per step; the
rest is the once-per-site form.  The generated source is compiled for the host (the helpers of test_generated_host.py)
and compared with the fixtures and the oracle; where the plan does not apply, or FAMSEQ_LANE_OUTER=0 says so, variants
8-11 must be the text of 4-7, which the names of their code objects (content hashes of the text) show.
"""
import os
import re

import numpy as np
import pytest

import famseq_amd as fs
import _variants as V
from _cases import load_cases
from test_generated_host import build_host_kernel, run_host

RTOL = 1e-9  # the project's tolerance on posteriors (atol 0)
ONCE = "prefix tables and marginals once per site"
OUTER = "super-leaf table once per step of the outermost loop"
CASES = {c.name: c for c in load_cases()}
HOST_ENV = dict(FAMSEQ_KEEP_SRC="1", FAMSEQ_LANE_BT="1", FAMSEQ_ELIM_BT="1", FAMSEQ_LANE_MINWAVES="1", FAMSEQ_JIT_SOURCE_ONLY="1")


def host_kernel(model, tmp_path, monkeypatch, variant=8):
    """build_host_kernel's lane kernel in `variant`: the pick is a note in the cache directory the helper is about to use,
    keyed by the variant-0 text of the one-lane workgroup the helper generates (hence its environment, set here first)."""
    cache = tmp_path / "cache_lane"
    cache.mkdir(exist_ok=True)
    for k, v in dict(HOST_ENV, FAMSEQ_KERNEL_CACHE=str(cache)).items():
        monkeypatch.setenv(k, v)
    ctx = fs.Context(model, device=-1)
    ctx.set_option("pick_lane", variant)
    ctx.close()
    fn = build_host_kernel(model, "lane", tmp_path, monkeypatch)
    return fn, open(cache / "k.cpp").read()


def check(fn, model, lk, flags, want_post, want_single, want_status, what):
    post, single, st = run_host(fn, model, lk, flags)
    assert np.array_equal(st, want_status), what
    ok, s_ok = (want_status & 3) == 0, (want_status & 3) != 1
    assert np.array_equal(single[s_ok].view(np.uint64), want_single[s_ok].view(np.uint64)), what
    nz = want_post[ok] > 0
    dev = np.max(np.abs(post[ok][nz] - want_post[ok][nz]) / want_post[ok][nz]) if nz.any() else 0.0
    print("%s: %d sites (%d full), largest relative deviation %.3e" % (what, len(st), int(ok.sum()), dev))
    np.testing.assert_allclose(post[ok], want_post[ok], rtol=RTOL, atol=0)
    assert np.all(np.isnan(post[~ok]))
    again = run_host(fn, model, lk, flags)  # the same sites twice: the same bits
    for a, b in zip((post, single, st), again):
        assert np.array_equal(a, b, equal_nan=True), what
    return dev


def plan_of(ped_or_name, variant, tmp_path, monkeypatch, mrate=None, impl=1):
    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1").items():
        monkeypatch.setenv(k, v)
    ped = fs.synthetic_pedigree(ped_or_name) if isinstance(ped_or_name, str) else ped_or_name
    ctx = fs.Context(fs.make_model(ped) if mrate is None else fs.make_model(ped, mrate=mrate), device=-1)
    try:
        if variant is not None:
            ctx.set_option("pick_lane", variant)
        if impl is not None:
            ctx.set_option("enum_impl", impl)
        return ctx.plan()
    finally:
        ctx.close()


def object_name(ped_name, variant, tmp_path, monkeypatch):
    return os.path.basename(plan_of(ped_name, variant, tmp_path, monkeypatch)["enum_lane_code_object"])[:-len(".hsaco")]


def counts(shape):
    """(once-per-site count, outer-leaf count) as enumgen_describe prints them for variants 8-11."""
    m = re.search(r"outer-leaf plan: .* \((\d+) fp64 statements per site against (\d+)\)", shape)
    assert m, shape
    return int(m.group(2)), int(m.group(1))


@pytest.mark.parametrize("name", ["bn_synth:ped10", "bn_synth:ped10_x"])
def test_ten_member_fixtures(name, tmp_path, monkeypatch):
    """Every fixture row of the ten-member pedigree, autosome and chrX (the super-leaf table is built per chrX pass)."""
    case = CASES[name]
    model = fs.make_model(case.pedigree(), **case.consts)
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    head = src.splitlines()[0]
    assert ONCE in head and OUTER in head and "variant 8" in head
    assert "outer (looped) members: 3 0 1 | unrolled block: 4 2 6 7 5 8 9 (2187 configurations per outer step)" in src
    check(fn, model, case.lk, case.flags, case.post, case.single, case.status, name)


def test_ten_members_every_flag_and_planted_site(tmp_path, monkeypatch):
    """All four (Known, chrX) combinations, a shortcut site, failed single posteriors, a BN failure, the -LRC boundary and
    row sums below 1e-290 (the variant matrices' batch), mutation rate 0, against the oracle."""
    ped = V.pedigree("ped10")
    model = fs.make_model(ped, mrate=V.MRATE)
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    assert OUTER in src.splitlines()[0]
    lk, flags, has_bn_fail = V.variant_batch(ped, 128)
    ref = V.reference(ped, lk, flags)
    assert has_bn_fail and 2 in ref[2] and 1 in ref[2] and 0x80 in ref[2]
    check(fn, model, lk, flags, ref[0], ref[1], ref[2], "ped10 planted sites")


@pytest.mark.parametrize("variant", [9, 10, 11])
def test_the_other_block_shapes_and_fencings(variant, tmp_path, monkeypatch):
    """Variants 9-11 (fenced single posterior; the six-member block, into which the innermost loop joins) on a few rows."""
    case = CASES["bn_synth:ped10_x"]
    model = fs.make_model(case.pedigree(), **case.consts)
    fn, src = host_kernel(model, tmp_path, monkeypatch, variant)
    assert OUTER in src.splitlines()[0] and "variant %d" % variant in src.splitlines()[0]
    n = min(24, len(case.status))
    check(fn, model, case.lk[:n], case.flags[:n], case.post[:n], case.single[:n], case.status[:n], "variant %d" % variant)


def test_the_switch_restores_the_once_per_site_text(tmp_path, monkeypatch):
    """FAMSEQ_LANE_OUTER=0: variants 8-11 have the code-object names of 4-7; without it they have names of their own."""
    base = {b: object_name("ped10", 4 + b, tmp_path, monkeypatch) for b in range(4)}
    assert base[0] == "f79b34478c5381a5"  # the shipped ten-member object keeps its text
    for b in range(4):
        assert object_name("ped10", 8 + b, tmp_path, monkeypatch) not in base.values()
    monkeypatch.setenv("FAMSEQ_LANE_OUTER", "0")
    for b in range(4):
        assert object_name("ped10", 8 + b, tmp_path, monkeypatch) == base[b]
        assert object_name("ped10", 4 + b, tmp_path, monkeypatch) == base[b]


@pytest.mark.parametrize("name", ["ped5", "ped15", "trio", "quad"])
def test_pedigrees_without_the_cut_have_one_text(name, tmp_path, monkeypatch):
    assert object_name(name, 8, tmp_path, monkeypatch) == object_name(name, 4, tmp_path, monkeypatch)
    assert "outer-leaf" not in plan_of(name, 8, tmp_path, monkeypatch)["enum_lane_shape"]


def test_the_ten_member_shape_and_the_cost_model(tmp_path, monkeypatch):
    """The generator's decision for ten members: founder 5 and its children 8 and 9 as the super-leaf, their other parent 3
    outermost, taken because it executes at least 1 % fewer fp64 statements than the once-per-site form."""
    shape = plan_of("ped10", 8, tmp_path, monkeypatch)["enum_lane_shape"]
    assert shape.startswith("looped members [3 0 1], unrolled block [4 2 6 7 5 8 9] = 2187 configurations per step, " + ONCE)
    once, outer = counts(shape)
    print("fp64 statements per site: once-per-site form %d, outer-leaf plan %d (%.2f %%)" % (once, outer, 100.0 * (once - outer) / once))
    four = plan_of("ped10", 4, tmp_path, monkeypatch)["enum_lane_shape"]
    assert "(%d fp64 statements per site against" % once in four  # variant 4's own count
    assert outer <= 0.99 * once


SEEDS = [188, 1025, 1371, 1819, 2480, 3796, 4775, 5862]  # random_pedigree seeds of 7-9 members with such a cut (found by a scan of 0..5999)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_pedigrees_that_take_the_plan(seed, tmp_path, monkeypatch):
    """Randomly grown pedigrees (two or three loops, blocks of five to seven members, founders and children as the
    outermost loop), adversarial likelihoods, every flag combination, against the oracle."""
    import oracle
    from famseq_amd.prebuild_sets import random_pedigree
    from famseq_amd.synth import random_likelihoods

    rng, ped = random_pedigree(seed)
    ped.relations()
    mu = [1e-7, 1e-7, 1e-4, 0.0][seed % 4]
    model = fs.make_model(ped, mrate=mu)
    (tmp_path / "plan").mkdir()
    shape = plan_of(ped, 8, tmp_path / "plan", monkeypatch, mrate=mu)["enum_lane_shape"]
    if "outer-leaf" not in shape:
        pytest.fail("seed %d no longer takes the plan: %s" % (seed, shape))
    once, outer = counts(shape)
    assert outer <= 0.99 * once
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    assert OUTER in src.splitlines()[0]
    lk, flags = random_likelihoods(rng, ped, 64)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=mu).bn_batch(lk, flags, threads=4)
    check(fn, model, lk, flags, ref[0], ref[1], ref[2], "random %d (%s)" % (seed, shape.split(" = ")[0]))


def test_at_least_five_of_the_seeds_take_the_plan(tmp_path, monkeypatch):
    from famseq_amd.prebuild_sets import random_pedigree

    taken = []
    for seed in SEEDS:
        ped = random_pedigree(seed)[1]
        ped.relations()
        if "outer-leaf" in plan_of(ped, 8, tmp_path, monkeypatch, mrate=[1e-7, 1e-7, 1e-4, 0.0][seed % 4])["enum_lane_shape"]:
            taken.append(seed)
    assert len(taken) >= 5, taken


def test_a_plan_only_context_reports_the_bulk_object(tmp_path, monkeypatch):
    """The selection rule without a device: a context that holds the lane kernel compiles the bulk object where variant 8 + b
    differs from 4 + b, and says which kernel, from how many sites on; a pedigree without the cut has none."""
    ten = plan_of("ped10", None, tmp_path, monkeypatch)
    assert ten["enum_lane_variant"] == 4 and ten["enum_bulk_variant"] == 8 and ten["enum_bulk_failed"] == 0
    assert ten["enum_bulk_code_object"].endswith(".hsaco") and ten["enum_bulk_code_object"] != ten["enum_lane_code_object"]
    assert ten["enum_bulk_code_object"] == plan_of("ped10", 8, tmp_path, monkeypatch)["enum_lane_code_object"]
    assert ten["enum_bulk_shape"].startswith("looped members [3 0 1], unrolled block [4 2 6 7 5 8 9]")
    assert ten["enum_lane_shape"].startswith("looped members [5 0 1], unrolled block [4 2 6 7 3 8 9]")  # still K_LANE's
    assert ten["enum_bulk_min_sites"] == 16 * 64 * 256 * 4 and ten["enum_last_kind"] == ""
    five = plan_of("ped5", None, tmp_path, monkeypatch)
    assert five["enum_bulk_code_object"] == "" and five["enum_bulk_variant"] == -1 and five["enum_bulk_shape"] == ""
    # the fenced six-member block: the bulk object follows K_LANE's block shape and fencing
    assert plan_of("ped10", 7, tmp_path, monkeypatch)["enum_bulk_variant"] == 11


def test_the_option_switches_the_slot_off(tmp_path, monkeypatch):
    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1").items():
        monkeypatch.setenv(k, v)
    ctx = fs.Context(fs.make_model(fs.synthetic_pedigree("ped10")), device=-1)
    ctx.set_option("bulk_min_sites", -1)
    ctx.set_option("enum_impl", 1)
    plan = ctx.plan()
    assert plan["enum_bulk_min_sites"] == -1 and plan["enum_bulk_code_object"] == ""
    ctx.set_option("bulk_min_sites", 320)
    plan = ctx.plan()
    assert plan["enum_bulk_min_sites"] == 320 and plan["enum_bulk_code_object"].endswith(".hsaco")
    with pytest.raises(Exception):
        ctx.set_option("bulk_min_sites", -3)
    ctx.close()
