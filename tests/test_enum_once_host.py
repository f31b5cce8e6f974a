"""The lane kernel's once-per-site form (csrc/enum_codegen.cpp, "The once-per-site form") without a GPU.

Where the cost model takes it, the innermost looped member joins the unrolled block, the prefix levels' tables
that mention no loop digit are built once per site (and chrX pass) into the lane's LDS row, and the prefix
members' marginals are formed after the loops.  The generated source is compiled for the host (the helpers of
test_generated_host.py) and compared with the fixtures and the oracle; the forms that must NOT change — small
pedigrees, lanes-per-site, the call path of variants 0-3, and everything under FAMSEQ_LANE_HOIST=0 — are pinned by the names
of their code objects, which are content hashes of the generated text, taken from the commit before this form.
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
CASES = {c.name: c for c in load_cases()}


def host_kernel(model, tmp_path, monkeypatch):
    fn = build_host_kernel(model, "lane", tmp_path, monkeypatch)
    return fn, open(tmp_path / "cache_lane" / "k.cpp").read()


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


@pytest.mark.parametrize("name", ["bn_synth:ped10", "bn_synth:ped10_x"])
def test_ten_member_fixtures(name, tmp_path, monkeypatch):
    """Every fixture of the ten-member pedigree, autosome and chrX (per-pass tables)."""
    case = CASES[name]
    model = fs.make_model(case.pedigree(), **case.consts)
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    assert ONCE in src.splitlines()[0] and "looped member 4 unrolled ahead of the block" in src.splitlines()[0]
    assert "unrolled block: 4 2 6 7 3 8 9 (2187 configurations per outer step)" in src
    check(fn, model, case.lk, case.flags, case.post, case.single, case.status, name)


def test_ten_members_every_flag_and_planted_site(tmp_path, monkeypatch):
    """All four (Known, chrX) combinations, a shortcut site, failed single posteriors, a BN failure, the -LRC boundary and
    row sums below 1e-290 (the variant matrices' batch), mutation rate 0, against the oracle."""
    ped = V.pedigree("ped10")
    model = fs.make_model(ped, mrate=V.MRATE)
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    assert ONCE in src.splitlines()[0]
    lk, flags, has_bn_fail = V.variant_batch(ped, 128)
    ref = V.reference(ped, lk, flags)
    assert has_bn_fail and 2 in ref[2] and 1 in ref[2] and 0x80 in ref[2]
    check(fn, model, lk, flags, ref[0], ref[1], ref[2], "ped10 planted sites")


def test_fifteen_members(tmp_path, monkeypatch):
    """Fifteen members run in whatever form the cost model takes (the per-prefix one: its seven-member block leaves no
    room for another level) — same checks."""
    ped = V.pedigree("ped15")
    model = fs.make_model(ped, mrate=V.MRATE)
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    probe = fs.Context(model, device=-1)
    assert (ONCE in probe.plan()["enum_lane_shape"]) == (ONCE in src.splitlines()[0])
    probe.close()
    from famseq_amd.synth import random_likelihoods

    lk, flags = random_likelihoods(np.random.RandomState(15), ped, 8)  # adversarial rows, every flag combination
    ref = V.reference(ped, lk, flags)
    check(fn, model, lk, flags, ref[0], ref[1], ref[2], "ped15")


@pytest.mark.parametrize("seed", [10, 26, 33])
def test_soak_pedigrees_that_take_the_form(seed, tmp_path, monkeypatch):
    """Randomly grown pedigrees on which the cost model takes the form: seven unrolled members (10, 26: unsequenced members,
    mutation rates 1e-4 and 0, a marriage loop) and six (33: the prefix tables of two members are rebuilt per step), adversarial likelihoods, every flag combination."""
    import oracle
    from famseq_amd.prebuild_sets import soak_pedigree
    from famseq_amd.synth import random_likelihoods

    rng, ped, mu = soak_pedigree(seed)
    model = fs.make_model(ped, mrate=mu)
    fn, src = host_kernel(model, tmp_path, monkeypatch)
    assert ONCE in src.splitlines()[0]
    lk, flags = random_likelihoods(rng, ped, 96)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=mu).bn_batch(lk, flags, threads=4)
    check(fn, model, lk, flags, ref[0], ref[1], ref[2], "soak %d" % seed)


# ---- the forms that keep their text: names of their code objects at the commit before this form ------------------------------

PARENT = {
    ("trio", 0, "plain"): "3e9c49728d76e829", ("quad", 0, "plain"): "e35dfddc1ae580da", ("ped5", 0, "plain"): "5373c27403a79f8d",
    ("trio", 2, "plain"): "ce2500b6395b01bf", ("quad", 2, "plain"): "af18035fbe452810", ("ped5", 2, "plain"): "18402820b7d52dcf",
    ("ped5", 2, "group1"): "d8c846c113890a8a", ("ped5", 2, "call"): "07ed6054d0745b6b",
    ("ped10", 2, "group1"): "62367186a388a0a0", ("ped10", 2, "group2"): "2df3cb65ce9a6564", ("ped10", 2, "group3"): "e13393715ae1ed84",
    ("ped10", 2, "group4"): "590a8b2bb8800d96", ("ped10", 2, "call"): "b79d433bd4513a51",
    ("ped15", 0, "plain"): "efdf43e78f08a299",
}
PARENT_HOIST_OFF = {("ped10", 0): "0fd7646fe4c924e6", ("ped10", 1): "7d0022c47cb89200", ("ped10", 2): "ae25fc17cceea40c",
                    ("ped10", 3): "83bad8b9d898d292"}


def object_name(ped_name, variant, form, tmp_path, monkeypatch):
    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1").items():
        monkeypatch.setenv(k, v)
    ctx = fs.Context(fs.make_model(fs.synthetic_pedigree(ped_name)), device=-1)
    try:
        ctx.set_option("pick_lane", variant)
        ctx.set_option("enum_impl", 1)
        if form == "plain":
            obj = ctx.plan()["enum_lane_code_object"]
        elif form == "call":
            ctx.set_option("call_kernels", 1)
            obj = ctx.plan()["enum_lane_call_code_object"]
        else:
            d = int(form[5:])
            ctx.set_option("group_digits", d)
            obj = ctx.plan()["enum_group_code_objects"][d - 1]
    finally:
        ctx.close()
    return os.path.basename(obj)[:-len(".hsaco")]


@pytest.mark.parametrize("key", sorted(PARENT), ids=["%s-v%d-%s" % k for k in sorted(PARENT)])
def test_other_forms_keep_their_text(key, tmp_path, monkeypatch):
    assert object_name(*key, tmp_path, monkeypatch) == PARENT[key]


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_the_variable_restores_the_per_prefix_text(variant, tmp_path, monkeypatch):
    """Variants 0-3 of the ten-member kernel are the text of the commit before, whatever the variable says; variants 4-7
    are the once-per-site form of 0-3, and FAMSEQ_LANE_HOIST=0 turns them into that text too, byte for byte."""
    want = PARENT_HOIST_OFF[("ped10", variant)]
    assert object_name("ped10", variant, "plain", tmp_path, monkeypatch) == want
    assert object_name("ped10", variant + 4, "plain", tmp_path, monkeypatch) != want
    monkeypatch.setenv("FAMSEQ_LANE_HOIST", "0")
    assert object_name("ped10", variant, "plain", tmp_path, monkeypatch) == want
    assert object_name("ped10", variant + 4, "plain", tmp_path, monkeypatch) == want


def test_the_call_path_form_keeps_the_per_prefix_text(tmp_path, monkeypatch):
    """The call path is not part of this form: a context on plain variant 4 or 6 builds its call-path kernel from the
    per-prefix text of the same block shape (the commit-before's b79d433bd4513a51 for the six-member block), so the fused
    kernel's posteriors differ from that context's plain kernel in their last bits."""
    assert object_name("ped10", 6, "call", tmp_path, monkeypatch) == PARENT[("ped10", 2, "call")]
    assert object_name("ped10", 4, "call", tmp_path, monkeypatch) == object_name("ped10", 0, "call", tmp_path, monkeypatch)


def test_declined_pedigrees_have_no_second_text(tmp_path, monkeypatch):
    """Where the cost model declines (fifteen members, five members) variants 4-7 ARE variants 0-3."""
    for name in ("ped15", "ped5"):
        assert object_name(name, 4, "plain", tmp_path, monkeypatch) == PARENT[(name, 0, "plain")]


def test_the_plan_names_the_form(tmp_path, monkeypatch):
    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1").items():
        monkeypatch.setenv(k, v)
    shapes = {}
    for name in ("ped5", "ped10"):
        ctx = fs.Context(fs.make_model(fs.synthetic_pedigree(name)), device=-1)
        ctx.set_option("enum_impl", 1)
        shapes[name] = ctx.plan()["enum_lane_shape"]
        ctx.close()
    assert ONCE not in shapes["ped5"]
    assert shapes["ped10"].startswith("looped members [5 0 1], unrolled block [4 2 6 7 3 8 9] = 2187 configurations per step, " + ONCE)


def test_the_plan_names_the_form_where_the_manifest_has_a_second_text(tmp_path, monkeypatch):
    """A context that is free to choose starts its variant contest at the once-per-site variants, and its plan says so, exactly
    for the pedigrees whose lane/4 differs from lane/0 in the manifest of generated sources (the generator answers the question
    from its decision function, the manifest from the texts)."""
    import json
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import source_digests as D

    with open(os.path.join(root, "tests", "golden", "generated_sources.json")) as f:
        golden = json.load(f)
    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1").items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("FAMSEQ_VARIANT_ONLY", raising=False)
    second_text, named = set(), set()
    for name in D.PEDIGREES:
        ped = D._named(name)
        if ped.n > fs.MAXN:
            continue
        ped.relations()
        if golden["%s lane/4" % name] != golden["%s lane/0" % name]:
            second_text.add(name)
        ctx = fs.Context(fs.make_model(ped), device=-1)
        ctx.set_option("enum_impl", 1)
        plan = ctx.plan()
        ctx.close()
        assert (plan["enum_lane_first_variant"] == 4) == (ONCE in plan["enum_lane_shape"]), name
        if ONCE in plan["enum_lane_shape"]:
            named.add(name)
    assert second_text == named
    assert {"ped10", "random99"} <= named
