"""The pedigrees on which the forced-variant matrices exercise the lane kernel's forms (famseq_amd/prebuild_sets.py
LANE_FORM_PEDIGREES) still take them.

The matrices (tests/test_generated_host.py, tests/test_gpu_variants.py) run a variant only where its text differs from every
lower variant's, so a generator change that makes a pedigree decline the once-per-site form or the outer-leaf plan would
quietly shrink them.  Here the number of distinct texts among variants 0-11 and which of 4 != 0, 6 != 2, 8 != 4, 10 != 6
hold are pinned per pedigree, from plan-only contexts (the names of the code objects are content hashes of the text; no
compiler runs).  A pedigree that fails here wants a replacement from a scan like the one that found
test_enum_outer_host.py's SEEDS, not a smaller number."""
import pytest

import _variants as V
from famseq_amd.prebuild_sets import LANE_FORM_PEDIGREES


@pytest.mark.parametrize("name", sorted(LANE_FORM_PEDIGREES))
def test_the_pedigree_takes_the_forms_it_is_listed_for(name, tmp_path, monkeypatch):
    distinct, relations = LANE_FORM_PEDIGREES[name]
    names, shapes = V.lane_texts(V.pedigree(name), tmp_path, monkeypatch)
    got = V.form_relations(names)
    if len(set(names)) != distinct or got != relations:
        pytest.fail("%s: %d distinct lane texts among variants 0-11 (listed: %d), 4 != 0, 6 != 2, 8 != 4, 10 != 6: %r (listed: %r)\n%s"
                    % (name, len(set(names)), distinct, got, relations, "\n".join("%2d %s %s" % (v, n, s) for v, (n, s) in enumerate(zip(names, shapes)))))
    # the plan's description says so too: the phrases appear exactly where the text is a form's own
    for v in range(4, V.LANE_VARIANTS):
        once, outer = names[v] != names[v & 3], v >= 8 and names[v] != names[v - 4]
        assert (V.ONCE in shapes[v]) == once, (name, v, shapes[v])
        assert (V.OUTER in shapes[v]) == outer, (name, v, shapes[v])
    for v in range(4):
        assert V.ONCE not in shapes[v] and V.OUTER not in shapes[v], (name, v, shapes[v])


def test_every_form_and_block_shape_is_exercised_on_four_pedigrees():
    """What the lists promise the matrices: each of 4 != 0, 6 != 2 on at least four pedigrees, 8 != 4 and 10 != 6 on at least
    four, and one pedigree that takes a form for one block shape only."""
    rel = [r for _, r in LANE_FORM_PEDIGREES.values()]
    assert all(sum(r[k] for r in rel) >= 4 for k in range(4))
    assert any(r[0] != r[1] for r in rel)


def test_the_matrices_own_pedigrees_have_no_form_but_ped10(tmp_path, monkeypatch):
    """(why the list exists: on every pedigree of V.PEDIGREES but ped10, variants 4-11 are the text of 0-3)"""
    for name in V.PEDIGREES:
        if name in LANE_FORM_PEDIGREES:
            continue
        (tmp_path / name.replace(":", "_")).mkdir()
        names, _ = V.lane_texts(V.pedigree(name), tmp_path / name.replace(":", "_"), monkeypatch)
        assert names[4:8] == names[:4] and names[8:] == names[:4], name


def plan_under_pick(ped, pick, cache, monkeypatch, digits=0, call=False):
    """The plan of a plan-only context that holds the lane kernel under pick_lane = `pick`, the lanes-per-site kernels up to
    `digits` digits and, if asked, the call-path form (no compiler runs: the names are what is compared)."""
    import famseq_amd as fs

    for k, v in dict(FAMSEQ_KERNEL_CACHE=str(cache), FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1").items():
        monkeypatch.setenv(k, v)
    ctx = fs.Context(fs.make_model(ped, mrate=V.MRATE), device=-1)
    try:
        ctx.set_option("pick_lane", pick)
        ctx.set_option("enum_impl", 1)
        for d in range(1, digits + 1):
            ctx.set_option("group_digits", d)
        if call:
            ctx.set_option("call_kernels", 2)
        plan = ctx.plan()
        assert plan["enum_lane_variant"] == pick
        return plan
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["ped10", "random1025", "grown11"])
def test_the_lanes_per_site_forms_do_not_follow_a_pick(name, tmp_path, monkeypatch):
    """enumgen_variant(v, d > 0) switches the once-per-site form and the outer-leaf plan off and takes the six-member block:
    under any pick of 4-11 the lanes-per-site kernels are the code objects they are under pick 2."""
    ped = V.pedigree(name)
    dmax = plan_under_pick(ped, 2, tmp_path, monkeypatch)["enum_group_digits_max"]
    assert dmax >= 2
    want = plan_under_pick(ped, 2, tmp_path, monkeypatch, digits=dmax)["enum_group_code_objects"]
    assert len(want) >= dmax and all(o.endswith(".hsaco") for o in want[:dmax]) and len(set(want[:dmax])) == dmax
    for v in range(4, V.LANE_VARIANTS):
        assert plan_under_pick(ped, v, tmp_path, monkeypatch, digits=dmax)["enum_group_code_objects"] == want, (name, v)


@pytest.mark.parametrize("name", sorted(LANE_FORM_PEDIGREES))
def test_the_call_path_keeps_the_per_prefix_text(name, tmp_path, monkeypatch):
    """enumgen_call_variant maps a lane pick v to the call variant of plain variant v & 3's block shape: under pick_lane = v,
    v in 4..11, the call-path form is the code object it is under pick_lane = v & 3, and none of the lane kernel's own."""
    ped = V.pedigree(name)
    names, _ = V.lane_texts(ped, tmp_path, monkeypatch)
    want = [plan_under_pick(ped, v, tmp_path, monkeypatch, call=True) for v in range(4)]
    for v in range(4, V.LANE_VARIANTS):
        plan = plan_under_pick(ped, v, tmp_path, monkeypatch, call=True)
        obj = plan["enum_lane_call_code_object"]
        assert obj.endswith(".hsaco") and obj == want[v & 3]["enum_lane_call_code_object"], (name, v)
        assert plan["enum_lane_call_variant"] == want[v & 3]["enum_lane_call_variant"], (name, v)
        assert obj.split("/")[-1][:-len(".hsaco")] not in names, (name, v)


@pytest.mark.parametrize("name", sorted(LANE_FORM_PEDIGREES))
def test_the_bulk_object_exists_where_the_outer_leaf_text_does(name, tmp_path, monkeypatch):
    """The bulk slot follows the lane kernel's block shape and fencing (variant 8 + b for lane variant 4 + b): a plan-only
    context reports a bulk object under the lane picks 4-7 exactly where 8 + b is a text of its own, and it is that text."""
    import os

    ped = V.pedigree(name)
    names, _ = V.lane_texts(ped, tmp_path, monkeypatch)
    for v in range(4, 8):
        plan = plan_under_pick(ped, v, tmp_path, monkeypatch)
        if names[v + 4] != names[v]:
            assert plan["enum_bulk_variant"] == v + 4 and os.path.basename(plan["enum_bulk_code_object"]) == names[v + 4] + ".hsaco", (name, v)
            assert V.OUTER in plan["enum_bulk_shape"] and V.OUTER not in plan["enum_lane_shape"], (name, v)
        else:
            assert plan["enum_bulk_code_object"] == "" and plan["enum_bulk_variant"] == -1 and plan["enum_bulk_shape"] == "", (name, v)
