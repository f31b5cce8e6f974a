"""The CPU half of the edge-pedigree tests (tests/test_gpu_edge_pedigrees.py runs the recipes on the device).

1. The table of famseq_amd/prebuild_sets.py EDGE_PEDIGREES, pinned from plan-only contexts that run no compiler: members,
   sequenced members, conditioned members; the three forms of relabel_source at 37, 38 / 39 and 40 members and the lean switch of
   the other side sources between 39 and 40, read from the emitted text.  A generator change that moves an edge fails here and
   names the recipe to move: the recipes exist to sit on these edges, so a recipe that no longer does wants a replacement on
   the edge's new place (and the table, the GPU test's record and DESIGN.md's paragraph with it), not a changed expectation.
2. The elimination references (tests/_maxproduct.py marginals and max_product, test_pattern_host._total under the model's and under
   site priors, tests/_af.py's founder rows) against the 3^N enumeration on loop12 and loop13: the same bars they are held to at
   ten members or fewer (test_map_host.test_the_helper_matches_the_enumeration: 1e-9; test_relabel_host.reference: 1e-12 on the
   totals), now with 3 and 2 conditioned members' worth of loops above ten members.
3. Every recipe's batch: on the references alone, what the products' own clear rules assert (tests/_edge.py).
4. build() has left every code object the device test loads in the in-tree cache."""
import os
import re
from unittest import mock

import numpy as np
import pytest

import _af as A
import _edge as ED
import _maxproduct as mp
import _prior as P
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets
from test_map_host import RTOL, brute_weights
from test_pattern_host import _total
from test_sample_host import prior_weights

IN_TREE = os.path.join(os.path.dirname(fs.__file__), "lib", "kernels")


def source_only(tmp_path):
    return mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1"))


def text_of(ctx, key):
    ctx.set_option(key + "_kernels", 1)
    return open(ctx.plan()[key + "_code_object"][:-len(".hsaco")] + ".hip").read()


def factor_macros(src):
    """The emitter's local factors as macros (`#define l12_0 ...`, six names per member in the lean form's own way)."""
    return len(re.findall(r"^#define [a-z]+\d+_\d ", src, re.M))


@pytest.mark.parametrize("name", ED.PEDIGREES)
def test_the_recipe_is_what_the_table_says(name, tmp_path):
    seed, n, loops, sequenced, conditioned, mrate = sets.EDGE_PEDIGREES[name]
    ped = sets.edge_pedigree(name)
    with source_only(tmp_path):
        ctx = fs.Context(fs.make_model(ped, mrate=mrate), device=-1)
        plan = ctx.plan()
        ctx.close()
    got = (ped.n, int(np.sum(ped.sequenced)), plan["elim_conditioned_members"])
    assert plan["elim_supported"] and got == (n, sequenced, conditioned), \
        "%s: (members, sequenced, conditioned) = %r, listed %r: find another seed for this edge" % (name, got, (n, sequenced, conditioned))
    assert (conditioned > 0) == loops
    assert plan["evidence_block_threads"] == ED.BT == plan["loo_block_threads"]


def test_the_recipes_cover_the_edges():
    t = sets.EDGE_PEDIGREES
    assert [t["edge%d" % n][1] for n in (37, 38, 39, 40)] == [37, 38, 39, 40]
    looped = [t[n] for n in ED.LOOPED]
    assert len(looped) == 5 and all(11 <= r[1] <= 20 for r in looped) and {r[4] for r in looped} == {1, 2, 3}
    assert {r[5] for r in t.values()} == {1e-7, 1e-4, 0.0} and {r[5] for r in looped} == {1e-7, 1e-4, 0.0}
    assert sum(r[1] <= sets.EDGE_LANE_MAX for r in looped) == 2


def test_relabels_three_forms_and_the_lean_switch(tmp_path):
    """relabel_source: the lane's rows in LDS up to 37 members; at 38 and 39 the shell reads the site's row from global memory
    (glb_cvd) while the emitter's local factors are still variables; from 40 on the emitter is lean too (its factors macros over
    the row).  evidence_source (every other side source's shell): no global row up to 39 members, lean from 40."""
    seen = {}
    for n in (37, 38, 39, 40):
        name = "edge%d" % n
        (tmp_path / name).mkdir()
        with source_only(tmp_path / name):
            ctx = fs.Context(fs.make_model(sets.edge_pedigree(name), mrate=sets.EDGE_PEDIGREES[name][5]), device=-1)
            relabel, evidence, sample = text_of(ctx, "relabel"), text_of(ctx, "evidence"), text_of(ctx, "sample")
            ctx.close()
        seen[n] = ("s_l[BT *" in relabel, "glb_cvd" in relabel, factor_macros(relabel), "glb_cvd" in evidence,
                   "#define l0_0 lgv[0]" in evidence, "lgv[" in sample)
        print(name, seen[n])
    assert [seen[n][0] for n in (37, 38, 39, 40)] == [True, False, False, False], "relabel's rows in LDS: edge37 and only edge37"
    assert [seen[n][1] for n in (37, 38, 39, 40)] == [False, True, True, True], "relabel's shell reads global rows from edge38 on"
    macros = [seen[n][2] for n in (37, 38, 39, 40)]
    assert macros[2] - macros[1] == 6 and macros[1] - macros[0] == 6, macros  # six names per member while the emitter is not lean
    assert macros[2] == 234 and macros[3] == 360, macros  # ... and the lean emitter's macros at forty
    for k in (3, 4, 5):  # the lean switch of the other side sources: between edge39 and edge40
        assert [seen[n][k] for n in (37, 38, 39, 40)] == [False, False, False, True], k


@pytest.mark.parametrize("name", ["loop12", "loop13"])
def test_the_elimination_matches_the_enumeration_above_ten_members_with_loops(name):
    c = ED.case(name)
    sites = slice(4, 12)  # eight sites, flags 0..3 twice, the planted ones among them
    lk, flags, want_st = c.lk[sites], c.flags[sites], c.want_status[sites]
    G, Wt, st = brute_weights(c.ped, c.mrate, lk, flags)
    assert np.array_equal(st, want_st)
    ok = st == 0
    Wt = Wt[ok]
    gt, wmax, z, mst = mp.max_product(c.ped, c.mrate, lk, flags)
    assert np.array_equal(mst, st)
    zt, fail = _total(c.ped, c.mrate, lk, flags, None)
    assert np.array_equal(fail, st == 1) and np.all(zt[st == 2] == 0)
    print("%s: worst relative error of Z %.3g, of the maximum %.3g" % (
        name, np.abs(zt[ok] / Wt.sum(axis=1) - 1).max(), np.abs(wmax[ok] / Wt.max(axis=1) - 1).max()))
    np.testing.assert_allclose(zt[ok], Wt.sum(axis=1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(z[ok], Wt.sum(axis=1), rtol=RTOL, atol=0)
    np.testing.assert_allclose(wmax[ok], Wt.max(axis=1), rtol=RTOL, atol=0)
    w_ret = mp.config_weight(c.ped, c.mrate, lk[ok], flags[ok], gt[ok])
    assert np.all(w_ret >= (1 - 1e-9) * Wt.max(axis=1))
    marg = mp.marginals(c.ped, c.mrate, lk[ok], flags[ok])
    for p in range(c.ped.n):
        ref = np.stack([np.where(G[p] == g, Wt, 0.0).sum(axis=1) for g in range(3)], axis=1) / Wt.sum(axis=1)[:, None]
        np.testing.assert_allclose(marg[:, p], ref, rtol=RTOL, atol=1e-300)
    del Wt
    # under site priors: the Hardy-Weinberg rows' total, and tests/_af.py's founder rows by the elimination against the
    # compiled oracle's (one model per site, which enumerates)
    _, Wh, hst = prior_weights(c.ped, c.mrate, lk, flags, c.hwe[sites])
    assert np.array_equal(hst, want_st)
    zh, _ = _total(c.ped, c.mrate, lk, flags, c.hwe[sites])
    np.testing.assert_allclose(zh[ok], Wh[ok].sum(axis=1), rtol=1e-12, atol=0)
    del Wh, G
    if name == "loop12":
        by_oracle = A.founder_rows(c.ped, c.mrate, lk[ok], flags[ok], c.hwe[sites][ok])
        by_elimination = A.founder_rows(c.ped, c.mrate, lk[ok], flags[ok], c.hwe[sites][ok], oracle_upto=10)
        assert list(by_oracle) == list(by_elimination) == A.founders_of(c.ped)
        for f, rows in by_elimination.items():
            np.testing.assert_allclose(rows / rows.sum(axis=1, keepdims=True), by_oracle[f], rtol=P.RTOL, atol=0)


@pytest.mark.parametrize("name", ED.PEDIGREES)
def test_the_references_of_the_batch_are_clear(name):
    c = ED.references_are_clear(name)
    assert len(c.lk) == 197 == 3 * ED.BT + 5 and c.planted.sum() == (2 if c.mrate == 0.0 else 1)
    assert np.array_equal(np.unique(c.flags[~c.planted]), [0, 1, 2, 3])
    assert np.all(c.lk[:, c.ped.sequenced == 0, :] == 1.0) and (c.ped.sequenced == 0).sum() == c.ped.n - c.n_sequenced > 0
    z = c.refs["joint", False].z[~c.planted]
    print("%s: smallest Z %.3g under the model's rows, %.3g under Hardy-Weinberg rows" % (name, z.min(), c.refs["joint", True].z[~c.planted].min()))


def edge_objects(ctx, ped):
    """Load what the device test loads into a context; -> {plan key: code object}."""
    if ped.n <= sets.EDGE_LANE_MAX:
        ctx.set_option("enum_impl", 1)
    if ped.n <= fs.MAXN:
        ctx.set_option("engine", fs.ENGINE_ELIM)
        ctx.set_option("call_kernels", 1)
    objects = {}
    for stem, forms, has_prior in sets.SIDE_PRODUCTS + sets.SIDE_PRODUCTS_SINCE:
        for key in [stem] + ([stem + "_prior"] if has_prior else []):
            for form in range(1, forms + 1):
                ctx.set_option(key + "_kernels", form)
                objects["%s form %d" % (key, form)] = ctx.plan()[key + "_code_object"]
    objects.update({k: v for k, v in ctx.plan().items() if k.endswith("_code_object") and v})
    return objects


@pytest.mark.parametrize("name", ED.PEDIGREES)
def test_build_left_the_code_objects_in_the_tree(name, monkeypatch):
    """No pedigree of the set needs a compile on the GPU box (here: this only hashes)."""
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN", "FAMSEQ_JIT_SOURCE_ONLY"):
        monkeypatch.delenv(key, raising=False)
    c = ED.case(name)
    before = set(os.listdir(IN_TREE))
    ctx = fs.Context(c.model, device=-1)
    try:
        objects = edge_objects(ctx, c.ped)
    finally:
        ctx.close()
    assert len(objects) >= 21, sorted(objects)
    for key, obj in objects.items():
        assert obj.endswith(".hsaco") and os.path.dirname(obj) == IN_TREE and os.path.getsize(obj) > 0, (name, key, obj)
        assert os.path.basename(obj) in before, "%s: %s was compiled here, not by build()" % (name, key)


@pytest.mark.parametrize("name", ["loop12", "loop13"])
def test_the_main_engines_host_reference_is_the_enumeration_oracles(name):
    """tests/_edge.py main_reference (the single posterior, the -LRC vote, the status and tests/_maxproduct.py's marginals) against
    the compiled enumeration oracle, on the recipe's batch and on its call-path batch: status and single posterior bit for bit,
    shortcut rows bit for bit, posteriors at 1e-9."""
    import oracle

    c = ED.case(name)
    ped = c.ped
    m = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=c.mrate)
    for what, lk in (("batch", c.lk), ("call-path batch", ED.call_batch(c)[2])):
        post, single, status, z = ED.main_reference(c, lk, c.flags)
        assert np.all(z[status == 0] >= ED.FLOOR), what
        P.check((post, single, status), m.bn_batch(lk, c.flags, threads=8), "%s, %s" % (name, what))
        assert what == "batch" or (status == 0x80).sum() >= 2
