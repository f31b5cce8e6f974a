"""Every fence level of every side-product kernel, forced one at a time and run on the device.

The ten side-product kernels (trio in its three output forms, map, evidence, loo, pattern, sample, af, relabel) and their nine
site-prior siblings each exist in four variants (kTrioVariants .. kRelabelVariants of csrc/elim_codegen.h); their contest
(csrc/jit.cpp jit_pick_variant) starts at 0 and takes the first that does not spill, so the rest of the GPU suite runs
whichever that is for its pedigrees.  Their host twins (test_the_four_variants_give_the_same_bits of tests/test_*_host.py)
compile the same text for the CPU, where a fence is a no-op.  Here each level is forced through $FAMSEQ_VARIANT_ONLY — set only
around the option that loads the kernel, the plan checked to name it —, run on tests/_side_variants.py's batch of each of three
pedigrees (loop-free; one conditioned member; three conditioned and three unsequenced members) and held to:
  - the product's own reference through the product's own check (tolerances: that module's, none defined here), status exact,
    NaN / -1 on the planted sites — for the plain form and for the site-prior form under Hardy-Weinberg rows;
  - the site-prior form on the model's own rows: the plain form's bits;
  - sub-batches of 1, BT - 1 and BT + 1 sites: the bits of the slices; the default grid: the bits of one workgroup's four trips;
  - the four levels: the same bits, NaN patterns included; the trio forms: the same bits in what they share.
$FAMSEQ_VARIANT_ONLY writes no pick note, so these tests use the ordinary kernel cache (build() has compiled every object they
load); the last test asserts that the cache's notes are what they were."""
import numpy as np
import pytest

import _side_variants as SV
import famseq_amd as fs
from test_side_variants_host import kernel_cache_dirs

pytestmark = pytest.mark.gpu

_NOTES = {}


def notes():
    out = {}
    for d in kernel_cache_dirs():
        for f in SV.pick_notes(d):
            out[d + "/" + f] = open(d + "/" + f).read()
    return out


@pytest.fixture(autouse=True)
def _ordinary_cache(monkeypatch):
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN"):
        monkeypatch.delenv(key, raising=False)
    _NOTES.setdefault("before", notes())
    yield


def load(c, p, v, monkeypatch):
    """A device context that holds every form of product p, plain and site-prior, at fence level v (the plan checked)."""
    ctx = fs.Context(c.model, device=0)
    try:
        for form in range(1, p.forms + 1):
            SV.forced(ctx, p.stem, form, v, monkeypatch)
            if p.has_prior:
                SV.forced(ctx, p.stem + "_prior", form, v, monkeypatch)
        ctx.set_option("grid_blocks", 1)
    except BaseException:
        ctx.close()
        raise
    return ctx


def one_variant(c, p, v, form, ctx):
    """-> (plain, Hardy-Weinberg) outputs of the whole batch on one workgroup, everything that concerns one variant asserted."""
    what = "%s: %s form %d variant %d" % (c.name, p.stem, form, v)
    n = len(c.lk)
    plain = p.run(ctx, c, n, None, form)
    p.check(c, plain, p.cached(c, False), what)
    SV.planted_fills(c, plain, p.fills)
    runs = [(None, plain)]
    if p.has_prior:
        assert SV.same_bits(p.run(ctx, c, n, c.rows, form), plain), what + ": the model's rows"
        hwe = p.run(ctx, c, n, c.hwe, form)
        p.check(c, hwe, p.cached(c, True), what + ", Hardy-Weinberg rows")
        SV.planted_fills(c, hwe, p.fills)
        runs.append((c.hwe, hwe))
    for prior, whole in runs:
        for s in (1, c.bt - 1, c.bt + 1):
            assert SV.same_bits(p.run(ctx, c, s, prior, form), SV.sub(whole, slice(0, s))), (what, s, prior is not None)
    ctx.set_option("grid_blocks", 0)
    for prior, whole in runs:
        assert SV.same_bits(p.run(ctx, c, n, prior, form), whole), (what, "default grid", prior is not None)
    ctx.set_option("grid_blocks", 1)
    return [whole for _, whole in runs]


@pytest.mark.parametrize("name", SV.PEDIGREES)
@pytest.mark.parametrize("stem", SV.PRODUCTS)
def test_every_variant(stem, name, monkeypatch):
    c, p = SV.case(name), SV.PRODUCTS[stem]
    forms = (3, 1, 2) if p.forms == 3 else (1,)
    out = {}
    for v in range(SV.N_VARIANTS):
        ctx = load(c, p, v, monkeypatch)
        try:
            for form in forms:
                out[v, form] = one_variant(c, p, v, form, ctx)
            plan = ctx.plan()
            assert plan[stem + "_variant"] == v and (not p.has_prior or plan[stem + "_prior_variant"] == v)
        finally:
            ctx.close()
        print("loaded and confirmed by the plan: %s, %s, variant %d" % (name, stem, v))
    for (v, form), runs in out.items():
        for got, want, kind in zip(runs, out[0, form], ("plain", "site-prior")):
            assert SV.same_bits(got, want), "%s: %s form %d, %s: variant %d differs from variant 0" % (name, stem, form, kind, v)
    if p.forms == 3:  # (joint, dnm, status): a form returns only its own outputs, and what two forms share has the same bits
        for v in range(SV.N_VARIANTS):
            for k in range(len(out[v, 3])):
                (j3, d3, s3), (j1, d1, s1), (j2, d2, s2) = out[v, 3][k], out[v, 1][k], out[v, 2][k]
                assert j1 is None and d2 is None
                assert SV.same_bits((d1, s1), (d3, s3)) and SV.same_bits((j2, s2), (j3, s3)), (name, v, k)


def test_the_caches_pick_notes_are_what_they_were():
    """Nothing above wrote a pick note (or moved one build() ships) into the kernel cache the rest of the suite loads from."""
    assert "before" in _NOTES and notes() == _NOTES["before"]
