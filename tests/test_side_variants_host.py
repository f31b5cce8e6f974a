"""The CPU half of the side products' variant matrix (tests/test_gpu_side_variants.py runs it on the device).

1. The batches: on the references alone, before anything goes to a GPU, every site of the three batches that is not planted
   has status 0, a total weight of at least 1e-200 and clear partial weights for every product, under the model's rows and
   under Hardy-Weinberg rows; the three pedigrees have 0, 1 and 3 conditioned members.
2. The code objects: with a plan-only context and $FAMSEQ_VARIANT_ONLY every (pedigree, product, output form, fence level,
   plain / site-prior) yields a gfx950 code object and the plan names the level; the four texts of a family differ (a code
   object's name is the hash of its text); an index of 4 is refused.  build() has compiled all of them, so this only hashes."""
import os

import pytest

import _side_variants as SV
import famseq_amd as fs


@pytest.mark.parametrize("name", SV.PEDIGREES)
def test_the_references_of_the_batch_are_clear(name):
    c = SV.references_are_clear(name)
    assert c.conditioned == {"trio": 0, "cousins": 1, "random15": 3}[name]
    assert len(c.lk) == 3 * c.bt + 5 and c.planted.sum() == (2 if c.mrate == 0.0 else 1)
    assert (c.ped.sequenced == 0).sum() == (3 if name == "random15" else 0)
    assert name != "trio" or c.ped.n % 4 != 0  # (the byte path of map_gt)


def kernel_cache_dirs():
    return [os.path.join(os.path.dirname(fs.__file__), "lib", "kernels"), "/tmp/famseq_kernels_%d" % os.getuid()]


@pytest.mark.parametrize("name", SV.PEDIGREES)
def test_every_variant_of_every_side_product_is_built_and_named(name, monkeypatch):
    monkeypatch.delenv("FAMSEQ_KERNEL_CACHE", raising=False)
    before = [SV.pick_notes(d) for d in kernel_cache_dirs()]
    c = SV.case(name)
    objects = {}
    for v in range(SV.N_VARIANTS):
        ctx = fs.Context(c.model, device=-1)
        for p in SV.PRODUCTS.values():
            for form in range(1, p.forms + 1):
                for key in [p.stem] + ([p.stem + "_prior"] if p.has_prior else []):
                    obj = SV.forced(ctx, key, form, v, monkeypatch)
                    assert os.path.getsize(obj) > 0
                    objects.setdefault((key, form), []).append(obj)
        ctx.close()
    assert len(objects) == 19
    for family, objs in objects.items():
        assert len(set(objs)) == SV.N_VARIANTS, family  # four texts
    assert len({o for objs in objects.values() for o in objs}) == 19 * SV.N_VARIANTS
    assert [SV.pick_notes(d) for d in kernel_cache_dirs()] == before  # ($FAMSEQ_VARIANT_ONLY writes no pick note)


def test_a_variant_index_of_four_is_refused(monkeypatch):
    c = SV.case("trio")
    ctx = fs.Context(c.model, device=-1)
    monkeypatch.setenv("FAMSEQ_VARIANT_ONLY", "4")
    for p in SV.PRODUCTS.values():
        for key in [p.stem] + ([p.stem + "_prior"] if p.has_prior else []):
            with pytest.raises(fs.FamseqError, match=r"FAMSEQ_VARIANT_ONLY=4: this kernel has variants 0\.\.3"):
                ctx.set_option(key + "_kernels", 1)
            assert ctx.plan()[key + "_variant"] == -1 and ctx.plan()[key + "_code_object"] == ""
    monkeypatch.delenv("FAMSEQ_VARIANT_ONLY")
    ctx.close()
