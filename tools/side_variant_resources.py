#!/usr/bin/env python3
"""What the variant contest of the side-product kernels does on the pedigrees of prebuild_sets.SIDE_VARIANT_PEDIGREES.

For each (pedigree, product, output form, plain / site-prior) a line with the scratch bytes per lane of fence levels 0..3 —
from the resource notes (<hash>.res) the compiler's remarks leave next to each code object, not from a disassembly — and the
level the unforced contest (csrc/jit.cpp jit_pick_variant: the first that spills at most 16 bytes, else the least) takes.
No GPU: plan-only contexts; after build() every object is a cache hit.

    python tools/side_variant_resources.py > profiles/side_variants/resources.txt
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import famseq_amd as fs  # noqa: E402
from famseq_amd import prebuild_sets as sets  # noqa: E402


def built(ped, key, form, variant=None):
    """-> (variant taken, scratch bytes per lane) of the kernel "<key>" in output form `form`; variant None: the contest."""
    if variant is None:
        os.environ.pop("FAMSEQ_VARIANT_ONLY", None)
    else:
        os.environ["FAMSEQ_VARIANT_ONLY"] = str(variant)
    ctx = fs.Context(fs.make_model(ped), device=-1)
    try:
        ctx.set_option(key + "_kernels", form)
        plan = ctx.plan()
    finally:
        ctx.close()
        os.environ.pop("FAMSEQ_VARIANT_ONLY", None)
    obj = plan[key + "_code_object"]
    with open(obj[:-6] + ".res") as f:
        return plan[key + "_variant"], int(f.read().split()[0])


def main():
    print("# scratch bytes per lane (gfx950, -O3) of every fence level of the side-product kernels, and the level the contest takes")
    print("# %-9s %-15s %4s | %5s %5s %5s %5s | %s" % ("pedigree", "kernel", "form", "v0", "v1", "v2", "v3", "contest"))
    for name in sets.SIDE_VARIANT_PEDIGREES:
        ped = sets.side_variant_pedigree(name)
        for stem, forms, has_prior in sets.SIDE_PRODUCTS:
            for form in range(1, forms + 1):
                for key in [stem] + ([stem + "_prior"] if has_prior else []):
                    scratch = []
                    for v in range(sets.SIDE_VARIANTS):
                        got, s = built(ped, key, form, v)
                        assert got == v
                        scratch.append(s)
                    taken, _ = built(ped, key, form)
                    print("  %-9s %-15s %4d | %5d %5d %5d %5d | v%d" % (name, key, form, *scratch, taken))


if __name__ == "__main__":
    main()
