#!/usr/bin/env python3
"""What the variant contest of the side-product kernels does on the pedigrees of prebuild_sets.SIDE_VARIANT_PEDIGREES.

For each (pedigree, product, output form, plain / site-prior) a line with the scratch bytes per lane of fence levels 0..3 —
from the resource notes (<hash>.res) the compiler's remarks leave next to each code object, not from a disassembly — and the
level the unforced contest (csrc/jit.cpp jit_pick_variant: the first that spills at most 16 bytes, else the least) takes.
No GPU: plan-only contexts; after build() every object is a cache hit.

    python tools/side_variant_resources.py > profiles/side_variants/resources.txt

With arguments, one product on pedigrees of the caller's choice, registers and LDS too:

    python tools/side_variant_resources.py weight trio ped10 wide32 wide48 > profiles/weight/resources.txt

prints, for each pedigree (a synthetic_pedigree name, or wide<N>) and each of the product's eight code objects (fence levels 0..3,
plain and site-prior), VGPRs, AGPRs, scratch, waves per SIMD and LDS from the compiler's remarks on the kept source (hipcc
--offload-arch=gfx950 with the flags of csrc/jit.cpp; no GPU), and the level the contest takes.
"""
import os
import re
import subprocess
import sys
import tempfile

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


def remarks(src):
    """The kernel-resource-usage remarks of one kept source -> {name: value}."""
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--genco",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True, check=True)
    return {k.strip(): int(v) for k, v in re.findall(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", p.stderr)}


def one_product(stem, names):
    print("# registers, scratch (bytes per lane), waves per SIMD and LDS (bytes per workgroup) of famseq_%s / famseq_%s_prior, every fence level" % (stem, stem))
    print("# (gfx950, -O3, -ffp-contract=off; from the compiler's remarks on each kept source), and the level the contest takes")
    with tempfile.TemporaryDirectory() as cache:
        os.environ["FAMSEQ_KERNEL_CACHE"], os.environ["FAMSEQ_KEEP_SRC"] = cache, "1"
        for name in names:
            ped = sets.wide_pedigree(int(name[4:])) if name.startswith("wide") else fs.synthetic_pedigree(name)
            print("== %s (%d members)" % (name, ped.n))
            for key in (stem, stem + "_prior"):
                taken = None
                for v in list(range(sets.SIDE_VARIANTS)) + [None]:
                    os.environ.pop("FAMSEQ_VARIANT_ONLY", None)
                    if v is not None:
                        os.environ["FAMSEQ_VARIANT_ONLY"] = str(v)
                    ctx = fs.Context(fs.make_model(ped), device=-1)
                    try:
                        ctx.set_option(key + "_kernels", 1)
                        plan = ctx.plan()
                    finally:
                        ctx.close()
                        os.environ.pop("FAMSEQ_VARIANT_ONLY", None)
                    if v is None:
                        taken = plan[key + "_variant"]
                        continue
                    assert plan[key + "_variant"] == v
                    r = remarks(plan[key + "_code_object"][:-6] + ".hip")
                    print("  %-14s v%d | VGPRs %3d  AGPRs %3d  scratch %4d  VGPRs spilled %3d  waves/SIMD %d  LDS %5d" %
                          (key, v, r["VGPRs"], r["AGPRs"], r["ScratchSize"], r["VGPRs Spill"], r["Occupancy"], r["LDS Size"]))
                print("  %-14s contest: v%d" % (key, taken))


if __name__ == "__main__":
    if len(sys.argv) > 2:
        one_product(sys.argv[1], sys.argv[2:])
    else:
        main()
