"""Seeded pedigree recipes shared by build() (which pre-compiles their generated kernels into the in-tree cache) and
by the tests that run them on the GPU box — one definition, so the two cannot drift, and build() needs neither pytest
nor the oracle (the recipes only grow pedigrees; nothing here computes a posterior)."""
import numpy as np

from .synth import grow_pedigree

SOAK_SEEDS = range(40)          # tests/test_gpu_soak.py
RANDOM_SEEDS = range(10)        # tests/test_gpu_random_pedigrees.py, tests/test_generated_host.py
WIDE_SIZES = (24, 32, 48)       # tests/golden/wide_peds.npz (oracle/gen_golden_wide.py)
WIDE_RANDOM_SEEDS = range(6)    # tests/test_gpu_wide.py
WIDE_EXTRA_SIZES = (128,)       # beyond what LDS rows could stage: tests/test_wide.py, tests/test_gpu_wide.py (against the numpy oracle)
# tests/test_gpu_side_variants.py, tests/test_side_variants_host.py: the smallest pedigrees that reach each body of the
# sum-product generator — loop-free, one conditioned member with everybody sequenced, three conditioned members with three
# members unsequenced — on which every fence level of every side-product kernel is forced in turn
SIDE_VARIANT_PEDIGREES = ("trio", "cousins", "random15")
SIDE_VARIANTS = 4               # kTrioVariants .. kMutrateVariants (csrc/elim_codegen.h)
# (stem, output forms, has a site-prior sibling): side_table() of csrc/kernels.cpp
SIDE_PRODUCTS = (("trio", 3, True), ("map", 1, True), ("evidence", 1, True), ("loo", 1, True), ("pattern", 1, True),
                 ("sample", 1, True), ("af", 1, False), ("relabel", 1, True))
# ... and the rows side_table() has gained since tests/_side_variants.py's matrix was drawn up (their own GPU tests force their
# levels: tests/test_gpu_mutrate.py); build() pre-builds the four levels of both lists
SIDE_PRODUCTS_SINCE = (("mutrate", 1, True),)


def soak_pedigree(seed, max_n=10):
    """-> (rng positioned after the pedigree draw, pedigree, mutation rate)."""
    rng = np.random.RandomState(9000 + seed)
    n = int(rng.randint(3, max_n + 1))
    ped = grow_pedigree(rng, n, allow_loops=seed % 2 == 0)
    ped.relations()
    return rng, ped, [1e-7, 1e-4, 0.0][seed % 3]


def random_pedigree(seed):
    """-> (rng positioned after the pedigree draw, pedigree): 3-9 members, loops on every third seed."""
    rng = np.random.RandomState(1000 + seed)
    ped = grow_pedigree(rng, int(rng.randint(3, 10)), allow_loops=seed % 3 == 0)
    return rng, ped


def wide_pedigree(n):
    """The fixture pedigree of n > 20 members: loop-free, about a quarter unsequenced (`NA`)."""
    return grow_pedigree(np.random.RandomState(7000 + n), n, allow_loops=False)


def wide_random_pedigree(seed):
    """-> (rng positioned after the pedigree draw, pedigree, mutation rate): 21-60 members, loop-free."""
    rng = np.random.RandomState(4200 + seed)
    ped = grow_pedigree(rng, int(rng.randint(21, 61)), allow_loops=False)
    return rng, ped, [1e-7, 1e-4, 0.0][seed % 3]


def side_variant_pedigree(name):
    """A pedigree of SIDE_VARIANT_PEDIGREES (or any synthetic_pedigree name, or random<seed>): `cousins` is a first-cousin
    marriage, nine members, one loop; random15 is random_pedigree(15), nine members of which three carry no reads."""
    from .pedigree import Pedigree, synthetic_pedigree

    if name == "cousins":
        ids, mids, fids = [1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 0, 2, 2, 0, 0, 5, 4, 8], [0, 0, 1, 1, 0, 0, 3, 6, 7]
        ped = Pedigree(ids, mids, fids, [1, 2, 1, 2, 2, 1, 1, 2, 1], ["s%d" % i for i in ids])
    elif name.startswith("random"):
        ped = random_pedigree(int(name[6:]))[1]
    else:
        ped = synthetic_pedigree(name)
    ped.relations()
    return ped
