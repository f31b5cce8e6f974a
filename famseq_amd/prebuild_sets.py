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
SIDE_VARIANTS = 4               # kTrioVariants .. kWeightVariants (csrc/elim_codegen.h)
# (stem, output forms, has a site-prior sibling): side_table() of csrc/kernels.cpp
SIDE_PRODUCTS = (("trio", 3, True), ("map", 1, True), ("evidence", 1, True), ("loo", 1, True), ("pattern", 1, True),
                 ("sample", 1, True), ("af", 1, False), ("relabel", 1, True))
# ... and the rows side_table() has gained since tests/_side_variants.py's matrix was drawn up (their own GPU tests force their
# levels: tests/test_gpu_mutrate.py, tests/test_gpu_origin.py, tests/test_gpu_weight.py); build() pre-builds the four levels of both
# lists
SIDE_PRODUCTS_SINCE = (("mutrate", 1, True), ("origin", 1, True), ("weight", 1, True))
# ... and since tests/_edge.py's matrix was drawn up over those two (its own GPU tests: tests/test_gpu_maxmarg.py); build()
# pre-builds this list as it does the others
SIDE_PRODUCTS_LATER = (("maxmarg", 1, True),)
# ... and since tests/golden/generated_sources_later.json was written over that one (tests/test_generated_sources_later.py pins the
# list with the manifest: a manifest that exists is a yardstick and is not rewritten): the characteristic-function kernel, whose
# texts tests/golden/generated_sources_newer.json records (tools/source_digests.py --newer) and whose own GPU tests are
# tests/test_gpu_charfn.py; build() pre-builds this list as it does the others
SIDE_PRODUCTS_NEWER = (("charfn", 1, True),)
# The pedigrees tests/test_gpu_maxmarg.py and tests/test_cli_mapq_gpu.py run beside the lists above (side_variant_pedigree's
# names and wide<n>; random0 and random6 are test_gpu_map.py's loop0 and loop1): build() compiles the max-marginal kernel and its
# site-prior sibling for each, so that no test waits for a compiler on the device
MAXMARG_PEDIGREES = ("trio", "quad", "ped5", "ped10", "ped15", "random0", "random6", "wide24", "wide64")
# The pedigrees tests/test_gpu_charfn.py and tests/test_cli_countdist_gpu.py run (side_variant_pedigree's names, an
# EDGE_PEDIGREES name, or fam<k>: tests/golden/testdata/fam<k>.ped): build() compiles the characteristic-function kernel and its
# site-prior sibling for each, and the evidence and pattern kernels the tests compare them with, so that no test waits for a
# compiler on the device.  random0 / random99 have one and two conditioned members, loop20 three; wide24 / wide25 are the two
# sides of the kernel's lean threshold (csrc/elim_codegen.cpp, kCharfnLeanFrom), edge39 / edge40 of every other side product's.
CHARFN_PEDIGREES = ("trio", "quad", "ped10", "cousins", "random15", "random0", "random99", "wide24", "wide25", "edge39", "edge40", "loop20",
                    "fam01")
CHARFN_LEAN_FROM = 25


# The pedigrees on which the lane kernel's variants 4-11 (csrc/enum_codegen.h: 4-7 the once-per-site form, 8-11 the outer-leaf
# plan) are texts of their own, at mutation rate 0: the forced-variant matrices (tests/test_gpu_variants.py and its host twin in
# tests/test_generated_host.py) run them beside their own pedigrees, on most of which 4-11 are the text of 0-3.
# name -> (distinct texts among variants 0-11, which of 4 != 0, 6 != 2, 8 != 4, 10 != 6 hold); tests/test_lane_form_pedigrees.py
# pins both from plan-only contexts, so that a generator change which makes one decline a form is seen.
#   ped10       10 members, 10 sequenced   the benchmark shape
#   random1025   9 /  7                    outer-leaf plan with unsequenced members in and beside the super-leaf
#   random188    7 /  5                    blocks of five unrolled members, two loop digits
#   random3796   9 /  6                    a second nine-member cut
#   soak26      10 /  6                    a marriage loop, the seven-member block; no outer-leaf text
#   soak33       8 /  6                    a six-member block, prefix tables of two members rebuilt per step
#   random1      8 /  5                    the once-per-site form taken for the six-member block only
#   grown11     11 / 10                    the once-per-site form above ten members
#   grown13     13 / 11                    six looped members ahead of a seven-member block
LANE_FORM_PEDIGREES = {
    "ped10": (12, (True, True, True, True)),
    "random1025": (12, (True, True, True, True)),
    "random188": (12, (True, True, True, True)),
    "random3796": (12, (True, True, True, True)),
    "soak26": (8, (True, True, False, False)),
    "soak33": (8, (True, True, False, False)),
    "random1": (6, (False, True, False, False)),
    "grown11": (8, (True, True, False, False)),
    "grown13": (8, (True, True, False, False)),
}
GROWN_SEEDS = {11: 32109, 13: 32319}  # grown<n>: RandomState seeds found by a scan of grown pedigrees of n members that take the form


# The edges of the sum-product generator's decision space that no other device test reaches (tests/test_gpu_edge_pedigrees.py
# runs every side product on all nine and the main engines on the looped five; tests/test_edge_pedigrees.py pins every column
# below, and the forms named here, from plan-only contexts, so that a generator change which moves an edge says which recipe to
# move).  Each is grow_pedigree(RandomState(seed), n, allow_loops) followed by relations().
#   edge37..edge40: loop-free, around two size edges.  Every side source is lean (likelihood rows read from memory where they
#     are used, the emitter's local factors macros over them) from 40 members on; 39 members are the widest register-resident
#     form, 117 doubles of likelihoods per lane, where the variant contest climbs highest.  relabel_source has three forms: up to
#     37 members the lane's rows in LDS (BT = 64: 64 936 of 65 536 bytes at 37), at 38 and 39 the shell reads the site's row
#     from global memory while the emitter is not lean, from 40 on both are lean.
#   loop12..loop20: marriage loops above ten members (1 to 3 conditioned members: 3, 9 or 27 passes over a long message
#     schedule, and the call path's 128-lane workgroups, which start at 11 members).
# name -> (seed, members, loops allowed, sequenced members, conditioned members, the mutation rate its tests make the model with)
EDGE_PEDIGREES = {
    "edge37": (53037, 37, False, 29, 0, 1e-7),
    "edge38": (53038, 38, False, 29, 0, 1e-4),
    "edge39": (53039, 39, False, 26, 0, 1e-7),
    "edge40": (53040, 40, False, 31, 0, 0.0),
    "loop12": (53202, 12, True, 8, 3, 0.0),
    "loop13": (53300, 13, True, 12, 2, 1e-4),
    "loop14": (53403, 14, True, 10, 1, 1e-7),
    "loop16": (53600, 16, True, 10, 3, 0.0),
    "loop20": (54000, 20, True, 18, 3, 1e-7),
}
EDGE_LANE_MAX = 13  # the looped recipes of at most this many members also run the lane enumeration kernel (3^13 per site)


def edge_pedigree(name):
    """A pedigree of EDGE_PEDIGREES."""
    seed, n, loops = EDGE_PEDIGREES[name][:3]
    ped = grow_pedigree(np.random.RandomState(seed), n, allow_loops=loops)
    ped.relations()
    return ped


def charfn_pedigree(name):
    """A pedigree of CHARFN_PEDIGREES."""
    import os

    from .pedigree import read_ped

    if name in EDGE_PEDIGREES:
        return edge_pedigree(name)
    if name.startswith("fam"):
        ped = read_ped(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "testdata", name + ".ped"))
        ped.relations()
        return ped
    return side_variant_pedigree(name)


def lane_form_pedigree(name):
    """A pedigree of LANE_FORM_PEDIGREES (the matrices run every one at mutation rate 0): a side_variant_pedigree name,
    soak<seed> (soak_pedigree's pedigree, not its mutation rate) or grown<n>."""
    if name.startswith("soak"):
        ped = soak_pedigree(int(name[4:]))[1]
    elif name.startswith("grown"):
        n = int(name[5:])
        ped = grow_pedigree(np.random.RandomState(GROWN_SEEDS[n]), n, allow_loops=False)
    else:
        return side_variant_pedigree(name)
    ped.relations()
    return ped


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
    elif name.startswith("wide"):
        ped = wide_pedigree(int(name[4:]))
    else:
        ped = synthetic_pedigree(name)
    ped.relations()
    return ped
