"""Pedigrees and batches of the variant matrices (tests/test_gpu_variants.py on the device, its host twin in
tests/test_generated_host.py).  Every generated kernel is emitted in several variants (csrc/enum_codegen.h kEnumVariants,
csrc/elim_codegen.h kElimVariants / kElimCallVariants); which one a pedigree gets depends on the static picker, the tuner
and the compiler's register allocation.  These fixtures let a test force each index in turn and compare."""
import numpy as np

import famseq_amd as fs
from famseq_amd.prebuild_sets import LANE_FORM_PEDIGREES, lane_form_pedigree

# trio .. ped15:12 (both the 7- and the 6-member block of the lane kernel exist from there on), a first-cousin loop
# (one conditioned member) and random_pedigree(15) (nine members, three unsequenced, three conditioned)
PEDIGREES = ("trio", "quad", "ped5", "ped10", "ped15:12", "cousins", "random15")
MRATE = 0.0  # mu = 0: a child that contradicts its parent is impossible, which the BN-failure site needs

# planted sites (indices into every batch; the PL-shaped rows fill the rest)
SHORTCUT, SINGLE_FAIL, BN_FAIL = 3, 5, 7
LRC_SITES = range(10, 26)    # every sequenced member sharp at PL 150..165: the -LRC vote (lc = 1) flips inside this range
TINY_SITES = range(30, 34)   # row sums below 1e-290: the guarded plain-division path of the normalisation


# ... and, for the lane kernel, the pedigrees on which its variants 4-11 are texts of their own (once-per-site form, outer-leaf
# plan): on the seven above, ped10 apart, they are the text of 0-3
LANE_PEDIGREES = PEDIGREES + tuple(n for n in LANE_FORM_PEDIGREES if n not in PEDIGREES)
LANE_VARIANTS = 12           # csrc/enum_codegen.h kEnumVariants
ONCE = "prefix tables and marginals once per site"   # enumgen_describe, variants 4-11 where the once-per-site form is taken
OUTER = "outer-leaf plan"                            # ... and 8-11 where the outer-leaf plan is


def pedigree(name):
    """(one definition with build(), which pre-builds the side products' variants for three of these)"""
    return lane_form_pedigree(name)


def lane_texts(ped, cache, monkeypatch):
    """(names, shapes) of the lane kernel's twelve variants for `ped` at MRATE, from a plan-only context that runs no compiler:
    the code objects' names (content hashes of the generated text, for the workgroup size the environment asks for) and the
    plan's description of each.  `cache` is a directory of its own: the pick notes and resource notes written here must not
    reach a cache that kernels are loaded from."""
    import os

    with monkeypatch.context() as m:
        for k, v in dict(FAMSEQ_KERNEL_CACHE=str(cache), FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_QUIET="1").items():
            m.setenv(k, v)
        m.delenv("FAMSEQ_VARIANT_ONLY", raising=False)
        ctx = fs.Context(fs.make_model(ped, mrate=MRATE), device=-1)
        try:
            names, shapes = [], []
            for v in range(LANE_VARIANTS):
                ctx.set_option("pick_lane", v)
                ctx.set_option("enum_impl", 1)
                plan = ctx.plan()
                assert plan["enum_lane_variant"] == v
                names.append(os.path.basename(plan["enum_lane_code_object"])[:-len(".hsaco")])
                shapes.append(plan["enum_lane_shape"])
        finally:
            ctx.close()
    return names, shapes


def first_with_text(names):
    """variant -> the lowest variant with the same text."""
    return [names.index(n) for n in names]


def form_relations(names):
    """Which of 4 != 0, 6 != 2, 8 != 4, 10 != 6 hold: where the once-per-site form and the outer-leaf plan are texts of their
    own, per block shape."""
    return tuple(names[a] != names[b] for a, b in ((4, 0), (6, 2), (8, 4), (10, 6)))


def largest_deviation(a, b):
    """Largest relative deviation between the posteriors of two runs on the sites both complete (information, never a bar)."""
    ok = ((a[2] & 3) == 0) & ((b[2] & 3) == 0)
    x, y = a[0][ok], b[0][ok]
    nz = y > 0
    return float(np.max(np.abs(x[nz] - y[nz]) / y[nz])) if nz.any() else 0.0


def check_lane_relations(name, names, runs, two_blocks, where, forms=(0, 1, 2)):
    """What the lane kernel's variants owe each other, on `runs` (variant -> (post, single, status)) of the distinct texts:
    a fencing pair (2k, 2k + 1) the same bits in every form and block shape; the two block shapes of one form (4f, 4f + 2)
    status and single posterior bit-identical and posteriors at 1e-12 where the 7- and the 6-member block differ (they group
    the enumeration's sums differently), the same bits where they do not; nothing between forms, each of which is held to the
    oracle — their largest relative deviation is printed."""
    first = first_with_text(names)
    out = lambda v: runs[first[v]]
    for f in forms:
        for v in (4 * f + 1, 4 * f + 3):
            assert same_bits(out(v), out(v - 1)), "%s (%s): lane variant %d differs from variant %d" % (name, where, v, v - 1)
        a, c = out(4 * f), out(4 * f + 2)
        if not two_blocks:
            assert same_bits(a, c), "%s (%s): lane variant %d differs from variant %d" % (name, where, 4 * f + 2, 4 * f)
            continue
        assert np.array_equal(a[2], c[2]) and np.array_equal(a[1].view(np.uint64), c[1].view(np.uint64)), (name, where, f)
        ok = (a[2] & 3) == 0
        np.testing.assert_allclose(a[0][ok], c[0][ok], rtol=1e-12, atol=0, err_msg="%s (%s): form %d" % (name, where, f))
    devs = [largest_deviation(out(v), out(w)) for v, w in ((4, 0), (6, 2), (8, 4), (10, 6), (8, 0), (10, 2))
            if first[v] != first[w] and (v // 4 in forms or w // 4 in forms) and first[v] in runs and first[w] in runs]
    print("%s (%s): largest relative deviation between forms %s %.3e" % (name, where, "+".join(str(f) for f in forms), max(devs) if devs else 0.0))


def variant_flags(n_sites):
    """All four (Known, chrX) combinations inside every wave of 64 lanes, and one wave uniform in chrX (sites 64..127)."""
    flags = (np.arange(n_sites) % 4).astype(np.uint8)
    flags[64:128] = 2 + (np.arange(64) % 2 == 1) * 1
    flags[BN_FAIL] = 0
    return flags


def variant_batch(ped, n_sites, seed=0, max_pl=100):
    """(lk, flags, has_bn_fail): PL-shaped rows (one genotype at PL 0, the others PL 1..max_pl - 1) and the planted sites
    above (the BN failure where a sequenced member has a sequenced mother).  Wide pedigrees want a smaller max_pl (see
    famseq_amd.synth.random_likelihoods)."""
    assert n_sites >= 128  # (variant_flags' uniform wave is sites 64..127)
    rng = np.random.RandomState(seed)
    n = ped.n
    seq = np.nonzero(ped.sequenced)[0]
    pl = rng.randint(1, max_pl, size=(n_sites, n, 3)).astype(float)
    pl[np.arange(n_sites)[:, None], np.arange(n)[None, :], rng.randint(0, 3, size=(n_sites, n))] = 0
    lk = 10.0 ** (-pl / 10.0)
    lk[SHORTCUT] = 1.0
    lk[SHORTCUT, seq] = [1.0, 1e-17, 1e-20]
    lk[SINGLE_FAIL, seq[-1]] = 0.0
    mo, fa = ped.relations()
    child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]]
    c = child[0] if child else None
    if c is not None:  # mother hom-ref, child hom-alt: impossible at mu = 0, autosome or chrX
        lk[BN_FAIL, mo[c]] = [1.0, 0.0, 0.0]
        lk[BN_FAIL, c] = [0.0, 0.0, 1.0]
    for j, s in enumerate(LRC_SITES):
        lk[s] = 1.0
        g = rng.randint(0, 3, size=len(seq))
        row = np.full((len(seq), 3), 10.0 ** (-(150 + j) / 10.0))
        row[np.arange(len(seq)), g] = 1.0
        lk[s, seq] = row
    for s in TINY_SITES:
        lk[s] = 1.0
        lk[s, seq[0]] = [1e-300, 3e-301, 2e-300]
    lk[:, ped.sequenced == 0, :] = 1.0
    return lk, variant_flags(n_sites), c is not None


def packed_batch(ped, lk, seq):
    """(pl16, lk_pl): the rows of `lk` as packed integer PLs in the column order `seq` (PL = round(-10 log10 lk); a hard
    zero 65534, beyond the table; the first site's first column missing: 0xFFFF x 3), and the fp64 rows the library's
    table gives for them (pow(10, -PL / 10) below 4096, 0 from there, 1 for a missing sample or an unsequenced member)."""
    import math

    with np.errstate(divide="ignore"):
        q = np.rint(-10 * np.log10(lk[:, seq, :]))
    pl = np.minimum(np.where(np.isfinite(q), q, 65534), 65534).astype(np.uint16)
    pl[0, 0] = fs.PL_MISSING
    table = np.append([math.pow(10.0, -i / 10.0) for i in range(4096)], 0.0)
    lk_pl = np.ones_like(lk)
    lk_pl[:, seq, :] = table[np.minimum(pl.astype(np.int64), 4096)]
    lk_pl[0, seq[0]] = 1.0
    return pl, lk_pl


def reference(ped, lk, flags):
    import oracle

    return oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=MRATE).bn_batch(lk, flags, threads=8)


def check_against_reference(post, single, status, ref, has_bn_fail=True, rtol=1e-9, what=""):
    """status bit-exact, single posterior bit-exact, BN posterior within rtol, NaN on failed rows, shortcut rows bit-exact."""
    assert np.array_equal(status, ref[2]), what
    assert status[SHORTCUT] == 0x80 and status[SINGLE_FAIL] == 1 and (status[BN_FAIL] == 2 or not has_bn_fail), what
    lrc = status[list(LRC_SITES)]
    assert (lrc == 0x80).any() and (lrc == 0).any(), what  # both sides of the -LRC boundary
    ok, s_ok = (status & 3) == 0, (status & 3) != 1
    assert np.array_equal(single[s_ok].view(np.uint64), ref[1][s_ok].view(np.uint64)), what
    cut = status == 0x80
    assert np.array_equal(post[cut].view(np.uint64), ref[0][cut].view(np.uint64)), what
    np.testing.assert_allclose(post[ok], ref[0][ok], rtol=rtol, atol=0, err_msg=what)
    assert np.all(np.isnan(post[~ok])) and np.all(np.isnan(single[~s_ok])), what


def same_bits(a, b):
    """Outputs of two variants of one kernel: bit-identical (NaN patterns included)."""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))
