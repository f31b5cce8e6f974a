"""Every variant of every generated kernel family, forced one at a time and run on the device.

Which variant a pedigree gets is decided by the static picker, the tuner and the compiler's register allocation
(csrc/jit.cpp jit_pick_variant); the rest of the GPU suite only runs the ones its pedigrees land on.  Here each index is
forced — the plain kernels through their pick notes (pick_lane / pick_elim), the call-path forms through
$FAMSEQ_VARIANT_ONLY — the plan is checked to name it, and its outputs go against the reference and against the other
variants of the same family, which must agree bit for bit (see tests/test_generated_host.py, the host twin, for why).
The site-prior kernel famseq_elim_prior has no contest of its own — it runs in the variant famseq_elim takes — and is moved
with it through pick_elim, all twelve.  (The side products' fence levels: tests/test_gpu_side_variants.py.)
The lane kernel's twelve variants are three forms of four (per-prefix text, once per site, outer-leaf plan); the later two are
texts of their own on some pedigrees only, so the lane family also runs on V.LANE_PEDIGREES (famseq_amd/prebuild_sets.py
LANE_FORM_PEDIGREES), a form to a test, and a variant whose code object has a lower variant's name is checked by that name.

Pick notes are written into a private kernel cache of this session: the in-tree cache and the per-user one, from which the
rest of the suite and bench.py load, never see them."""
import numpy as np
import pytest

import _prior as P
import _variants as V
import famseq_amd as fs

pytestmark = pytest.mark.gpu

VARIANTS = dict(lane=V.LANE_VARIANTS, elim=12, lane_call=4, elim_call=8)
ORACLE_SITES = 128  # distinct sites of the grown pedigrees (eleven and thirteen members: 3^11 and 3^13 configurations per site in the oracle)
# One launch per call (chunk_sites: the host would otherwise split a call into launches of 256 sites) on a grid of 2
# workgroups: at 1600 sites every workgroup wraps its persistent loop at least three times, for every workgroup size the
# generated kernels use (BT <= 256), so what carries from one iteration to the next (LDS reuse after the stage-out, the
# loop-top barrier, the prefetch of the next chunk) runs.
N_SITES = 1600
GRID = 2
WIDE = {24: range(12), 40: range(12), 64: range(8, 12)}


@pytest.fixture(scope="session")
def private_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("variant_kernels"))


@pytest.fixture(autouse=True)
def _private_cache(private_cache, monkeypatch):
    monkeypatch.setenv("FAMSEQ_KERNEL_CACHE", private_cache)
    monkeypatch.setenv("FAMSEQ_KEEP_SRC", "1")  # (to read each kernel's workgroup size: the chunk of sites)
    monkeypatch.delenv("FAMSEQ_VARIANT_ONLY", raising=False)
    monkeypatch.delenv("FAMSEQ_VARIANT_MIN", raising=False)
    yield


_REF = {}


def batch(name):
    if name not in _REF:
        ped = V.pedigree(name)
        if name.startswith("grown"):
            # the oracle answers ORACLE_SITES distinct sites (every planted one among them) and the batch repeats them by index:
            # every output row is compared with the oracle's row for its site (waves 64..127 of each repeat stay uniform in chrX)
            lk, flags, has_bn_fail = V.variant_batch(ped, ORACLE_SITES, seed=len(name))
            idx = np.arange(N_SITES) % ORACLE_SITES
            ref = tuple(np.ascontiguousarray(x[idx]) for x in V.reference(ped, lk, flags))
            _REF[name] = (ped, np.ascontiguousarray(lk[idx]), np.ascontiguousarray(flags[idx]), has_bn_fail, ref)
        else:
            lk, flags, has_bn_fail = V.variant_batch(ped, N_SITES, seed=len(name))
            _REF[name] = (ped, lk, flags, has_bn_fail, V.reference(ped, lk, flags))
    return _REF[name]


def block_threads(code_object):
    src = open(code_object[:-6] + ".hip").read()
    return int(src.split("#define BT ")[1].split()[0])


def load(ped, family, v, base=0, monkeypatch=None):
    """A device context running variant v of `family` (grid_blocks 3), the plan checked to name it."""
    model = fs.make_model(ped, mrate=V.MRATE)
    ctx = fs.Context(model, device=0)
    one_launch(ctx)
    seq = np.nonzero(ped.sequenced)[0][::-1].astype(np.int32).copy()
    try:
        if family == "lane":
            ctx.set_option("pick_lane", v)
            ctx.set_option("enum_impl", 1)
            ctx.set_option("group_digits", 0)
            plan = ctx.plan()
            assert plan["enum_lane_variant"] == v
            obj = plan["enum_lane_code_object"]
        elif family == "elim":
            ctx.set_option("pick_elim", v)
            ctx.set_option("engine", fs.ENGINE_ELIM)
            plan = ctx.plan()
            assert plan["elim_variant"] == v
            obj = plan["elim_code_object"]
        elif family == "prior":  # famseq_elim_prior has no contest of its own: it runs in the variant famseq_elim takes
            ctx.set_option("pick_elim", v)
            ctx.set_option("engine", fs.ENGINE_ELIM)
            ctx.set_option("prior_kernels", 1)
            plan = ctx.plan()
            assert plan["elim_variant"] == v and plan["prior_variant"] == v
            obj = plan["prior_code_object"]
            assert obj.endswith(".hsaco") and obj != plan["elim_code_object"]
        elif family == "lane_call":
            ctx.set_option("pick_lane", base)
            ctx.set_option("enum_impl", 1)
            ctx.set_option("group_digits", 0)
            monkeypatch.setenv("FAMSEQ_VARIANT_ONLY", str(v))
            ctx.set_option("call_kernels", 2)
            monkeypatch.delenv("FAMSEQ_VARIANT_ONLY")
            plan = ctx.plan()
            assert plan["enum_lane_variant"] == base and plan["enum_lane_call_variant"] == v
            obj = plan["enum_lane_call_code_object"]
        else:
            monkeypatch.setenv("FAMSEQ_VARIANT_ONLY", str(v))
            ctx.set_option("engine", fs.ENGINE_ELIM)
            ctx.set_option("call_kernels", 2)
            monkeypatch.delenv("FAMSEQ_VARIANT_ONLY")
            plan = ctx.plan()
            assert plan["elim_call_variant"] == v
            obj = plan["elim_call_code_object"]
    except BaseException:
        ctx.close()
        raise
    print("loaded and confirmed by the plan: members %d, %s, base %d, variant %d" % (ped.n, family, base, v))
    return ctx, seq, block_threads(obj)


def one_launch(ctx):
    ctx.set_option("grid_blocks", GRID)
    ctx.set_option("chunk_sites", N_SITES)


def wraps(n_sites, sites_per_chunk):
    """Does every workgroup of a launch of n_sites run its persistent loop at least three times?"""
    return -(-n_sites // sites_per_chunk) >= 3 * GRID


def run(ctx, family, seq, lk, flags):
    if family.endswith("_call"):
        return ctx.bn_call_batch(seq, lk=lk, flags=flags)
    return ctx.bn_batch(lk, flags)


def sizes(bt):
    return sorted({1, bt - 1, bt + 1})


def lane_bases(ped, monkeypatch):
    model = fs.make_model(ped, mrate=V.MRATE)
    ctx = fs.Context(model, device=-1)
    shapes = []
    for b in (0, 2):
        ctx.set_option("pick_lane", b)
        ctx.set_option("enum_impl", 1)
        shapes.append(ctx.plan()["enum_lane_shape"])
    ctx.close()
    return [0] if shapes[0] == shapes[1] else [0, 2]


def plain_runs(name, family, variants, monkeypatch, also=None):
    ped, lk, flags, has_bn_fail, ref = batch(name)
    runs = {}
    for v in variants:
        ctx, seq, bt = load(ped, family, v, monkeypatch=monkeypatch)
        try:
            assert wraps(len(flags), bt), (name, family, v, bt)
            runs[v] = run(ctx, family, seq, lk, flags)
            V.check_against_reference(*runs[v], ref, has_bn_fail, what="%s: %s variant %d" % (name, family, v))
            for s in sizes(bt):  # the same context again, ragged around its chunk of sites (one launch each)
                out = run(ctx, family, seq, lk[:s], flags[:s])
                assert V.same_bits(out, tuple(x[:s] for x in runs[v])), (name, family, v, s)
            if also:
                also(ctx, v, runs[v])
        finally:
            ctx.close()
    return runs


# every plain family on V.PEDIGREES; the lane family also on the pedigrees that take its once-per-site form and outer-leaf plan
PLAIN = [(n, f) for n in V.PEDIGREES for f in ("lane", "elim")] + [(n, "lane") for n in V.LANE_PEDIGREES[len(V.PEDIGREES):]]
_LANE_RUNS = {}  # name -> {lane variant: its outputs}: what a later form of the same pedigree is compared with


def lane_plan_checks(name, names, shapes):
    """plain_runs' `also` for a lane variant, on the loaded context: the code object is the text the plan-only context named, the
    plan's description carries the once-per-site and the outer-leaf phrase exactly where that text is the form's own, and one
    call through the resident entry (famseq_bn_batch_device on arrays that live on the device) gives the host entry's bits."""
    import os

    from test_gpu_enum_once import resident

    _, lk, flags, _, _ = batch(name)

    def check(ctx, v, out):
        plan = ctx.plan()
        assert plan["enum_lane_variant"] == v and os.path.basename(plan["enum_lane_code_object"]) == names[v] + ".hsaco", (name, v)
        once, outer = v >= 4 and names[v] != names[v & 3], v >= 8 and names[v] != names[v - 4]
        assert plan["enum_lane_shape"] == shapes[v] and (V.ONCE in shapes[v]) == once and (V.OUTER in shapes[v]) == outer, (name, v, shapes[v])
        assert V.same_bits(resident(ctx, lk, flags), out), "%s: lane variant %d, the resident entry" % (name, v)
        assert ctx.plan()["enum_last_kind"] == "lane" and ctx.plan()["enum_group_digits_last"] == 0, (name, v)

    return check


@pytest.mark.parametrize("name,family", PLAIN)
def test_every_plain_variant(name, family, tmp_path, monkeypatch):
    """(the lane family: its variants 0-3, the per-prefix text; 4-11 in test_the_later_forms_of_the_lane_kernel)"""
    ped = batch(name)[0]
    also = None
    if family == "lane":
        names, shapes = V.lane_texts(ped, tmp_path, monkeypatch)
        also = lane_plan_checks(name, names, shapes)
    runs = plain_runs(name, family, range(4 if family == "lane" else VARIANTS[family]), monkeypatch, also)
    two_blocks = family == "lane" and lane_bases(ped, monkeypatch) == [0, 2]
    for v, out in runs.items():
        b = (v & 2) if two_blocks else 0
        assert V.same_bits(out, runs[b]), "%s: %s variant %d differs from variant %d" % (name, family, v, b)
    if two_blocks:  # the 7- and the 6-member block group the enumeration's sums differently (enum_codegen.cpp)
        a, c = runs[0], runs[2]
        assert np.array_equal(a[2], c[2]) and np.array_equal(a[1].view(np.uint64), c[1].view(np.uint64))
        ok = (a[2] & 3) == 0
        np.testing.assert_allclose(a[0][ok], c[0][ok], rtol=1e-12, atol=0)
    if family == "lane":
        _LANE_RUNS.setdefault(name, {}).update(runs)


@pytest.mark.parametrize("form", [1, 2], ids=["once-per-site", "outer-leaf"])
@pytest.mark.parametrize("name", V.LANE_PEDIGREES)
def test_the_later_forms_of_the_lane_kernel(name, form, tmp_path, monkeypatch):
    """Lane variants 4-7 (the once-per-site form) and 8-11 (the outer-leaf plan), four to a test.  A variant whose code object
    has the name of a lower variant's is that text (the name is a content hash): the equality is asserted and nothing is
    loaded, which is all there is to do on most of V.PEDIGREES; tests/test_lane_form_pedigrees.py pins where the texts differ.
    Every text of its own runs through plain_runs as variants 0-3 do — the oracle, one launch on a grid of 2 that wraps,
    ragged sizes — and lane_plan_checks.  Within the form: a fencing pair the same bits, the two block shapes as variants 0
    and 2 (V.check_lane_relations).  Between forms nothing is asserted; each is held to the oracle, their largest deviation
    is printed.
    A context with $FAMSEQ_KERNEL_CACHE set consults that directory only (csrc/jit.cpp jit_compile), so nothing build()
    could pre-build would be found from the private cache: the up to four kernels of a test are compiled where it runs,
    about a second each."""
    ped = batch(name)[0]
    names, shapes = V.lane_texts(ped, tmp_path, monkeypatch)
    first = V.first_with_text(names)
    if name in V.LANE_FORM_PEDIGREES:
        assert (len(set(names)), V.form_relations(names)) == V.LANE_FORM_PEDIGREES[name], (name, names)
    group = range(4 * form, 4 * form + 4)
    own = [v for v in group if first[v] == v]
    for v in group:
        assert first[v] == v or (first[v] < 4 * form and names[v] == names[v - 4]), (name, v, names)
    if not own:
        return
    have = _LANE_RUNS.setdefault(name, {})
    also = lane_plan_checks(name, names, shapes)
    have.update(plain_runs(name, "lane", own, monkeypatch, also))
    # (a variant of this form that is a lower form's text, and the lower forms for the deviation: from their own tests where
    # those ran in this session, else loaded here — from the private cache of the session where it holds them)
    missing = sorted({first[v] for v in group} | {first[v & 3] for v in group} - set(have))
    have.update(plain_runs(name, "lane", [v for v in missing if v not in have], monkeypatch))
    V.check_lane_relations(name, names, have, shapes[0] != shapes[2], "device", forms=[form])


def phred(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(-10 * np.log10(p))
    return np.where(np.isinf(q), 99999.0, q)


@pytest.mark.parametrize("family", ["lane_call", "elim_call"])
@pytest.mark.parametrize("name", V.PEDIGREES)
def test_every_call_variant(name, family, monkeypatch):
    ped, lk, flags, has_bn_fail, ref = batch(name)
    bases = lane_bases(ped, monkeypatch) if family == "lane_call" else [0]
    pl, lk_pl = V.packed_batch(ped, lk, np.nonzero(ped.sequenced)[0][::-1])
    for b in bases:
        calls, packed = {}, {}
        for v in range(VARIANTS[family]):
            ctx, seq, bt = load(ped, family, v, base=b, monkeypatch=monkeypatch)
            try:
                assert wraps(len(flags), bt), (name, family, b, v, bt)
                calls[v] = run(ctx, family, seq, lk, flags)
                for s in sizes(bt):
                    out = run(ctx, family, seq, lk[:s], flags[:s])
                    assert V.same_bits(out, tuple(x[:s] for x in calls[v])), (name, family, b, v, s)
                # packed integer PLs in (the call forms' own unpacking and staging), against fp64 rows of the table's values
                if family == "lane_call":
                    assert ctx.plan()["enum_lane_call_reads_rows"] == 0  # (else packed input would take the separate stages)
                packed[v] = ctx.bn_call_batch(seq, pl16=pl, flags=flags)
                assert V.same_bits(packed[v], ctx.bn_call_batch(seq, lk=lk_pl, flags=flags)), (name, family, b, v, "packed")
                s = bt + 1
                assert V.same_bits(ctx.bn_call_batch(seq, pl16=pl[:s], flags=flags[:s]), tuple(x[:s] for x in packed[v])), (name, family, b, v, s)
            finally:
                ctx.close()
        for v, out in calls.items():
            assert V.same_bits(out, calls[0]), "%s: %s variant %d (base %d) differs from variant 0" % (name, family, v, b)
            assert V.same_bits(packed[v], packed[0]), "%s: %s variant %d (base %d), packed input, differs from variant 0" % (name, family, v, b)
        assert ((packed[0][3] & 3) == 0).sum() > len(flags) // 2
        # the Phred formula and the genotype call of the plain kernel's posteriors (the lane call form runs its base's block;
        # every variant of one family gives the same bits, so one plain run stands for all)
        gpp, fpp, fgt, st = calls[0]
        plain, pv = ("lane", b) if family == "lane_call" else ("elim", 0)
        post, single, pst = plain_runs(name, plain, [pv], monkeypatch)[pv]
        seq_ = np.nonzero(ped.sequenced)[0][::-1]
        assert np.array_equal(st, pst) and np.array_equal(st, ref[2])
        ok, s_ok = (st & 3) == 0, (st & 3) != 1
        np.testing.assert_allclose(gpp[s_ok], phred(single[s_ok][:, seq_]), rtol=1e-12, atol=0)
        np.testing.assert_allclose(fpp[ok], phred(post[ok][:, seq_]), rtol=1e-12, atol=0)
        assert np.array_equal(fgt[ok], fs.call_genotypes(post[ok][:, seq_]).reshape(-1, len(seq_)))
        assert np.all(np.isnan(fpp[~ok])) and np.all(fgt[~ok] == -1) and np.all(np.isnan(gpp[~s_ok]))


PRIOR_PEDIGREES = ("quad", "cousins", "random15")  # loop-free, one conditioned member, three (and three members without reads)
_PRIOR_REF, _PRIOR_RUNS = {}, {}


def prior_batch(name):
    """The variant batch of the pedigree with Hardy-Weinberg rows of frequencies uniform in (0.01, 0.5), and the per-site oracle
    of tests/_prior.py on them, asserted well-conditioned (on the oracle alone); computed once."""
    if name not in _PRIOR_REF:
        ped, lk, flags, _, _ = batch(name)
        hwe = fs.hwe_priors(np.random.RandomState(len(name)).uniform(0.01, 0.5, len(lk)))
        ref = P.reference(ped, lk, flags, hwe, mrate=V.MRATE)
        P.assert_well_conditioned(ped, lk, flags, hwe, ref, mrate=V.MRATE)
        assert set(np.unique(ref[2])) >= {0, 1, 2, 0x80}
        _PRIOR_REF[name] = (hwe, ref)
    return _PRIOR_REF[name]


@pytest.mark.parametrize("v", range(12))
@pytest.mark.parametrize("name", PRIOR_PEDIGREES)
def test_the_site_prior_kernel_in_every_variant(name, v, monkeypatch):
    """famseq_elim_prior (K_PRIOR) in each of famseq_elim's twelve variants, the registers-first (4-7) and the no-LDS family
    (8-11) included: on the model's own rows famseq_elim's bits in the same variant, on Hardy-Weinberg rows the per-site
    oracle at tests/_prior.py's tolerances, ragged sub-batches the bits of the slices, and every variant variant 0's bits."""
    ped, lk, flags, has_bn_fail, ref = batch(name)
    hwe, href = prior_batch(name)
    ctx, _, bt = load(ped, "prior", v)
    try:
        assert wraps(len(flags), bt), (name, v, bt)
        model = fs.make_model(ped, mrate=V.MRATE)
        plain = ctx.bn_batch(lk, flags)
        V.check_against_reference(*plain, ref, has_bn_fail, what="%s: elim variant %d" % (name, v))
        assert V.same_bits(ctx.bn_prior_batch(lk, P.model_rows(model, flags), flags), plain), (name, v, "the model's rows")
        out = ctx.bn_prior_batch(lk, hwe, flags)
        P.check(out, href, "%s: site-prior kernel, variant %d, Hardy-Weinberg rows" % (name, v))
        for s in sizes(bt):
            assert V.same_bits(ctx.bn_prior_batch(lk[:s], hwe[:s], flags[:s]), tuple(x[:s] for x in out)), (name, v, s)
        plan = ctx.plan()
        assert plan["elim_variant"] == v and plan["prior_variant"] == v
    finally:
        ctx.close()
    first = _PRIOR_RUNS.setdefault(name, (v, out, plain))
    assert V.same_bits(out, first[1]), "%s: site-prior kernel, variant %d differs from variant %d" % (name, v, first[0])
    assert V.same_bits(plain, first[2]), "%s: famseq_elim, variant %d differs from variant %d" % (name, v, first[0])


def lanes_per_site_forms(name, digits=None, pick=None):
    """The lanes-per-site kernels of `digits` (default: every one the pedigree has), each on a context of its own — under the
    lane pick `pick`, if given — against the oracle; small sub-batches the bits of the slices."""
    ped, lk, flags, has_bn_fail, ref = batch(name)
    model = fs.make_model(ped, mrate=V.MRATE)
    ctx = fs.Context(model, device=0)
    dmax = ctx.plan()["enum_group_digits_max"]
    ctx.close()
    assert dmax >= 2
    for d in range(1, dmax + 1) if digits is None else sorted({min(d, dmax) for d in digits}):
        ctx = fs.Context(model, device=0)
        try:
            one_launch(ctx)
            if pick is not None:
                ctx.set_option("pick_lane", pick)
            ctx.set_option("enum_impl", 1)
            ctx.set_option("group_digits", d)
            out = ctx.bn_batch(lk, flags)
            assert ctx.plan()["enum_group_digits_last"] == d
            assert pick is None or ctx.plan()["enum_lane_variant"] == pick
            V.check_against_reference(*out, ref, has_bn_fail, what="%s: lanes-per-site d = %d" % (name, d))
            for s in (1, 2, 3, 65):
                assert V.same_bits(ctx.bn_batch(lk[:s], flags[:s]), tuple(x[:s] for x in out)), (name, d, s)
        finally:
            ctx.close()
        print("loaded and confirmed by the plan: members %d, lanes-per-site d = %d%s" % (ped.n, d, "" if pick is None else ", lane pick %d" % pick))


@pytest.mark.parametrize("name", ["ped10", "ped15:12"])
def test_every_lanes_per_site_form(name, monkeypatch):
    lanes_per_site_forms(name)


@pytest.mark.parametrize("name", ["random1025", "grown11"])
def test_lanes_per_site_forms_beside_an_outer_leaf_pick(name, monkeypatch):
    """The lanes-per-site forms switch the once-per-site form and the outer-leaf plan off (enumgen_variant(v, d > 0)): with
    pick_lane = 8 in the cache, 3 lanes per site and the most lanes per site the pedigree has, against the oracle.  (That
    their code objects are those of pick 2: tests/test_lane_form_pedigrees.py.)"""
    lanes_per_site_forms(name, digits=(1, 99), pick=8)


def test_the_call_path_under_an_outer_leaf_pick(monkeypatch):
    """The call-path form keeps the per-prefix text (enumgen_call_variant): on random1025, whose variant 8 is the outer-leaf plan,
    famseq_bn_call_batch under pick_lane = 8 gives the bits it gives under pick_lane = 0, each on a context of its own."""
    ped, lk, flags, _, ref = batch("random1025")
    outs = {}
    for pick in (0, 8):
        ctx = fs.Context(fs.make_model(ped, mrate=V.MRATE), device=0)
        try:
            one_launch(ctx)
            ctx.set_option("pick_lane", pick)
            ctx.set_option("enum_impl", 1)
            ctx.set_option("group_digits", 0)
            ctx.set_option("call_kernels", 2)
            seq = np.nonzero(ped.sequenced)[0][::-1].astype(np.int32).copy()
            outs[pick] = ctx.bn_call_batch(seq, lk=lk, flags=flags)
            plan = ctx.plan()
            assert plan["enum_lane_variant"] == pick and plan["enum_lane_call_code_object"].endswith(".hsaco")
            assert (V.OUTER in plan["enum_lane_shape"]) == (pick == 8)
            outs[pick, "object"] = plan["enum_lane_call_code_object"]
        finally:
            ctx.close()
    assert outs[0, "object"] == outs[8, "object"]
    assert np.array_equal(outs[0][3], ref[2]) and ((ref[2] & 3) == 0).sum() > len(flags) // 2
    assert V.same_bits(outs[8], outs[0])


@pytest.mark.parametrize("n", sorted(WIDE))
def test_every_variant_on_wide_pedigrees(n, monkeypatch):
    """The sum-product kernel of wide pedigrees (LDS-staged up to 39 members, rows straight from global memory from 40),
    every variant forced, against the numpy sum-product oracle on the sites its double arithmetic is sound on."""
    import oracle.sum_product as sp
    from famseq_amd.prebuild_sets import wide_pedigree

    ped = wide_pedigree(n)
    ped.relations()
    lk, flags, has_bn_fail = V.variant_batch(ped, N_SITES, seed=n, max_pl=40)
    want = sp.pedigree_posterior(ped, lk, flags, mrate=V.MRATE)
    true = sp.pedigree_posterior(ped, lk, flags, mrate=V.MRATE, dtype=np.longdouble)
    sound = (want[2] == true[2]) & np.all(np.isclose(want[0], true[0].astype(np.float64), rtol=1e-10, atol=1e-35, equal_nan=True), axis=(1, 2))
    # (the -LRC vote is a double-precision rule: in long double 1 + 1e-17 is not 1, so shortcut sites never count as sound;
    # the kernel has to reproduce the double oracle's vote and rows there exactly)
    cut = want[2] == 0x80
    assert sound.mean() > 0.8 and cut[V.SHORTCUT] and sound[V.SINGLE_FAIL] and sound[list(V.TINY_SITES)].all()
    runs = {}
    for v in WIDE[n]:
        ctx, seq, bt = load(ped, "elim", v, monkeypatch=monkeypatch)
        try:
            assert wraps(len(flags), bt), (n, v, bt)
            post, single, st = runs[v] = ctx.bn_batch(lk, flags)
            for s in sizes(bt):
                assert V.same_bits(ctx.bn_batch(lk[:s], flags[:s]), tuple(x[:s] for x in runs[v])), (n, v, s)
        finally:
            ctx.close()
        assert np.array_equal(st[sound | cut], want[2][sound | cut]) and st[V.SHORTCUT] == 0x80 and st[V.SINGLE_FAIL] == 1
        assert not has_bn_fail or st[V.BN_FAIL] == 2
        ok, s_ok = sound & ((st & 3) == 0), (want[2] & 3) != 1
        assert np.array_equal(single[s_ok].view(np.uint64), want[1][s_ok].view(np.uint64))
        assert np.array_equal(post[cut].view(np.uint64), want[0][cut].view(np.uint64))
        # (atol as in `sound`: below 1e-35 the double oracle itself is only vouched for to that absolute level — a posterior of
        # 1e-62 comes out of different orders of products a few 1e-3 apart, relatively)
        np.testing.assert_allclose(post[ok], want[0][ok], rtol=1e-9, atol=1e-35)
        assert np.all(np.isnan(post[(st & 3) != 0]))
        assert V.same_bits(runs[v], runs[min(runs)]), "%d members: elim variant %d differs from variant %d" % (n, v, min(runs))


@pytest.mark.parametrize("engine", [fs.ENGINE_ENUM, fs.ENGINE_ELIM])
def test_tune_reloads_every_kernel_it_dropped(engine, tmp_path, monkeypatch):
    """famseq_set_option "tune" on a context that holds a plain kernel AND its call-path form: both are dropped and loaded
    again from the picks.  A posterior batch and a call batch on that context are then bit-identical to a fresh context's
    (which starts from the same picks), the plan names the variants loaded, and the call-path forms are back.
    (ped5: the sum-product kernel's four candidates are all that is compiled.)"""
    monkeypatch.setenv("FAMSEQ_KERNEL_CACHE", str(tmp_path))
    ped = fs.synthetic_pedigree("ped5")
    model = fs.make_model(ped)
    mo, fa = ped.relations()
    lk, flags = fs.synth.gen_batch(mo, fa, 600, 1)
    seq = np.arange(ped.n, dtype=np.int32)

    def results(ctx):
        return tuple(ctx.bn_batch(lk, flags)) + tuple(ctx.bn_call_batch(seq, lk=lk, flags=flags))

    ctx = fs.Context(model, enum_impl=1, engine=engine)
    ctx.set_option("call_kernels", 1)
    results(ctx)  # every kernel of this engine's path is loaded
    ctx.set_option("tune", 1)
    tuned = results(ctx)
    plan = ctx.plan()
    ctx.close()
    assert ("loaded: enumeration v%d" % plan["enum_lane_variant"]) in plan["tune"], plan["tune"]
    assert plan["enum_lane_variant"] >= 0 and plan["enum_lane_code_object"] and plan["enum_lane_call_code_object"]
    assert plan["enum_lane_call_variant"] >= 0 and plan["enum_lane_call_reads_rows"] == 0 and plan["elim_call_code_object"]
    if engine == fs.ENGINE_ELIM:
        assert (" sum-product v%d" % plan["elim_variant"]) in plan["tune"].split("loaded:")[1] and plan["elim_code_object"]
    fresh_ctx = fs.Context(model, enum_impl=1, engine=engine)
    fresh_ctx.set_option("call_kernels", 1)
    fresh = results(fresh_ctx)
    fresh_plan = fresh_ctx.plan()
    fresh_ctx.close()
    for key in ("enum_lane_code_object", "enum_lane_call_code_object", "enum_lane_variant", "enum_lane_call_variant", "elim_call_code_object",
                "elim_call_variant") + (("elim_code_object", "elim_variant") if engine == fs.ENGINE_ELIM else ()):
        assert plan[key] == fresh_plan[key], key
    for got, want in zip(tuned, fresh):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
