"""Max-marginals and the runner-up on the device: famseq_maxmarg_batch / famseq_maxmarg_prior_batch and their device entries
through the Python binding over the C ABI.  References and what a comparison asks: tests/_maxmarg.py (the 3^N enumeration up to
twelve members, the bucket elimination in the max semiring beyond; exact zeros by support, 1e-9 relative above 1e-280).  Bits
wherever two routes must agree: top[0] against famseq_map_batch's map_post, batch sizes and chunks, packed against fp64 input,
host against device entries, a stream of the caller's, NULL outputs, the site-prior form on the model's rows, the four variants.
"""
import numpy as np
import pytest

import _maxmarg as M
import _prior as P
import _side_variants as SV
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets
from famseq_amd.synth import random_likelihoods
from test_gpu_map import loop_pedigree, same_bits, small_cases
from test_map_host import clear_likelihoods

pytestmark = pytest.mark.gpu

RTOL = M.RTOL


@pytest.fixture(autouse=True)
def _ordinary_cache(monkeypatch):
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN"):
        monkeypatch.delenv(key, raising=False)
    yield


def test_the_prebuilt_names_are_the_tests_pedigrees():
    """loop0 / loop1 of test_gpu_map.py are the random pedigrees famseq_amd/prebuild_sets.py names for build()."""
    for k, name in ((0, "random0"), (1, "random6")):
        a, b = loop_pedigree(k)[1], sets.side_variant_pedigree(name)
        assert name in sets.MAXMARG_PEDIGREES and (a.ids, a.mids, a.fids, a.genders, a.names) == (b.ids, b.mids, b.fids, b.genders, b.names)


def mixed_batch(ped, seed, n=192):
    """Half adversarial (integer PLs, hard zeros, sharp sites, unsequenced members, failures), half clear; flags 0..3 in both."""
    rng = np.random.RandomState(seed)
    a, fa = random_likelihoods(rng, ped, n // 2)
    b, fb = clear_likelihoods(rng, ped, n - n // 2)
    return np.concatenate([a, b]), np.concatenate([fa, fb])


@pytest.mark.parametrize("mrate", [1e-7, 0.0])
@pytest.mark.parametrize("case", ["trio", "quad", "ped5", "ped10", "loop0", "loop1"])
def test_against_the_enumeration(case, mrate):
    ped = dict(small_cases())[case]
    ped.relations()
    lk, flags = mixed_batch(ped, 31)
    ref = M.brute(ped, mrate, lk, flags)
    ctx = fs.Context(fs.make_model(ped, mrate=mrate))
    out = ctx.maxmarg_batch(lk=lk, flags=flags)
    _, post, mst = ctx.map_batch(lk=lk, flags=flags)
    ctx.close()
    compared = M.check(out, ref, "%s mrate %g" % (case, mrate))
    ok = out[2] == 0
    assert ok.sum() > 0.5 * len(lk) and compared > 0.5 * (3 * ped.n + 2) * ok.sum()
    assert np.array_equal(out[2], mst) and np.array_equal(out[1][:, 0].view(np.uint64), post.view(np.uint64))
    np.testing.assert_allclose(out[0][ok].max(axis=2), np.broadcast_to(out[1][ok][:, :1], (ok.sum(), ped.n)), rtol=RTOL, atol=0)
    if mrate == 0.0:
        assert (ref.maxmarg[ok] == 0).any()
    jgt, jgq = fs.joint_call_quality(out[0])
    assert np.all(jgt[~ok] == -1) and np.all(np.isnan(jgq[~ok])) and np.all(jgq[ok] >= 0)


@pytest.mark.parametrize("name", ["ped15", "wide24", "wide64"])
def test_against_the_helper(name):
    """Sites whose total lies below 1e-280: status only (test_gpu_map.check_against_helper's rule)."""
    ped = sets.side_variant_pedigree(name)
    lk, flags = random_likelihoods(np.random.RandomState(ped.n), ped, 256, max_pl=40)
    ref = M.elimination(ped, 1e-7, lk, flags)
    ctx = fs.Context(fs.make_model(ped))
    out = ctx.maxmarg_batch(lk=lk, flags=flags)
    _, post, mst = ctx.map_batch(lk=lk, flags=flags)
    ctx.close()
    st = out[2]
    tiny = (ref.status != 1) & ~(ref.z >= M.TINY)
    differ = (st == 0) != (ref.status == 0)
    assert np.all(tiny[differ]) and np.array_equal(st == 1, ref.status == 1)
    ok = (st == 0) & (ref.status == 0) & ~tiny
    assert ok.sum() > 20
    compared = M.check(out, ref._replace(status=np.where(tiny, st, ref.status).astype(np.uint8)), name, sites=ok)
    print("%s: %d sites compared, %d tiny, %d entries at RTOL" % (name, ok.sum(), tiny.sum(), compared))
    assert compared > 0.5 * (3 * ped.n + 2) * ok.sum()
    assert np.array_equal(st, mst) and np.array_equal(out[1][:, 0].view(np.uint64), post.view(np.uint64))


@pytest.mark.parametrize("name", ["edge40", "loop20"])
def test_identities_on_the_edge_pedigrees(name):
    """The 40-member recipe (the lean form, several components) and a looped one of twenty members, three conditioned: what the
    header promises of the entry against its siblings, no reference of the tests' own."""
    mrate = sets.EDGE_PEDIGREES[name][5]
    ped = sets.edge_pedigree(name)
    n = 64
    lk, _ = clear_likelihoods(np.random.RandomState(700 + ped.n), ped, n)
    lk[:, np.asarray(ped.sequenced) == 0, :] = 1.0
    flags = (np.arange(n) % 4).astype(np.uint8)
    ctx = fs.Context(fs.make_model(ped, mrate=mrate, lc=2.0), engine=fs.ENGINE_ELIM)  # (lc > 1: no site takes the -LRC shortcut)
    assert (ctx.plan()["elim_conditioned_members"] > 0) == (name == "loop20")
    mm, top, st = ctx.maxmarg_batch(lk=lk, flags=flags)
    _, post, mst = ctx.map_batch(lk=lk, flags=flags)
    marg, _, bst = ctx.bn_batch(lk, flags)
    ll, _, est = ctx.evidence_batch(lk=lk, flags=flags)
    assert np.all(st == 0) and np.all(mst == 0) and np.all(bst == 0) and np.all(est == 0)
    assert np.array_equal(top[:, 0].view(np.uint64), post.view(np.uint64))
    np.testing.assert_allclose(mm.max(axis=2), np.broadcast_to(top[:, :1], (n, ped.n)), rtol=RTOL, atol=0)
    assert np.all(mm <= (1 + RTOL) * marg)
    assert np.all(top[:, 1] <= top[:, 0] * (1 + RTOL)) and np.all(top[:, 1] > 0)
    # the clamp identity: maxmarg[p][a] * Z is the maximum weight on the rows with member p's row zeroed except entry a
    compared = zeros = 0
    for p in np.linspace(0, ped.n - 1, 8).astype(int):
        for a in range(3):
            rows = lk.copy()
            rows[:, p, [g for g in range(3) if g != a]] = 0.0
            _, cpost, cst = ctx.map_batch(lk=rows, flags=flags)
            cll, _, cest = ctx.evidence_batch(lk=rows, flags=flags)
            good = (cst == 0) & (cest == 0)
            assert np.array_equal(cst == 0, cest == 0)
            np.testing.assert_allclose(mm[good, p, a], cpost[good] * 10.0 ** (cll[good] - ll[good]), rtol=RTOL, atol=0)
            assert np.all(mm[~good, p, a] == 0.0)
            compared, zeros = compared + int(good.sum()), zeros + int((~good).sum())
    ctx.close()
    print("%s: clamp identity on %d entries, %d exact zeros" % (name, compared, zeros))
    assert compared > 0.5 * 24 * n


def test_batch_sizes_and_chunks():
    """Every site's result is its own: batches of 1, 63, 64, 65 and 1,000, and one that spans several chunks of the host entry
    and several loop trips of every workgroup, give the bits of the whole batch.  Flags cycle 0..3 inside every wave."""
    import torch

    ped = fs.synthetic_pedigree("ped10")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * 4 * n_cu * 4 + 37  # at one to four 64-lane workgroups per CU: at least three trips each, and a ragged tail
    rng = np.random.RandomState(8)
    base_lk, _ = random_likelihoods(rng, ped, 4096)
    lk = base_lk[rng.randint(0, 4096, n)]
    flags = (np.arange(n) % 4).astype(np.uint8)
    ctx = fs.Context(fs.make_model(ped, mrate=1e-4))
    whole = ctx.maxmarg_batch(lk=lk, flags=flags)  # the default chunking: several chunks at this size
    for k in (1, 63, 64, 65, 1000):
        assert same_bits(ctx.maxmarg_batch(lk=lk[:k], flags=flags[:k]), [x[:k] for x in whole])
    ctx.set_option("chunk_sites", n)  # one launch for the whole batch: n / (64 * resident workgroups) >= 3 trips per workgroup
    assert same_bits(ctx.maxmarg_batch(lk=lk, flags=flags), whole)
    ctx.set_option("chunk_sites", 128)
    assert same_bits(ctx.maxmarg_batch(lk=lk[:1000], flags=flags[:1000]), [x[:1000] for x in whole])
    ctx.close()
    M.check([x[:96] for x in whole], M.brute(ped, 1e-4, lk[:96], flags[:96]), "the first 96 sites")


def test_routes_that_must_give_the_same_bits():
    """ped10, 1000 sites: packed against fp64 input, host against device entries, the device entry on a stream of the caller's,
    outputs individually NULL, the site-prior form on the model's rows against the plain form."""
    import torch

    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    n = 1000
    pl = rng.randint(0, 300, size=(n, len(seq), 3)).astype(np.uint16)
    pl[rng.rand(n, len(seq)) < 0.05] = fs.PL_MISSING
    flags = rng.randint(0, 4, n).astype(np.uint8)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    lk[7, seq[0]] = 0.0  # a failed site among them, on the fp64 route and the packed one's stand-in alike
    model = fs.make_model(ped, mrate=1e-4)
    ctx = fs.Context(model)
    want = ctx.maxmarg_batch(lk=lk, flags=flags)
    assert want[2][7] == 1 and (want[2] == 0).sum() > 900
    good = np.arange(n) != 7
    packed = ctx.maxmarg_batch(pl16=pl, seq_members=seq, flags=flags)
    assert same_bits([x[good] for x in packed], [x[good] for x in want])
    # outputs individually NULL on the host entries
    a = ctx.maxmarg_batch(lk=lk, flags=flags, want_top=False)
    b = ctx.maxmarg_batch(lk=lk, flags=flags, want_maxmarg=False)
    assert a[1] is None and b[0] is None and same_bits((a[0], a[2], b[1], b[2]), (want[0], want[2], want[1], want[2]))
    # the site-prior form on the model's rows
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.maxmarg_prior_batch(rows, lk=lk, flags=flags), want)
    # the device entries: the default stream and one of the caller's, every combination of outputs
    dev = torch.device("cuda")
    t_lk, t_fl, t_rows = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev), torch.from_numpy(rows).to(dev)
    t_pl = torch.from_numpy(pl.view(np.int16)).to(dev)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, side):
        for wanted in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]:
            for prior in (False, True):
                t_m = torch.full((n, ped.n, 3), -5.0, dtype=torch.float64, device=dev)
                t_t = torch.full((n, 2), -5.0, dtype=torch.float64, device=dev)
                t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                kw = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_maxmarg=t_m.data_ptr() if wanted[0] else 0,
                          d_top=t_t.data_ptr() if wanted[1] else 0, d_status=t_s.data_ptr() if wanted[2] else 0,
                          stream=stream.cuda_stream if stream is not None else 0)
                if prior:
                    ctx.maxmarg_prior_device(n, t_rows.data_ptr(), **kw)
                else:
                    ctx.maxmarg_device(n, **kw)
                (stream or torch.cuda.current_stream()).synchronize()
                got = (t_m.cpu().numpy(), t_t.cpu().numpy(), t_s.cpu().numpy())
                untouched = (np.full((n, ped.n, 3), -5.0), np.full((n, 2), -5.0), np.full(n, 55, np.uint8))
                for k in range(3):
                    assert same_bits([got[k]], [want[k] if wanted[k] else untouched[k]]), (stream is not None, wanted, prior, k)
    # ... and packed input on the device entry
    t_m = torch.full((n, ped.n, 3), -5.0, dtype=torch.float64, device=dev)
    t_t = torch.full((n, 2), -5.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.maxmarg_device(n, d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(), d_maxmarg=t_m.data_ptr(),
                             d_top=t_t.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    assert same_bits((t_m.cpu().numpy(), t_t.cpu().numpy(), t_s.cpu().numpy()), packed)
    plan = ctx.plan()
    ctx.close()
    assert plan["maxmarg_code_object"].endswith(".hsaco") and 0 <= plan["maxmarg_variant"] < 4
    assert plan["maxmarg_prior_code_object"].endswith(".hsaco") and plan["maxmarg_prior_variant"] == plan["maxmarg_variant"]


@pytest.mark.parametrize("name", ["trio", "ped10", "random6"])
def test_site_prior_form_on_hardy_weinberg_rows(name):
    ped = sets.side_variant_pedigree(name)
    lk, flags = mixed_batch(ped, 17)
    hwe = fs.hwe_priors(np.random.RandomState(7 + ped.n).uniform(0.01, 0.5, len(lk)))
    for mrate in (1e-7, 0.0):
        ref = M.elimination(ped, mrate, lk, flags, hwe)
        ctx = fs.Context(fs.make_model(ped, mrate=mrate))
        out = ctx.maxmarg_prior_batch(hwe, lk=lk, flags=flags)
        _, post, mst = ctx.map_prior_batch(hwe, lk=lk, flags=flags)
        plain = ctx.maxmarg_batch(lk=lk, flags=flags)
        ctx.close()
        compared = M.check(out, ref, "%s mrate %g, Hardy-Weinberg rows" % (name, mrate))
        assert compared > 0.5 * (3 * ped.n + 2) * (out[2] == 0).sum() > 0
        assert np.array_equal(out[2], mst) and np.array_equal(out[1][:, 0].view(np.uint64), post.view(np.uint64))
        assert not same_bits(out[:2], plain[:2])


@pytest.mark.parametrize("name", sets.SIDE_VARIANT_PEDIGREES)
def test_every_variant_gives_the_same_bits(name, monkeypatch):
    """Each fence level forced through $FAMSEQ_VARIANT_ONLY (build() has compiled all four, plain and site-prior), the plan
    checked to name it: the reference, the bits of the contest's variant, the site-prior form on the model's rows."""
    mrate = SV.PEDIGREES[name][0]
    ped = sets.side_variant_pedigree(name)
    lk, flags = mixed_batch(ped, 23, n=197)
    model = fs.make_model(ped, mrate=mrate)
    rows = P.model_rows(model, flags)
    hwe = fs.hwe_priors(np.random.RandomState(5).uniform(0.01, 0.5, len(lk)))
    ctx = fs.Context(model)
    want = ctx.maxmarg_batch(lk=lk, flags=flags)
    hwant = ctx.maxmarg_prior_batch(hwe, lk=lk, flags=flags)
    ctx.close()
    M.check(want, M.brute(ped, mrate, lk, flags), name)
    for v in range(sets.SIDE_VARIANTS):
        ctx = fs.Context(model, device=0)
        try:
            SV.forced(ctx, "maxmarg", 1, v, monkeypatch)
            SV.forced(ctx, "maxmarg_prior", 1, v, monkeypatch)
            ctx.set_option("grid_blocks", 1)
            assert same_bits(ctx.maxmarg_batch(lk=lk, flags=flags), want), (name, v)
            assert same_bits(ctx.maxmarg_prior_batch(rows, lk=lk, flags=flags), want), (name, v, "the model's rows")
            assert same_bits(ctx.maxmarg_prior_batch(hwe, lk=lk, flags=flags), hwant), (name, v, "Hardy-Weinberg rows")
            for k in (1, 63, 65):
                assert same_bits(ctx.maxmarg_batch(lk=lk[:k], flags=flags[:k]), [x[:k] for x in want])
        finally:
            ctx.close()
