"""The characteristic-function entries on the device: famseq_charfn_batch / famseq_charfn_prior_batch and their device entries
through the Python binding over the C ABI, and Context.count_batch on top of them.  Tables, reference and bar
(|cf - reference| <= 1e-12 A, absolute): tests/_charfn.py; every batch asserts on the reference alone, before anything goes to
the device, status 0 everywhere except the planted failures and Z >= 1e-200, so no site is left out.

Shapes: 197 sites per pedigree (three whole 64-lane workgroups and five lanes), the reference computed once; 1, 63, 64 and 65
sites as slices of it; table counts 1, 2, a batch's own and 64.  Flags 0..3 in turn, so every wave holds all four.  Pedigrees:
a trio, random0 / random99 (one and two conditioned members), wide24 / wide25 (the two sides of the kernel's own lean threshold),
edge39 / edge40 (every other side product's), loop20 (three conditioned members, twenty of them), the ten-member fixture, and
the side-variant pedigrees with every fence level forced.  build() has compiled every kernel these tests run
(prebuild_sets.CHARFN_PEDIGREES): each test asserts that the kernel cache holds no code object it did not hold before.
"""
import glob
import os

import numpy as np
import pytest

import _charfn as X
import _prior as P
import _side_variants as SV
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets
from test_map_host import clear_likelihoods
from test_pattern_host import allowed, batch_masks, cycled, same_bits

pytestmark = pytest.mark.gpu

N_SITES = 197
SITE_COUNTS = (1, 63, 64, 65)
MODEL_RATE = {"trio": 1e-7, "random0": 1e-4, "random99": 1e-7, "wide24": 1e-7, "wide25": 1e-4, "edge39": 1e-7, "edge40": 0.0, "loop20": 1e-7,
              "ped10": 1e-7, "cousins": 0.0, "random15": 1e-4}
SINGLE_FAIL, BN_FAIL = 6, 9  # the planted sites
_CASES = {}


@pytest.fixture(autouse=True)
def _nothing_is_compiled_here(monkeypatch):
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN"):
        monkeypatch.delenv(key, raising=False)
    cache = os.path.join(os.path.dirname(os.path.abspath(fs.__file__)), "lib", "kernels", "*.hsaco")
    before = set(glob.glob(cache))
    assert before, "build() leaves the generated kernels' code objects in famseq_amd/lib/kernels"
    yield
    assert set(glob.glob(cache)) <= before, "a kernel was compiled on the device: prebuild_sets.CHARFN_PEDIGREES lacks its pedigree"


class Case:
    pass


def case(name):
    """ped, model, tables, lk, flags, planted, the reference and (trio, wide25) the Hardy-Weinberg rows' — computed once."""
    if name not in _CASES:
        c = Case()
        c.name, c.mrate = name, MODEL_RATE[name]
        c.ped = ped = sets.charfn_pedigree(name)
        assert name in sets.CHARFN_PEDIGREES
        c.model = fs.make_model(ped, mrate=c.mrate)
        rng = np.random.RandomState(900 + ped.n)
        c.lk, _ = clear_likelihoods(rng, ped, N_SITES)
        seq = np.nonzero(ped.sequenced)[0]
        c.lk[:, np.asarray(ped.sequenced) == 0, :] = 1.0
        c.flags = cycled(c.lk)
        c.masks = batch_masks(rng, ped)
        c.tables, c.at = X.batch_tables(ped, c.masks)
        c.planted = [SINGLE_FAIL]
        c.lk[SINGLE_FAIL, seq[-1]] = 0.0
        if c.mrate == 0.0:  # tests/_variants.py's construction: mother certain 0/0, child certain 1/1
            mo, _ = ped.relations()
            child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]][0]
            c.lk[BN_FAIL, mo[child]] = [1.0, 0.0, 0.0]
            c.lk[BN_FAIL, child] = [0.0, 0.0, 1.0]
            c.planted.append(BN_FAIL)
        c.ref = X.reference(ped, c.mrate, c.lk, c.flags, c.tables)
        X.clear(c.ref, name, c.planted)
        assert c.ref[3][SINGLE_FAIL] == 1 and (c.mrate != 0.0 or c.ref[3][BN_FAIL] == 2)
        c.hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, N_SITES))
        c.href = None
        if name in ("trio", "wide25"):
            c.href = X.reference(ped, c.mrate, c.lk, c.flags, c.tables, c.hwe)
            X.clear(c.href, name + ", Hardy-Weinberg rows", c.planted)
        c.rows = P.model_rows(c.model, c.flags)
        _CASES[name] = c
    return _CASES[name]


def same(a, b):
    """(cf, loglik, status) twice: the same bits."""
    if not (np.array_equal(np.isnan(a[0].real), np.isnan(b[0].real)) and same_bits(a[1:], b[1:])):
        return False
    ok = ~np.isnan(a[0].real)  # (a failed site's NaN: any NaN)
    return X.same_cf(a[0][ok], b[0][ok])


def take(out, index):
    return tuple(x[index] for x in out)


@pytest.mark.parametrize("name", ["trio", "random0", "random99", "wide24", "wide25", "edge39", "edge40", "loop20"])
def test_parity_and_the_bit_contracts(name):
    c = case(name)
    lean = c.ped.n >= sets.CHARFN_LEAN_FROM
    ctx = fs.Context(c.model)
    whole = cf, ll, st = ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags)
    assert cf.shape == (N_SITES, len(c.tables)) and cf.dtype == np.complex128 and ll.shape == (N_SITES,)
    X.check(whole, c.ref, "%s (%d members, %s form)" % (name, c.ped.n, "lean" if lean else "register"))
    good = st == 0
    assert same(ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags), whole)  # the same batch twice
    ev = ctx.evidence_batch(lk=c.lk, flags=c.flags)
    assert same_bits([ll, st], [ev[0], ev[2]])  # loglik: the evidence entry's bits
    assert same(ctx.charfn_prior_batch(c.rows, c.tables, lk=c.lk, flags=c.flags), whole)  # the model's rows: the plain form's bits
    assert same(ctx.charfn_batch(X.as_pairs(c.tables), lk=c.lk, flags=c.flags), whole)  # the real [M, N, 3, 2] layout
    for n in SITE_COUNTS:
        assert same(ctx.charfn_batch(c.tables, lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n))), (name, n)
        assert same(ctx.charfn_prior_batch(c.rows[:n], c.tables, lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n))), (name, n)
    last = len(c.tables) - 1
    for pick in ([0], [last], [7, 0], [last - 3, 5]):  # 1 and 2 tables: a column depends neither on n_tables nor on the other tables
        sub = ctx.charfn_batch(c.tables[pick], lk=c.lk, flags=c.flags)
        assert same(sub, (cf[:, pick], ll, st)), (name, pick)
    assert same(ctx.charfn_batch(c.tables[3], lk=c.lk, flags=c.flags), (cf[:, [3]], ll, st))  # one [N, 3] table
    # 64 tables: the batch's own columns as they were, equal tables equal bits
    many = np.concatenate([c.tables, c.tables])[:fs.MAX_CWEIGHTS - 2]
    many = np.concatenate([many, np.tile(c.tables[:1], (fs.MAX_CWEIGHTS - len(many), 1, 1))])
    big = ctx.charfn_batch(many[:, :, :], lk=c.lk, flags=c.flags)
    k = min(len(c.tables), fs.MAX_CWEIGHTS - 2)
    assert len(many) == 64 and same((big[0][:, :k], big[1], big[2]), (cf[:, :k], ll, st))
    assert X.same_cf(big[0][good, 62], big[0][good, 63]) and X.same_cf(big[0][good, 63], cf[good, 0])
    # a table of (1, 0), and frequency 0 of both counts: exactly (1.0, +0.0)
    for col in (c.at["ones"].start, c.at["carriers"].start, c.at["alleles"].start):
        assert np.all(cf[good, col].real == 1.0) and not np.any(np.ascontiguousarray(cf[good, col].imag).view(np.uint64))
    # conjugate tables: the conjugate, exactly (a zero imaginary part compares equal whatever its sign)
    cj = ctx.charfn_batch(np.conj(c.tables), lk=c.lk, flags=c.flags)[0]
    assert same_bits([cj[good].real], [cf[good].real]) and np.array_equal(cj[good].imag, -cf[good].imag)
    # 0/1 tables with +0.0 imaginary parts: the pattern entry's posteriors bit for bit, imaginary parts +0.0
    got = ctx.charfn_batch(allowed(c.masks).astype(np.complex128), lk=c.lk, flags=c.flags)
    pp, p_ll, p_st = ctx.pattern_batch(c.masks, lk=c.lk, flags=c.flags)
    assert np.array_equal(got[2], p_st) and same_bits([got[1]], [p_ll]) and same_bits([got[0][good].real], [pp[good]])
    assert not np.any(np.ascontiguousarray(got[0][good].imag).view(np.uint64))
    # a split batch against the whole: two calls, and one host call forced into several chunks through both slots
    a, b = ctx.charfn_batch(c.tables, lk=c.lk[:70], flags=c.flags[:70]), ctx.charfn_batch(c.tables, lk=c.lk[70:], flags=c.flags[70:])
    assert same(tuple(np.concatenate(x) for x in zip(a, b)), whole)
    ctx.set_option("chunk_sites", 67)
    assert same(ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags), whole)
    assert same(ctx.charfn_prior_batch(c.rows, c.tables[[2, last]], lk=c.lk, flags=c.flags), (cf[:, [2, last]], ll, st))
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 2)  # two workgroups: two trips of the chunk loop each, the last one partial
    assert same(ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags), whole)
    ctx.set_option("grid_blocks", 0)
    if c.href is not None:
        hout = ctx.charfn_prior_batch(c.hwe, c.tables, lk=c.lk, flags=c.flags)
        X.check(hout, c.href, name + ", Hardy-Weinberg rows")
        hev = ctx.evidence_prior_batch(c.hwe, lk=c.lk, flags=c.flags)
        assert same_bits([hout[1], hout[2]], [hev[0], hev[2]]) and not same_bits([hout[1]], [ll])
    plan = ctx.plan()
    assert plan["charfn_code_object"].endswith(".hsaco") and 0 <= plan["charfn_variant"] < X.N_VARIANTS
    assert plan["charfn_prior_code_object"].endswith(".hsaco") and plan["charfn_prior_variant"] == plan["charfn_variant"]
    ctx.close()


def test_pl16_and_lk_give_the_same_bits_on_host_and_device_entries():
    import torch

    c = case("ped10")
    ped, n_all = c.ped, N_SITES
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    pl = rng.randint(0, 61, size=(n_all, len(seq), 3)).astype(np.uint16)
    pl[np.arange(n_all), :, rng.randint(0, 3, n_all)] = 0
    pl[rng.rand(n_all, len(seq)) < 0.05] = fs.PL_MISSING
    lk = np.ones((n_all, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for col, p in enumerate(seq):
        miss = (pl[:, col] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, col], 4095)])
    flags = c.flags
    tables = c.tables[[1, 3, c.at["unit"].start, c.at["inside"].start, c.at["row"].start]]
    ref = X.reference(ped, c.mrate, lk, flags, tables)
    X.clear(ref, "ped10, packed PLs")
    ctx = fs.Context(c.model)
    b = ctx.charfn_batch(tables, lk=lk, flags=flags)
    X.check(b, ref, "ped10, packed PLs")
    assert same(ctx.charfn_batch(tables, pl16=pl, seq_members=seq, flags=flags), b)
    assert same(ctx.charfn_prior_batch(c.rows, tables, pl16=pl, seq_members=seq, flags=flags), b)
    dev = torch.device("cuda")
    t_pl, t_lk, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    t_pr = torch.from_numpy(c.rows).to(dev)
    for n_tables in (1, 2, 5):
        t_cw = torch.from_numpy(X.as_pairs(tables[:n_tables])).to(dev)
        for n in (1, 65, n_all):
            for packed in (False, True):
                for prior in (False, True):
                    t_c = torch.full((n, n_tables, 2), -1.0, dtype=torch.float64, device=dev)
                    t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
                    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                    io = dict(d_pl16=t_pl.data_ptr(), seq_members=seq) if packed else dict(d_lk=t_lk.data_ptr())
                    io.update(d_flags=t_fl.data_ptr(), d_cf=t_c.data_ptr(), d_loglik=t_l.data_ptr(), d_status=t_s.data_ptr())
                    if prior:
                        ctx.charfn_prior_device(n, t_pr.data_ptr(), t_cw.data_ptr(), n_tables, **io)
                    else:
                        ctx.charfn_device(n, t_cw.data_ptr(), n_tables, **io)
                    torch.cuda.synchronize()
                    got = (t_c.cpu().numpy().view(np.complex128)[..., 0], t_l.cpu().numpy(), t_s.cpu().numpy())
                    assert same(got, (b[0][:n, :n_tables], b[1][:n], b[2][:n])), (n_tables, n, packed, prior)
    ctx.close()


def test_device_entries_null_outputs_two_streams_and_refusals():
    import torch

    c = case("ped10")
    n, m = N_SITES, len(c.tables)
    ctx = fs.Context(c.model)
    cf, ll, st = full = ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags)
    X.check(full, c.ref, "ped10")
    hfull = ctx.charfn_prior_batch(c.hwe, c.tables, lk=c.lk, flags=c.flags)
    assert not same_bits([hfull[1]], [ll])
    c1, l1, s1 = ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags, want_loglik=False)
    c2, l2, s2 = ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags, want_cf=False)
    assert l1 is None and c2 is None and same((c1, l2, s1), full) and np.array_equal(s2, st)
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(c.lk).to(dev), torch.from_numpy(c.flags).to(dev)
    t_pr, t_cw = torch.from_numpy(c.hwe).to(dev), torch.from_numpy(X.as_pairs(c.tables)).to(dev)
    torch.cuda.synchronize()
    for want in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)]:
        for prior in (False, True):
            t_c = torch.full((n, m, 2), -1.0, dtype=torch.float64, device=dev)
            t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
            t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
            out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_cf=t_c.data_ptr() if want[0] else 0,
                       d_loglik=t_l.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0)
            if prior:
                ctx.charfn_prior_device(n, t_pr.data_ptr(), t_cw.data_ptr(), m, **out)
            else:
                ctx.charfn_device(n, t_cw.data_ptr(), m, **out)
            torch.cuda.synchronize()
            exp = hfull if prior else full
            got = t_c.cpu().numpy().view(np.complex128)[..., 0]
            ok = exp[2] == 0
            assert (X.same_cf(got[ok], exp[0][ok]) and np.all(np.isnan(got[~ok].real))) if want[0] else bool((t_c == -1.0).all())
            assert same_bits([t_l.cpu().numpy()], [exp[1]]) if want[1] else bool((t_l == -1.0).all())
            assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
    # two calls with d_lk on two streams, in flight together: the bits of the serial calls (with d_lk an entry keeps no state)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k, stream in enumerate(streams):
        t_c = torch.full((n, m, 2), -1.0, dtype=torch.float64, device=dev)
        t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
        outs.append((t_c, t_l, t_s))
    torch.cuda.synchronize()
    ctx.charfn_device(n, t_cw.data_ptr(), m, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_cf=outs[0][0].data_ptr(),
                      d_loglik=outs[0][1].data_ptr(), d_status=outs[0][2].data_ptr(), stream=streams[0].cuda_stream)
    ctx.charfn_prior_device(n, t_pr.data_ptr(), t_cw.data_ptr(), m, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_cf=outs[1][0].data_ptr(),
                            d_loglik=outs[1][1].data_ptr(), d_status=outs[1][2].data_ptr(), stream=streams[1].cuda_stream)
    for stream in streams:
        stream.synchronize()
    for (t_c, t_l, t_s), exp in zip(outs, (full, hfull)):
        assert same((t_c.cpu().numpy().view(np.complex128)[..., 0], t_l.cpu().numpy(), t_s.cpu().numpy()), exp)
    # the refusals, with their messages
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_tables must be 1\.\.64, got 65"):
        ctx.charfn_device(n, t_cw.data_ptr(), 65, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_tables must be 1\.\.64, got 0"):
        ctx.charfn_prior_device(n, t_pr.data_ptr(), t_cw.data_ptr(), 0, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*d_cweights must be given"):
        ctx.charfn_device(n, 0, 1, d_lk=t_lk.data_ptr())
    t = c.tables[:3].copy()
    t[2, 1, 0] = complex(1.0, np.nan)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0, imaginary part is nan$"):
        ctx.charfn_batch(t, lk=c.lk, flags=c.flags)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0, imaginary part is nan$"):
        ctx.charfn_prior_batch(c.hwe, t, lk=c.lk, flags=c.flags)
    ctx.close()


@pytest.mark.parametrize("name", sets.SIDE_VARIANT_PEDIGREES)
def test_every_variant_gives_the_same_bits(name, monkeypatch):
    """Each fence level forced through $FAMSEQ_VARIANT_ONLY (build() has compiled all four, plain and site-prior), the plan
    checked to name it: the reference, the bits of variant 0, the site-prior form on the model's rows."""
    c = case(name)
    X.check(_forced(c, 0, monkeypatch)[0], c.ref, name)
    want, hwant = _forced(c, 0, monkeypatch)
    for v in range(1, sets.SIDE_VARIANTS):
        got, hgot = _forced(c, v, monkeypatch)
        assert same(got, want) and same(hgot, hwant), (name, v)


def _forced(c, v, monkeypatch):
    ctx = fs.Context(c.model, device=0)
    try:
        SV.forced(ctx, "charfn", 1, v, monkeypatch)
        SV.forced(ctx, "charfn_prior", 1, v, monkeypatch)
        out = ctx.charfn_batch(c.tables, lk=c.lk, flags=c.flags)
        assert same(ctx.charfn_prior_batch(c.rows, c.tables, lk=c.lk, flags=c.flags), out), (c.name, v, "the model's rows")
        for k in (1, 65):
            assert same(ctx.charfn_batch(c.tables[:2], lk=c.lk[:k], flags=c.flags[:k]), (out[0][:k, :2], out[1][:k], out[2][:k]))
        plan = ctx.plan()
        assert plan["charfn_variant"] == v and plan["charfn_prior_variant"] == v
        return out, ctx.charfn_prior_batch(c.hwe, c.tables, lk=c.lk, flags=c.flags)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["trio", "ped10"])
def test_count_batch_against_the_enumeration(name):
    """Context.count_batch against the distribution binned directly from the 3^N enumeration, at 1e-12 absolute: carriers,
    alleles and homalt, over all members and over a subset; rows sum to 1; a failed site's row is NaN; the prior form."""
    c = case(name)
    n = 64
    lk, flags = c.lk[:n], c.flags[:n]
    some = [0, c.ped.n - 1] if c.ped.n < 5 else [1, 2, 5, 8]
    ctx = fs.Context(c.model)
    worst = 0.0
    for kind in ("carriers", "alleles", "homalt"):
        for members in (None, some):
            scores = fs.count_scores(c.ped.n, members, kind)
            want, D = X.brute_distribution(c.ped, c.mrate, lk, flags, scores)
            dist, ll, st = ctx.count_batch(scores, lk=lk, flags=flags)
            assert dist.shape == want.shape and np.array_equal(st, c.ref[3][:n]) and np.array_equal(np.isnan(want[:, 0]), st != 0)
            ok = st == 0
            assert np.all(np.isnan(dist[~ok])) and same_bits([ll], [ctx.evidence_batch(lk=lk, flags=flags)[0]])
            worst = max(worst, np.abs(dist[ok] - want[ok]).max(), np.abs(dist[ok].sum(axis=1) - 1.0).max())
            assert np.all(np.abs(dist[ok] - want[ok]) <= X.DIST_ATOL) and np.all(dist[ok] >= 0)
            assert np.all(np.abs(dist[ok].sum(axis=1) - 1.0) <= X.DIST_ATOL)
            assert same_bits(ctx.count_batch(scores, lk=lk, flags=flags, prior=c.rows[:n]), (dist, ll, st))
    print("%s: worst |dist - enumeration| and |sum - 1| %.3g (bar %g)" % (name, worst, X.DIST_ATOL))
    scores = fs.count_scores(c.ped.n)
    dist, ll, st = ctx.count_batch(scores, lk=lk, flags=flags, prior=c.hwe[:n])
    pref = ctx.evidence_prior_batch(c.hwe[:n], lk=lk, flags=flags)[1]
    ok = st == 0
    assert np.all(np.abs(dist[ok].sum(axis=1) - 1.0) <= X.DIST_ATOL) and np.all(np.abs(dist[ok, 0] - pref[ok]) <= X.DIST_ATOL)
    ctx.close()


def test_failures_exact_zeros_the_enumeration_engine_and_unserved_pedigrees():
    """An all-zero row status 1, 1e160 rows status 2, both NaN in every output; a table that gives a member three zeros (0.0, 0.0)
    at every good site; a context on the enumeration engine answers as one on the sum-product engine; four conditioned members
    are refused."""
    from test_gpu_denovo import four_loops

    ped = sets.charfn_pedigree("quad")
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    dead = np.exp(1j * np.ones((1, ped.n, 3)))
    dead[0, 2] = 0.0
    tables = np.concatenate([X.batch_tables(ped, batch_masks(np.random.RandomState(5), ped))[0], dead])
    ref = X.reference(ped, 1e-7, lk, flags, tables)
    X.clear(ref, "quad", (70,))
    model = fs.make_model(ped, mrate=1e-7)
    ctx = fs.Context(model)
    good = np.arange(96) != 70
    for out in (ctx.charfn_batch(tables, lk=lk, flags=flags), ctx.charfn_prior_batch(P.model_rows(model, flags), tables, lk=lk, flags=flags)):
        X.check(out, ref, "planted zero and failure")
        assert out[2][70] == 1 and np.all(np.isnan(out[0][70].real)) and np.all(np.isnan(out[0][70].imag)) and np.isnan(out[1][70])
        assert np.all(out[0][good, -1] == 0) and np.all(np.isfinite(out[1][good]))
    big = np.full((70, ped.n, 3), 1e160)
    cf, ll, st = ctx.charfn_batch(tables, lk=big, flags=np.zeros(70, np.uint8))
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(cf.real)) and np.all(np.isnan(cf.imag))
    ctx.close()
    c = case("ped10")
    a = fs.Context(c.model, engine=fs.ENGINE_ENUM)
    b = fs.Context(c.model, engine=fs.ENGINE_ELIM)
    assert same(a.charfn_batch(c.tables[:3], lk=c.lk, flags=c.flags), b.charfn_batch(c.tables[:3], lk=c.lk, flags=c.flags))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.charfn_batch(np.ones((1, ped.n, 3), np.complex128), lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.charfn_prior_batch(np.ones((4, 6)), np.ones((1, ped.n, 3), np.complex128), lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.count_batch(fs.count_scores(ped.n), lk=np.ones((4, ped.n, 3)))
    ctx.close()
