"""Per-member genotype weights on the device: famseq_weight_batch / famseq_weight_prior_batch and their device entries through
the Python binding over the C ABI.  References and rules: tests/_weight.py — status exact, wt_loglik -inf exactly where the
reference's Z_m is exactly 0, elsewhere and for loglik an absolute 1e-9, failed sites NaN — and bits where two routes must
agree, above all the roundabout route users had before: famseq_evidence_batch on rows premultiplied in double on the host,
which column m equals bit for bit wherever that call has status 0.  Every batch asserts on the reference alone, before anything
goes to the device, status 0 everywhere except the planted failures and Z and every non-zero Z_m >= 1e-200, so no site is left
out.

Shapes: 5000 sites per pedigree (78 whole 64-lane workgroups and eight lanes of a 79th), the reference computed once; 1, 63, 64
and 65 sites as slices of it; M = 11 (test_weight_host's ten tables and one that gives a member no weight at all), 32, 2 and 1.
Flags 0..3 in turn, so every wave holds all four.  Pedigrees: trio, quad, the ten-member fixture, cousins (one conditioned
member, model rate 0: a planted status-2 site), random15 (three conditioned, three unsequenced members), random99 (two
conditioned), 24 members, 48 members (the lean form).
"""
import numpy as np
import pytest

import _prior as P
import _side_variants as SV
import _weight as W
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets
from test_map_host import clear_likelihoods
from test_pattern_host import allowed, batch_masks, cycled, pedigree, same_bits

pytestmark = pytest.mark.gpu

N_SITES = 5000
SITE_COUNTS = (1, 63, 64, 65, N_SITES)
N_HWE = 197  # the Hardy-Weinberg reference's sites (three whole workgroups and five lanes)
MODEL_RATE = {"trio": 1e-7, "quad": 1e-7, "ped10": 1e-7, "cousins": 0.0, "random15": 1e-4, "random99": 1e-7, "wide24": 1e-7, "wide48": 1e-4}
SINGLE_FAIL, BN_FAIL = 6, 9  # the planted sites
_CASES = {}


@pytest.fixture(autouse=True)
def _ordinary_cache(monkeypatch):
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN"):
        monkeypatch.delenv(key, raising=False)
    yield


class Case:
    pass


def case(name):
    """ped, model, weights[11], lk, flags, planted, the reference and (trio, wide48) the Hardy-Weinberg rows' — computed once."""
    if name not in _CASES:
        c = Case()
        c.name, c.mrate = name, MODEL_RATE[name]
        if name in ("cousins", "random15"):
            c.ped = ped = sets.side_variant_pedigree(name)
        else:
            c.ped = ped = pedigree(name) if name.startswith(("random", "wide")) else fs.synthetic_pedigree(name)
        ped.relations()
        c.model = fs.make_model(ped, mrate=c.mrate)
        dead = np.ones((1, ped.n, 3))
        dead[0, ped.n // 2] = 0.0  # a member without any weight: -inf at every good site
        c.weights = np.concatenate([W.batch_weights(ped), dead])
        rng = np.random.RandomState(500 + ped.n)
        c.lk, _ = clear_likelihoods(rng, ped, N_SITES)
        seq = np.nonzero(ped.sequenced)[0]
        c.lk[:, np.asarray(ped.sequenced) == 0, :] = 1.0
        c.flags = cycled(c.lk)
        c.planted = [SINGLE_FAIL]
        c.lk[SINGLE_FAIL, seq[-1]] = 0.0
        if c.mrate == 0.0:  # tests/_variants.py's construction: mother certain 0/0, child certain 1/1
            mo, _ = ped.relations()
            child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]][0]
            c.lk[BN_FAIL, mo[child]] = [1.0, 0.0, 0.0]
            c.lk[BN_FAIL, child] = [0.0, 0.0, 1.0]
            c.planted.append(BN_FAIL)
        c.ref = W.reference(ped, c.mrate, c.lk, c.flags, c.weights, brute=False)
        W.clear(c.ref, name, c.planted)
        assert c.ref[2][SINGLE_FAIL] == 1 and (c.mrate != 0.0 or c.ref[2][BN_FAIL] == 2)
        good = np.delete(np.arange(N_SITES), c.planted)
        assert np.all(c.ref[1][good, -1] == 0)
        c.hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, N_SITES))
        c.href = None
        if name in ("trio", "wide48"):
            c.href = W.reference(ped, c.mrate, c.lk[:N_HWE], c.flags[:N_HWE], c.weights, c.hwe[:N_HWE], brute=False)
            W.clear(c.href, name + ", Hardy-Weinberg rows", c.planted)
        c.rows = P.model_rows(c.model, c.flags)
        _CASES[name] = c
    return _CASES[name]


def take(out, index):
    return tuple(x[index] for x in out)


def against_evidence(c, ctx, out, weights, prior=None, n=N_SITES):
    """The roundabout route: column m is the loglik of evidence_batch on the rows lk * weights[m] formed in double on the host,
    bit for bit, wherever that call has status 0; where it has not on a good site Z_m is 0 and the column holds -inf.
    -> the entries compared: every one whose Z_m is not 0."""
    compared = 0
    for m, w in enumerate(weights):
        rows = c.lk[:n] * w
        ll, _, st = ctx.evidence_batch(lk=rows, flags=c.flags[:n]) if prior is None else ctx.evidence_prior_batch(prior[:n], lk=rows, flags=c.flags[:n])
        good = (st == 0) & (out[2] == 0)
        assert same_bits([out[0][good, m]], [ll[good]]), (c.name, m)
        assert np.all(np.isneginf(out[0][(st != 0) & (out[2] == 0), m])), (c.name, m)
        compared += int(good.sum())
    return compared


@pytest.mark.parametrize("name", list(MODEL_RATE))
def test_parity_site_counts_and_table_counts(name):
    c = case(name)
    ctx = fs.Context(c.model)
    whole = ctx.weight_batch(c.weights, lk=c.lk, flags=c.flags)
    assert whole[0].shape == (N_SITES, 11) and whole[1].shape == (N_SITES,)
    W.check(whole, c.ref, name)
    assert same_bits(ctx.weight_batch(c.weights, lk=c.lk, flags=c.flags), whole)  # the same batch twice
    assert against_evidence(c, ctx, whole, c.weights) == int((c.ref[1][c.ref[2] == 0] > 0).sum()) >= 8 * (N_SITES - 2)
    ev = ctx.evidence_batch(lk=c.lk, flags=c.flags)
    assert same_bits([whole[1], whole[2]], [ev[0], ev[2]])  # loglik: the evidence entry's bits on the rows as they are
    assert same_bits(ctx.weight_prior_batch(c.rows, c.weights, lk=c.lk, flags=c.flags), whole)  # the model's rows: the plain form's bits
    for n in SITE_COUNTS[:-1]:
        assert same_bits(ctx.weight_batch(c.weights, lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n)))
        assert same_bits(ctx.weight_prior_batch(c.rows[:n], c.weights, lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n)))
    for pick in ([0], [10], [7, 0], [9, 5]):  # M = 1 and 2: a column depends neither on n_weights nor on the other tables
        for n in (65, N_SITES):
            sub = ctx.weight_batch(c.weights[pick], lk=c.lk[:n], flags=c.flags[:n])
            assert same_bits(sub, (whole[0][:n, pick], whole[1][:n], whole[2][:n])), (name, pick, n)
    assert same_bits(ctx.weight_batch(c.weights[3], lk=c.lk, flags=c.flags), (whole[0][:, [3]], whole[1], whole[2]))  # one [N, 3] table
    # 32 tables: ones give loglik's bits, equal tables equal bits, the others the columns they had among eleven
    many = np.concatenate([c.weights, np.ones((1, c.ped.n, 3)), c.weights[[4, 4]], np.tile(c.weights[:9], (2, 1, 1))])
    assert len(many) == fs.MAX_WEIGHTS
    big = ctx.weight_batch(many, lk=c.lk[:197], flags=c.flags[:197])
    assert same_bits([big[0][:, :11], big[1], big[2]], [whole[0][:197], whole[1][:197], whole[2][:197]])
    assert same_bits([big[0][:, 11]], [big[1]]) and same_bits([big[0][:, 12], big[0][:, 13]], [big[0][:, 4], big[0][:, 4]])
    assert same_bits([big[0][:, 14:23], big[0][:, 23:32]], [big[0][:, :9], big[0][:, :9]])
    # 0/1 tables: the pattern entry's posteriors (its own division's rounding apart) and its exact zeros
    masks = batch_masks(np.random.RandomState(7), c.ped)
    wl, ll, st = ctx.weight_batch(allowed(masks), lk=c.lk[:197], flags=c.flags[:197])
    pp, p_ll, p_st = ctx.pattern_batch(masks, lk=c.lk[:197], flags=c.flags[:197])
    ok = st == 0
    assert np.array_equal(st, p_st) and same_bits([ll], [p_ll]) and np.array_equal(np.isneginf(wl[ok]), pp[ok] == 0.0)
    some = ok[:, None] & (pp != 0.0)
    np.testing.assert_allclose((10.0 ** (wl - ll[:, None]))[some], pp[some], rtol=1e-9, atol=0)
    # a split batch against the whole: two calls, and one host call forced into several chunks through both slots
    a, b = ctx.weight_batch(c.weights, lk=c.lk[:70], flags=c.flags[:70]), ctx.weight_batch(c.weights, lk=c.lk[70:], flags=c.flags[70:])
    assert same_bits(tuple(np.concatenate(x) for x in zip(a, b)), whole)
    ctx.set_option("chunk_sites", 1667)
    assert same_bits(ctx.weight_batch(c.weights, lk=c.lk, flags=c.flags), whole)
    assert same_bits(ctx.weight_prior_batch(c.rows, c.weights[[2, 9]], lk=c.lk, flags=c.flags), (whole[0][:, [2, 9]], whole[1], whole[2]))
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 2)  # two workgroups: forty trips of the chunk loop each, the last one partial
    assert same_bits(ctx.weight_batch(c.weights, lk=c.lk, flags=c.flags), whole)
    ctx.set_option("grid_blocks", 0)
    if c.href is not None:
        hout = ctx.weight_prior_batch(c.hwe[:N_HWE], c.weights, lk=c.lk[:N_HWE], flags=c.flags[:N_HWE])
        W.check(hout, c.href, name + ", Hardy-Weinberg rows")
        assert against_evidence(c, ctx, hout, c.weights, c.hwe, N_HWE) == int((c.href[1][c.href[2] == 0] > 0).sum()) >= 8 * (N_HWE - 2)
        assert same_bits(take(ctx.weight_prior_batch(c.hwe, c.weights, lk=c.lk, flags=c.flags), slice(0, N_HWE)), hout)
    plan = ctx.plan()
    assert plan["weight_code_object"].endswith(".hsaco") and 0 <= plan["weight_variant"] < 4
    assert plan["weight_prior_code_object"].endswith(".hsaco") and plan["weight_prior_variant"] == plan["weight_variant"]
    ctx.close()


@pytest.mark.parametrize("name", ["ped10", "random15"])
def test_pl16_and_lk_give_the_same_bits_on_host_and_device_entries(name):
    import torch

    c = case(name)
    ped, n_all = c.ped, 197
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
    flags = c.flags[:n_all]
    weights = c.weights[[0, 3, 10, 7, 9]]
    ref = W.reference(ped, c.mrate, lk, flags, weights, brute=False)
    W.clear(ref, name + ", packed PLs")
    ctx = fs.Context(c.model)
    b = ctx.weight_batch(weights, lk=lk, flags=flags)
    W.check(b, ref, name + ", packed PLs")
    assert same_bits(ctx.weight_batch(weights, pl16=pl, seq_members=seq, flags=flags), b)
    assert same_bits(ctx.weight_prior_batch(c.rows[:n_all], weights, pl16=pl, seq_members=seq, flags=flags), b)
    dev = torch.device("cuda")
    t_pl, t_lk, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    t_pr = torch.from_numpy(c.rows[:n_all]).to(dev)
    for n_weights in (1, 2, 5):
        t_wt = torch.from_numpy(weights[:n_weights]).to(dev)
        for n in (1, 63, 65, n_all):
            for packed in (False, True):
                for prior in (False, True):
                    t_w = torch.full((n, n_weights), -1.0, dtype=torch.float64, device=dev)
                    t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
                    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                    io = dict(d_pl16=t_pl.data_ptr(), seq_members=seq) if packed else dict(d_lk=t_lk.data_ptr())
                    io.update(d_flags=t_fl.data_ptr(), d_wt_loglik=t_w.data_ptr(), d_loglik=t_l.data_ptr(), d_status=t_s.data_ptr())
                    if prior:
                        ctx.weight_prior_device(n, t_pr.data_ptr(), t_wt.data_ptr(), n_weights, **io)
                    else:
                        ctx.weight_device(n, t_wt.data_ptr(), n_weights, **io)
                    torch.cuda.synchronize()
                    got = (t_w.cpu().numpy(), t_l.cpu().numpy(), t_s.cpu().numpy())
                    assert same_bits(got, (b[0][:n, :n_weights], b[1][:n], b[2][:n])), (name, n_weights, n, packed, prior)
    ctx.close()


def test_device_entries_on_a_stream_null_outputs_and_refusals():
    import torch

    c = case("ped10")
    n, m = 197, 11
    lk, flags, hwe = c.lk[:n], c.flags[:n], c.hwe[:n]
    ctx = fs.Context(c.model)
    wl, ll, st = full = ctx.weight_batch(c.weights, lk=lk, flags=flags)
    hfull = ctx.weight_prior_batch(hwe, c.weights, lk=lk, flags=flags)
    assert not same_bits(hfull[:2], full[:2])
    w1, l1, s1 = ctx.weight_batch(c.weights, lk=lk, flags=flags, want_loglik=False)
    w2, l2, s2 = ctx.weight_batch(c.weights, lk=lk, flags=flags, want_wt=False)
    assert l1 is None and w2 is None and same_bits((w1, s1, l2, s2), (wl, st, ll, st))
    w3, l3, s3 = ctx.weight_prior_batch(hwe, c.weights, lk=lk, flags=flags, want_wt=False, want_loglik=False)
    assert w3 is None and l3 is None and np.array_equal(s3, hfull[2])
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
        t_pr, t_wt = torch.from_numpy(hwe).to(dev), torch.from_numpy(c.weights).to(dev)
        for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
            for prior in (False, True):
                t_w = torch.full((n, m), -1.0, dtype=torch.float64, device=dev)
                t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
                t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_wt_loglik=t_w.data_ptr() if want[0] else 0,
                           d_loglik=t_l.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0, stream=stream.cuda_stream)
                if prior:
                    ctx.weight_prior_device(n, t_pr.data_ptr(), t_wt.data_ptr(), m, **out)
                else:
                    ctx.weight_device(n, t_wt.data_ptr(), m, **out)
                stream.synchronize()
                exp = hfull if prior else full
                assert same_bits([t_w.cpu().numpy()], [exp[0]]) if want[0] else bool((t_w == -1.0).all())
                assert same_bits([t_l.cpu().numpy()], [exp[1]]) if want[1] else bool((t_l == -1.0).all())
                assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
    # the refusals, with their messages
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_weights must be 1\.\.32, got 33"):
        ctx.weight_device(n, t_wt.data_ptr(), 33, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_weights must be 1\.\.32, got 0"):
        ctx.weight_prior_device(n, t_pr.data_ptr(), t_wt.data_ptr(), 0, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*d_weights must be given"):
        ctx.weight_device(n, 0, 1, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_weights must be 1\.\.32, got 33"):
        ctx.weight_batch(np.ones((33, c.ped.n, 3)), lk=lk, flags=flags)
    for bad, text in ((-0.5, "-0.5"), (np.nan, "nan"), (np.inf, "inf")):
        t = c.weights[:3].copy()
        t[2, 1, 0] = t[2, 5, 1] = bad
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0 is %s$" % text):
            ctx.weight_batch(t, lk=lk, flags=flags)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*weight table 2, member 1, genotype 0 is %s$" % text):
            ctx.weight_prior_batch(hwe, t, lk=lk, flags=flags)
    rc = fs.lib().famseq_weight_batch(ctx._h, 1, None, None, None, 0, None, None, 1, None, None, None)
    assert rc == -1 and "weights must be given" in fs.lib().famseq_last_error(ctx._h).decode()
    ctx.close()


def test_failures_overflow_and_a_member_without_weight():
    """test_weight_host's planted sites in a batch of more than one workgroup: an all-zero row status 1; 1e160 rows status 2; a
    table that overflows Z_m gives +inf, a member without weight -inf, at every good site."""
    ped = fs.synthetic_pedigree("quad")
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    dead = np.ones((1, ped.n, 3))
    dead[0, 2] = 0.0
    weights = np.concatenate([W.batch_weights(ped), dead, np.full((1, ped.n, 3), 1e100)])
    ref = W.reference(ped, 1e-7, lk, flags, weights[:-1])
    W.clear(ref, "quad", (70,))
    model = fs.make_model(ped, mrate=1e-7)
    ctx = fs.Context(model)
    for out in (ctx.weight_batch(weights, lk=lk, flags=flags), ctx.weight_prior_batch(P.model_rows(model, flags), weights, lk=lk, flags=flags)):
        W.check((out[0][:, :-1], out[1], out[2]), ref, "planted zero and failure")
        good = np.arange(96) != 70
        assert out[2][70] == 1 and np.all(np.isnan(out[0][70])) and np.isnan(out[1][70])
        assert np.all(np.isneginf(out[0][good, -2])) and np.all(out[0][good, -1] == np.inf) and np.all(np.isfinite(out[1][good]))
    big = np.full((70, ped.n, 3), 1e160)
    wl, ll, st = ctx.weight_batch(weights, lk=big, flags=np.zeros(70, np.uint8))
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(wl))
    ctx.close()


@pytest.mark.parametrize("name", sets.SIDE_VARIANT_PEDIGREES)
def test_every_variant_gives_the_same_bits(name, monkeypatch):
    """Each fence level forced through $FAMSEQ_VARIANT_ONLY (build() has compiled all four, plain and site-prior), the plan
    checked to name it: the reference, the bits of the contest's variant, the site-prior form on the model's rows."""
    c = case(name)
    n = 197
    lk, flags, rows, hwe = c.lk[:n], c.flags[:n], c.rows[:n], c.hwe[:n]
    ctx = fs.Context(c.model)
    want = ctx.weight_batch(c.weights, lk=lk, flags=flags)
    hwant = ctx.weight_prior_batch(hwe, c.weights, lk=lk, flags=flags)
    ctx.close()
    W.check(want, take(c.ref, slice(0, n)), name)
    for v in range(sets.SIDE_VARIANTS):
        ctx = fs.Context(c.model, device=0)
        try:
            SV.forced(ctx, "weight", 1, v, monkeypatch)
            SV.forced(ctx, "weight_prior", 1, v, monkeypatch)
            ctx.set_option("grid_blocks", 1)
            assert same_bits(ctx.weight_batch(c.weights, lk=lk, flags=flags), want), (name, v)
            assert same_bits(ctx.weight_prior_batch(rows, c.weights, lk=lk, flags=flags), want), (name, v, "the model's rows")
            assert same_bits(ctx.weight_prior_batch(hwe, c.weights, lk=lk, flags=flags), hwant), (name, v, "Hardy-Weinberg rows")
            for k in (1, 63, 65):
                assert same_bits(ctx.weight_batch(c.weights[:2], lk=lk[:k], flags=flags[:k]), (want[0][:k, :2], want[1][:k], want[2][:k]))
            plan = ctx.plan()
            assert plan["weight_variant"] == v and plan["weight_prior_variant"] == v
        finally:
            ctx.close()


def test_the_enumeration_engine_and_unserved_pedigrees():
    """A context on the enumeration engine answers as the other side products do; four conditioned members are refused."""
    from test_gpu_denovo import four_loops

    c = case("ped10")
    a = fs.Context(c.model, engine=fs.ENGINE_ENUM)
    b = fs.Context(c.model, engine=fs.ENGINE_ELIM)
    assert same_bits(a.weight_batch(c.weights[:3], lk=c.lk[:197], flags=c.flags[:197]), b.weight_batch(c.weights[:3], lk=c.lk[:197], flags=c.flags[:197]))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.weight_batch(np.ones((1, ped.n, 3)), lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.weight_prior_batch(np.ones((4, 6)), np.ones((1, ped.n, 3)), lk=np.ones((4, ped.n, 3)))
    ctx.close()
