"""The mutation-rate likelihood profile on the device: famseq_mutrate_batch / famseq_mutrate_prior_batch and their device entries
through the Python binding over the C ABI.  References and rules as in test_mutrate_host.py: status exact, rate_loglik -inf
exactly where the reference's Z_r is exactly 0, elsewhere and for loglik an absolute 1e-9, failed sites NaN, bits where two routes
must agree — above all famseq_evidence_batch of a context made at rates[r], which column r equals bit for bit wherever that call
has status 0.  Every batch asserts on the reference alone, before anything goes to the device, status 0 everywhere except the
planted failures and Z and every non-zero Z_r >= 1e-200, so no site is left out.

Shapes: 197 sites per pedigree (three whole 64-lane workgroups and five lanes of a fourth), the reference computed once; 1, 63
and 65 sites (one lane, one less and one more than the block) as slices of it; R = 32 (FAMSEQ_MAX_RATES), 2 and 1.  Flags 0..3 in
turn, so every wave holds all four.  Pedigrees: trio, cousins (one conditioned member, model rate 0: a planted status-2 site),
random15 (three conditioned, three unsequenced members), the ten-member fixture, 48 members (the lean form).
"""
import numpy as np
import pytest

import _prior as P
import _side_variants as SV
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets
from test_map_host import clear_likelihoods
from test_mutrate_host import check, clear, reference
from test_pattern_host import cycled, same_bits

pytestmark = pytest.mark.gpu

N_SITES = 197
SITE_COUNTS = (1, 63, 65, 197)
MODEL_RATE = {"trio": 1e-7, "cousins": 0.0, "random15": 1e-4, "ped10": 1e-7, "wide48": 1e-4}
SINGLE_FAIL, BN_FAIL = 6, 9  # the planted sites
_CASES = {}


@pytest.fixture(autouse=True)
def _ordinary_cache(monkeypatch):
    for key in ("FAMSEQ_KERNEL_CACHE", "FAMSEQ_VARIANT_ONLY", "FAMSEQ_VARIANT_MIN"):
        monkeypatch.delenv(key, raising=False)
    yield


def rate_grid(mrate):
    """32 rates: the named ones, the model's own, one of them twice more, the rest log-uniform in [1e-10, 1]."""
    rng = np.random.RandomState(32)
    named = [0.0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 0.5, 1.0, mrate, 1e-3]
    return np.concatenate([named, 10.0 ** rng.uniform(-10, 0, fs.MAX_RATES - len(named))])


class Case:
    pass


def case(name):
    """ped, model, rates[32], lk, flags, planted, the reference and (trio, wide48) the Hardy-Weinberg rows' — computed once."""
    if name not in _CASES:
        c = Case()
        c.name, c.mrate = name, MODEL_RATE[name]
        c.ped = ped = sets.wide_pedigree(48) if name == "wide48" else sets.side_variant_pedigree(name)
        ped.relations()
        c.model = fs.make_model(ped, mrate=c.mrate)
        c.rates = rate_grid(c.mrate)
        rng = np.random.RandomState(500 + ped.n)
        c.lk, _ = clear_likelihoods(rng, ped, N_SITES)
        seq = np.nonzero(ped.sequenced)[0]
        c.lk[:, ped.sequenced == 0, :] = 1.0
        c.flags = cycled(c.lk)
        c.planted = [SINGLE_FAIL]
        c.lk[SINGLE_FAIL, seq[-1]] = 0.0
        if c.mrate == 0.0:  # tests/_variants.py's construction: mother certain 0/0, child certain 1/1
            mo, _ = ped.relations()
            child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]][0]
            c.lk[BN_FAIL, mo[child]] = [1.0, 0.0, 0.0]
            c.lk[BN_FAIL, child] = [0.0, 0.0, 1.0]
            c.planted.append(BN_FAIL)
        c.ref = reference(ped, c.mrate, c.lk, c.flags, c.rates, brute=False)
        clear(c.ref, name, c.planted)
        assert c.ref[2][SINGLE_FAIL] == 1 and (c.mrate != 0.0 or c.ref[2][BN_FAIL] == 2)
        c.hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, N_SITES))
        c.href = None
        if name in ("trio", "wide48"):
            c.href = reference(ped, c.mrate, c.lk, c.flags, c.rates, c.hwe, brute=False)
            clear(c.href, name + ", Hardy-Weinberg rows", c.planted)
        c.rows = P.model_rows(c.model, c.flags)
        _CASES[name] = c
    return _CASES[name]


def take(out, index):
    return tuple(x[index] for x in out)


def against_evidence(c, out, prior=None, columns=None):
    """Column r is the loglik of evidence_batch on a context made at rates[r], bit for bit, wherever that call has status 0; where
    it has status 2 on a good site Z_r is 0 and the column holds -inf.  -> the entries compared."""
    compared = 0
    for r in range(len(c.rates)) if columns is None else columns:
        ctx = fs.Context(fs.make_model(c.ped, mrate=float(c.rates[r])))
        ll, _, st = ctx.evidence_batch(lk=c.lk, flags=c.flags) if prior is None else ctx.evidence_prior_batch(prior, lk=c.lk, flags=c.flags)
        ctx.close()
        good = (st == 0) & (out[2] == 0)
        assert same_bits([out[0][good, r]], [ll[good]]), (c.name, r, c.rates[r])
        assert np.all(np.isneginf(out[0][(st == 2) & (out[2] == 0), r])), (c.name, r)
        compared += int(good.sum())
    return compared


@pytest.mark.parametrize("name", list(MODEL_RATE))
def test_parity_site_counts_and_rate_counts(name):
    c = case(name)
    ctx = fs.Context(c.model)
    whole = ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags)
    assert whole[0].shape == (N_SITES, 32) and whole[1].shape == (N_SITES,)
    check(whole, c.ref, name)
    assert same_bits(ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags), whole)  # the same batch twice
    assert against_evidence(c, whole) > 30 * (N_SITES - 2)
    ev = ctx.evidence_batch(lk=c.lk, flags=c.flags)
    assert same_bits([whole[1], whole[2]], [ev[0], ev[2]])  # loglik: the evidence entry's bits under the context's own tables
    own = int(np.nonzero(c.rates == c.mrate)[0][0])
    assert same_bits([whole[0][:, own]], [whole[1]])  # a rate equal to the model's
    assert same_bits([whole[0][:, 7]], [whole[0][:, 11]])  # equal rates
    assert same_bits(ctx.mutrate_prior_batch(c.rows, c.rates, lk=c.lk, flags=c.flags), whole)  # the model's rows: the plain form's bits
    for n in SITE_COUNTS[:-1]:
        assert same_bits(ctx.mutrate_batch(c.rates, lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n)))
        assert same_bits(ctx.mutrate_prior_batch(c.rows[:n], c.rates, lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n)))
    for pick in ([0], [31], [13, 0], [own, 5]):  # R = 1 and 2: a column depends neither on n_rates nor on the other rates
        for n in (65, N_SITES):
            sub = ctx.mutrate_batch(c.rates[pick], lk=c.lk[:n], flags=c.flags[:n])
            assert same_bits(sub, (whole[0][:n, pick], whole[1][:n], whole[2][:n])), (name, pick, n)
    assert same_bits(ctx.mutrate_batch(c.rates[3], lk=c.lk, flags=c.flags), (whole[0][:, [3]], whole[1], whole[2]))  # a scalar
    # a split batch against the whole: two calls, and one host call forced into several chunks through both slots
    a, b = ctx.mutrate_batch(c.rates, lk=c.lk[:70], flags=c.flags[:70]), ctx.mutrate_batch(c.rates, lk=c.lk[70:], flags=c.flags[70:])
    assert same_bits(tuple(np.concatenate(x) for x in zip(a, b)), whole)
    ctx.set_option("chunk_sites", 67)
    assert same_bits(ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags), whole)
    assert same_bits(ctx.mutrate_prior_batch(c.rows, c.rates[[2, 9]], lk=c.lk, flags=c.flags), (whole[0][:, [2, 9]], whole[1], whole[2]))
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags), whole)
    ctx.set_option("grid_blocks", 0)
    if c.href is not None:
        hout = ctx.mutrate_prior_batch(c.hwe, c.rates, lk=c.lk, flags=c.flags)
        check(hout, c.href, name + ", Hardy-Weinberg rows")
        assert against_evidence(c, hout, c.hwe, columns=(0, 3, 6, 9, 10, 20)) > 5 * (N_SITES - 2)
    plan = ctx.plan()
    assert plan["mutrate_code_object"].endswith(".hsaco") and 0 <= plan["mutrate_variant"] < 4
    assert plan["mutrate_prior_code_object"].endswith(".hsaco") and plan["mutrate_prior_variant"] == plan["mutrate_variant"]
    ctx.close()


@pytest.mark.parametrize("name", ["ped10", "random15"])
def test_pl16_and_lk_give_the_same_bits_on_host_and_device_entries(name):
    import torch

    c = case(name)
    ped = c.ped
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    pl = rng.randint(0, 61, size=(N_SITES, len(seq), 3)).astype(np.uint16)
    pl[np.arange(N_SITES), :, rng.randint(0, 3, N_SITES)] = 0
    pl[rng.rand(N_SITES, len(seq)) < 0.05] = fs.PL_MISSING
    lk = np.ones((N_SITES, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for col, p in enumerate(seq):
        miss = (pl[:, col] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, col], 4095)])
    rates = c.rates[[0, 3, 10, 7, 9]]
    ref = reference(ped, c.mrate, lk, c.flags, rates, brute=False)
    clear(ref, name + ", packed PLs")
    ctx = fs.Context(c.model)
    b = ctx.mutrate_batch(rates, lk=lk, flags=c.flags)
    check(b, ref, name + ", packed PLs")
    assert same_bits(ctx.mutrate_batch(rates, pl16=pl, seq_members=seq, flags=c.flags), b)
    assert same_bits(ctx.mutrate_prior_batch(c.rows, rates, pl16=pl, seq_members=seq, flags=c.flags), b)
    dev = torch.device("cuda")
    t_pl, t_lk, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(lk).to(dev), torch.from_numpy(c.flags).to(dev)
    t_pr = torch.from_numpy(c.rows).to(dev)
    for n_rates in (1, 2, 5):
        t_tab = torch.from_numpy(ctx.rate_tables(rates[:n_rates])).to(dev)
        for n in SITE_COUNTS:
            for packed in (False, True):
                for prior in (False, True):
                    t_r = torch.full((n, n_rates), -1.0, dtype=torch.float64, device=dev)
                    t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
                    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                    io = dict(d_pl16=t_pl.data_ptr(), seq_members=seq) if packed else dict(d_lk=t_lk.data_ptr())
                    io.update(d_flags=t_fl.data_ptr(), d_rate_loglik=t_r.data_ptr(), d_loglik=t_l.data_ptr(), d_status=t_s.data_ptr())
                    if prior:
                        ctx.mutrate_prior_device(n, t_pr.data_ptr(), t_tab.data_ptr(), n_rates, **io)
                    else:
                        ctx.mutrate_device(n, t_tab.data_ptr(), n_rates, **io)
                    torch.cuda.synchronize()
                    got = (t_r.cpu().numpy(), t_l.cpu().numpy(), t_s.cpu().numpy())
                    assert same_bits(got, (b[0][:n, :n_rates], b[1][:n], b[2][:n])), (name, n_rates, n, packed, prior)
    ctx.close()


def test_device_entries_on_a_stream_null_outputs_and_refusals():
    import torch

    c = case("ped10")
    n, r = N_SITES, 32
    ctx = fs.Context(c.model)
    rl, ll, st = full = ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags)
    hfull = ctx.mutrate_prior_batch(c.hwe, c.rates, lk=c.lk, flags=c.flags)
    assert not same_bits(hfull[:2], full[:2])
    r1, l1, s1 = ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags, want_loglik=False)
    r2, l2, s2 = ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags, want_rates=False)
    assert l1 is None and r2 is None and same_bits((r1, s1, l2, s2), (rl, st, ll, st))
    r3, l3, s3 = ctx.mutrate_prior_batch(c.hwe, c.rates, lk=c.lk, flags=c.flags, want_rates=False, want_loglik=False)
    assert r3 is None and l3 is None and np.array_equal(s3, hfull[2])
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_lk, t_fl = torch.from_numpy(c.lk).to(dev), torch.from_numpy(c.flags).to(dev)
        t_pr, t_tab = torch.from_numpy(c.hwe).to(dev), torch.from_numpy(ctx.rate_tables(c.rates)).to(dev)
        for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
            for prior in (False, True):
                t_r = torch.full((n, r), -1.0, dtype=torch.float64, device=dev)
                t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
                t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_rate_loglik=t_r.data_ptr() if want[0] else 0,
                           d_loglik=t_l.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0, stream=stream.cuda_stream)
                if prior:
                    ctx.mutrate_prior_device(n, t_pr.data_ptr(), t_tab.data_ptr(), r, **out)
                else:
                    ctx.mutrate_device(n, t_tab.data_ptr(), r, **out)
                stream.synchronize()
                exp = hfull if prior else full
                assert same_bits([t_r.cpu().numpy()], [exp[0]]) if want[0] else bool((t_r == -1.0).all())
                assert same_bits([t_l.cpu().numpy()], [exp[1]]) if want[1] else bool((t_l == -1.0).all())
                assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_rates must be 1\.\.32, got 33"):
        ctx.mutrate_device(n, t_tab.data_ptr(), 33, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*d_tables must be given"):
        ctx.mutrate_device(n, 0, 1, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*rates\[2\] must be a finite number in \[0, 1\]"):
        ctx.mutrate_batch([0.0, 1.0, 1.5], lk=c.lk, flags=c.flags)
    ctx.close()


def test_a_mendel_impossible_site_and_failures():
    """test_mutrate_host's planted sites in a batch of more than one workgroup: parents (1, 0, 0) and a child (0, 1, 0) give -inf at
    rate 0 and a finite value at every rate in (0, 1); an all-zero row status 1; 1e160 rows status 2."""
    ped = fs.synthetic_pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    lk[80] = (1.0, 0.0, 0.0)
    lk[80, child] = (0.0, 1.0, 0.0)
    rates = np.array([0.0, 1e-9, 1e-7, 1e-3, 0.5])
    ref = reference(ped, 1e-7, lk, flags, rates)
    clear(ref, "quad", (70,))
    assert ref[2][70] == 1 and ref[1][80, 0] == 0 and np.all(ref[1][80, 1:] > 0)
    model = fs.make_model(ped, mrate=1e-7)
    ctx = fs.Context(model)
    for out in (ctx.mutrate_batch(rates, lk=lk, flags=flags), ctx.mutrate_prior_batch(P.model_rows(model, flags), rates, lk=lk, flags=flags)):
        check(out, ref, "planted zero and failure")
        assert out[2][70] == 1 and np.all(np.isnan(out[0][70])) and np.isnan(out[1][70])
        assert np.isneginf(out[0][80, 0]) and np.all(np.isfinite(out[0][80, 1:])) and np.isfinite(out[1][80]) and out[2][80] == 0
    big = np.full((70, ped.n, 3), 1e160)
    rl, ll, st = ctx.mutrate_batch(rates, lk=big, flags=np.zeros(70, np.uint8))
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(rl))
    ctx.close()


@pytest.mark.parametrize("name", sets.SIDE_VARIANT_PEDIGREES)
def test_every_variant_gives_the_same_bits(name, monkeypatch):
    """Each fence level forced through $FAMSEQ_VARIANT_ONLY (build() has compiled all four, plain and site-prior), the plan
    checked to name it: the reference, the bits of the contest's variant, the site-prior form on the model's rows."""
    c = case(name)
    ctx = fs.Context(c.model)
    want = ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags)
    hwant = ctx.mutrate_prior_batch(c.hwe, c.rates, lk=c.lk, flags=c.flags)
    ctx.close()
    check(want, c.ref, name)
    for v in range(sets.SIDE_VARIANTS):
        ctx = fs.Context(c.model, device=0)
        try:
            SV.forced(ctx, "mutrate", 1, v, monkeypatch)
            SV.forced(ctx, "mutrate_prior", 1, v, monkeypatch)
            ctx.set_option("grid_blocks", 1)
            assert same_bits(ctx.mutrate_batch(c.rates, lk=c.lk, flags=c.flags), want), (name, v)
            assert same_bits(ctx.mutrate_prior_batch(c.rows, c.rates, lk=c.lk, flags=c.flags), want), (name, v, "the model's rows")
            assert same_bits(ctx.mutrate_prior_batch(c.hwe, c.rates, lk=c.lk, flags=c.flags), hwant), (name, v, "Hardy-Weinberg rows")
            for n in (1, 63, 65):
                assert same_bits(ctx.mutrate_batch(c.rates[:2], lk=c.lk[:n], flags=c.flags[:n]), (want[0][:n, :2], want[1][:n], want[2][:n]))
            plan = ctx.plan()
            assert plan["mutrate_variant"] == v and plan["mutrate_prior_variant"] == v
        finally:
            ctx.close()


def test_the_enumeration_engine_and_unserved_pedigrees():
    """A context on the enumeration engine answers as the other side products do; four conditioned members are refused."""
    from test_gpu_denovo import four_loops

    c = case("ped10")
    a = fs.Context(c.model, engine=fs.ENGINE_ENUM)
    b = fs.Context(c.model, engine=fs.ENGINE_ELIM)
    assert same_bits(a.mutrate_batch(c.rates[:3], lk=c.lk, flags=c.flags), b.mutrate_batch(c.rates[:3], lk=c.lk, flags=c.flags))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.mutrate_batch([1e-7], lk=np.ones((4, ped.n, 3)))
    ctx.close()
