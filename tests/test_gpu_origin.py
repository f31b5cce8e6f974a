"""Phase by transmission on the device: famseq_origin_batch / famseq_origin_prior_batch and their device entries through the
Python binding over the C ABI.  Reference and rules as in test_origin_host.py (tests/_origin.py): status exact, origin rows sum to 1
within 1e-12, both outputs at RTOL by test_trio_host.check_joint's rule, at rate 0 every entry the reference has as 0 exactly
0.0, origin summed to genotypes and hettx's pairs equal to the marginals, failed sites NaN, bits where two routes must agree.
Up to ten members the reference is the 3^N enumeration; at 48 the sum-product oracle's marginals.  It is computed once per
pedigree, before anything goes to the device, and asserted status 0 outside the planted sites, so no site is left out.

Shapes: 197 sites per pedigree (three whole 64-lane workgroups and five lanes of a fourth); 1, 63 and 65 sites as slices of it.
Flags 0..3 in turn, so every wave holds all four.  Pedigrees: trio, cousins (one conditioned member, model rate 0: a planted
status-2 site), random15 (three conditioned, three unsequenced members), the ten-member fixture, 48 members (the lean form).
"""
import numpy as np
import pytest

import _origin as O
import _prior as P
import _side_variants as SV
import famseq_amd as fs
from famseq_amd import prebuild_sets as sets
from test_map_host import clear_likelihoods
from test_pattern_host import cycled
from test_trio_host import wide_likelihoods

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


class Case:
    pass


def same_bits(a, b):
    return all((x is None and y is None) or
               (x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)))
               for x, y in zip(a, b))


def take(out, index):
    return tuple(x[index] for x in out)


class WideRef:
    """At 48 members: the oracle's marginals and status."""


def wide_reference(ped, mrate, lk, flags):
    import oracle.sum_product as sp

    r = WideRef()
    r.post, _, r.status = sp.pedigree_posterior(ped, lk, flags, mrate=mrate, lc=2.0)  # lc > 1: no shortcut
    r.ped, r.flags = ped, flags
    return r


def check_wide(out, r, what):
    origin, hettx, st = out
    assert np.array_equal(st, r.status), what
    ok = r.status == 0
    assert np.all(np.isnan(origin[~ok])) and np.all(np.isnan(hettx[~ok])), what
    np.testing.assert_allclose(origin[ok].sum(axis=-1), 1.0, rtol=1e-12, atol=0, err_msg=what)
    mo, fa = r.ped.relations()
    kids = [p for p in range(r.ped.n) if mo[p] >= 0]
    flags = r.flags[ok]
    for k, c in enumerate(kids):
        o, h = origin[ok][:, k], hettx[ok][:, k]
        son_x = ((flags & 2) != 0) & (r.ped.genders[c] == 1)
        child = np.where(son_x[:, None], np.stack([o[:, 0] + o[:, 1], 0 * o[:, 0], o[:, 2] + o[:, 3]], axis=1),
                         np.stack([o[:, 0], o[:, 1] + o[:, 2], o[:, 3]], axis=1))
        O.close(child, r.post[ok][:, c], what)
        pairs = np.stack([h[:, 0] + h[:, 1], h[:, 2] + h[:, 3]], axis=1)
        want = np.stack([r.post[ok][:, mo[c], 1], r.post[ok][:, fa[c], 1]], axis=1)
        sel = want >= 1e-280
        np.testing.assert_allclose(pairs[sel], want[sel], rtol=O.RTOL, atol=0, err_msg=what)
        assert np.all(np.abs(pairs - want)[~sel] <= 1e-270), what


def case(name):
    """ped, model, lk, flags, planted, the reference and (trio) the Hardy-Weinberg rows' — computed once."""
    if name not in _CASES:
        c = Case()
        c.name, c.mrate = name, MODEL_RATE[name]
        c.ped = ped = sets.wide_pedigree(48) if name == "wide48" else sets.side_variant_pedigree(name)
        mo, _ = ped.relations()
        c.model = fs.make_model(ped, mrate=c.mrate)
        c.k = int((np.asarray(mo) >= 0).sum())
        rng = np.random.RandomState(700 + ped.n)
        c.lk, _ = clear_likelihoods(rng, ped, N_SITES)
        if name == "wide48":
            # test_trio_host.wide_likelihoods' rows: with its floor of 1e-2 the all-ref configuration alone keeps Z above 1e-110.
            # The floor is raised under the rows' hard zeros too: a male whose row is 0 wherever his chrX prior is not fails the
            # single posterior, and no site but the planted one may fail.
            c.lk, _ = wide_likelihoods(ped, 48, N_SITES)
            c.lk[c.lk < 1e-2] = 1e-2
        seq = np.nonzero(ped.sequenced)[0]
        c.lk[:, ped.sequenced == 0, :] = 1.0
        c.flags = cycled(c.lk)
        c.planted = [SINGLE_FAIL]
        c.lk[SINGLE_FAIL, seq[-1]] = 0.0
        if c.mrate == 0.0:  # tests/_variants.py's construction: mother certain 0/0, child certain 1/1
            child = [i for i in seq if mo[i] >= 0 and ped.sequenced[mo[i]]][0]
            c.lk[BN_FAIL, mo[child]] = [1.0, 0.0, 0.0]
            c.lk[BN_FAIL, child] = [0.0, 0.0, 1.0]
            c.planted.append(BN_FAIL)
        c.wide = name == "wide48"
        c.ref = wide_reference(ped, c.mrate, c.lk, c.flags) if c.wide else O.reference(ped, c.mrate, c.lk, c.flags)
        want = np.zeros(N_SITES, np.uint8)
        want[SINGLE_FAIL] = 1
        if c.mrate == 0.0:
            want[BN_FAIL] = 2
        assert np.array_equal(c.ref.status, want), name
        c.hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, N_SITES))
        c.href = None
        if name == "trio":
            c.href = O.reference(ped, c.mrate, c.lk, c.flags, prior=c.hwe)
            assert np.array_equal(c.href.status, want), name
        c.rows = P.model_rows(c.model, c.flags)
        c.check = check_wide if c.wide else (lambda out, r, what: O.check(out, r, what, zero_exact=c.mrate == 0.0))
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", list(MODEL_RATE))
def test_parity_and_site_counts(name):
    c = case(name)
    ctx = fs.Context(c.model)
    whole = ctx.origin_batch(lk=c.lk, flags=c.flags)
    assert whole[0].shape == (N_SITES, c.k, 4) and whole[1].shape == (N_SITES, c.k, 4)
    c.check(whole, c.ref, name)
    assert same_bits(ctx.origin_batch(lk=c.lk, flags=c.flags), whole)  # the same batch twice
    assert same_bits(ctx.origin_prior_batch(c.rows, lk=c.lk, flags=c.flags), whole)  # the model's rows: the plain form's bits
    for n in SITE_COUNTS[:-1]:
        assert same_bits(ctx.origin_batch(lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n))), (name, n)
        assert same_bits(ctx.origin_prior_batch(c.rows[:n], lk=c.lk[:n], flags=c.flags[:n]), take(whole, slice(0, n))), (name, n)
    # a split batch against the whole: two calls, and one host call forced into several chunks through both slots
    a, b = ctx.origin_batch(lk=c.lk[:70], flags=c.flags[:70]), ctx.origin_batch(lk=c.lk[70:], flags=c.flags[70:])
    assert same_bits(tuple(np.concatenate(x) for x in zip(a, b)), whole)
    ctx.set_option("chunk_sites", 67)
    assert same_bits(ctx.origin_batch(lk=c.lk, flags=c.flags), whole)
    assert same_bits(ctx.origin_prior_batch(c.rows, lk=c.lk, flags=c.flags), whole)
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.origin_batch(lk=c.lk, flags=c.flags), whole)
    ctx.set_option("grid_blocks", 0)
    # NULL outputs
    o1, h1, s1 = ctx.origin_batch(lk=c.lk, flags=c.flags, want_hettx=False)
    o2, h2, s2 = ctx.origin_batch(lk=c.lk, flags=c.flags, want_origin=False)
    assert h1 is None and o2 is None and same_bits((o1, s1, h2, s2), (whole[0], whole[2], whole[1], whole[2]))
    if c.href is not None:
        hout = ctx.origin_prior_batch(c.hwe, lk=c.lk, flags=c.flags)
        assert not same_bits(hout[:2], whole[:2])
        O.check(hout, c.href, name + ", Hardy-Weinberg rows")
    plan = ctx.plan()
    assert plan["origin_code_object"].endswith(".hsaco") and 0 <= plan["origin_variant"] < 4
    assert plan["origin_prior_code_object"].endswith(".hsaco") and plan["origin_prior_variant"] == plan["origin_variant"]
    assert plan["origin_mrate"] == c.mrate
    assert O.same_bits(ctx.allele_tables(), O.allele_rows(c.mrate))
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
    ref = O.reference(ped, c.mrate, lk, c.flags)
    assert np.all(ref.status == 0)
    ctx = fs.Context(c.model)
    b = ctx.origin_batch(lk=lk, flags=c.flags)
    O.check(b, ref, name + ", packed PLs")
    assert same_bits(ctx.origin_batch(pl16=pl, seq_members=seq, flags=c.flags), b)
    assert same_bits(ctx.origin_prior_batch(c.rows, pl16=pl, seq_members=seq, flags=c.flags), b)
    dev = torch.device("cuda")
    t_pl, t_lk, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(lk).to(dev), torch.from_numpy(c.flags).to(dev)
    t_pr = torch.from_numpy(c.rows).to(dev)
    for n in SITE_COUNTS:
        for packed in (False, True):
            for prior in (False, True):
                t_o = torch.full((n, c.k, 4), -1.0, dtype=torch.float64, device=dev)
                t_h = torch.full((n, c.k, 4), -1.0, dtype=torch.float64, device=dev)
                t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                io = dict(d_pl16=t_pl.data_ptr(), seq_members=seq) if packed else dict(d_lk=t_lk.data_ptr())
                io.update(d_flags=t_fl.data_ptr(), d_origin=t_o.data_ptr(), d_hettx=t_h.data_ptr(), d_status=t_s.data_ptr())
                if prior:
                    ctx.origin_prior_device(n, t_pr.data_ptr(), **io)
                else:
                    ctx.origin_device(n, **io)
                torch.cuda.synchronize()
                got = (t_o.cpu().numpy(), t_h.cpu().numpy(), t_s.cpu().numpy())
                assert same_bits(got, take(b, slice(0, n))), (name, n, packed, prior)
    ctx.close()


def test_device_entries_on_a_stream_null_outputs_and_refusals():
    """The first call of the context is a device call on a stream of its own (the allele rows' upload with it); every call's outputs
    are read through a copy enqueued behind it on that stream."""
    import torch

    c = case("ped10")
    n = N_SITES
    ref_ctx = fs.Context(c.model)
    full = ref_ctx.origin_batch(lk=c.lk, flags=c.flags)
    hfull = ref_ctx.origin_prior_batch(c.hwe, lk=c.lk, flags=c.flags)
    ref_ctx.close()
    assert not same_bits(hfull[:2], full[:2])
    ctx = fs.Context(c.model)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_lk, t_fl = torch.from_numpy(c.lk).to(dev), torch.from_numpy(c.flags).to(dev)
        t_pr = torch.from_numpy(c.hwe).to(dev)
        for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
            for prior in (False, True):
                t_o = torch.full((n, c.k, 4), -1.0, dtype=torch.float64, device=dev)
                t_h = torch.full((n, c.k, 4), -1.0, dtype=torch.float64, device=dev)
                t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_origin=t_o.data_ptr() if want[0] else 0,
                           d_hettx=t_h.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0, stream=stream.cuda_stream)
                if prior:
                    ctx.origin_prior_device(n, t_pr.data_ptr(), **out)
                else:
                    ctx.origin_device(n, **out)
                # the copies follow the entry on its stream; nothing else orders them with the kernel
                h_o, h_h, h_s = (torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in (t_o, t_h, t_s))
                h_o.copy_(t_o, non_blocking=True), h_h.copy_(t_h, non_blocking=True), h_s.copy_(t_s, non_blocking=True)
                stream.synchronize()
                exp = hfull if prior else full
                assert same_bits([h_o.numpy()], [exp[0]]) if want[0] else bool((h_o == -1.0).all())
                assert same_bits([h_h.numpy()], [exp[1]]) if want[1] else bool((h_h == -1.0).all())
                assert np.array_equal(h_s.numpy(), exp[2]) if want[2] else bool((h_s == 55).all())
    ctx.close()
    # argument errors are raised before the device is asked: a context without one says them too
    off = fs.Context(c.model, device=-1)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*exactly one of lk / pl16"):
        off.origin_device(n, d_lk=0, d_pl16=0)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*d_prior must be given"):
        off.origin_prior_device(n, 0, d_lk=8)
    with pytest.raises(ValueError):
        off.origin_batch(lk=c.lk, pl16=np.zeros((n, 10, 3), np.uint16), flags=c.flags)
    off.close()
    custom = fs.make_model(c.ped, mrate=1e-7)
    custom.pcp2[4] = np.nextafter(custom.pcp2[4], 1.0)
    ctx = fs.Context(custom)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*no allele-level model for custom"):
        ctx.origin_batch(lk=c.lk, flags=c.flags)
    ctx.close()


def test_failures_in_a_batch_of_more_than_one_workgroup():
    """An all-zero row: status 1; 1e160 rows: every normaliser overflows, status 2; at rate 0 a Mendel-impossible trio is status 2
    while the same rows at a positive rate are a result."""
    ped = fs.synthetic_pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    lk[80] = (1.0, 0.0, 0.0)
    lk[80, child] = (0.0, 1.0, 0.0)
    for mrate in (1e-7, 0.0):
        ref = O.reference(ped, mrate, lk, flags)
        assert ref.status[70] == 1 and ref.status[80] == (2 if mrate == 0.0 else 0) and (ref.status != 0).sum() == (2 if mrate == 0.0 else 1)
        model = fs.make_model(ped, mrate=mrate)
        ctx = fs.Context(model)
        for out in (ctx.origin_batch(lk=lk, flags=flags), ctx.origin_prior_batch(P.model_rows(model, flags), lk=lk, flags=flags)):
            O.check(out, ref, "planted failures, rate %g" % mrate, zero_exact=mrate == 0.0)
        if mrate != 0.0:
            big = np.full((70, ped.n, 3), 1e160)
            o, h, st = ctx.origin_batch(lk=big, flags=np.zeros(70, np.uint8))
            assert np.all(st == 2) and np.all(np.isnan(o)) and np.all(np.isnan(h))
        ctx.close()


@pytest.mark.parametrize("name", sets.SIDE_VARIANT_PEDIGREES)
def test_every_variant_against_the_reference(name, monkeypatch):
    """Each fence level forced through $FAMSEQ_VARIANT_ONLY (build() has compiled all four, plain and site-prior), the plan
    checked to name it: the reference, the contest's variant at RTOL (levels 1 to 3 are the same statements: their bits), the
    site-prior form on the model's rows."""
    c = case(name)
    outs = []
    for v in range(sets.SIDE_VARIANTS):
        ctx = fs.Context(c.model, device=0)
        try:
            SV.forced(ctx, "origin", 1, v, monkeypatch)
            SV.forced(ctx, "origin_prior", 1, v, monkeypatch)
            ctx.set_option("grid_blocks", 1)
            out = ctx.origin_batch(lk=c.lk, flags=c.flags)
            c.check(out, c.ref, "%s, variant %d" % (name, v))
            assert same_bits(ctx.origin_prior_batch(c.rows, lk=c.lk, flags=c.flags), out), (name, v, "the model's rows")
            for n in (1, 63, 65):
                assert same_bits(ctx.origin_batch(lk=c.lk[:n], flags=c.flags[:n]), take(out, slice(0, n))), (name, v, n)
            plan = ctx.plan()
            assert plan["origin_variant"] == v and plan["origin_prior_variant"] == v
            outs.append(out)
        finally:
            ctx.close()
    assert same_bits(outs[2], outs[1]) and same_bits(outs[3], outs[1])


def test_the_enumeration_engine_and_unserved_pedigrees():
    """A context on the enumeration engine answers as the other side products do; four conditioned members are refused."""
    from test_gpu_denovo import four_loops

    c = case("ped10")
    a = fs.Context(c.model, engine=fs.ENGINE_ENUM)
    b = fs.Context(c.model, engine=fs.ENGINE_ELIM)
    assert same_bits(a.origin_batch(lk=c.lk, flags=c.flags), b.origin_batch(lk=c.lk, flags=c.flags))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.origin_batch(lk=np.ones((4, ped.n, 3)))
    ctx.close()
