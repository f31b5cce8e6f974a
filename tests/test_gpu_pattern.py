"""Genotype-pattern posteriors on the device: famseq_pattern_batch / famseq_pattern_prior_batch and their device entries through
the Python binding over the C ABI.  References and rules as in test_pattern_host.py: status exact, ppost == 0.0 exactly where
the reference's Z_m is exactly 0, elsewhere rtol 1e-9, ppost == 1.0 exactly for a row of 7s and <= 1.0 everywhere, loglik at an
absolute 1e-9, failed sites NaN, bits where two routes must agree.  Every batch asserts on the reference alone status 0 and Z
and every non-zero Z_m >= 1e-200 before anything goes to the device, so no site is left out.

Shapes, the smallest at which the shell can go wrong: 1 site (a block of padding lanes but one), one less and one more than the
block, 3 BT + 5 sites against the reference (computed once per pedigree), 1,000 sites (that batch repeated: sixteen blocks, the
last partial) and a host call forced into several chunks, against the reference-checked rows bit for bit.  Flags 0..3 in turn,
so every wave holds all four.  Pedigrees: trio, the ten-member fixture, a looped random pedigree, 48 members (the lean form).
"""
import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd.prebuild_sets import wide_pedigree
from test_gpu_denovo import four_loops
from test_gpu_map import loop_pedigree
from test_map_host import clear_likelihoods
from test_pattern_host import FLOOR, RTOL, allowed, batch_masks, check, cycled, reference, same_bits

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """-> (ped, BT, lk, flags, masks, reference, Hardy-Weinberg rows, their reference): 3 BT + 5 clear sites, computed once."""
    if name not in _CASES:
        ped = {"trio": lambda: fs.synthetic_pedigree("trio"), "ped10": lambda: fs.synthetic_pedigree("ped10"),
               "loop": lambda: loop_pedigree(0)[1], "wide48": lambda: wide_pedigree(48)}[name]()
        ped.relations()
        ctx = fs.Context(fs.make_model(ped), device=-1)
        bt = ctx.plan()["evidence_block_threads"]  # (every side product's kernel runs in these workgroups)
        ctx.close()
        assert bt >= 2
        rng = np.random.RandomState(80 + ped.n)
        lk, _ = clear_likelihoods(rng, ped, 3 * bt + 5)
        flags = cycled(lk)
        masks = batch_masks(rng, ped)
        hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, len(lk)))
        ref = reference(ped, 1e-7, lk, flags, masks)
        href = reference(ped, 1e-7, lk, flags, masks, hwe) if name in ("trio", "wide48") else None
        for r in (ref, href):
            assert r is None or (np.all(r[2] == 0) and np.all(r[0] >= FLOOR) and np.all((r[1] == 0) | (r[1] >= FLOOR)))
        _CASES[name] = (ped, bt, lk, flags, masks, ref, hwe, href)
    return _CASES[name]


def take(out, index):
    return tuple(x[index] for x in out)


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "wide48"])
def test_parity_and_site_counts(name):
    ped, bt, lk, flags, masks, ref, hwe, href = case(name)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    assert (ctx.plan()["elim_conditioned_members"] > 0) == (name == "loop")
    whole = ctx.pattern_batch(masks, lk=lk, flags=flags)
    assert whole[0].shape == (len(lk), len(masks)) and whole[1].shape == (len(lk),)
    check(whole, ref, masks, name)
    assert same_bits(ctx.pattern_batch(masks, lk=lk, flags=flags), whole)  # the same batch twice
    # loglik is the evidence entry's, bit for bit (the unmasked pass keeps its statements); the all-1 row its pref
    ll, p0, st = ctx.evidence_batch(lk=lk, flags=flags)
    assert np.all(st == 0) and same_bits([whole[1]], [ll])
    np.testing.assert_allclose(whole[0][:, 1], p0, rtol=RTOL, atol=0)
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.pattern_prior_batch(rows, masks, lk=lk, flags=flags), whole)  # the model's rows: the plain form's bits
    for n in (1, bt - 1, bt + 1):
        assert same_bits(ctx.pattern_batch(masks, lk=lk[:n], flags=flags[:n]), take(whole, slice(0, n)))
        assert same_bits(ctx.pattern_prior_batch(rows[:n], masks, lk=lk[:n], flags=flags[:n]), take(whole, slice(0, n)))
    # 1,000 sites: the batch over and over (the flags keep their turn: its length is 1 mod 4 ... so take them with the rows)
    idx = np.arange(1000) % len(lk)
    big = ctx.pattern_batch(masks, lk=lk[idx], flags=flags[idx])
    assert same_bits(big, take(whole, idx))
    ctx.set_option("chunk_sites", 2 * bt + 3)  # a host call in several chunks, the last one partial, through both slots
    assert same_bits(ctx.pattern_batch(masks, lk=lk[idx], flags=flags[idx]), big)
    assert same_bits(ctx.pattern_prior_batch(rows[idx], masks, lk=lk[idx], flags=flags[idx]), big)
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.pattern_batch(masks, lk=lk, flags=flags), whole)
    ctx.set_option("grid_blocks", 0)
    if href is not None:
        check(ctx.pattern_prior_batch(hwe, masks, lk=lk, flags=flags), href, masks, name + ", Hardy-Weinberg rows")
    plan = ctx.plan()
    assert plan["pattern_code_object"].endswith(".hsaco") and 0 <= plan["pattern_variant"] < 4
    assert plan["pattern_prior_code_object"].endswith(".hsaco") and plan["pattern_prior_variant"] == plan["pattern_variant"]
    ctx.close()


@pytest.mark.parametrize("name", ["ped10", "wide48"])
def test_one_three_and_thirty_two_patterns(name):
    """A pattern's posterior does not depend on how many others the call holds; the masks of a call replace the last call's."""
    ped, bt, lk, flags, masks, ref, _, _ = case(name)
    rng = np.random.RandomState(5)
    many = np.concatenate([masks, rng.randint(1, 8, size=(32 - len(masks), ped.n)).astype(np.uint8)])
    ctx = fs.Context(fs.make_model(ped))
    out = ctx.pattern_batch(many, lk=lk, flags=flags)
    assert out[0].shape == (len(lk), 32)
    check((out[0][:, :len(masks)], out[1], out[2]), ref, masks, name + ", 32 patterns")
    assert np.all(out[0] <= 1.0) and np.all(out[0] >= 0.0)
    for pick in ([31], [0], [30, 2, 17], list(range(len(masks)))):
        sub = ctx.pattern_batch(many[pick], lk=lk, flags=flags)
        assert same_bits(sub, (out[0][:, pick], out[1], out[2]))
    one_row = ctx.pattern_batch(many[4], lk=lk, flags=flags)  # a single row [N]
    assert same_bits(one_row, (out[0][:, [4]], out[1], out[2]))
    ctx.close()


def test_against_the_evidence_entry_on_masked_rows():
    """Today's roundabout route: famseq_evidence_batch on host-masked rows, 10**(loglik_m - loglik).  A pattern the masked rows
    give no weight fails there (status 1 or 2) and is 0.0 here."""
    ped, bt, lk, flags, masks, ref, _, _ = case("wide48")
    ctx = fs.Context(fs.make_model(ped))
    pp, ll, st = ctx.pattern_batch(masks, lk=lk, flags=flags)
    assert np.all(st == 0)
    compared = 0
    for m, keep in enumerate(allowed(masks)):
        ll_m, _, st_m = ctx.evidence_batch(lk=lk * keep, flags=flags)
        ok = st_m == 0
        assert np.all(pp[~ok, m] == 0.0) and np.all(ref[1][~ok, m] == 0)
        np.testing.assert_allclose(pp[ok, m], 10.0 ** (ll_m[ok] - ll[ok]), rtol=RTOL, atol=0)
        compared += int(ok.sum())
    assert compared > 5 * len(lk)
    ctx.close()


def test_pl16_and_lk_give_the_same_bits():
    import torch

    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    n = 200
    pl = rng.randint(0, 300, size=(n, len(seq), 3)).astype(np.uint16)
    pl[rng.rand(n, len(seq)) < 0.05] = fs.PL_MISSING
    flags = cycled(pl)
    masks = batch_masks(rng, ped)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    a = ctx.pattern_batch(masks, pl16=pl, seq_members=seq, flags=flags)
    b = ctx.pattern_batch(masks, lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.pattern_prior_batch(rows, masks, pl16=pl, seq_members=seq, flags=flags), b)
    dev = torch.device("cuda")
    t_pl, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(flags).to(dev)
    t_mk = torch.from_numpy(masks).to(dev)
    t_p = torch.full((n, len(masks)), -1.0, dtype=torch.float64, device=dev)
    t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.pattern_batch_device(n, t_mk.data_ptr(), len(masks), d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(),
                             d_pat_post=t_p.data_ptr(), d_loglik=t_l.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert same_bits((t_p.cpu().numpy(), t_l.cpu().numpy(), t_s.cpu().numpy()), b)


def test_device_entries_and_null_outputs():
    import torch

    ped, bt, lk, flags, masks, ref, hwe, _ = case("ped10")
    n, m = len(lk), len(masks)
    ctx = fs.Context(fs.make_model(ped))
    pp, ll, st = full = ctx.pattern_batch(masks, lk=lk, flags=flags)
    hfull = ctx.pattern_prior_batch(hwe, masks, lk=lk, flags=flags)
    assert not same_bits(hfull[:2], full[:2])
    p1, l1, s1 = ctx.pattern_batch(masks, lk=lk, flags=flags, want_loglik=False)
    p2, l2, s2 = ctx.pattern_batch(masks, lk=lk, flags=flags, want_post=False)
    assert l1 is None and p2 is None and same_bits((p1, s1, l2, s2), (pp, st, ll, st))
    p3, l3, s3 = ctx.pattern_prior_batch(hwe, masks, lk=lk, flags=flags, want_post=False, want_loglik=False)
    assert p3 is None and l3 is None and np.array_equal(s3, hfull[2])
    dev = torch.device("cuda")
    t_lk, t_fl, t_mk = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev), torch.from_numpy(masks).to(dev)
    t_pr = torch.from_numpy(hwe).to(dev)
    for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
        for prior in (False, True):
            t_p = torch.full((n, m), -1.0, dtype=torch.float64, device=dev)
            t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
            t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
            out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_pat_post=t_p.data_ptr() if want[0] else 0,
                       d_loglik=t_l.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0)
            if prior:
                ctx.pattern_prior_batch_device(n, t_pr.data_ptr(), t_mk.data_ptr(), m, **out)
            else:
                ctx.pattern_batch_device(n, t_mk.data_ptr(), m, **out)
            torch.cuda.synchronize()
            exp = hfull if prior else full
            assert same_bits([t_p.cpu().numpy()], [exp[0]]) if want[0] else bool((t_p == -1.0).all())
            assert same_bits([t_l.cpu().numpy()], [exp[1]]) if want[1] else bool((t_l == -1.0).all())
            assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_patterns must be 1\.\.32"):
        ctx.pattern_batch_device(n, t_mk.data_ptr(), 33, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*masks must be given"):
        ctx.pattern_batch_device(n, 0, 1, d_lk=t_lk.data_ptr())
    ctx.close()


def test_planted_failures():
    """test_pattern_host.test_failure_statuses' sites on a quad at mutation rate 0, in a batch of more than one workgroup."""
    ped = fs.synthetic_pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    lk[75] = (1.0, 0.0, 0.0)
    lk[75, child] = (0.0, 0.0, 1.0)
    masks = batch_masks(np.random.RandomState(4), ped)
    ref = reference(ped, 0.0, lk, flags, masks)
    assert ref[2][70] == 1 and ref[2][75] == 2 and np.all(np.delete(ref[2], [70, 75]) == 0)
    model = fs.make_model(ped, mrate=0.0)
    ctx = fs.Context(model)
    for out in (ctx.pattern_batch(masks, lk=lk, flags=flags), ctx.pattern_prior_batch(P.model_rows(model, flags), masks, lk=lk, flags=flags)):
        check(out, ref, masks, "planted failures", clear=False)
        assert out[2][70] == 1 and out[2][75] == 2 and np.all(np.isnan(out[0][[70, 75]])) and np.all(np.isnan(out[1][[70, 75]]))
    bad = masks.copy()
    bad[2, 1] = 9
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*pattern 2, member 1 is 9"):
        ctx.pattern_batch(bad, lk=lk, flags=flags)
    ctx.close()


def test_the_enumeration_engine_and_unserved_pedigrees():
    """A context on the enumeration engine answers as the other side products do; four conditioned members are refused."""
    ped, bt, lk, flags, masks, ref, _, _ = case("ped10")
    a = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ENUM)
    b = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ELIM)
    assert same_bits(a.pattern_batch(masks, lk=lk, flags=flags), b.pattern_batch(masks, lk=lk, flags=flags))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.pattern_batch(np.full((1, ped.n), 7, np.uint8), lk=np.ones((4, ped.n, 3)))
    ctx.close()
