"""The founders' allele frequency by maximum likelihood on the device: famseq_af_batch and its device entry through the Python
binding over the C ABI.  Reference and rules as in test_af_host.py: status exact, af at rtol 1e-9 (atol 1e-300), both loglik
entries at an absolute 1e-9, -inf exactly where the reference's Z(0) is 0, failed sites NaN, bits where two routes must agree.
Every batch asserts on the reference alone status 0 and every Z(q_t) >= 1e-200 (tests/_af.py) before anything goes to the device.

Shapes, the smallest at which the shell can go wrong (test_gpu_pattern.py's): 1 site, one less and one more than the block,
3 BT + 5 sites against the reference (computed once per pedigree), 1,000 sites (that batch repeated) and a host call forced into
several chunks — which is what takes the 8-byte start values through both staging slots — against the reference-checked rows bit
for bit.  Flags 0..3 in turn, so every wave holds all four.  Pedigrees: trio, the ten-member fixture, a looped random pedigree,
48 members (the lean form).
"""
import numpy as np
import pytest

import _af as A
import famseq_amd as fs
from famseq_amd.prebuild_sets import wide_pedigree
from test_af_host import LL_ATOL, RTOL, check
from test_gpu_denovo import four_loops
from test_gpu_map import loop_pedigree
from test_map_host import clear_likelihoods
from test_pattern_host import cycled, same_bits

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """-> (ped, BT, lk, flags, af0, T, reference): 3 BT + 5 clear sites, T = 4 steps (wide48: 2), computed once."""
    if name not in _CASES:
        ped = {"trio": lambda: fs.synthetic_pedigree("trio"), "ped10": lambda: fs.synthetic_pedigree("ped10"),
               "loop": lambda: loop_pedigree(0)[1], "wide48": lambda: wide_pedigree(48)}[name]()
        ped.relations()
        ctx = fs.Context(fs.make_model(ped), device=-1)
        bt = ctx.plan()["evidence_block_threads"]  # (every side product's kernel runs in these workgroups)
        ctx.close()
        assert bt >= 2
        rng = np.random.RandomState(90 + ped.n)
        lk, _ = clear_likelihoods(rng, ped, 3 * bt + 5)
        flags = cycled(lk)
        af0 = rng.uniform(0.01, 0.9, len(lk))
        steps = 2 if name == "wide48" else 4
        _CASES[name] = (ped, bt, lk, flags, af0, steps, A.reference(ped, 1e-7, lk, flags, af0, steps))
    return _CASES[name]


def take(out, index):
    return tuple(x[index] for x in out)


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "wide48"])
def test_parity_and_site_counts(name):
    ped, bt, lk, flags, af0, steps, ref = case(name)
    ctx = fs.Context(fs.make_model(ped))
    assert (ctx.plan()["elim_conditioned_members"] > 0) == (name == "loop")
    whole = ctx.af_batch(af0, steps, lk=lk, flags=flags)
    assert whole[0].shape == (len(lk),) and whole[1].shape == (len(lk), 2) and whole[2].shape == (len(lk),)
    check(whole, ref, steps, name)
    assert same_bits(ctx.af_batch(af0, steps, lk=lk, flags=flags), whole)  # the same batch twice
    for n in (1, bt - 1, bt + 1):
        assert same_bits(ctx.af_batch(af0[:n], steps, lk=lk[:n], flags=flags[:n]), take(whole, slice(0, n)))
    # 1,000 sites: the batch over and over (the flags and the start values travel with their rows)
    idx = np.arange(1000) % len(lk)
    big = ctx.af_batch(af0[idx], steps, lk=lk[idx], flags=flags[idx])
    assert same_bits(big, take(whole, idx))
    ctx.set_option("chunk_sites", 2 * bt + 3)  # a host call in several chunks, the last one partial, through both slots
    assert same_bits(ctx.af_batch(af0[idx], steps, lk=lk[idx], flags=flags[idx]), big)
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.af_batch(af0, steps, lk=lk, flags=flags), whole)
    ctx.set_option("grid_blocks", 0)
    # a scalar start value is every site's
    assert same_bits(ctx.af_batch(0.25, steps, lk=lk, flags=flags), ctx.af_batch(np.full(len(lk), 0.25), steps, lk=lk, flags=flags))
    plan = ctx.plan()
    assert plan["af_code_object"].endswith(".hsaco") and 0 <= plan["af_variant"] < 4 and "af_prior_code_object" not in plan
    ctx.close()


@pytest.mark.parametrize("name", ["ped10", "loop", "wide48"])
def test_chaining_and_no_steps(name):
    """a steps, then b from their result: the bits of a + b.  No steps: af0's bits, and famseq_evidence_prior's loglik (at 1e-9)
    and status on hwe_priors(af0)."""
    ped, bt, lk, flags, af0, steps, ref = case(name)
    ctx = fs.Context(fs.make_model(ped))
    whole = ctx.af_batch(af0, steps, lk=lk, flags=flags)
    first = ctx.af_batch(af0, 1, lk=lk, flags=flags)
    check(first, ref, 1, name)
    assert same_bits(ctx.af_batch(first[0], steps - 1, lk=lk, flags=flags), whole)
    none = ctx.af_batch(af0, 0, lk=lk, flags=flags)
    check(none, ref, 0, name)
    assert same_bits([none[0]], [af0]) and same_bits(ctx.af_batch(whole[0], 0, lk=lk, flags=flags), whole)
    ll, _, st = ctx.evidence_prior_batch(fs.hwe_priors(af0), lk=lk, flags=flags)
    assert np.array_equal(st, none[2])
    np.testing.assert_allclose(none[1][:, 0], ll, rtol=0, atol=LL_ATOL)
    # the likelihood does not decrease (within the comparison's own tolerance)
    assert np.all(first[1][:, 0] >= none[1][:, 0] - 1e-9) and np.all(whole[1][:, 0] >= first[1][:, 0] - 1e-9)
    ctx.close()


@pytest.mark.parametrize("name", ["ped10", "loop"])
def test_against_the_posterior_entry_step_by_step(name):
    """Today's route: one launch of famseq_bn_prior_batch per step on hwe_priors(q), the update in numpy on the founders' rows."""
    ped, bt, lk, flags, af0, steps, ref = case(name)
    ctx = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ELIM)
    chrx = (flags & fs.FLAG_CHRX) != 0
    founders = A.founders_of(ped)
    q = af0.copy()
    for _ in range(steps):
        post, _, st = ctx.bn_prior_batch(lk, fs.hwe_priors(q), flags=flags)
        assert np.all(st == 0)  # (no site takes the -LRC shortcut: continuous rows)
        a = np.zeros(len(q))
        for f in founders:
            m = post[:, f]
            male = ped.genders[f] == 1
            a = a + np.where(chrx & male, m[:, 2], m[:, 1] + 2 * m[:, 2]) / ((m[:, 0] + m[:, 1]) + m[:, 2])
        n_male = sum(ped.genders[f] == 1 for f in founders)
        q = np.minimum(a / np.where(chrx, 2.0 * (len(founders) - n_male) + n_male, 2.0 * len(founders)), 1.0)
    af, _, st = ctx.af_batch(af0, steps, lk=lk, flags=flags)
    assert np.all(st == 0)
    print("%s: worst relative difference of the two routes %.3g" % (name, np.abs(af / q - 1).max()))
    np.testing.assert_allclose(af, q, rtol=RTOL, atol=0)
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
    af0 = rng.uniform(0.01, 0.9, n)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    ctx = fs.Context(fs.make_model(ped))
    a = ctx.af_batch(af0, 4, pl16=pl, seq_members=seq, flags=flags)
    b = ctx.af_batch(af0, 4, lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    dev = torch.device("cuda")
    t_pl, t_fl, t_q = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(flags).to(dev), torch.from_numpy(af0).to(dev)
    t_a = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_l = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.af_batch_device(n, t_q.data_ptr(), 4, d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(), d_af=t_a.data_ptr(),
                        d_loglik=t_l.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert same_bits((t_a.cpu().numpy(), t_l.cpu().numpy(), t_s.cpu().numpy()), b)


def test_device_entry_and_null_outputs():
    import torch

    ped, bt, lk, flags, af0, steps, ref = case("ped10")
    n = len(lk)
    ctx = fs.Context(fs.make_model(ped))
    af, ll, st = full = ctx.af_batch(af0, steps, lk=lk, flags=flags)
    a1, l1, s1 = ctx.af_batch(af0, steps, lk=lk, flags=flags, want_loglik=False)
    a2, l2, s2 = ctx.af_batch(af0, steps, lk=lk, flags=flags, want_af=False)
    assert l1 is None and a2 is None and same_bits((a1, s1, l2, s2), (af, st, ll, st))
    dev = torch.device("cuda")
    t_lk, t_fl, t_q = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev), torch.from_numpy(af0).to(dev)
    for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
        t_a = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        t_l = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
        t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
        ctx.af_batch_device(n, t_q.data_ptr(), steps, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_af=t_a.data_ptr() if want[0] else 0,
                            d_loglik=t_l.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0)
        torch.cuda.synchronize()
        assert same_bits([t_a.cpu().numpy()], [af]) if want[0] else bool((t_a == -1.0).all())
        assert same_bits([t_l.cpu().numpy()], [ll]) if want[1] else bool((t_l == -1.0).all())
        assert np.array_equal(t_s.cpu().numpy(), st) if want[2] else bool((t_s == 55).all())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_iter must be 0\.\.64"):
        ctx.af_batch_device(n, t_q.data_ptr(), 65, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*af0 must be given"):
        ctx.af_batch_device(n, 0, 1, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*af0 entries must be finite numbers in \[0, 1\] \(site 7\)"):
        ctx.af_batch(np.where(np.arange(n) == 7, 1.5, af0), steps, lk=lk, flags=flags)
    ctx.close()


def test_planted_sites():
    """test_af_host.test_planted_sites' sites on a quad at mutation rate 0, in a batch of more than one workgroup; the start value
    the host entry would refuse reaches the kernel through the device entry."""
    import torch

    ped = fs.synthetic_pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    lk[75] = (1.0, 0.0, 0.0)
    lk[75, child] = (0.0, 0.0, 1.0)
    lk[80, A.founders_of(ped)[0], 0] = 0.0
    af0 = np.full(96, 0.3)
    ctx = fs.Context(fs.make_model(ped, mrate=0.0))
    af, ll, st = ctx.af_batch(af0, 3, lk=lk, flags=flags)
    good = np.delete(np.arange(96), [70, 75])
    assert st[70] == 1 and st[75] == 2 and np.all(st[good] == 0)
    assert np.all(np.isnan(af[[70, 75]])) and np.all(np.isnan(ll[[70, 75]]))
    assert ll[80, 1] == -np.inf and np.isfinite(ll[80, 0]) and np.isfinite(af[80])
    check(take((af, ll, st), good), A.reference(ped, 0.0, lk[good], flags[good], af0[good], 3), 3, "quad, planted sites")
    dev = torch.device("cuda")
    af0[90] = 1.5
    t_lk, t_fl, t_q = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev), torch.from_numpy(af0).to(dev)
    t_a = torch.full((96,), -1.0, dtype=torch.float64, device=dev)
    t_l = torch.full((96, 2), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((96,), 55, dtype=torch.uint8, device=dev)
    ctx.af_batch_device(96, t_q.data_ptr(), 3, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_af=t_a.data_ptr(), d_loglik=t_l.data_ptr(),
                        d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    d_af, d_ll, d_st = t_a.cpu().numpy(), t_l.cpu().numpy(), t_s.cpu().numpy()
    assert d_st[90] == 2 and np.isnan(d_af[90]) and np.all(np.isnan(d_ll[90]))
    keep = np.delete(np.arange(96), 90)
    assert same_bits(take((d_af, d_ll, d_st), keep), take((af, ll, st), keep))
    ctx.close()


def test_the_enumeration_engine_and_unserved_pedigrees():
    """A context on the enumeration engine answers as the other side products do; four conditioned members are refused."""
    ped, bt, lk, flags, af0, steps, ref = case("ped10")
    a = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ENUM)
    b = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ELIM)
    assert same_bits(a.af_batch(af0, steps, lk=lk, flags=flags), b.af_batch(af0, steps, lk=lk, flags=flags))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.af_batch(0.5, 2, lk=np.ones((4, ped.n, 3)))
    ctx.close()
