"""Exact joint posterior draws on the device: famseq_sample_batch / famseq_sample_batch_device (and the site-prior entries)
through the C ABI.  The device kernel against the host-compiled kernel of test_sample_host.py bit for bit (the decision rule has
no division and contraction is off; samp_post, which ends in one, at 1e-9), the enumeration's checks and a reduced form of the
law on the device, and what a draw may depend on: not the batch, not the chunking, not the entry."""
import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd.prebuild_sets import wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_gpu_denovo import four_loops
from test_gpu_map import loop_pedigree
from test_map_host import brute_weights
from test_sample_host import RTOL, build_sample_host, check_draws, law_checks, law_inputs, run_sample

pytestmark = pytest.mark.gpu


def pedigree(case):
    if case == "loop":
        ped = loop_pedigree(0)[1]
    elif case.startswith("wide"):
        ped = wide_pedigree(int(case[4:]))
    else:
        ped = fs.synthetic_pedigree(case)
    ped.relations()
    return ped


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["trio", "ped5", "ped10", "loop", "wide48"])
def test_the_device_takes_the_host_kernels_decisions(case, tmp_path):
    ped = pedigree(case)
    model = fs.make_model(ped, mrate=1e-4)
    lk, flags = random_likelihoods(np.random.RandomState(41), ped, 333, max_pl=300 if ped.n <= 20 else 40)
    fn, _, _ = build_sample_host(model, tmp_path / "k")
    h_gt, h_post, h_st = run_sample(fn, model, lk, flags, 3, seed=5, site_base=12)
    ctx = fs.Context(model)
    gt, post, st = ctx.sample_batch(3, seed=5, site_base=12, lk=lk, flags=flags)
    ctx.close()
    ok = st == 0
    assert ok.sum() > 100
    assert np.array_equal(st, h_st) and np.array_equal(gt, h_gt)
    assert np.all(np.isnan(post[~ok])) and np.all(np.isnan(h_post[~ok]))
    np.testing.assert_allclose(post[ok], h_post[ok], rtol=RTOL, atol=0)


@pytest.mark.parametrize("case", ["ped10", "loop"])
def test_draws_and_their_law_on_the_device(case):
    ped = pedigree(case)
    for mrate in (1e-4, 0.0):
        ctx = fs.Context(fs.make_model(ped, mrate=mrate))
        lk, flags = random_likelihoods(np.random.RandomState(17), ped, 200)
        out = ctx.sample_batch(5, seed=99, lk=lk, flags=flags)
        G, W, ref_st = brute_weights(ped, mrate, lk, flags)
        check_draws(ped, mrate, flags, out, G, W, ref_st)
        if mrate == 0.0:
            ctx.close()
            continue
        rows, repeat = 4, 1024
        lk4, fl4, lk, flags = law_inputs(ped, rows, repeat)
        gt, post, st = ctx.sample_batch(16, seed=20261019, lk=lk, flags=flags)
        ctx.close()
        G, W, ref_st = brute_weights(ped, mrate, lk4, fl4)
        assert np.all(ref_st == 0) and np.all(st == 0)
        assert law_checks(ped, gt, G, W, rows, repeat, False) > 50


def test_batch_sizes_and_chunking():
    """Batches of 1, 63, 64, 65 and 1,000 sites give the bits of the whole batch's rows; so does a batch of several chunks and
    several trips of every workgroup under the default chunking, as one launch and in chunks of 128: a chunk that forgot its
    offset would draw the first chunk's numbers again."""
    import torch

    ped = fs.synthetic_pedigree("ped10")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * 4 * n_cu * 4 + 37
    rng = np.random.RandomState(8)
    base_lk, _ = random_likelihoods(rng, ped, 4096)
    lk = base_lk[rng.randint(0, 4096, n)]
    flags = (np.arange(n) % 4).astype(np.uint8)
    ctx = fs.Context(fs.make_model(ped, mrate=1e-4))
    whole = ctx.sample_batch(2, seed=3, lk=lk, flags=flags)
    ok = whole[2] == 0
    assert ok.mean() > 0.5
    # (the same row at two sites draws different configurations: the site's index is in the counter)
    for k in (1, 63, 64, 65, 1000):
        assert same_bits(ctx.sample_batch(2, seed=3, lk=lk[:k], flags=flags[:k]), [x[:k] for x in whole])
    a = 70001
    assert same_bits(ctx.sample_batch(2, seed=3, site_base=a, lk=lk[a:a + 500], flags=flags[a:a + 500]), [x[a:a + 500] for x in whole])
    ctx.set_option("chunk_sites", n)
    assert same_bits(ctx.sample_batch(2, seed=3, lk=lk, flags=flags), whole)
    ctx.set_option("chunk_sites", 128)
    m = 5000
    assert same_bits(ctx.sample_batch(2, seed=3, lk=lk[:m], flags=flags[:m]), [x[:m] for x in whole])
    assert same_bits(ctx.sample_batch(2, seed=3, site_base=n - m, lk=lk[n - m:], flags=flags[n - m:]), [x[n - m:] for x in whole])
    ctx.close()


def test_entries_and_bounds():
    import torch

    ped = fs.synthetic_pedigree("ped5")  # N % 4 != 0: rows that start at every alignment
    lk, flags = random_likelihoods(np.random.RandomState(2), ped, 333)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    k = 3
    gt, post, st = ctx.sample_batch(k, seed=11, site_base=5, lk=lk, flags=flags)
    assert (st == 0).sum() > 100
    g1, p1, s1 = ctx.sample_batch(k, seed=11, site_base=5, lk=lk, flags=flags, want_post=False)
    g2, p2, s2 = ctx.sample_batch(k, seed=11, site_base=5, lk=lk, flags=flags, want_gt=False)
    assert p1 is None and g2 is None and same_bits((g1, s1, p2, s2), (gt, st, post, st))
    # the site-prior entry under the model's own rows: the plain entry's bits
    assert same_bits(ctx.sample_prior_batch(P.model_rows(model, flags), k, seed=11, site_base=5, lk=lk, flags=flags), (gt, post, st))
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    t_p = torch.full((333, k), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((333,), 55, dtype=torch.uint8, device=dev)
    raw = torch.full((333 * k * ped.n + 8,), 55, dtype=torch.int8, device=dev)
    for off in (0, 1, 3):
        raw.fill_(55)
        ctx.sample_batch_device(333, k, seed=11, site_base=5, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_samp_gt=raw.data_ptr() + off,
                                d_samp_post=t_p.data_ptr(), d_status=t_s.data_ptr())
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        assert np.array_equal(got[off:off + gt.size].reshape(gt.shape), gt)
        assert np.all(got[:off] == 55) and np.all(got[off + gt.size:] == 55)  # nothing outside the rows
        assert same_bits((t_p.cpu().numpy(), t_s.cpu().numpy()), (post, st))
    t_s.fill_(55)
    ctx.sample_batch_device(333, k, seed=11, site_base=5, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_status=t_s.data_ptr())  # status alone
    torch.cuda.synchronize()
    assert np.array_equal(t_s.cpu().numpy(), st)
    # one draw and the most an entry takes, on a batch one site longer than a workgroup
    most = ctx.sample_batch(256, seed=11, site_base=5, lk=lk[:65], flags=flags[:65])
    one = ctx.sample_batch(1, seed=11, site_base=5, lk=lk[:65], flags=flags[:65])
    assert same_bits(one, (most[0][:, :1], most[1][:, :1], most[2]))
    assert same_bits((most[0][:, :k], most[1][:, :k], most[2]), (gt[:65], post[:65], st[:65]))
    good = most[2] == 0
    assert np.all((most[0][good] >= 0) & (most[0][good] <= 2)) and np.all(most[0][~good] == -1)
    ctx.close()


def test_pl16_and_lk_give_the_same_bits():
    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()
    n = 500
    pl = rng.randint(0, 300, size=(n, len(seq), 3)).astype(np.uint16)
    pl[rng.rand(n, len(seq)) < 0.05] = fs.PL_MISSING
    flags = rng.randint(0, 4, n).astype(np.uint8)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    ctx = fs.Context(fs.make_model(ped))
    a = ctx.sample_batch(4, seed=1, pl16=pl, seq_members=seq, flags=flags)
    b = ctx.sample_batch(4, seed=1, lk=lk, flags=flags)
    ctx.close()
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)


def test_planted_failures():
    ped = fs.synthetic_pedigree("ped10")
    lk, flags = random_likelihoods(np.random.RandomState(9), ped, 256)
    lk = np.clip(lk, 1e-3, None)
    flags[:] = 0
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk[7, 0, :] = 0.0  # an all-zero row: the single-posterior rule
    lk[70] = 1.0       # every parent 0/0 for certain, the child 1/1 for certain, no mutation: no configuration has weight
    lk[70, :, 1:] = 0.0
    lk[70, child] = (0.0, 0.0, 1.0)
    ctx = fs.Context(fs.make_model(ped, mrate=0.0))
    gt, post, st = ctx.sample_batch(3, lk=lk, flags=flags)
    ctx.close()
    assert st[7] == 1 and st[70] == 2
    good = np.ones(256, bool)
    good[[7, 70]] = False
    assert np.all(st[good] == 0)
    assert np.all(gt[~good] == -1) and np.all(np.isnan(post[~good]))
    assert np.all((gt[good] >= 0) & (gt[good] <= 2)) and np.all(post[good] > 0)


def test_four_conditioned_members_are_refused():
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.sample_batch(2, lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.set_option("sample_kernels", 1)
    ctx.close()
