"""The joint MAP configuration on the device: famseq_map_batch / famseq_map_batch_device through the C ABI.  Criteria as in
test_map_host.py: against the 3^N enumeration up to twelve members, against tests/_maxproduct.py beyond; the returned
configuration's weight within 1e-9 of the maximum (ties may resolve differently under another order of multiplication),
map_post at rtol 1e-9."""
import numpy as np
import pytest

import _maxproduct as mp
import famseq_amd as fs
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_gpu_denovo import four_loops
from test_map_host import NEAR_TIE, RTOL, brute_weights, check_failed_sites, clear_likelihoods, config_index

pytestmark = pytest.mark.gpu


def loop_pedigree(k):
    """The k-th random pedigree (3-9 members) that has a loop."""
    seeds = [s for s in range(0, 30, 3)]
    found = []
    for s in seeds:
        _, ped = random_pedigree(s)
        ctx = fs.Context(fs.make_model(ped), device=-1)
        if ctx.plan()["elim_conditioned_members"] > 0:
            found.append(s)
        ctx.close()
    return random_pedigree(found[k])


def small_cases():
    out = [(name, fs.synthetic_pedigree(name)) for name in ("trio", "quad", "ped5", "ped10")]
    out += [("loop%d" % k, loop_pedigree(k)[1]) for k in range(2)]
    return out


def check_against_enumeration(ped, mrate, lk, flags, gt, post, st, exact):
    G, W, ref_st = brute_weights(ped, mrate, lk, flags)
    assert np.array_equal(st, ref_st)
    check_failed_sites(gt, post, st)
    ok = st == 0
    assert ok.sum() > 0.5 * len(st)
    idx = config_index(gt[ok])
    w_ret, w_max = W[ok][np.arange(ok.sum()), idx], W[ok].max(axis=1)
    print("worst w_returned / w_max = %.17g" % (w_ret / w_max).min())
    assert np.all(w_ret >= (1 - 1e-9) * w_max)
    np.testing.assert_allclose(post[ok], w_max / W[ok].sum(axis=1), rtol=RTOL, atol=0)
    if exact:
        top2 = np.sort(W[ok], axis=1)[:, -2:]
        near = top2[:, 0] >= (1 - NEAR_TIE) * top2[:, 1]
        assert near.sum() <= 0.01 * ok.sum()
        assert np.array_equal(gt[ok][~near], G[:, np.argmax(W[ok], axis=1)].T[~near])


@pytest.mark.parametrize("mrate", [1e-7, 0.0])
@pytest.mark.parametrize("case", ["trio", "quad", "ped5", "ped10", "loop0", "loop1"])
def test_map_matches_the_enumeration(case, mrate):
    ped = dict(small_cases())[case]
    ped.relations()
    assert ped.n <= 12
    rng = np.random.RandomState(31)
    ctx = fs.Context(fs.make_model(ped, mrate=mrate))
    lk, flags = random_likelihoods(rng, ped, 192)
    gt, post, st = ctx.map_batch(lk=lk, flags=flags)
    check_against_enumeration(ped, mrate, lk, flags, gt, post, st, exact=False)
    lk, flags = clear_likelihoods(rng, ped, 192)
    gt, post, st = ctx.map_batch(lk=lk, flags=flags)
    ctx.close()
    check_against_enumeration(ped, mrate, lk, flags, gt, post, st, exact=True)


def check_against_helper(ped, mrate, lk, flags, gt, post, st):
    _, wmax, z, ref_st = mp.max_product(ped, mrate, lk, flags)
    check_failed_sites(gt, post, st)
    tiny = (ref_st != 1) & ~(z >= 1e-280)  # total mass below 1e-280: status only (and status 2 may fall on one side only)
    differ = (st == 0) != (ref_st == 0)
    assert np.all(tiny[differ]) and np.array_equal(st == 1, ref_st == 1)
    ok = (st == 0) & (ref_st == 0) & ~tiny
    assert ok.sum() > 20
    w_ret = mp.config_weight(ped, mrate, lk[ok], flags[ok], gt[ok])
    print("%d sites compared; worst w_returned / w_max = %.17g" % (ok.sum(), (w_ret / wmax[ok]).min()))
    assert np.all(w_ret >= (1 - 1e-9) * wmax[ok])
    np.testing.assert_allclose(post[ok], w_ret / z[ok], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", ["ped15", 24, 64])
def test_map_matches_the_helper(name):
    if isinstance(name, str):
        ped = fs.synthetic_pedigree(name)
        lk, flags = random_likelihoods(np.random.RandomState(15), ped, 256)
    else:
        ped = wide_pedigree(name)
        lk, flags = random_likelihoods(np.random.RandomState(name), ped, 256, max_pl=40)
    ped.relations()
    ctx = fs.Context(fs.make_model(ped))
    gt, post, st = ctx.map_batch(lk=lk, flags=flags)
    ctx.close()
    check_against_helper(ped, 1e-7, lk, flags, gt, post, st)


def ped10_batch(n, seed=3):
    ped = fs.synthetic_pedigree("ped10")
    lk, flags = random_likelihoods(np.random.RandomState(seed), ped, n)
    return ped, lk, flags


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


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
    whole = ctx.map_batch(lk=lk, flags=flags)  # the default chunking: several chunks at this size
    check_failed_sites(*whole)
    for k in (1, 63, 64, 65, 1000):
        assert same_bits(ctx.map_batch(lk=lk[:k], flags=flags[:k]), [x[:k] for x in whole])
    ctx.set_option("chunk_sites", n)  # one launch for the whole batch: n / (64 * resident workgroups) >= 3 trips per workgroup
    assert same_bits(ctx.map_batch(lk=lk, flags=flags), whole)
    ctx.set_option("chunk_sites", 128)
    assert same_bits(ctx.map_batch(lk=lk[:1000], flags=flags[:1000]), [x[:1000] for x in whole])
    ctx.close()
    check_against_enumeration(ped, 1e-4, lk[:96], flags[:96], *[x[:96] for x in whole], exact=False)


def test_odd_member_count_rows_are_packed_right():
    """N % 4 != 0 takes the byte-staged form of the genotype rows; a batch whose first byte is not 4-aligned the byte stores."""
    import torch

    ped = fs.synthetic_pedigree("ped5")
    lk, flags = random_likelihoods(np.random.RandomState(2), ped, 333)
    ctx = fs.Context(fs.make_model(ped))
    gt, post, st = ctx.map_batch(lk=lk, flags=flags)
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    raw = torch.full((333 * ped.n + 8,), 55, dtype=torch.int8, device=dev)
    for off in (0, 1, 3):
        raw.fill_(55)
        ctx.map_batch_device(333, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_map_gt=raw.data_ptr() + off)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        assert np.array_equal(got[off:off + 333 * ped.n].reshape(333, ped.n), gt)
        assert np.all(got[:off] == 55) and np.all(got[off + 333 * ped.n:] == 55)  # nothing outside the rows
    ctx.close()


def test_pl16_and_lk_give_the_same_bits():
    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    n = 500
    pl = rng.randint(0, 300, size=(n, len(seq), 3)).astype(np.uint16)
    pl[rng.rand(n, len(seq)) < 0.05] = fs.PL_MISSING
    flags = rng.randint(0, 4, n).astype(np.uint8)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    ctx = fs.Context(fs.make_model(ped))
    a = ctx.map_batch(pl16=pl, seq_members=seq, flags=flags)
    b = ctx.map_batch(lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    import torch

    dev = torch.device("cuda")
    t_pl, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(flags).to(dev)
    t_g = torch.full((n, ped.n), 55, dtype=torch.int8, device=dev)
    t_p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.map_batch_device(n, d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(), d_map_gt=t_g.data_ptr(),
                         d_map_post=t_p.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert same_bits((t_g.cpu().numpy(), t_p.cpu().numpy(), t_s.cpu().numpy()), b)


def test_device_entry_and_null_outputs():
    import torch

    ped, lk, flags = ped10_batch(1000, seed=5)
    ctx = fs.Context(fs.make_model(ped, mrate=1e-4))
    gt, post, st = ctx.map_batch(lk=lk, flags=flags)
    g1, p1, s1 = ctx.map_batch(lk=lk, flags=flags, want_post=False)
    g2, p2, s2 = ctx.map_batch(lk=lk, flags=flags, want_gt=False)
    g3, p3, s3 = ctx.map_batch(lk=lk, flags=flags, want_gt=False, want_post=False)
    assert p1 is None and g2 is None and g3 is None and p3 is None
    assert np.array_equal(g1, gt) and np.array_equal(p2.view(np.uint64), post.view(np.uint64))
    assert np.array_equal(s1, st) and np.array_equal(s2, st) and np.array_equal(s3, st)
    no_flags = ctx.map_batch(lk=lk[flags == 0])
    assert same_bits(no_flags, (gt[flags == 0], post[flags == 0], st[flags == 0]))
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
        t_g = torch.full((len(lk), ped.n), 55, dtype=torch.int8, device=dev)
        t_p = torch.full((len(lk),), -1.0, dtype=torch.float64, device=dev)
        t_s = torch.full((len(lk),), 55, dtype=torch.uint8, device=dev)
        ctx.map_batch_device(len(lk), d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_map_gt=t_g.data_ptr() if want[0] else 0,
                             d_map_post=t_p.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0)
        torch.cuda.synchronize()
        assert np.array_equal(t_g.cpu().numpy(), gt) if want[0] else bool((t_g == 55).all())
        assert np.array_equal(t_p.cpu().numpy().view(np.uint64), post.view(np.uint64)) if want[1] else bool((t_p == -1.0).all())
        assert np.array_equal(t_s.cpu().numpy(), st) if want[2] else bool((t_s == 55).all())
    ctx.close()
    ctx = fs.Context(fs.make_model(ped, mrate=1e-4))  # a second context on the same model: the same bits
    assert same_bits(ctx.map_batch(lk=lk, flags=flags), (gt, post, st))
    assert ctx.plan()["map_code_object"].endswith(".hsaco") and 0 <= ctx.plan()["map_variant"] < 4
    ctx.close()


def test_planted_failures():
    ped, lk, flags = ped10_batch(256, seed=9)
    lk = np.clip(lk, 1e-3, None)  # (no hard zeros, no 1e-40: at mutation rate 0 every other site keeps a configuration with weight)
    flags[:] = 0
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk[7, 0, :] = 0.0  # an all-zero row: the single-posterior rule
    lk[70] = 1.0       # every parent 0/0 for certain, the child 1/1 for certain, no mutation: no configuration has weight
    lk[70, :, 1:] = 0.0
    lk[70, child] = (0.0, 0.0, 1.0)
    ctx = fs.Context(fs.make_model(ped, mrate=0.0))
    gt, post, st = ctx.map_batch(lk=lk, flags=flags)
    ctx.close()
    assert st[7] == 1 and st[70] == 2
    good = np.ones(256, bool)
    good[[7, 70]] = False
    assert np.all(st[good] == 0)
    check_failed_sites(gt, post, st)


def test_four_conditioned_members_are_refused():
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.map_batch(lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.set_option("map_kernels", 1)
    ctx.close()
