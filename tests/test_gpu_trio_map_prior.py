"""The trio and MAP kernels under site priors on the device (famseq_trio_prior_batch / famseq_map_prior_batch and their device
entries through the Python binding), against tests/_prior_joint.py — the numpy elimination over per-site-prior factors, pinned
there to the compiled oracle — and against the plain kernels under the model's own rows."""
import numpy as np
import pytest

import _prior as P
import _prior_joint as J
import famseq_amd as fs

pytestmark = pytest.mark.gpu

# trio: N % 4 != 0, the byte path of map_gt; quad: the word path; cousins: the conditioned body; wide48: the lean shell
PEDIGREES = ("trio", "quad", "ped10", "cousins", "wide32", "wide48")
COUNTS = (1, 63, 64, 65, 1000)  # one lane, a wave less one, a whole wave, a wave and a lane (the clamped tail), a ragged last block


def reference(name):
    """1000 sites of the pedigree and the helper's results.  Beyond 24 members the 200 checked sites five times over, as
    test_gpu_prior.py does (a chunk of 256 sites still starts at a different row of the 200 each time)."""
    n = 1000 if P.pedigree(name).n <= 24 else 200
    ped, lk, flags, prior, r = J.reference(name, n)
    if n < 1000:
        r = r.take(np.tile(np.arange(n), 5))
    return ped, r.lk, r.flags, r.prior, r


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", PEDIGREES)
def test_site_counts_against_the_helper(name):
    ped, lk, flags, prior, ref = reference(name)
    ctx = fs.Context(fs.make_model(ped), device=0)
    for n in COUNTS:
        sub = ref.take(slice(0, n))
        kids, joint, dnm, st = ctx.trio_prior_batch(prior[:n], lk=lk[:n], flags=flags[:n])
        assert kids.tolist() == J.children_of(ped)
        J.check_trio((joint, dnm, st), sub, "%s, %d sites" % (name, n))
        ok = st == 0  # the de novo mass of the joint under the mask
        np.testing.assert_allclose(dnm[ok], np.where(J.dnm_mask(ped, flags[:n]), joint, 0.0).sum(axis=2)[ok], rtol=J.RTOL, atol=0)
        compared = J.check_map(ctx.map_prior_batch(prior[:n], lk=lk[:n], flags=flags[:n]), sub, "%s, %d sites, MAP" % (name, n))
        assert compared >= 0.9 * n - 1
    whole_t = ctx.trio_prior_batch(prior, lk=lk, flags=flags)[1:]
    whole_m = ctx.map_prior_batch(prior, lk=lk, flags=flags)
    # the three output forms give one another's bits
    only_d = ctx.trio_prior_batch(prior, lk=lk, flags=flags, want_joint=False)[1:]
    only_j = ctx.trio_prior_batch(prior, lk=lk, flags=flags, want_dnm=False)[1:]
    assert only_d[0] is None and only_j[1] is None
    assert same_bits(only_d[1:], whole_t[1:]) and same_bits((only_j[0], only_j[2]), (whole_t[0], whole_t[2]))
    # two calls, the same bits
    assert same_bits(ctx.trio_prior_batch(prior, lk=lk, flags=flags)[1:], whole_t)
    assert same_bits(ctx.map_prior_batch(prior, lk=lk, flags=flags), whole_m)
    plan = ctx.plan()
    assert plan["trio_prior_code_object"].endswith(".hsaco") and plan["map_prior_code_object"].endswith(".hsaco")
    ctx.set_option("chunk_sites", 256)  # four chunks, the last of 232 sites: the prior's offsets in the host pipeline
    assert same_bits(ctx.trio_prior_batch(prior, lk=lk, flags=flags)[1:], whole_t)
    assert same_bits(ctx.map_prior_batch(prior, lk=lk, flags=flags), whole_m)
    ctx.close()


@pytest.mark.parametrize("name", ("trio", "quad", "ped10", "wide48"))
def test_device_entries_give_the_host_entries_bits(name):
    import torch

    ped, lk, flags, prior, _ = reference(name)
    n, k = len(lk), len(J.children_of(ped))
    ctx = fs.Context(fs.make_model(ped), device=0)
    want_t = ctx.trio_prior_batch(prior, lk=lk, flags=flags)[1:]
    want_m = ctx.map_prior_batch(prior, lk=lk, flags=flags)
    d_lk, d_fl = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (lk, flags))
    raw = torch.zeros(prior.size + 1, dtype=torch.float64, device="cuda")  # a prior array that is only 8-byte aligned
    raw[1:] = torch.from_numpy(prior).cuda().reshape(-1)
    d_pr = raw[1:].data_ptr()
    assert d_pr % 16 == 8
    s = torch.cuda.current_stream().cuda_stream
    joint = torch.full((n, k, 27), -1.0, dtype=torch.float64, device="cuda")
    dnm = torch.full((n, k), -1.0, dtype=torch.float64, device="cuda")
    st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    ctx.trio_prior_batch_device(n, d_pr, d_lk=d_lk.data_ptr(), d_flags=d_fl.data_ptr(), d_joint=joint.data_ptr(), d_dnm=dnm.data_ptr(),
                                d_status=st.data_ptr(), stream=s)
    gt = torch.full((n, ped.n), 55, dtype=torch.int8, device="cuda")
    post = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    st_m = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    ctx.map_prior_batch_device(n, d_pr, d_lk=d_lk.data_ptr(), d_flags=d_fl.data_ptr(), d_map_gt=gt.data_ptr(), d_map_post=post.data_ptr(),
                               d_status=st_m.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert same_bits((joint.cpu().numpy(), dnm.cpu().numpy(), st.cpu().numpy()), want_t)
    assert same_bits((gt.cpu().numpy(), post.cpu().numpy(), st_m.cpu().numpy()), want_m)
    # null outputs: the de novo posteriors alone (the dnm-only form), the genotypes alone; nothing else is written
    dnm2 = torch.full((n, k), -1.0, dtype=torch.float64, device="cuda")
    gt2 = torch.full((n, ped.n), 55, dtype=torch.int8, device="cuda")
    ctx.trio_prior_batch_device(n, d_pr, d_lk=d_lk.data_ptr(), d_flags=d_fl.data_ptr(), d_dnm=dnm2.data_ptr(), stream=s)
    ctx.map_prior_batch_device(n, d_pr, d_lk=d_lk.data_ptr(), d_flags=d_fl.data_ptr(), d_map_gt=gt2.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert same_bits((dnm2.cpu().numpy(), gt2.cpu().numpy()), (want_t[1], want_m[0]))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*d_prior must be given"):
        ctx.trio_prior_batch_device(n, 0, d_lk=d_lk.data_ptr(), d_dnm=dnm2.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*d_prior must be given"):
        ctx.map_prior_batch_device(n, 0, d_lk=d_lk.data_ptr(), d_map_gt=gt2.data_ptr())
    ctx.close()


def test_pl16_and_lk_give_the_same_bits():
    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    n = 500
    pl = rng.randint(0, 300, size=(n, len(seq), 3)).astype(np.uint16)
    pl[rng.rand(n, len(seq)) < 0.05] = fs.PL_MISSING
    flags = rng.randint(0, 4, n).astype(np.uint8)
    prior = fs.hwe_priors(10.0 ** rng.uniform(-6, -0.001, n))
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    ctx = fs.Context(fs.make_model(ped), device=0)
    a = ctx.trio_prior_batch(prior, pl16=pl, seq_members=seq, flags=flags)[1:]
    b = ctx.trio_prior_batch(prior, lk=lk, flags=flags)[1:]
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    a = ctx.map_prior_batch(prior, pl16=pl, seq_members=seq, flags=flags)
    b = ctx.map_prior_batch(prior, lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    ctx.close()


@pytest.mark.parametrize("name", PEDIGREES)
def test_model_constant_rows_give_the_plain_entries_bits(name):
    ped, lk, flags, _, _ = reference(name)
    model = fs.make_model(ped)
    rows = P.model_rows(model, flags)
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    ctx = fs.Context(model, device=0)  # the same context serves both
    assert same_bits(ctx.trio_prior_batch(rows, lk=lk, flags=flags)[1:], ctx.trio_batch(lk=lk, flags=flags)[1:])
    assert same_bits(ctx.map_prior_batch(rows, lk=lk, flags=flags), ctx.map_batch(lk=lk, flags=flags))
    plan = ctx.plan()
    assert 0 <= plan["trio_prior_variant"] == plan["trio_variant"] and 0 <= plan["map_prior_variant"] == plan["map_variant"]
    ctx.close()


def test_arguments():
    ped, lk, flags, prior, _ = reference("trio")
    ctx = fs.Context(fs.make_model(ped), device=0)
    for call in (ctx.trio_prior_batch, ctx.map_prior_batch):
        bad = prior[:8].copy()
        bad[3, 1] = -0.5
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*finite and >= 0 \(site 3\)"):
            call(bad, lk=lk[:8], flags=flags[:8])
        bad[3, 1] = np.inf
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*\(site 3\)"):
            call(bad, lk=lk[:8], flags=flags[:8])
        ok = prior[:8].copy()
        ok[:, 3:] = np.nan  # the male chrX row is not checked, or read, off chrX
        zero = np.zeros(8, np.uint8)
        assert same_bits(call(ok, lk=lk[:8], flags=zero)[-3:], call(prior[:8], lk=lk[:8], flags=zero)[-3:])
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*\(site 0\)"):
            call(ok, lk=lk[:8], flags=zero | fs.FLAG_CHRX)
        with pytest.raises(ValueError):
            call(prior[:7], lk=lk[:8])
        assert len(call(prior[:0], lk=lk[:0], flags=flags[:0])[-1]) == 0
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*prior must be given"):
        ctx._check(fs.lib().famseq_trio_prior_batch(ctx._h, 1, fs._p(lk[:1].copy(), fs.C.c_double), None, None, 0, None, None, None,
                                                    fs._p(np.empty(1), fs.C.c_double), None), "famseq_trio_prior_batch")
    ctx.close()


def test_a_pedigree_the_engine_does_not_serve_is_refused():
    from test_gpu_denovo import four_loops

    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped), device=0)
    for call in (ctx.trio_prior_batch, ctx.map_prior_batch):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            call(fs.hwe_priors([0.1, 0.2]), lk=np.ones((2, ped.n, 3)))
    for key in ("trio_prior_kernels", "map_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*site priors.*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
