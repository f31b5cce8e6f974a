"""Founder priors per site on the device (famseq_bn_prior_batch / _device through the Python binding), against the per-site
oracle of tests/_prior.py and against the plain sum-product kernel under the model's own rows."""
import numpy as np
import pytest

import _prior as P
import famseq_amd as fs

pytestmark = pytest.mark.gpu

PEDIGREES = ("trio", "quad", "ped10", "cousins", "wide24", "wide32", "wide48")
COUNTS = (1, 63, 64, 65, 1000)  # one lane, a wave less one, a whole wave, a wave and a lane, many workgroups with a ragged tail

_REF = {}


def reference(name):
    """1000 sites of the pedigree and their per-site oracle (asserted well-conditioned), computed once; every test slices it.
    Beyond 24 members the host test's 200 sites five times over: among a thousand fresh sharp sites of a 48-member pedigree a
    few always carry posterior entries near 1e-300, which the oracle itself does not reproduce under a rescaling of its input
    (a chunk of 256 sites still starts at a different row of the 200 each time)."""
    if name not in _REF:
        ped = P.pedigree(name)
        lk, flags, prior = P.batch(ped, 1000 if ped.n <= 24 else 200)
        ref = P.reference(ped, lk, flags, prior)
        P.assert_well_conditioned(ped, lk, flags, prior, ref)
        if len(lk) < 1000:
            lk, flags, prior = (np.concatenate([a] * 5) for a in (lk, flags, prior))
            ref = tuple(np.concatenate([r] * 5) for r in ref)
        _REF[name] = (ped, lk, flags, prior, ref)
    return _REF[name]


@pytest.mark.parametrize("name", PEDIGREES)
def test_site_counts_against_the_per_site_oracle(name):
    ped, lk, flags, prior, ref = reference(name)
    ctx = fs.Context(fs.make_model(ped), device=0)
    for n in COUNTS:
        out = ctx.bn_prior_batch(lk[:n], prior[:n], flags[:n])
        P.check(out, tuple(r[:n] for r in ref), "%s, %d sites" % (name, n))
    whole = ctx.bn_prior_batch(lk, prior, flags)
    assert np.array_equal(ctx.bn_prior_batch(lk, prior, flags)[0], whole[0], equal_nan=True)  # two calls, the same bits
    plan = ctx.plan()
    assert plan["prior_code_object"].endswith(".hsaco") and 0 <= plan["prior_variant"] < 12
    ctx.set_option("chunk_sites", 256)  # four chunks, the last of 232 sites: the prior's offsets in the host pipeline
    for a, b in zip(ctx.bn_prior_batch(lk, prior, flags), whole):
        assert np.array_equal(a, b, equal_nan=True)
    ctx.close()
    assert set(np.unique(ref[2])) >= {0, 0x80}


@pytest.mark.parametrize("name", ("trio", "ped10", "wide32", "wide48"))
def test_device_entry_gives_the_host_entrys_bits(name):
    import torch

    ped, lk, flags, prior, _ = reference(name)
    ctx = fs.Context(fs.make_model(ped), device=0)
    want = ctx.bn_prior_batch(lk, prior, flags)
    d_lk, d_fl, d_pr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (lk, flags, prior))
    post, single = torch.full_like(d_lk, -1.0), torch.full_like(d_lk, -1.0)
    st = torch.full((len(lk),), 77, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.bn_prior_batch_device(len(lk), d_lk.data_ptr(), d_fl.data_ptr(), d_pr.data_ptr(), post.data_ptr(), single.data_ptr(), st.data_ptr(), s)
    torch.cuda.synchronize()
    for a, b in zip((post, single, st), want):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)
    # a prior array that is only 8-byte aligned, outputs the caller does not want
    raw = torch.zeros(prior.size + 1, dtype=torch.float64, device="cuda")
    raw[1:] = d_pr.reshape(-1)
    assert raw[1:].data_ptr() % 16 == 8
    post2 = torch.full_like(d_lk, -1.0)
    ctx.bn_prior_batch_device(len(lk), d_lk.data_ptr(), d_fl.data_ptr(), raw[1:].data_ptr(), post2.data_ptr(), 0, 0, s)
    torch.cuda.synchronize()
    assert np.array_equal(post2.cpu().numpy(), want[0], equal_nan=True)
    ctx.close()


@pytest.mark.parametrize("name", ("trio", "quad", "ped10", "cousins", "wide24", "wide32", "wide48"))
def test_model_constant_rows_give_bn_batchs_bits(name):
    ped, lk, flags, _, _ = reference(name)
    model = fs.make_model(ped)
    plain = fs.Context(model, device=0, engine=fs.ENGINE_ELIM)
    want = plain.bn_batch(lk, flags)
    got = plain.bn_prior_batch(lk, P.model_rows(model, flags), flags)  # the same context serves both
    assert plain.plan()["prior_variant"] == plain.plan()["elim_variant"]
    plain.close()
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)


def test_a_context_on_the_enumeration_engine_serves_the_call():
    ped, lk, flags, prior, ref = reference("ped10")
    ctx = fs.Context(fs.make_model(ped), device=0)
    assert ctx.plan()["engine"] == fs.ENGINE_ENUM
    P.check(ctx.bn_prior_batch(lk[:300], prior[:300], flags[:300]), tuple(r[:300] for r in ref))
    assert ctx.plan()["engine"] == fs.ENGINE_ENUM
    post, single, status = ctx.bn_prior_batch(lk[:70], prior[:70], flags[:70], want_single=False, want_status=False)
    assert single is None and status is None
    np.testing.assert_allclose(post[(ref[2][:70] & 3) == 0], ref[0][:70][(ref[2][:70] & 3) == 0], rtol=P.RTOL, atol=0)
    ctx.close()


def test_arguments():
    ped, lk, flags, prior, _ = reference("trio")
    ctx = fs.Context(fs.make_model(ped), device=0)
    bad = prior[:8].copy()
    bad[3, 1] = -0.5
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*finite and >= 0 \(site 3\)"):
        ctx.bn_prior_batch(lk[:8], bad, flags[:8])
    bad[3, 1] = np.nan
    with pytest.raises(fs.FamseqError, match=r"\(-1\)"):
        ctx.bn_prior_batch(lk[:8], bad, flags[:8])
    ok = prior[:8].copy()
    ok[:, 3:] = np.nan  # the male chrX row is not read off chrX
    out = ctx.bn_prior_batch(lk[:8], ok, np.zeros(8, np.uint8))
    assert np.array_equal(out[0], ctx.bn_prior_batch(lk[:8], prior[:8], np.zeros(8, np.uint8))[0], equal_nan=True)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*prior must be given"):
        ctx._check(fs.lib().famseq_bn_prior_batch(ctx._h, 1, fs._p(lk[:1].copy(), fs.C.c_double), None, None, fs._p(np.empty((1, 3, 3)), fs.C.c_double),
                                                  None, None), "famseq_bn_prior_batch")
    assert ctx.bn_prior_batch(lk[:0], prior[:0], flags[:0])[0].shape == (0, ped.n, 3)
    ctx.close()


def test_a_pedigree_the_engine_does_not_serve_is_refused():
    from test_gpu_denovo import four_loops

    ped = four_loops()  # four loops that need a conditioned member each: one more than the engine takes
    ctx = fs.Context(fs.make_model(ped), device=0)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*site priors.*more than three"):
        ctx.bn_prior_batch(np.ones((2, ped.n, 3)), fs.hwe_priors([0.1, 0.2]))
    ctx.close()
