"""What the side products' entries take beside the common arguments (masks, assignments, rates, weights, start values; the
sampling entries' seed and site_base; the origin kernels' allele rows) reaches the kernels through one staging block and one
buffer per product (csrc/capi.cpp stage_extra, famseq_ctx::d_extra) and, chunk by chunk, through side_batch's PerChunk.  What
that can get wrong and the products' own tests do not ask: a product's table landing in, or read from, another product's buffer;
a table of an earlier call (or the caller's array, overwritten after the call) being read by a later one; a chunk of a host call
getting another chunk's site_base or start values.

Two pedigrees, the trio and synth.py's ped5 (N % 4 != 0), 203 sites, host calls in chunks of 67 (four chunks, the last one
partial, through both slots).  Everything is compared bit for bit: a call on the context that has served the other products with
the same call on a fresh context, and a host entry with the device entry in one launch on tables the test uploads."""
import functools

import numpy as np
import pytest

import famseq_amd as fs
from famseq_amd.synth import random_likelihoods

pytestmark = pytest.mark.gpu

S, CHUNK = 203, 67
PEDS = ["trio", "ped5"]


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pedigree, lk, flags, Hardy-Weinberg prior rows): shared, never written."""
    ped = fs.synthetic_pedigree(name)
    rng = np.random.RandomState(21)
    lk, flags = random_likelihoods(rng, ped, S)
    hwe = fs.hwe_priors(rng.uniform(0.01, 0.6, S))
    for a in (lk, flags, hwe):
        a.setflags(write=False)
    return ped, lk, flags, hwe


def context(name, chunk=CHUNK):
    ctx = fs.Context(fs.make_model(case(name)[0], mrate=1e-4))
    ctx.set_option("chunk_sites", chunk)
    return ctx


def tables(ped, product, count, seed):
    """A product's table for `count` passes, as its host entry takes it."""
    rng = np.random.RandomState(1000 * seed + count)
    return {"pattern": lambda: rng.randint(1, 8, size=(count, ped.n)).astype(np.uint8),
            "relabel": lambda: rng.randint(-1, ped.n, size=(count, ped.n)).astype(np.int32),
            "weight": lambda: rng.uniform(0.0, 2.0, size=(count, ped.n, 3)),
            "mutrate": lambda: rng.uniform(0.0, 0.01, size=count)}[product]()


# the calls of test 1, in their order: (product, with the site prior, count, seed of the table)
SEQUENCE = [("pattern", False, 3, 1), ("pattern", True, 3, 1), ("relabel", False, 2, 2), ("weight", False, 4, 3), ("mutrate", False, 3, 4),
            ("pattern", False, 1, 5), ("weight", False, 1, 6)]


def host_call(ctx, name, product, site_prior, table):
    ped, lk, flags, hwe = case(name)
    fn = getattr(ctx, "%s%s_batch" % (product, "_prior" if site_prior else ""))
    return fn(*((hwe,) if site_prior else ()), table, lk=lk, flags=flags)


def device_call(ctx, name, product, site_prior, table):
    """The device entry in one launch, on a table the test uploads (mutrate: the factor tables of the rates, rate_tables())."""
    import torch

    ped, lk, flags, hwe = case(name)
    dev = torch.device("cuda")
    t_lk, t_fl, t_pr = torch.from_numpy(lk.copy()).to(dev), torch.from_numpy(flags.copy()).to(dev), torch.from_numpy(hwe.copy()).to(dev)
    t_tab = torch.from_numpy(ctx.rate_tables(table) if product == "mutrate" else table).to(dev)
    count = len(table)
    t_a = torch.full((S, count), -1.0, dtype=torch.float64, device=dev)
    t_b = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((S,), 55, dtype=torch.uint8, device=dev)
    stem = {"pattern": "pattern%s_batch_device", "relabel": "relabel%s_device", "weight": "weight%s_device", "mutrate": "mutrate%s_device"}[product]
    fn = getattr(ctx, stem % ("_prior" if site_prior else ""))
    out = {"pattern": "d_pat_post", "relabel": "d_alt", "weight": "d_wt_loglik", "mutrate": "d_rate_loglik"}[product]
    fn(S, *((t_pr.data_ptr(),) if site_prior else ()), t_tab.data_ptr(), count, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(),
       d_loglik=t_b.data_ptr(), d_status=t_s.data_ptr(), **{out: t_a.data_ptr()})
    torch.cuda.synchronize()
    return t_a.cpu().numpy(), t_b.cpu().numpy(), t_s.cpu().numpy()


@functools.lru_cache(maxsize=None)
def fresh(name, product, site_prior, count, seed):
    """The call on a context that has served nothing else (unchunked: one launch)."""
    ctx = context(name, chunk=0)
    out = host_call(ctx, name, product, site_prior, tables(case(name)[0], product, count, seed))
    ctx.close()
    assert (out[2] == 0).sum() > S // 2
    return out


@pytest.mark.parametrize("overwrite", [False, True], ids=["arrays kept", "arrays overwritten after each call"])
@pytest.mark.parametrize("name", PEDS)
def test_buffers_do_not_cross_products(name, overwrite):
    """One context serves pattern (3), pattern with site priors (3), relabel (2), weight (4), mutrate (3), pattern (1, other masks)
    and weight (1) in turn: each the bits of a fresh context's and of the device entry's.  overwrite: the caller's array is
    filled with another valid table as soon as the host entry has returned, and the next call brings a new one."""
    ped = case(name)[0]
    ctx = context(name)
    for product, site_prior, count, seed in SEQUENCE:
        table = tables(ped, product, count, seed)
        kept = table.copy()
        want = fresh(name, product, site_prior, count, seed)
        got = host_call(ctx, name, product, site_prior, table)
        if overwrite:
            table[...] = tables(ped, product, count, seed + 50)
        assert same_bits(got, want), (product, site_prior, count)
        assert same_bits(device_call(ctx, name, product, site_prior, kept), want), (product, site_prior, count, "device")
    # ... and the first call again, after all the others
    product, site_prior, count, seed = SEQUENCE[0]
    assert same_bits(host_call(ctx, name, product, site_prior, tables(ped, product, count, seed)), fresh(name, product, site_prior, count, seed))
    ctx.close()


@pytest.mark.parametrize("site_prior", [False, True], ids=["plain", "site priors"])
@pytest.mark.parametrize("name", PEDS)
def test_every_chunk_gets_its_own_site_base(name, site_prior):
    """sample_batch at site_base 1000 in four chunks: the bits of one launch of the device entry with the same seed and site_base
    (a chunk that took the call's site_base, or another chunk's, would draw other numbers)."""
    import torch

    ped, lk, flags, hwe = case(name)
    k, seed, base = 3, 17, 1000
    ctx = context(name)
    lead = (hwe,) if site_prior else ()
    host = getattr(ctx, "sample_prior_batch" if site_prior else "sample_batch")(*lead, k, seed=seed, site_base=base, lk=lk, flags=flags)
    assert (host[2] == 0).sum() > S // 2
    dev = torch.device("cuda")
    t_lk, t_fl, t_pr = torch.from_numpy(lk.copy()).to(dev), torch.from_numpy(flags.copy()).to(dev), torch.from_numpy(hwe.copy()).to(dev)
    t_g = torch.full((S, k, ped.n), 55, dtype=torch.int8, device=dev)
    t_p = torch.full((S, k), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((S,), 55, dtype=torch.uint8, device=dev)
    io = dict(seed=seed, site_base=base, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_samp_gt=t_g.data_ptr(), d_samp_post=t_p.data_ptr(),
              d_status=t_s.data_ptr())
    if site_prior:
        ctx.sample_prior_batch_device(S, t_pr.data_ptr(), k, **io)
    else:
        ctx.sample_batch_device(S, k, **io)
    torch.cuda.synchronize()
    assert same_bits((t_g.cpu().numpy(), t_p.cpu().numpy(), t_s.cpu().numpy()), host)
    # (and the site's index is in the draw: the same call at another site_base gives other configurations)
    other = getattr(ctx, "sample_prior_batch" if site_prior else "sample_batch")(*lead, k, seed=seed, site_base=base + CHUNK, lk=lk, flags=flags)
    assert not np.array_equal(other[0], host[0])
    ctx.close()


@pytest.mark.parametrize("name", PEDS)
def test_every_chunk_gets_its_own_start_values(name):
    """af_batch in four chunks with a start value of its own at every site: the bits of one launch of the device entry."""
    import torch

    ped, lk, flags, hwe = case(name)
    af0 = np.random.RandomState(4).uniform(0.001, 0.9, S)
    assert len(np.unique(af0)) == S
    steps = 3
    ctx = context(name)
    host = ctx.af_batch(af0, steps, lk=lk, flags=flags)
    assert (host[2] == 0).sum() > S // 2
    dev = torch.device("cuda")
    t_lk, t_fl, t_af0 = torch.from_numpy(lk.copy()).to(dev), torch.from_numpy(flags.copy()).to(dev), torch.from_numpy(af0).to(dev)
    t_af = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
    t_ll = torch.full((S, 2), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((S,), 55, dtype=torch.uint8, device=dev)
    ctx.af_batch_device(S, t_af0.data_ptr(), steps, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_af=t_af.data_ptr(), d_loglik=t_ll.data_ptr(),
                        d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    assert same_bits((t_af.cpu().numpy(), t_ll.cpu().numpy(), t_s.cpu().numpy()), host)
    # no steps: every site's own start value comes back, chunk by chunk
    assert np.array_equal(ctx.af_batch(af0, 0, lk=lk, flags=flags)[0], af0)
    ctx.close()


@pytest.mark.parametrize("name", PEDS)
def test_the_origin_rows_are_built_once(name):
    """Two host calls and a device call on one context (the allele rows are uploaded by the first and kept): a fresh context's bits."""
    import torch

    ped, lk, flags, hwe = case(name)
    other = context(name, chunk=0)
    want = other.origin_batch(lk=lk, flags=flags)
    other.close()
    assert (want[2] == 0).sum() > S // 2
    ctx = context(name)
    assert same_bits(ctx.origin_batch(lk=lk, flags=flags), want)
    assert same_bits(ctx.origin_batch(lk=lk, flags=flags), want)
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk.copy()).to(dev), torch.from_numpy(flags.copy()).to(dev)
    t_o = torch.full(want[0].shape, -1.0, dtype=torch.float64, device=dev)
    t_h = torch.full(want[1].shape, -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((S,), 55, dtype=torch.uint8, device=dev)
    ctx.origin_device(S, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_origin=t_o.data_ptr(), d_hettx=t_h.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    assert same_bits((t_o.cpu().numpy(), t_h.cpu().numpy(), t_s.cpu().numpy()), want)
    # ... and a device call as the first use of a context
    first = context(name)
    t_o.fill_(-1.0), t_h.fill_(-1.0), t_s.fill_(55)
    first.origin_device(S, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_origin=t_o.data_ptr(), d_hettx=t_h.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    assert same_bits((t_o.cpu().numpy(), t_h.cpu().numpy(), t_s.cpu().numpy()), want)
    first.close()
    ctx.close()
