"""The lane kernel's once-per-site form (csrc/enum_codegen.cpp, "The once-per-site form") on the device: the
ten-member benchmark pedigree, whose kernel takes it, at the batch shapes where it can go wrong, and the
fifteen-member one, against the CPU oracle as in test_gpu_parity.py — status byte and single posterior
bit-exact, posteriors to RTOL; the resident entry must give the host entry's bits."""
import numpy as np
import pytest

import famseq_amd as fs
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ONCE = "prefix tables and marginals once per site"
UNIQUE = 320  # distinct sites the oracle answers; larger batches repeat them


def check(got, ref, what):
    post, single, st = got
    rpost, rsingle, rst = ref
    assert np.array_equal(st, rst), what
    ok, s_ok = (rst & 3) == 0, (rst & 3) != 1
    assert np.array_equal(single[s_ok].view(np.uint64), rsingle[s_ok].view(np.uint64)), what
    np.testing.assert_allclose(post[ok], rpost[ok], rtol=RTOL, atol=0, err_msg=what)
    assert np.all(np.isnan(post[~ok])) and np.all(np.isnan(single[~s_ok])), what
    short = (rst & 0x80) != 0
    assert np.array_equal(post[short].view(np.uint64), rpost[short].view(np.uint64)), what


def resident(ctx, lk, flags):
    """The same call through famseq_bn_batch_device on arrays that live on the device."""
    import torch

    dev = torch.device("cuda", 0)
    d_lk, d_fl = torch.from_numpy(np.ascontiguousarray(lk)).to(dev), torch.from_numpy(np.ascontiguousarray(flags)).to(dev)
    d_post, d_single = torch.empty_like(d_lk), torch.empty_like(d_lk)
    d_st = torch.empty(len(flags), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.bn_batch_device(len(flags), d_lk.data_ptr(), d_fl.data_ptr(), d_post.data_ptr(), d_single.data_ptr(), d_st.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_post.cpu().numpy(), d_single.cpu().numpy(), d_st.cpu().numpy()


@pytest.fixture(scope="module")
def ped10():
    """(pedigree, lk, flags, oracle's answer) for UNIQUE sites; the Known bit as generated, no chrX."""
    ped = fs.synthetic_pedigree("ped10")
    mo, fa = ped.relations()
    lk, flags = fs.synth.gen_batch(mo, fa, UNIQUE, 2)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    return ped, lk, flags, ref


def lane_ctx(ped):
    """A context that runs the one-lane-per-site kernel at any batch size (the shapes below are about the kernel)."""
    return fs.Context(fs.make_model(ped), enum_impl=1)


def assert_once_form_served(ctx):
    plan = ctx.plan()
    assert plan["enum_group_digits_last"] == 0  # one lane per site
    assert plan["enum_lane_variant"] == 4  # the shipped pick: variant 0 in the once-per-site form
    assert ONCE in plan["enum_lane_shape"] and plan["enum_lane_shape"].startswith("looped members [5 0 1], unrolled block [4 2 6 7 3 8 9]")
    assert plan["enum_lane_code_object"].endswith(".hsaco")
    assert plan["enum_lane_blocks_per_cu"] == 4  # its LDS rows leave room for a wave on every SIMD


def test_ten_members_where_a_default_context_turns_to_one_lane_per_site(ped10):
    """A context with default options spreads a small batch over several lanes per site and takes the one-lane-per-site kernel
    from some batch size on.  That size is found here from what the plan reports after each call (bisection between 30 sites,
    81 lanes per site, and 400,000), asserted to be the switch, and the kernel is checked there: n, n + 1 and n + 63 sites (whole
    chunks and a partial last one).  The batches repeat UNIQUE distinct sites, each row compared with the oracle's."""
    ped, lk0, fl0, ref0 = ped10
    top = 400_000
    idx = np.arange(top + 63) % UNIQUE
    lk, flags = np.ascontiguousarray(lk0[idx]), np.ascontiguousarray(fl0[idx])
    ctx = fs.Context(fs.make_model(ped), chunk_sites=1 << 20)

    def digits(n):
        ctx.bn_batch(lk[:n], flags[:n], want_single=False, want_status=False)
        return ctx.plan()["enum_group_digits_last"]

    lo, hi = 30, top
    assert digits(lo) > 0 and digits(hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if digits(mid) == 0:
            hi = mid
        else:
            lo = mid
    n0 = hi
    assert digits(n0 - 1) > 0 and digits(n0) == 0  # the smallest batch the plan says runs one lane per site
    for n in (n0, n0 + 1, n0 + 63):
        got = ctx.bn_batch(lk[:n], flags[:n])
        assert_once_form_served(ctx)
        check(got, tuple(x[idx[:n]] for x in ref0), "n = %d" % n)
        again = resident(ctx, lk[:n], flags[:n])
        for a, b in zip(got, again):
            assert np.array_equal(a, b, equal_nan=True)
    ctx.close()


@pytest.mark.parametrize("n", [256, 257, 319])
def test_ten_members_whole_and_partial_chunks(ped10, n):
    ped, lk, flags, ref = ped10
    ctx = lane_ctx(ped)
    got = ctx.bn_batch(lk[:n], flags[:n])
    assert_once_form_served(ctx)
    check(got, tuple(x[:n] for x in ref), "n = %d" % n)
    again = resident(ctx, lk[:n], flags[:n])
    ctx.close()
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)


def test_ten_members_known_and_chrx_mixed_in_every_wave(ped10):
    """All four (Known, chrX) combinations next to each other: both chrX passes run in every wave, each on tables built
    for that pass in the rows of its own lanes."""
    ped, lk, _, _ = ped10
    n = 257
    flags = (np.arange(n) % 4).astype(np.uint8)
    flags[1::7] ^= 2
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk[:n], flags, threads=8)
    ctx = lane_ctx(ped)
    got = ctx.bn_batch(lk[:n], flags)
    assert_once_form_served(ctx)
    check(got, ref, "mixed flags")
    again = resident(ctx, lk[:n], flags)
    ctx.close()
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)


def test_ten_members_lanes_that_skip_the_body(ped10):
    """-LRC shortcut sites (every sequenced member sharp) and failed single posteriors (a member with no possible genotype)
    interleaved with sites that run the enumeration: lanes that skip the body must leave the others' rows alone."""
    ped, lk, flags, _ = ped10
    n = 257
    lk, flags = lk[:n].copy(), flags[:n].copy()
    flags[::2] |= fs.FLAG_CHRX
    lk[::3] = [1.0, 1e-17, 1e-20]
    lk[1::5, 9] = 0.0
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    assert (ref[2] == 0x80).sum() > 60 and (ref[2] == 1).sum() > 30 and (ref[2] == 0).sum() > 100
    ctx = lane_ctx(ped)
    got = ctx.bn_batch(lk, flags)
    assert_once_form_served(ctx)
    check(got, ref, "skipping lanes")
    again = resident(ctx, lk, flags)
    ctx.close()
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)


def test_fifteen_members_4096_sites():
    """Fifteen members run in the form the cost model takes for them.  The oracle needs a third of a second per site
    (3^15 configurations), so the 4,096 sites are sixteen distinct ones (every flag combination) in a shuffled order:
    every output row is compared with the oracle's row for its site."""
    ped = fs.synthetic_pedigree("ped15")
    mo, fa = ped.relations()
    lk16, fl16 = fs.synth.gen_batch(mo, fa, 16, 4)
    fl16 = ((fl16 & 1) | (2 * (np.arange(16) % 2))).astype(np.uint8)
    ref16 = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk16, fl16, threads=16)
    pick = np.random.RandomState(4096).randint(0, 16, 4096)
    lk, flags = np.ascontiguousarray(lk16[pick]), np.ascontiguousarray(fl16[pick])
    ctx = lane_ctx(ped)
    got = ctx.bn_batch(lk, flags)
    plan = ctx.plan()
    assert plan["enum_group_digits_last"] == 0 and plan["enum_lane_code_object"].endswith(".hsaco")
    check(got, tuple(x[pick] for x in ref16), "ped15")
    again = resident(ctx, lk, flags)
    ctx.close()
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)
