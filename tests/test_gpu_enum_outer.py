"""The lane kernel's outer-leaf plan (csrc/enum_codegen.cpp, outer_leaf_shape; lane variants 8-11) on the device, and the
bulk slot that serves large one-lane-per-site batches with it (csrc/kernels.cpp, bulk_serves).

The ten-member benchmark pedigree against the CPU oracle as in test_gpu_enum_once.py: status byte and single posterior
bit-exact, posteriors to RTOL; the resident entry must give the host entry's bits.  The kernel itself runs through
pick_lane = 8 with enum_impl = 1 (exactly the lane kernel, at any batch size); the selection through a default context
whose bulk_min_sites is lowered to the test's sizes, and once at the default threshold."""
import numpy as np
import pytest

import famseq_amd as fs
import oracle
import _variants as V
from test_gpu_enum_once import check, resident

pytestmark = pytest.mark.gpu

OUTER = "outer-leaf plan"
UNIQUE = 384  # distinct sites the oracle answers; the large batch repeats the first 320


@pytest.fixture(scope="module")
def ped10():
    """(pedigree, lk, flags, oracle's answer) for UNIQUE sites; the Known bit as generated, no chrX."""
    ped = fs.synthetic_pedigree("ped10")
    mo, fa = ped.relations()
    lk, flags = fs.synth.gen_batch(mo, fa, UNIQUE, 2)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    return ped, lk, flags, ref


def outer_ctx(ped):
    """A context that runs variant 8 through the lane kernel's own slot at any batch size.  The pick is a note in the kernel
    cache that every later context for the pedigree would start from: it is put back, to the variant a context loads today,
    as soon as this one has loaded its kernel."""
    model = fs.make_model(ped)
    probe = fs.Context(model, device=-1)
    probe.set_option("enum_impl", 1)
    before = probe.plan()["enum_lane_variant"]
    ctx = fs.Context(model)
    try:
        ctx.set_option("pick_lane", 8)
        ctx.set_option("enum_impl", 1)
    finally:
        probe.set_option("pick_lane", before)
        probe.close()
    plan = ctx.plan()
    assert plan["enum_lane_variant"] == 8 and OUTER in plan["enum_lane_shape"]
    assert plan["enum_lane_shape"].startswith("looped members [3 0 1], unrolled block [4 2 6 7 5 8 9]")
    assert plan["enum_lane_blocks_per_cu"] == 4  # its LDS rows leave room for a wave on every SIMD, as variant 4's do
    return ctx


def run_both(ctx, lk, flags, ref, what, kind="lane"):
    got = ctx.bn_batch(lk, flags)
    plan = ctx.plan()
    assert plan["enum_last_kind"] == kind and plan["enum_group_digits_last"] == 0, what
    check(got, ref, what)
    ok = (ref[2] & 3) == 0
    nz = ref[0][ok] > 0
    print("%s: largest relative deviation %.3e" % (what, np.max(np.abs(got[0][ok][nz] - ref[0][ok][nz]) / ref[0][ok][nz])))
    again = resident(ctx, lk, flags)
    assert ctx.plan()["enum_last_kind"] == kind, what
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True), what
    return got


@pytest.mark.parametrize("n", [256, 257, 319])
def test_whole_and_partial_chunks(ped10, n):
    ped, lk, flags, ref = ped10
    ctx = outer_ctx(ped)
    run_both(ctx, lk[:n], flags[:n], tuple(x[:n] for x in ref), "n = %d" % n)
    ctx.close()


def test_known_and_chrx_mixed_in_every_wave(ped10):
    """All four (Known, chrX) combinations next to each other: both chrX passes run in every wave, and each builds the
    super-leaf table from that pass's transmission entries."""
    ped, lk, _, _ = ped10
    n = 257
    flags = (np.arange(n) % 4).astype(np.uint8)
    flags[1::7] ^= 2
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk[:n], flags, threads=8)
    ctx = outer_ctx(ped)
    run_both(ctx, lk[:n], flags, ref, "mixed flags")
    ctx.close()


def test_lanes_that_skip_the_body(ped10):
    """-LRC shortcut sites and failed single posteriors interleaved with sites that run the enumeration."""
    ped, lk, flags, _ = ped10
    n = 257
    lk, flags = lk[:n].copy(), flags[:n].copy()
    flags[::2] |= fs.FLAG_CHRX
    lk[::3] = [1.0, 1e-17, 1e-20]
    lk[1::5, 9] = 0.0
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    assert (ref[2] == 0x80).sum() > 60 and (ref[2] == 1).sum() > 30 and (ref[2] == 0).sum() > 100
    ctx = outer_ctx(ped)
    run_both(ctx, lk, flags, ref, "skipping lanes")
    ctx.close()


# ---- the selection ---------------------------------------------------------------------------------------------------------


def test_the_threshold_decides(ped10):
    """bulk_min_sites = 320 on a context with default options otherwise: 319 sites go wherever the batch size sends them
    (several lanes per site), 320 and 383 to the bulk object, one lane per site; the lane slot keeps variant 4.  A host call
    in small chunks goes the way of the whole call and gives the resident call's bits."""
    ped, lk, flags, ref = ped10
    ctx = fs.Context(fs.make_model(ped))
    ctx.set_option("bulk_min_sites", 320)
    for n, bulk in ((319, False), (320, True), (383, True)):
        got = ctx.bn_batch(lk[:n], flags[:n])
        plan = ctx.plan()
        assert (plan["enum_last_kind"] == "bulk") == bulk, n
        check(got, tuple(x[:n] for x in ref), "%d sites, threshold 320" % n)
        again = resident(ctx, lk[:n], flags[:n])
        assert (ctx.plan()["enum_last_kind"] == "bulk") == bulk, n
        for a, b in zip(got, again):
            assert np.array_equal(a, b, equal_nan=True), n
        if bulk:
            assert plan["enum_group_digits_last"] == 0 and plan["enum_bulk_variant"] == 8 and plan["enum_bulk_failed"] == 0
            assert plan["enum_bulk_code_object"].endswith(".hsaco") and plan["enum_bulk_min_sites"] == 320
            assert plan["enum_lane_variant"] == 4 and plan["enum_lane_shape"].startswith("looped members [5 0 1]")
            ctx.set_option("chunk_sites", 100)  # chunks of 100 sites and a short last one, each below the threshold
            chunked = ctx.bn_batch(lk[:n], flags[:n])
            assert ctx.plan()["enum_last_kind"] == "bulk"
            ctx.set_option("chunk_sites", 0)
            for a, b in zip(again, chunked):
                assert np.array_equal(a, b, equal_nan=True), n
    ctx.close()


@pytest.mark.parametrize("opt", [dict(enum_impl=1), dict(group_digits=0), dict(bulk_min_sites=-1)], ids=lambda o: "%s=%d" % list(o.items())[0])
def test_an_explicit_choice_is_not_overruled(ped10, opt):
    """enum_impl = 1 and group_digits = 0 are exactly the lane kernel at any size, and -1 switches the slot off."""
    ped, lk, flags, ref = ped10
    ctx = fs.Context(fs.make_model(ped))
    ctx.set_option("bulk_min_sites", 320)
    for k, v in opt.items():
        ctx.set_option(k, v)
    n = 383
    got = ctx.bn_batch(lk[:n], flags[:n])
    assert ctx.plan()["enum_last_kind"] != "bulk"
    check(got, tuple(x[:n] for x in ref), "%r" % opt)
    ctx.close()


def test_the_default_threshold_on_resident_arrays(ped10):
    """1,048,576 + 63 sites (320 distinct ones, repeated) through famseq_bn_batch_device with default options: the bulk
    object serves, the lane kernel's plan keys still describe variant 4, every row is the oracle's row for its site; one
    site fewer than the threshold is served by the lane kernel."""
    import torch

    ped, lk0, fl0, ref0 = ped10
    ctx = fs.Context(fs.make_model(ped))
    n_min = ctx.plan()["enum_bulk_min_sites"]
    assert n_min == 16 * 64 * ctx.plan()["cus"] * 4
    n = n_min + 63
    dev = torch.device("cuda", 0)
    idx = torch.arange(n, device=dev) % 320
    d_lk = torch.from_numpy(np.ascontiguousarray(lk0[:320])).to(dev)[idx].contiguous()
    d_fl = torch.from_numpy(np.ascontiguousarray(fl0[:320])).to(dev)[idx].contiguous()
    d_post, d_single = torch.empty_like(d_lk), torch.empty_like(d_lk)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ctx.bn_batch_device(n_min - 1, d_lk.data_ptr(), d_fl.data_ptr(), d_post.data_ptr(), d_single.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    assert ctx.plan()["enum_last_kind"] == "lane"
    ctx.bn_batch_device(n, d_lk.data_ptr(), d_fl.data_ptr(), d_post.data_ptr(), d_single.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    plan = ctx.plan()
    ctx.close()
    assert plan["enum_last_kind"] == "bulk" and plan["enum_lane_variant"] == 4 and plan["enum_bulk_variant"] == 8
    # equal sites give equal bits wherever they sit in the batch ...
    for d_out in (d_post, d_single):
        bits = d_out.view(torch.int64)
        assert torch.equal(bits, bits[:320][idx])
    assert torch.equal(d_st, d_st[:320][idx])
    # ... and the first 320 rows are the oracle's
    check((d_post[:320].cpu().numpy(), d_single[:320].cpu().numpy(), d_st[:320].cpu().numpy()), tuple(x[:320] for x in ref0), "default threshold")


# ---- the bulk slot on pedigrees other than the ten-member one ----------------------------------------------------------------

_OTHER = {}


def other(name):
    """(pedigree, lk, flags, has_bn_fail, oracle's answer) for UNIQUE sites of the variant matrices' batch (tests/_variants.py:
    every flag combination in every wave, the planted shortcut, failure, -LRC and tiny-row-sum sites), mutation rate 0."""
    if name not in _OTHER:
        ped = V.pedigree(name)
        lk, flags, has_bn_fail = V.variant_batch(ped, UNIQUE, seed=len(name))
        _OTHER[name] = (ped, lk, flags, has_bn_fail, V.reference(ped, lk, flags))
    return _OTHER[name]


@pytest.fixture
def own_cache(tmp_path, monkeypatch):
    """A kernel cache of the test's own: the lane picks below are notes that no other context may start from.  (Such a
    context consults that directory only, so the two or three kernels of a test are compiled where it runs.)"""
    monkeypatch.setenv("FAMSEQ_KERNEL_CACHE", str(tmp_path))


@pytest.mark.parametrize("pick", [4, 5, 6, 7])
@pytest.mark.parametrize("name", ["random1025", "random188"])
def test_the_bulk_slot_follows_the_lane_pick_on_other_pedigrees(name, pick, own_cache):
    """Nine members of which two carry no reads (in and beside the super-leaf) and seven members with a five-member block, under
    each lane pick of the once-per-site form: bulk_min_sites = 320 on a context with default options otherwise sends 319 sites
    wherever the batch size does, 320 and 383 to the bulk object, which is variant 8 + (pick & 3); the lane slot keeps the pick.
    Outputs against the oracle; the resident call and a host call in chunks below the threshold the host call's bits."""
    ped, lk, flags, has_bn_fail, ref = other(name)
    ctx = fs.Context(fs.make_model(ped, mrate=V.MRATE))
    try:
        ctx.set_option("pick_lane", pick)
        ctx.set_option("bulk_min_sites", 320)
        for n, bulk in ((319, False), (320, True), (383, True)):
            got = ctx.bn_batch(lk[:n], flags[:n])
            plan = ctx.plan()
            assert (plan["enum_last_kind"] == "bulk") == bulk, (n, plan["enum_last_kind"])
            V.check_against_reference(*got, tuple(x[:n] for x in ref), has_bn_fail, what="%s, lane pick %d: %d sites, threshold 320" % (name, pick, n))
            again = resident(ctx, lk[:n], flags[:n])
            assert (ctx.plan()["enum_last_kind"] == "bulk") == bulk, n
            assert V.same_bits(got, again), n
            if bulk:
                assert plan["enum_group_digits_last"] == 0 and plan["enum_bulk_variant"] == 8 + (plan["enum_lane_variant"] & 3) and plan["enum_bulk_failed"] == 0
                assert plan["enum_lane_variant"] == pick and plan["enum_bulk_min_sites"] == 320
                assert plan["enum_bulk_code_object"].endswith(".hsaco") and plan["enum_bulk_code_object"] != plan["enum_lane_code_object"]
                assert OUTER in plan["enum_bulk_shape"] and OUTER not in plan["enum_lane_shape"] and V.ONCE in plan["enum_lane_shape"]
                ctx.set_option("chunk_sites", 100)  # chunks of 100 sites and a short last one, each below the threshold
                chunked = ctx.bn_batch(lk[:n], flags[:n])
                assert ctx.plan()["enum_last_kind"] == "bulk"
                ctx.set_option("chunk_sites", 0)
                assert V.same_bits(again, chunked), n
                print("served by the bulk object: %s, members %d, lane pick %d, bulk variant %d, %d sites" % (name, ped.n, pick, plan["enum_bulk_variant"], n))
    finally:
        ctx.close()


def test_a_pedigree_without_the_cut_is_never_served_by_a_bulk_object(own_cache):
    """soak26 (a marriage loop; the once-per-site form, no outer-leaf text) with default options and a lowered threshold: at
    and above it a host call goes wherever the batch size sends it, and a resident call of one site per lane of a chip at
    one wave per SIMD — where the cost model of small batches takes one lane per site for every pedigree — runs on the lane
    kernel; there is no bulk object.  (The large batch repeats the UNIQUE sites by index, each row the oracle's for its site.)"""
    ped, lk, flags, has_bn_fail, ref = other("soak26")
    ctx = fs.Context(fs.make_model(ped, mrate=V.MRATE))
    try:
        ctx.set_option("bulk_min_sites", 320)
        for n in (320, 383):
            got = ctx.bn_batch(lk[:n], flags[:n])
            plan = ctx.plan()
            assert plan["enum_last_kind"] in ("lane", "group", "team") and plan["enum_bulk_code_object"] == "" and plan["enum_bulk_variant"] == -1, (n, plan["enum_last_kind"])
            V.check_against_reference(*got, tuple(x[:n] for x in ref), has_bn_fail, what="soak26: %d sites" % n)
            assert V.same_bits(got, resident(ctx, lk[:n], flags[:n])), n
        idx = np.arange(plan["cus"] * 256) % UNIQUE
        got = resident(ctx, np.ascontiguousarray(lk[idx]), np.ascontiguousarray(flags[idx]))
        plan = ctx.plan()
        assert plan["enum_last_kind"] == "lane" and plan["enum_group_digits_last"] == 0 and plan["enum_bulk_code_object"] == "" and plan["enum_bulk_failed"] == 0
        assert V.ONCE in plan["enum_lane_shape"] and OUTER not in plan["enum_lane_shape"]
        V.check_against_reference(*got, tuple(x[idx] for x in ref), has_bn_fail, what="soak26: %d sites" % len(idx))
    finally:
        ctx.close()
