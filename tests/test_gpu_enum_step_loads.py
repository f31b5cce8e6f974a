"""The once-per-site form's loads one step ahead (csrc/enum_codegen.cpp, FAMSEQ_LANE_PRE) on the device.

Two contexts on the ten-member benchmark pedigree, one lane per site at any batch size: one generated with the default (entries
and LDS reads of the innermost loop a step ahead), one with FAMSEQ_LANE_PRE=0 (the text before: every load where it is used).
The variable is read when the kernel is generated, so each context has a kernel cache directory of its own.  Only where loads
are issued differs between the two texts: their outputs must be the same bits, and both must agree with the CPU oracle — status
byte and single posterior bit-exact, posteriors to RTOL."""
import os

import numpy as np
import pytest

import famseq_amd as fs
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ONCE = "prefix tables and marginals once per site"
PARENT_OBJECT = "9a2b09063e603740"  # the text before this change (ten members, lane variant 4)
UNIQUE = 320  # distinct sites the oracle answers


@pytest.fixture(scope="module")
def ped10():
    ped = fs.synthetic_pedigree("ped10")
    mo, fa = ped.relations()
    lk, flags = fs.synth.gen_batch(mo, fa, UNIQUE, 2)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    return ped, lk, flags, ref


@pytest.fixture(scope="module")
def contexts(ped10, tmp_path_factory):
    """(default text, FAMSEQ_LANE_PRE=0 text): contexts whose kernels are generated and loaded here."""
    ped = ped10[0]
    mp = pytest.MonkeyPatch()
    made = []
    try:
        for pre in (None, "0"):
            mp.setenv("FAMSEQ_KERNEL_CACHE", str(tmp_path_factory.mktemp("pre_" + (pre or "default"))))
            if pre is None:
                mp.delenv("FAMSEQ_LANE_PRE", raising=False)
            else:
                mp.setenv("FAMSEQ_LANE_PRE", pre)
            ctx = fs.Context(fs.make_model(ped), enum_impl=1)
            made.append(ctx)
            lk, flags = ped10[1][:1], ped10[2][:1]
            ctx.bn_batch(lk, flags)  # generates, compiles and loads the kernel under this setting
    finally:
        mp.undo()
    plans = [c.plan() for c in made]
    for p in plans:
        assert p["enum_group_digits_last"] == 0 and p["enum_lane_variant"] == 4 and ONCE in p["enum_lane_shape"]
        assert p["enum_lane_blocks_per_cu"] == 4
    names = [os.path.basename(p["enum_lane_code_object"]) for p in plans]
    assert names[1] == PARENT_OBJECT + ".hsaco" and names[0] != names[1]
    yield made
    for c in made:
        c.close()


def check(got, ref, what):
    post, single, st = got
    rpost, rsingle, rst = ref
    assert np.array_equal(st, rst), what
    ok, s_ok = (rst & 3) == 0, (rst & 3) != 1
    assert np.array_equal(single[s_ok].view(np.uint64), np.ascontiguousarray(rsingle[s_ok]).view(np.uint64)), what
    np.testing.assert_allclose(post[ok], rpost[ok], rtol=RTOL, atol=0, err_msg=what)
    assert np.all(np.isnan(post[~ok])) and np.all(np.isnan(single[~s_ok])), what


def both(contexts, lk, flags, ref, what):
    new, old = (c.bn_batch(lk, flags) for c in contexts)
    for a, b, name in zip(new, old, ("post", "single", "status")):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        same = np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)
        assert same, "%s: %s differs between the two texts" % (what, name)
    for c in contexts:
        assert c.plan()["enum_group_digits_last"] == 0  # one lane per site served the call
    check(new, ref, what)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 321])
def test_batch_sizes(ped10, contexts, n):
    """A single lane, a chunk short by one, exactly one chunk, a chunk plus one, five chunks with a ragged last."""
    _, lk0, fl0, ref0 = ped10
    idx = np.arange(n) % UNIQUE
    both(contexts, np.ascontiguousarray(lk0[idx]), np.ascontiguousarray(fl0[idx]), tuple(x[idx] for x in ref0), "n = %d" % n)


def test_both_chrx_passes_in_every_wave(ped10, contexts):
    """Known and chrX bits alternate inside every wave: both passes run, each primes its own carried entries."""
    ped, lk0, _, _ = ped10
    n = 128
    lk = np.ascontiguousarray(lk0[:n])
    flags = (np.arange(n) % 4).astype(np.uint8)
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    both(contexts, lk, flags, ref, "alternating flags")


def test_lanes_that_skip_the_body(ped10, contexts):
    """Every second lane skips the body: half of those are -LRC shortcut sites (every member sharp), half have a member with
    no possible genotype (failed single posterior: NaN rows)."""
    ped, lk0, fl0, _ = ped10
    n = 128
    lk, flags = lk0[:n].copy(), fl0[:n].copy()
    flags[::8] |= fs.FLAG_CHRX
    lk[1::4] = [1.0, 1e-17, 1e-20]
    lk[3::4, 9] = 0.0
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=8)
    assert np.all(ref[2][1::4] == 0x80) and np.all(ref[2][3::4] == 1) and (ref[2][::2] == 0).sum() > 32
    both(contexts, lk, flags, ref, "skipping lanes")
    post, single, _ = contexts[0].bn_batch(lk, flags)
    assert np.all(np.isnan(post[3::4])) and np.all(np.isnan(single[3::4]))
