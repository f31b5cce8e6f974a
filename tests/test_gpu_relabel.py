"""Relabelling evidence on the device: famseq_relabel_batch / famseq_relabel_prior_batch and their device entries through the
Python binding over the C ABI.  References and rules as in test_relabel_host.py: status exact, alt_loglik -inf exactly where the
reference's Z_a is exactly 0, elsewhere and for loglik an absolute 1e-9, failed sites NaN, bits where two routes must agree —
above all famseq_evidence_batch on the rows rearranged on the host, which every column equals bit for bit.  Every batch asserts
on the reference alone status 0 and Z and every non-zero Z_a >= 1e-200 before anything goes to the device, so no site is left out.

Shapes, the smallest at which the shell can go wrong: 1 site (a block of padding lanes but one), one less and one more than the
block, 3 BT + 5 sites against the reference (computed once per pedigree), 1,000 sites (that batch repeated: sixteen blocks, the
last partial) and a host call forced into several chunks, against the reference-checked rows bit for bit.  Flags 0..3 in turn,
so every wave holds all four.  Pedigrees: trio, the ten-member fixture (rows in the lanes' LDS rows), a looped random pedigree,
48 members (the lean form).
"""
import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd.prebuild_sets import wide_pedigree
from test_gpu_denovo import four_loops
from test_gpu_map import loop_pedigree
from test_map_host import clear_likelihoods
from test_pattern_host import cycled, same_bits
from test_relabel_host import batch_assign, check, clear, rearranged, reference

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """-> (ped, BT, lk, flags, assign, reference, Hardy-Weinberg rows, their reference): 3 BT + 5 clear sites, computed once."""
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
        assign = batch_assign(rng, ped.n)
        hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, len(lk)))
        ref = reference(ped, 1e-7, lk, flags, assign, brute=ped.n < 10)  # (the enumeration of ten members: test_relabel_host.py)
        href = reference(ped, 1e-7, lk, flags, assign, hwe) if name in ("trio", "wide48") else None
        for r in (ref, href):
            if r is not None:
                clear(r, name)
        _CASES[name] = (ped, bt, lk, flags, assign, ref, hwe, href)
    return _CASES[name]


def take(out, index):
    return tuple(x[index] for x in out)


def against_evidence(ctx, lk, flags, assign, out, prior=None):
    """Every column is the evidence entry's loglik on the rows rearranged on the host, bit for bit, wherever that call has status
    0; where it has status 2 on a good site Z_a is 0 and the column holds -inf.  -> the entries compared."""
    ev = (lambda rows: ctx.evidence_batch(lk=rows, flags=flags)) if prior is None else (lambda rows: ctx.evidence_prior_batch(prior, lk=rows, flags=flags))
    ll, _, st = ev(lk)
    assert np.array_equal(st, out[2]) and same_bits([out[1]], [ll])
    compared = 0
    for j, a in enumerate(assign):
        a_ll, _, a_st = ev(rearranged(lk, a))
        good = (a_st == 0) & (st == 0)
        assert same_bits([out[0][good, j]], [a_ll[good]])
        assert np.all(np.isneginf(out[0][(a_st == 2) & (st == 0), j]))
        compared += int(good.sum())
        if np.array_equal(a, np.arange(len(a))):
            assert same_bits([out[0][:, j]], [out[1]])
    return compared


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "wide48"])
def test_parity_and_site_counts(name):
    ped, bt, lk, flags, assign, ref, hwe, href = case(name)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    assert (ctx.plan()["elim_conditioned_members"] > 0) == (name == "loop")
    whole = ctx.relabel_batch(assign, lk=lk, flags=flags)
    assert whole[0].shape == (len(lk), len(assign)) and whole[1].shape == (len(lk),)
    check(whole, ref, name)
    assert same_bits(ctx.relabel_batch(assign, lk=lk, flags=flags), whole)  # the same batch twice
    assert against_evidence(ctx, lk, flags, assign, whole) > len(lk)
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.relabel_prior_batch(rows, assign, lk=lk, flags=flags), whole)  # the model's rows: the plain form's bits
    for n in (1, bt - 1, bt + 1):
        assert same_bits(ctx.relabel_batch(assign, lk=lk[:n], flags=flags[:n]), take(whole, slice(0, n)))
        assert same_bits(ctx.relabel_prior_batch(rows[:n], assign, lk=lk[:n], flags=flags[:n]), take(whole, slice(0, n)))
    # 1,000 sites: the batch over and over (the flags keep their turn: its length is 1 mod 4 ... so take them with the rows)
    idx = np.arange(1000) % len(lk)
    big = ctx.relabel_batch(assign, lk=lk[idx], flags=flags[idx])
    assert same_bits(big, take(whole, idx))
    ctx.set_option("chunk_sites", 2 * bt + 3)  # a host call in several chunks, the last one partial, through both slots
    assert same_bits(ctx.relabel_batch(assign, lk=lk[idx], flags=flags[idx]), big)
    assert same_bits(ctx.relabel_prior_batch(rows[idx], assign, lk=lk[idx], flags=flags[idx]), big)
    ctx.set_option("chunk_sites", 0)
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.relabel_batch(assign, lk=lk, flags=flags), whole)
    ctx.set_option("grid_blocks", 0)
    if href is not None:
        hout = ctx.relabel_prior_batch(hwe, assign, lk=lk, flags=flags)
        check(hout, href, name + ", Hardy-Weinberg rows")
        assert against_evidence(ctx, lk, flags, assign, hout, hwe) > len(lk)
    plan = ctx.plan()
    assert plan["relabel_code_object"].endswith(".hsaco") and 0 <= plan["relabel_variant"] < 4
    assert plan["relabel_prior_code_object"].endswith(".hsaco") and plan["relabel_prior_variant"] == plan["relabel_variant"]
    ctx.close()


@pytest.mark.parametrize("name", ["ped10", "wide48"])
def test_one_three_and_sixty_four_assignments(name):
    """A column does not depend on how many others the call holds or on what they are; the table of a call replaces the last call's."""
    ped, bt, lk, flags, assign, ref, _, _ = case(name)
    rng = np.random.RandomState(5)
    many = np.concatenate([assign, rng.randint(-1, ped.n, size=(fs.MAX_RELABEL - len(assign), ped.n)).astype(np.int32)])
    ctx = fs.Context(fs.make_model(ped))
    out = ctx.relabel_batch(many, lk=lk, flags=flags)
    assert out[0].shape == (len(lk), 64)
    check((out[0][:, :len(assign)], out[1], out[2]), ref, name + ", 64 assignments")
    assert not np.any(np.isnan(out[0])) and not np.any(np.isposinf(out[0]))
    for pick in ([63], [0], [40, 2, 17], list(range(len(assign)))):
        sub = ctx.relabel_batch(many[pick], lk=lk, flags=flags)
        assert same_bits(sub, (out[0][:, pick], out[1], out[2]))
    one_row = ctx.relabel_batch(many[4], lk=lk, flags=flags)  # a single row [N]
    assert same_bits(one_row, (out[0][:, [4]], out[1], out[2]))
    swaps, pairs = fs.swap_assignments(ped.n, range(min(ped.n, 11)))
    sw = ctx.relabel_batch(swaps, lk=lk, flags=flags)
    assert sw[0].shape[1] == len(pairs) and same_bits(sw[1:], out[1:]) and against_evidence(ctx, lk, flags, swaps[::7], (sw[0][:, ::7], sw[1], sw[2])) > 0
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
    assign = batch_assign(rng, ped.n)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    a = ctx.relabel_batch(assign, pl16=pl, seq_members=seq, flags=flags)
    b = ctx.relabel_batch(assign, lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.relabel_prior_batch(rows, assign, pl16=pl, seq_members=seq, flags=flags), b)
    dev = torch.device("cuda")
    t_pl, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(flags).to(dev)
    t_as = torch.from_numpy(assign).to(dev)
    t_a = torch.full((n, len(assign)), -1.0, dtype=torch.float64, device=dev)
    t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.relabel_device(n, t_as.data_ptr(), len(assign), d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(),
                             d_alt=t_a.data_ptr(), d_loglik=t_l.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert same_bits((t_a.cpu().numpy(), t_l.cpu().numpy(), t_s.cpu().numpy()), b)


def test_device_entries_on_a_stream_and_null_outputs():
    import torch

    ped, bt, lk, flags, assign, ref, hwe, _ = case("ped10")
    n, m = len(lk), len(assign)
    ctx = fs.Context(fs.make_model(ped))
    alt, ll, st = full = ctx.relabel_batch(assign, lk=lk, flags=flags)
    hfull = ctx.relabel_prior_batch(hwe, assign, lk=lk, flags=flags)
    assert not same_bits(hfull[:2], full[:2])
    a1, l1, s1 = ctx.relabel_batch(assign, lk=lk, flags=flags, want_loglik=False)
    a2, l2, s2 = ctx.relabel_batch(assign, lk=lk, flags=flags, want_alt=False)
    assert l1 is None and a2 is None and same_bits((a1, s1, l2, s2), (alt, st, ll, st))
    a3, l3, s3 = ctx.relabel_prior_batch(hwe, assign, lk=lk, flags=flags, want_alt=False, want_loglik=False)
    assert a3 is None and l3 is None and np.array_equal(s3, hfull[2])
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_lk, t_fl, t_as = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev), torch.from_numpy(assign).to(dev)
        t_pr = torch.from_numpy(hwe).to(dev)
        # an entry outside 0 .. N-1 reaches the kernel unchecked through the device entries: taken as -1
        wild, tame = assign.copy(), assign.copy()
        wild[0, 3], wild[1, 0], wild[2, ped.n - 1] = ped.n, -9, 2 ** 31 - 1
        tame[0, 3] = tame[1, 0] = tame[2, ped.n - 1] = -1
        t_wild = torch.from_numpy(wild).to(dev)
        for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
            for prior in (False, True):
                t_a = torch.full((n, m), -1.0, dtype=torch.float64, device=dev)
                t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
                t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
                out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_alt=t_a.data_ptr() if want[0] else 0,
                           d_loglik=t_l.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0, stream=stream.cuda_stream)
                if prior:
                    ctx.relabel_prior_device(n, t_pr.data_ptr(), t_as.data_ptr(), m, **out)
                else:
                    ctx.relabel_device(n, t_as.data_ptr(), m, **out)
                stream.synchronize()
                exp = hfull if prior else full
                assert same_bits([t_a.cpu().numpy()], [exp[0]]) if want[0] else bool((t_a == -1.0).all())
                assert same_bits([t_l.cpu().numpy()], [exp[1]]) if want[1] else bool((t_l == -1.0).all())
                assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
        t_a = torch.full((n, m), -1.0, dtype=torch.float64, device=dev)
        ctx.relabel_device(n, t_wild.data_ptr(), m, d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_alt=t_a.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert same_bits([t_a.cpu().numpy()], [ctx.relabel_batch(tame, lk=lk, flags=flags)[0]])
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_assign must be 1\.\.64"):
        ctx.relabel_device(n, t_as.data_ptr(), 65, d_lk=t_lk.data_ptr())
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*assign must be given"):
        ctx.relabel_device(n, 0, 1, d_lk=t_lk.data_ptr())
    ctx.close()


def test_planted_zeros_and_failures():
    """test_relabel_host's planted sites in batches of more than one workgroup: a Mendel-impossible exchange at mutation rate 0, a
    male handed a certain heterozygote's row on chrX, an all-zero row (status 1), the quad_mu0 shape (status 2), 1e160 rows."""
    ped = fs.synthetic_pedigree("quad")
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    father, mother = fa[child], mo[child]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[70, 1, :] = 0.0
    lk[75] = (1.0, 0.0, 0.0)
    lk[75, child] = (0.0, 0.0, 1.0)
    lk[80] = (0.0, 1.0, 0.0)  # hom-alt father, hom-ref mother, het children: possible as given, impossible with father and child exchanged
    lk[80, father] = (0.0, 0.0, 1.0)
    lk[80, mother] = (1.0, 0.0, 0.0)
    lk[85, mother] = (0.0, 1.0, 0.0)  # chrX: the mother a certain heterozygote
    flags[85] = 2
    swap = np.arange(ped.n, dtype=np.int32)
    swap[father], swap[child] = child, father
    give = np.arange(ped.n, dtype=np.int32)
    give[father] = mother
    assign = np.concatenate([batch_assign(np.random.RandomState(4), ped.n), swap[None], give[None]])
    ref = reference(ped, 0.0, lk, flags, assign)
    assert ref[2][70] == 1 and ref[2][75] == 2 and np.all(np.delete(ref[2], [70, 75]) == 0)
    assert ref[1][80, -2] == 0 and ref[1][80, 0] > 0 and ref[1][85, -1] == 0 and ref[1][85, 0] > 0
    model = fs.make_model(ped, mrate=0.0)
    ctx = fs.Context(model)
    for out in (ctx.relabel_batch(assign, lk=lk, flags=flags), ctx.relabel_prior_batch(P.model_rows(model, flags), assign, lk=lk, flags=flags)):
        check(out, ref, "planted zeros and failures")
        assert out[2][70] == 1 and out[2][75] == 2 and np.all(np.isnan(out[0][[70, 75]])) and np.all(np.isnan(out[1][[70, 75]]))
        assert np.isneginf(out[0][80, -2]) and np.isneginf(out[0][85, -1]) and np.isfinite(out[1][80]) and np.isfinite(out[1][85])
    big = np.full((bt_sites := 70, ped.n, 3), 1e160)
    alt, ll, st = ctx.relabel_batch(assign, lk=big, flags=np.zeros(bt_sites, np.uint8))
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(alt))
    bad = assign.copy()
    bad[2, 1] = ped.n
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*assignment 2, member 1 is %d" % ped.n):
        ctx.relabel_batch(bad, lk=lk, flags=flags)
    ctx.close()


def test_the_enumeration_engine_and_unserved_pedigrees():
    """A context on the enumeration engine answers as the other side products do; four conditioned members are refused."""
    ped, bt, lk, flags, assign, ref, _, _ = case("ped10")
    a = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ENUM)
    b = fs.Context(fs.make_model(ped), engine=fs.ENGINE_ELIM)
    assert same_bits(a.relabel_batch(assign, lk=lk, flags=flags), b.relabel_batch(assign, lk=lk, flags=flags))
    a.close()
    b.close()
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.relabel_batch(np.arange(ped.n, dtype=np.int32)[None], lk=np.ones((4, ped.n, 3)))
    ctx.close()
