"""Leave-one-out posteriors and per-member fit on the device: famseq_loo_batch / famseq_loo_prior_batch and their device entries
through the C ABI, and `FamSeq vcf -loo`.  Reference and tolerances as in test_loo_host.py: tests/_loo.py, loo and fit at rtol
1e-9 with atol 0 (an exact 0 must be an exact 0), status exact, failed sites NaN, bits where two routes must agree; on the clear
batches used here the reference has status 0 and Z and every Z_-p >= 1e-200 (asserted on the reference alone, before anything
goes to the device), so no site is left out.

Shapes: the smallest that can still go wrong — 1, BT - 1 and 3 BT + 5 sites (a padding-lane-only block, a partial last chunk,
several loop trips of a workgroup where the grid is forced to one workgroup), at trio, ped10, a looped pedigree, 32 members
(registers-first, one wave) and 48 members (likelihoods re-read at each use)."""
import subprocess

import numpy as np
import pytest

import _loo as L
import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from famseq_amd.prebuild_sets import wide_pedigree
from test_cli_gpu import CLI, TD, run_cli
from test_gpu_denovo import four_loops
from test_gpu_evidence import phred, vcf_inputs
from test_gpu_map import loop_pedigree
from test_loo_host import cycled, same_bits
from test_map_host import clear_likelihoods

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """-> (ped, BT, lk, flags, reference, Hardy-Weinberg rows, their reference): 3 BT + 5 clear sites, computed once."""
    if name not in _CASES:
        ped = {"trio": lambda: fs.synthetic_pedigree("trio"), "ped10": lambda: fs.synthetic_pedigree("ped10"),
               "loop": lambda: loop_pedigree(0)[1], "wide32": lambda: wide_pedigree(32), "wide48": lambda: wide_pedigree(48)}[name]()
        ped.relations()
        ctx = fs.Context(fs.make_model(ped), device=-1)
        bt = ctx.plan()["loo_block_threads"]
        ctx.close()
        assert bt >= 2
        rng = np.random.RandomState(60 + ped.n)
        lk, _ = clear_likelihoods(rng, ped, 3 * bt + 5)
        flags = cycled(lk)
        hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, len(lk)))
        ref = L.analyse(ped, 1e-7, lk, flags)
        assert L.is_clear(ref)
        href = L.analyse(ped, 1e-7, lk, flags, hwe) if name in ("trio", "wide32") else None
        assert href is None or L.is_clear(href)
        _CASES[name] = (ped, bt, lk, flags, ref, hwe, href)
    return _CASES[name]


def take(out, n):
    return tuple(x[:n] for x in out)


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "wide32", "wide48"])
def test_parity_and_site_counts(name):
    L.pinned()
    ped, bt, lk, flags, ref, hwe, href = case(name)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    plan = ctx.plan()
    assert (plan["elim_conditioned_members"] > 0) == (name == "loop")
    whole = ctx.loo_batch(lk=lk, flags=flags)
    assert whole[0].shape == (len(lk), ped.n, 3) and whole[1].shape == (len(lk), ped.n)
    L.check(whole, ref, name)
    assert same_bits(ctx.loo_batch(lk=lk, flags=flags), whole)  # the same batch twice
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.loo_prior_batch(rows, lk=lk, flags=flags), whole)  # the model's rows: the plain form's bits
    for n in (1, bt - 1):
        assert same_bits(ctx.loo_batch(lk=lk[:n], flags=flags[:n]), take(whole, n))
        assert same_bits(ctx.loo_prior_batch(rows[:n], lk=lk[:n], flags=flags[:n]), take(whole, n))
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.loo_batch(lk=lk, flags=flags), whole)
    assert same_bits(ctx.loo_prior_batch(rows, lk=lk, flags=flags), whole)
    ctx.set_option("grid_blocks", 0)
    if href is not None:
        L.check(ctx.loo_prior_batch(hwe, lk=lk, flags=flags), href, name + ", Hardy-Weinberg rows")
    plan = ctx.plan()
    assert plan["loo_code_object"].endswith(".hsaco") and 0 <= plan["loo_variant"] < 4
    assert plan["loo_prior_code_object"].endswith(".hsaco") and plan["loo_prior_variant"] == plan["loo_variant"]
    assert plan["loo_block_threads"] == bt
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
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    a = ctx.loo_batch(pl16=pl, seq_members=seq, flags=flags)
    b = ctx.loo_batch(lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.loo_prior_batch(rows, pl16=pl, seq_members=seq, flags=flags), b)
    dev = torch.device("cuda")
    t_pl, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(flags).to(dev)
    t_l = torch.full((n, ped.n, 3), -1.0, dtype=torch.float64, device=dev)
    t_f = torch.full((n, ped.n), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.loo_batch_device(n, d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(), d_loo=t_l.data_ptr(), d_fit=t_f.data_ptr(),
                         d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert same_bits((t_l.cpu().numpy(), t_f.cpu().numpy(), t_s.cpu().numpy()), b)


def test_device_entries_and_null_outputs():
    import torch

    ped, bt, lk, flags, ref, hwe, _ = case("ped10")
    n = len(lk)
    ctx = fs.Context(fs.make_model(ped))
    loo, fit, st = full = ctx.loo_batch(lk=lk, flags=flags)
    hfull = ctx.loo_prior_batch(hwe, lk=lk, flags=flags)
    assert not same_bits(hfull[:2], full[:2])
    l1, f1, s1 = ctx.loo_batch(lk=lk, flags=flags, want_fit=False)
    l2, f2, s2 = ctx.loo_batch(lk=lk, flags=flags, want_loo=False)
    assert f1 is None and l2 is None and same_bits((l1, s1, f2, s2), (loo, st, fit, st))
    l3, f3, s3 = ctx.loo_prior_batch(hwe, lk=lk, flags=flags, want_loo=False, want_fit=False)
    assert l3 is None and f3 is None and np.array_equal(s3, hfull[2])
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    # the prior rows at a 16-byte aligned address and at one that is only 8-byte aligned
    raw = torch.zeros(6 * n + 2, dtype=torch.float64, device=dev)
    off = (raw.data_ptr() % 16) // 8
    t_pr = {16: raw[off:off + 6 * n], 8: raw[off + 1:off + 1 + 6 * n]}
    assert t_pr[16].data_ptr() % 16 == 0 and t_pr[8].data_ptr() % 16 == 8
    for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
        for align in (None, 16, 8):
            t_l = torch.full((n, ped.n, 3), -1.0, dtype=torch.float64, device=dev)
            t_f = torch.full((n, ped.n), -1.0, dtype=torch.float64, device=dev)
            t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
            out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_loo=t_l.data_ptr() if want[0] else 0,
                       d_fit=t_f.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0)
            if align is None:
                ctx.loo_batch_device(n, **out)
            else:
                t_pr[align].copy_(torch.from_numpy(hwe.reshape(-1)).to(dev))
                ctx.loo_prior_batch_device(n, t_pr[align].data_ptr(), **out)
            torch.cuda.synchronize()
            exp = full if align is None else hfull
            assert same_bits([t_l.cpu().numpy()], [exp[0]]) if want[0] else bool((t_l == -1.0).all())
            assert same_bits([t_f.cpu().numpy()], [exp[1]]) if want[1] else bool((t_f == -1.0).all())
            assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
    ctx.close()


def test_planted_cases():
    """test_loo_host.test_planted_cases' sites on a trio at mutation rate 0, in a batch of more than one workgroup."""
    ped = fs.synthetic_pedigree("trio")
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    for site, row in ((70, (0.0, 1.0, 0.0)), (75, (0.0, 0.0, 1.0))):
        lk[site] = (1.0, 0.0, 0.0)  # both parents hom-ref for certain
        lk[site, child] = row       # the child het (site 70: every fit 0.0) / hom-alt (site 75: the mother's cavity has no weight)
    lk[7, 1, :] = 0.0               # an all-zero row: the single-posterior rule
    lk[80, child, 1] = 0.0          # single exact zeros where the cavity is positive
    lk[80, mo[child], 0] = 0.0
    ref = L.analyse(ped, 0.0, lk, flags)
    assert list(ref.status[[7, 70, 75, 80]]) == [1, 0, 2, 0] and np.all(np.delete(ref.status, [7, 75]) == 0)
    model = fs.make_model(ped, mrate=0.0)
    ctx = fs.Context(model)
    for out in (ctx.loo_batch(lk=lk, flags=flags), ctx.loo_prior_batch(P.model_rows(model, flags), lk=lk, flags=flags)):
        loo, fit, st = out
        L.check(out, ref, "planted cases", clear=False)
        assert list(st[[7, 70, 75, 80]]) == [1, 0, 2, 0]
        assert np.all(fit[70] == 0.0) and np.all(np.isfinite(loo[70])) and np.abs(loo[70].sum(axis=1) - 1.0).max() < 1e-12
        assert loo[80, child, 1] > 0 and loo[80, mo[child], 0] > 0 and np.all(fit[80] > 0)
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*site 3"):
        bad = P.model_rows(model, flags)
        bad[3, 1] = -1.0
        ctx.loo_prior_batch(bad, lk=lk, flags=flags)
    ctx.close()


def test_four_conditioned_members_are_refused():
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.loo_batch(lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.loo_prior_batch(np.ones((4, 6)), lk=np.ones((4, ped.n, 3)))
    ctx.close()


# ---- FamSeq vcf -loo -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [[], ["-afTagAll", "AF", "-dnm", "-map", "-siteQ"]])
def test_cli_loo(extra, tmp_path):
    vcf, pedf = TD + "/test_subset.vcf", TD + "/fam01.ped"
    ped = pedmod.read_ped(pedf)
    ped.relations()
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf]
    plain, lo = tmp_path / "plain.vcf", tmp_path / "loo.vcf"
    run_cli(base + ["-method", "2"] + extra, plain)
    run_cli(base + ["-loo"] + extra, lo)  # (implies -method 2)
    got, want = open(lo).read().split("\n"), open(plain).read().split("\n")
    fmt_lines = [l for l in got if l.startswith(("##FORMAT=<ID=LOP,Number=G,Type=Float", "##FORMAT=<ID=LOF,Number=1,Type=Float"))]
    assert len(fmt_lines) == 2
    got = [l for l in got if l not in fmt_lines]
    assert len(got) == len(want)
    inputs = vcf_inputs(vcf, ped, "AF" if extra else None)
    header = [l for l in got if l.startswith("#CHROM")][0].rstrip("\t").split("\t")[9:]  # (the title line ends in a tab)
    member = [list(ped.names).index(nm) for nm in header]
    sites = []
    for a, b in zip(got, want):
        if not a or a.startswith("#"):
            assert a == b
            continue
        t, u = a.rstrip("\t").split("\t"), b.rstrip("\t").split("\t")
        if ":GPP:FPP:FGT" not in t[8]:
            assert a == b  # a line that is no site is echoed as it came
            continue
        assert t[:8] == u[:8] and t[8] == u[8] + ":LOP:LOF" and len(t) == len(u) == 9 + len(member)
        fields = []
        for x, y in zip(t[9:], u[9:]):  # every column byte for byte the output without -loo, but for the two new fields
            assert x.startswith(y + ":") and x[len(y) + 1:].count(":") == 1
            fields.append(x[len(y) + 1:])
        sites.append(((t[0], t[1]), fields, ":NA:NA:NA" in u[9]))
    assert len(sites) >= 12
    lk = np.array([inputs[k][0] for k, _, _ in sites])
    flags = np.array([inputs[k][1] for k, _, _ in sites], np.uint8)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    if extra:
        prior = P.model_rows(model, flags)
        for s, (k, _, _) in enumerate(sites):
            if inputs[k][2] is not None:
                prior[s] = fs.hwe_priors([inputs[k][2]])[0]
        assert sum(inputs[k][2] is not None for k, _, _ in sites) >= 3
        loo, fit, st = ctx.loo_prior_batch(prior, lk=lk, flags=flags)
        assert not same_bits((loo, fit), ctx.loo_batch(lk=lk, flags=flags)[:2])
    else:
        loo, fit, st = ctx.loo_batch(lk=lk, flags=flags)
    ctx.close()
    assert (st == 0).sum() >= 12
    for s, (k, fields, failed) in enumerate(sites):
        for j, p in enumerate(member):
            if failed or st[s] != 0:
                assert fields[j] == "NA:NA"
            else:
                exp = "%s:%g" % (",".join("%g" % phred(x) for x in loo[s, p]), phred(fit[s, p]))
                assert fields[j] == exp, (k, j, fields[j], exp)


def test_cli_loo_forms_and_notices(tmp_path):
    """NA:NA where the site failed; the notice outside vcf mode, the refusals, -h."""
    ped = fs.synthetic_pedigree("trio")
    ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"
    body = "1\t10\t.\tA\tC\t50\tPASS\t.\tGT:PL\t0/0:0,30,60\t0/1:20,0,40\t0/0:0,25,50\n"
    # a site whose single posterior fails: every PL beyond the table (likelihood 0) for one member
    body += "1\t40\t.\tA\tC\t50\tPASS\tDP=1\tGT:PL\t0/0:9000,9000,9000\t0/1:20,0,40\t0/0:0,25,50\n"
    open(vcf, "w").write(head + body)
    out = tmp_path / "o.vcf"
    run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-loo"], out)
    lines = [l.rstrip("\t").split("\t") for l in open(out).read().split("\n") if l and not l.startswith("#")]
    assert len(lines) == 2 and all(l[8].endswith(":GPP:FPP:FGT:LOP:LOF") for l in lines)
    for f in lines[0][9:]:
        lop, lof = f.rsplit(":", 2)[1:]
        assert lop.count(",") == 2 and "NA" not in lop + lof and float(lof) >= 0
    assert all(f.endswith(":NA:NA:NA:NA:NA") for f in lines[1][9:])
    p = subprocess.run([CLI, "LK", "-lkFile", TD + "/loftest.txt", "-pedFile", TD + "/fam04.ped", "-loo", "-output", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "-loo applies to vcf mode only; ignored here." in p.stdout
    p = subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-loo", "-afTag", "AF", "-output", str(tmp_path / "q.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-afTag cannot be combined with -dnm or -map" in p.stdout
    pedmod.write_ped(four_loops(), pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-loo", "-output", str(tmp_path / "r.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-loo cannot serve this pedigree: " in p.stdout and "more than three" in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-loo\t" in p.stdout + p.stderr
