"""The evidence on the device: famseq_evidence_batch / famseq_evidence_prior_batch and their device entries through the C ABI,
and `FamSeq vcf -siteQ`.  References and tolerances as in test_evidence_host.py: loglik = log10(z) - 7 at an absolute 1e-9,
pref = w0 / z at rtol 1e-9, status exact, bits where two routes must agree; on the clear batches used here every reference has
status 0 and z, w0 >= 1e-200 (asserted), so no site is left out.

Shapes: the smallest that can still go wrong — 1, BT - 1 and 3 BT + 5 sites (a padding-lane-only block, a partial last chunk,
several loop trips of a workgroup where the grid is forced to one workgroup), at trio, ped10, a looped pedigree, 32 members
(registers-first, one wave) and 48 members (likelihoods re-read at each use)."""
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from famseq_amd.prebuild_sets import wide_pedigree
from test_cli_gpu import CLI, TD, run_cli
from test_evidence_host import check, cycled, prior_reference, reference, same_bits
from test_gpu_denovo import four_loops
from test_gpu_map import loop_pedigree
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
        bt = ctx.plan()["evidence_block_threads"]
        ctx.close()
        assert bt >= 2
        rng = np.random.RandomState(60 + ped.n)
        lk, _ = clear_likelihoods(rng, ped, 3 * bt + 5)
        flags = cycled(lk)
        hwe = fs.hwe_priors(rng.uniform(0.01, 0.5, len(lk)))
        ref = reference(ped, 1e-7, lk, flags)
        # the site-prior reference where the issue asks for it (trio, 32 members)
        pref = prior_reference(ped, 1e-7, lk, flags, hwe) if name in ("trio", "wide32") else None
        _CASES[name] = (ped, bt, lk, flags, ref, hwe, pref)
    return _CASES[name]


def take(ref, n):
    return tuple(x[:n] for x in ref)


@pytest.mark.parametrize("name", ["trio", "ped10", "loop", "wide32", "wide48"])
def test_parity_and_site_counts(name):
    ped, bt, lk, flags, ref, hwe, href = case(name)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    plan = ctx.plan()
    assert (plan["elim_conditioned_members"] > 0) == (name == "loop")
    whole = ctx.evidence_batch(lk=lk, flags=flags)
    check(whole, ref, name)
    assert same_bits(ctx.evidence_batch(lk=lk, flags=flags), whole)  # the same batch twice
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.evidence_prior_batch(rows, lk=lk, flags=flags), whole)  # the model's rows: the plain form's bits
    for n in (1, bt - 1):
        assert same_bits(ctx.evidence_batch(lk=lk[:n], flags=flags[:n]), take(whole, n))
        assert same_bits(ctx.evidence_prior_batch(rows[:n], lk=lk[:n], flags=flags[:n]), take(whole, n))
    ctx.set_option("grid_blocks", 1)  # one workgroup: four trips of its chunk loop, the last one partial
    assert same_bits(ctx.evidence_batch(lk=lk, flags=flags), whole)
    assert same_bits(ctx.evidence_prior_batch(rows, lk=lk, flags=flags), whole)
    ctx.set_option("grid_blocks", 0)
    if href is not None:
        check(ctx.evidence_prior_batch(hwe, lk=lk, flags=flags), href, name + ", Hardy-Weinberg rows")
    plan = ctx.plan()
    assert plan["evidence_code_object"].endswith(".hsaco") and 0 <= plan["evidence_variant"] < 4
    assert plan["evidence_prior_variant"] == plan["evidence_variant"]
    ctx.close()


def test_pl16_and_lk_give_the_same_bits():
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
    a = ctx.evidence_batch(pl16=pl, seq_members=seq, flags=flags)
    b = ctx.evidence_batch(lk=lk, flags=flags)
    assert (a[2] == 0).sum() > 100 and same_bits(a, b)
    rows = P.model_rows(model, flags)
    assert same_bits(ctx.evidence_prior_batch(rows, pl16=pl, seq_members=seq, flags=flags), b)
    import torch

    dev = torch.device("cuda")
    t_pl, t_fl = torch.from_numpy(pl.view(np.int16)).to(dev), torch.from_numpy(flags).to(dev)
    t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
    ctx.evidence_batch_device(n, d_pl16=t_pl.data_ptr(), seq_members=seq, d_flags=t_fl.data_ptr(), d_loglik=t_l.data_ptr(),
                              d_pref=t_p.data_ptr(), d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert same_bits((t_l.cpu().numpy(), t_p.cpu().numpy(), t_s.cpu().numpy()), b)


def test_device_entries_and_null_outputs():
    import torch

    ped, bt, lk, flags, ref, hwe, _ = case("ped10")
    n = len(lk)
    ctx = fs.Context(fs.make_model(ped))
    ll, p0, st = full = ctx.evidence_batch(lk=lk, flags=flags)
    hfull = ctx.evidence_prior_batch(hwe, lk=lk, flags=flags)
    assert not same_bits(hfull[:2], full[:2])
    l1, q1, s1 = ctx.evidence_batch(lk=lk, flags=flags, want_pref=False)
    l2, q2, s2 = ctx.evidence_batch(lk=lk, flags=flags, want_loglik=False)
    assert q1 is None and l2 is None and same_bits((l1, s1, q2, s2), (ll, st, p0, st))
    l3, q3, s3 = ctx.evidence_prior_batch(hwe, lk=lk, flags=flags, want_loglik=False, want_pref=False)
    assert l3 is None and q3 is None and np.array_equal(s3, hfull[2])
    no_flags = ctx.evidence_batch(lk=lk[flags == 0])
    assert same_bits(no_flags, tuple(x[flags == 0] for x in full))
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    # the prior rows at a 16-byte aligned address and at one that is only 8-byte aligned
    raw = torch.zeros(6 * n + 2, dtype=torch.float64, device=dev)
    off = (raw.data_ptr() % 16) // 8
    t_pr = {16: raw[off:off + 6 * n], 8: raw[off + 1:off + 1 + 6 * n]}
    for t in t_pr.values():
        assert t.data_ptr() % 8 == 0
    assert t_pr[16].data_ptr() % 16 == 0 and t_pr[8].data_ptr() % 16 == 8
    for want in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
        for align in (None, 16, 8):
            t_l = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
            t_p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
            t_s = torch.full((n,), 55, dtype=torch.uint8, device=dev)
            out = dict(d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_loglik=t_l.data_ptr() if want[0] else 0,
                       d_pref=t_p.data_ptr() if want[1] else 0, d_status=t_s.data_ptr() if want[2] else 0)
            if align is None:
                ctx.evidence_batch_device(n, **out)
            else:
                t_pr[align].copy_(torch.from_numpy(hwe.reshape(-1)).to(dev))
                ctx.evidence_prior_batch_device(n, t_pr[align].data_ptr(), **out)
            torch.cuda.synchronize()
            exp = full if align is None else hfull
            assert same_bits([t_l.cpu().numpy()], [exp[0]]) if want[0] else bool((t_l == -1.0).all())
            assert same_bits([t_p.cpu().numpy()], [exp[1]]) if want[1] else bool((t_p == -1.0).all())
            assert np.array_equal(t_s.cpu().numpy(), exp[2]) if want[2] else bool((t_s == 55).all())
    ctx.close()


def test_planted_failures():
    ped = fs.synthetic_pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 96)
    flags = np.zeros(96, np.uint8)
    lk[7, 1, :] = 0.0            # an all-zero row: the single-posterior rule
    lk[70] = (1.0, 0.0, 0.0)     # both parents hom-ref, a child hom-alt, no mutation: no configuration has weight
    lk[70, child] = (0.0, 0.0, 1.0)
    lk[80, child, 0] = 0.0       # no hom-ref configuration: pref 0.0, the site stands
    ref = reference(ped, 0.0, lk, flags)
    model = fs.make_model(ped, mrate=0.0)
    ctx = fs.Context(model)
    for out in (ctx.evidence_batch(lk=lk, flags=flags), ctx.evidence_prior_batch(P.model_rows(model, flags), lk=lk, flags=flags)):
        check(out, ref, "planted failures", clear=False)
        assert out[2][7] == 1 and out[2][70] == 2 and out[1][80] == 0.0 and (np.delete(out[2], [7, 70]) == 0).all()
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*site 3"):
        bad = P.model_rows(model, flags)
        bad[3, 1] = -1.0
        ctx.evidence_prior_batch(bad, lk=lk, flags=flags)
    ctx.close()


def test_four_conditioned_members_are_refused():
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.evidence_batch(lk=np.ones((4, ped.n, 3)))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
        ctx.evidence_prior_batch(np.ones((4, 6)), lk=np.ones((4, ped.n, 3)))
    ctx.close()


# ---- FamSeq vcf -siteQ -----------------------------------------------------------------------------------------------

def vcf_inputs(vcf, ped, af_key=None):
    """The driver's reading of a VCF, per (CHROM, POS): (lk row [N, 3], flags, allele frequency of INFO or None)."""
    col, out = {}, {}
    index = {nm: p for p, nm in enumerate(ped.names)}
    for line in open(vcf):
        t = line.rstrip("\n").split("\t")
        if line.startswith("#CHROM"):
            col = {nm: k for k, nm in enumerate(t[9:])}
        if line.startswith("#") or len(t) < 10:
            continue
        fmt = t[8].split(":")
        i_pl = max([k for k, f in enumerate(fmt) if f in ("PL", "GL")], default=-1)
        if i_pl < 0:
            continue
        lk = np.ones((ped.n, 3))
        for nm, k in col.items():
            f = t[9 + k]
            if nm not in index or len(f) < 5 or len(f.split(":")) != len(fmt):
                continue
            lk[index[nm]] = [10.0 ** (-abs(float(x)) / 10.0) for x in f.split(":")[i_pl].split(",")]
        flags = (fs.FLAG_KNOWN if t[2] != "." else 0) | (fs.FLAG_CHRX if t[0] in ("X", "chrX") else 0)
        af = None
        for kv in t[7].split(";"):
            if af_key and kv.startswith(af_key + "="):
                try:
                    x = float(kv[len(af_key) + 1:].split(",")[0])
                    af = x if 0 < x < 1 else None
                except ValueError:
                    pass
                break
        out[(t[0], t[1])] = (lk, flags, af)
    return out


def info_without_keys(info):
    kept = [kv for kv in info.split(";") if not kv.startswith(("FQ=", "FLL="))]
    return ";".join(kept) if kept else "."


def phred(p):
    return 99999.0 if p == 0 else abs(-10.0 * np.log10(p))


@pytest.mark.parametrize("extra", [[], ["-afTagAll", "AF", "-dnm", "-map"]])
def test_cli_siteq(extra, tmp_path):
    vcf, pedf = TD + "/test_subset.vcf", TD + "/fam01.ped"
    ped = pedmod.read_ped(pedf)
    ped.relations()
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf]
    plain, sq = tmp_path / "plain.vcf", tmp_path / "siteq.vcf"
    run_cli(base + ["-method", "2"] + extra, plain)
    run_cli(base + ["-siteQ"] + extra, sq)  # (implies -method 2)
    got, want = open(sq).read().split("\n"), open(plain).read().split("\n")
    info_lines = [l for l in got if l.startswith(("##INFO=<ID=FQ,Number=1,Type=Float", "##INFO=<ID=FLL,Number=1,Type=Float"))]
    assert len(info_lines) == 2
    got = [l for l in got if l not in info_lines]
    assert len(got) == len(want)
    inputs = vcf_inputs(vcf, ped, "AF" if extra else None)
    model = fs.make_model(ped)
    sites = []
    for a, b in zip(got, want):
        if not a or a.startswith("#"):
            assert a == b
            continue
        t, u = a.split("\t"), b.split("\t")
        assert t[:7] == u[:7] and t[8:] == u[8:]  # every column but INFO byte for byte
        if ":GPP:FPP:FGT" not in t[8]:
            assert a == b  # a line that is no site is echoed as it came
            continue
        assert info_without_keys(t[7]) == u[7]
        sites.append(((t[0], t[1]), t[7], u[7]))
    assert len(sites) >= 12
    lk = np.array([inputs[k][0] for k, _, _ in sites])
    flags = np.array([inputs[k][1] for k, _, _ in sites], np.uint8)
    ctx = fs.Context(model)
    if extra:
        prior = P.model_rows(model, flags)
        for s, (k, _, _) in enumerate(sites):
            if inputs[k][2] is not None:
                prior[s] = fs.hwe_priors([inputs[k][2]])[0]
        assert sum(inputs[k][2] is not None for k, _, _ in sites) >= 3
        ll, p0, st = ctx.evidence_prior_batch(prior, lk=lk, flags=flags)
        assert not same_bits((ll, p0), ctx.evidence_batch(lk=lk, flags=flags)[:2])
    else:
        ll, p0, st = ctx.evidence_batch(lk=lk, flags=flags)
    ctx.close()
    assert (st == 0).sum() >= 12
    for s, (k, info, old) in enumerate(sites):
        if st[s] != 0:
            assert info == old  # a failed site gets neither key
            continue
        tail = "FQ=%g;FLL=%g" % (phred(p0[s]), ll[s])
        assert info == (tail if old == "." else old + ";" + tail), (k, info, tail)


def test_cli_siteq_info_forms_and_notices(tmp_path):
    """An INFO of "." is replaced, anything else joined with ';'; a failed site keeps its INFO; the notices."""
    ped = fs.synthetic_pedigree("trio")
    ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"
    rows = [("1", "10", ".", "."), ("1", "20", "rs1", "DP=4;AF=0.25"), ("X", "30", ".", "DP=9")]
    body = "".join("%s\t%s\t%s\tA\tC\t50\tPASS\t%s\tGT:PL\t0/0:0,30,60\t0/1:20,0,40\t0/0:0,25,50\n" % r for r in rows)
    # a site whose single posterior fails: every PL beyond the table (likelihood 0) for one member
    body += "1\t40\t.\tA\tC\t50\tPASS\tDP=1\tGT:PL\t0/0:9000,9000,9000\t0/1:20,0,40\t0/0:0,25,50\n"
    open(vcf, "w").write(head + body)
    out = tmp_path / "o.vcf"
    run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-siteQ"], out)
    lines = [l.split("\t") for l in open(out).read().split("\n") if l and not l.startswith("#")]
    assert len(lines) == 4
    assert lines[0][7].startswith("FQ=") and ";FLL=" in lines[0][7]
    assert lines[1][7].startswith("DP=4;AF=0.25;FQ=") and lines[2][7].startswith("DP=9;FQ=")
    assert lines[3][7] == "DP=1" and ":NA:NA:NA" in lines[3][9]
    p = subprocess.run([CLI, "LK", "-lkFile", TD + "/loftest.txt", "-pedFile", TD + "/fam04.ped", "-siteQ", "-output", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "-siteQ applies to vcf mode only; ignored here." in p.stdout
    pedmod.write_ped(four_loops(), pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-siteQ", "-output", str(tmp_path / "r.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-siteQ cannot serve this pedigree: " in p.stdout and "more than three" in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-siteQ\t" in p.stdout + p.stderr
