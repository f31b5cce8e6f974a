"""`FamSeq vcf -mRateScan FILE [-mRateGrid r1,r2,...]`: the report's per-rate sums are the numpy reference's (tests/_maxproduct.py's
Z at each rate on the rows the driver reads) to the six decimals printed, its site and n_impossible counts are right, the VCF
output is the run's without the option byte for byte, the report does not depend on FAMSEQ_BATCH, a file simulated with de novo
events ranks a rate >= 1e-4 above 1e-9, -afTagAll brings the line's prior, and the option's refusals.  The refusals are said
before a device is touched: that part is not marked gpu.

The bar for a value: per site 2e-9 (rate_loglik and loglik at 1e-9 absolute each: test_mutrate_host.py), times the sites of the
file, plus the %.6f rounding, 5e-7 — test_cli_relabel_gpu.py's derivation; 200 x 2e-9 + 5e-7 on its 200-site family file."""
import os
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from test_cli_gpu import CLI, run_cli
from test_cli_relabel_gpu import N_SITES, write_family_vcf
from test_gpu_evidence import vcf_inputs
from test_pattern_host import _total

BAR = N_SITES * 2e-9 + 5e-7
MRATE = 1e-7
DEFAULT_GRID = [0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3]
N_DENOVO_SITES = 400
DENOVO_RATE = 1e-3  # per transmission


def numpy_report(ped, vcf, grid, af_key=None):
    """-> (sum[rate], impossible[rate], used, skipped, own sum) from the elimination of tests/_maxproduct.py on the rows the driver
    reads; the sums taken in file order, one -inf making a sum -inf."""
    inputs = vcf_inputs(vcf, ped, af_key)
    keys = sorted(inputs, key=lambda k: int(k[1]))
    lk = np.array([inputs[k][0] for k in keys])
    flags = np.array([inputs[k][1] for k in keys], np.uint8)
    prior = None
    if af_key:
        prior = P.model_rows(fs.make_model(ped, mrate=MRATE), flags)
        has = np.array([inputs[k][2] is not None for k in keys])
        prior[has] = fs.hwe_priors(np.array([inputs[k][2] for k in keys if inputs[k][2] is not None]))
    z, fail = _total(ped, MRATE, lk, flags, prior)
    ok = ~fail & (z > 0) & np.isfinite(z)
    assert np.all(z[ok] >= 1e-200)
    sums, imp = [], []
    for r in grid:
        zr = _total(ped, float(r), lk, flags, prior)[0][ok]
        assert np.all((zr == 0) | (zr >= 1e-200))
        total = 0.0
        with np.errstate(divide="ignore"):
            for x in np.log10(zr) - 7.0:  # in file order
                total += x
        sums.append(total)
        imp.append(int((zr == 0).sum()))
    own = 0.0
    for x in np.log10(z[ok]) - 7.0:
        own += x
    return np.array(sums), imp, int(ok.sum()), int((~ok).sum()), own


def read_report(path):
    """-> (used, skipped, -mRate as printed, own sum, rates as printed, log10_lik[rate], delta[rate], n_impossible[rate], best as printed)."""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[1] == "rate\tlog10_lik\tdelta\tn_impossible"
    head = lines[0].split()
    assert lines[0].startswith("# -mRateScan: ") and head[3:5] == ["sites", "used,"] and head[6] == "skipped;" and head[7] == "-mRate" and head[9] == "log10_lik"
    assert len(head[10].split(".")[1]) == 6  # %.6f
    rows = [l.split("\t") for l in lines[2:-2]]
    for r in rows:
        assert len(r) == 4 and all(v == "-inf" or len(v.split(".")[1]) == 6 for v in r[1:3])
    last = lines[-2].split("\t")
    assert last[0] == "best" and len(last) == 2
    return (int(head[2]), int(head[5]), head[8], float(head[10]), [r[0] for r in rows], np.array([float(r[1]) for r in rows]),
            np.array([float(r[2]) for r in rows]), [int(r[3]) for r in rows], last[1])


def compare(report, want, grid, what, bar=BAR):
    used, skipped, mrate, own, rates, ll, delta, imp, best = read_report(report)
    w_sum, w_imp, w_used, w_skipped, w_own = want
    finite = np.isfinite(w_sum)
    print("%s: %d rates, %d sites used, %d skipped, n_impossible %s, worst |log10_lik error| %.3g, worst |delta error| %.3g (bar %.3g), own sum's error %.3g" %
          (what, len(rates), used, skipped, imp, np.abs(ll[finite] - w_sum[finite]).max(initial=0),
           np.abs(delta[finite] - (w_sum[finite] - w_own)).max(initial=0), bar, abs(own - w_own)))
    assert rates == ["%g" % r for r in grid] and mrate == "%g" % MRATE
    assert (used, skipped, imp) == (w_used, w_skipped, w_imp)
    assert np.array_equal(np.isneginf(ll), ~finite) and np.array_equal(np.isneginf(delta), ~finite)
    assert np.array_equal(~finite, np.array(w_imp) > 0)  # one -inf site makes the sum -inf
    np.testing.assert_allclose(ll[finite], w_sum[finite], rtol=0, atol=bar)
    np.testing.assert_allclose(delta[finite], w_sum[finite] - w_own, rtol=0, atol=bar)
    assert abs(own - w_own) <= bar
    # the first rate of the grid with the largest log10_lik, in the report's own numbers and in the reference's
    assert best == rates[int(np.argmax(ll))]
    margin = np.sort(w_sum)[-1] - np.sort(w_sum)[-2] if len(grid) > 1 else np.inf
    assert margin <= 2 * bar or best == "%g" % grid[int(np.argmax(w_sum))]
    return ll, best


def write_denovo_vcf(ped, path, seed):
    """N_DENOVO_SITES autosomal sites of a family whose founders carry the allele at frequency 0.2 and whose children inherit
    one allele of each parent, every transmitted allele flipped with probability DENOVO_RATE.  PL 0 at the true genotype and
    20..60 elsewhere; at a site with a flipped allele the data are certain (9000 elsewhere), so that the site is impossible
    without a mutation wherever the flip shows (a heterozygous parent's flipped allele is its other one).  -> the number of sites
    with a flipped allele."""
    mo, fa = ped.relations()
    rng = np.random.RandomState(seed)
    lines = ["##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"]
    events = 0
    for s in range(N_DENOVO_SITES):
        g = np.zeros(ped.n, int)
        flipped = False
        for p in range(ped.n):  # (parents stand in front of their children in these pedigrees)
            if mo[p] < 0:
                g[p] = rng.binomial(2, 0.2)
                continue
            for parent in (mo[p], fa[p]):
                allele = rng.binomial(1, g[parent] / 2.0)
                if rng.rand() < DENOVO_RATE:
                    allele, flipped = 1 - allele, True
                g[p] += allele
        events += flipped
        cols = []
        for p in range(ped.n):
            pl = np.full(3, 9000) if flipped else rng.randint(20, 61, 3)
            pl[g[p]] = 0
            cols.append("%s:%d,%d,%d" % (("0/0", "0/1", "1/1")[g[p]], pl[0], pl[1], pl[2]))
        lines.append("1\t%d\t.\tA\tC\t50\tPASS\tDP=%d\tGT:PL\t%s\n" % (100 + s, 10 + s, "\t".join(cols)))
    open(path, "w").write("".join(lines))
    return events


def denovo_case(tmp_path):
    ped = fs.synthetic_pedigree("ped10")
    vcf = str(tmp_path / "denovo.vcf")
    events = write_denovo_vcf(ped, vcf, 21)
    return ped, vcf, events, numpy_report(ped, vcf, DEFAULT_GRID)


def test_the_de_novo_simulation_prefers_a_high_rate_in_the_reference(tmp_path):
    """On the CPU, the numpy reference alone: the simulated file holds de novo events, those that show are impossible at rate 0
    and at no other rate, and the likelihood ranks every rate >= 1e-4 of the grid above 1e-9."""
    ped, vcf, events, want = denovo_case(tmp_path)
    sums, imp, used, skipped, _ = want
    print("de novo simulation: %d sites with an event of %d; sums %s" % (events, N_DENOVO_SITES, sums))
    assert 2 <= events <= 20 and used == N_DENOVO_SITES and skipped == 0
    assert 2 <= imp[0] <= events and imp[1:] == [0] * (len(DEFAULT_GRID) - 1) and np.isneginf(sums[0])
    assert sums[6] > sums[1] + 1.0 and sums[7] > sums[1] + 1.0 and int(np.argmax(sums)) >= 6


@pytest.mark.gpu
def test_cli_rate_scan_on_a_de_novo_file(tmp_path):
    ped, vcf, events, want = denovo_case(tmp_path)
    pedf, rep = str(tmp_path / "p.ped"), tmp_path / "report.txt"
    pedmod.write_ped(ped, pedf)
    run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7", "-mRateScan", str(rep)], tmp_path / "out.vcf")
    ll, best = compare(rep, want, DEFAULT_GRID, "de novo file", N_DENOVO_SITES * 2e-9 + 5e-7)
    assert float(best) >= 1e-4 and ll[6] > ll[1] and ll[7] > ll[1] and np.isneginf(ll[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quad", "ped10"])
def test_cli_rate_scan(name, tmp_path):
    ped = fs.synthetic_pedigree(name)
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    write_family_vcf(ped, vcf, 11)
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7"]
    plain, with_scan, small = tmp_path / "plain.vcf", tmp_path / "scan.vcf", tmp_path / "small.vcf"
    rep, rep_small = tmp_path / "report.txt", tmp_path / "report_small.txt"
    want = numpy_report(ped, vcf, DEFAULT_GRID)
    assert want[2] == N_SITES - 1 and want[3] == 1  # one failed site
    run_cli(base + ["-method", "2"], plain)
    run_cli(base + ["-mRateScan", str(rep)], with_scan)  # (implies -method 2)
    assert open(with_scan, "rb").read() == open(plain, "rb").read()
    p = subprocess.run([CLI] + base + ["-mRateScan", str(rep_small), "-output", str(small)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FAMSEQ_BATCH="7"))
    assert p.returncode == 0, p.stdout + p.stderr
    assert open(rep_small, "rb").read() == open(rep, "rb").read() and open(small, "rb").read() == open(plain, "rb").read()
    ll, _ = compare(rep, want, DEFAULT_GRID, name)
    assert abs(read_report(rep)[6][3]) <= BAR  # delta at the run's own -mRate
    # a grid of the caller's, with the extremes and one rate twice; beside every other side option: their output unchanged
    grid = [0.5, 1e-7, 0, 1, 1e-7, 2.5e-5]
    others = ["-siteQ", "-dnm", "-loo", "-map", "-swapCheck", str(tmp_path / "swap.txt")]
    both, alone, rep_grid = tmp_path / "both.vcf", tmp_path / "alone.vcf", tmp_path / "report_grid.txt"
    run_cli(base + others, alone)
    run_cli(base + others + ["-mRateScan", str(rep_grid), "-mRateGrid", ",".join("%g" % r for r in grid)], both)
    assert open(both, "rb").read() == open(alone, "rb").read()
    ll, _ = compare(rep_grid, numpy_report(ped, vcf, grid), grid, name + ", a grid of six")
    assert ll[1] == ll[4]


@pytest.mark.gpu
def test_cli_rate_scan_with_site_priors(tmp_path):
    ped = fs.synthetic_pedigree("quad")
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    write_family_vcf(ped, vcf, 12, af=True)
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7", "-afTagAll", "AF"]
    plain, with_scan, rep = tmp_path / "plain.vcf", tmp_path / "scan.vcf", tmp_path / "report.txt"
    run_cli(base, plain)
    run_cli(base + ["-mRateScan", str(rep)], with_scan)
    assert open(with_scan, "rb").read() == open(plain, "rb").read()
    want = numpy_report(ped, vcf, DEFAULT_GRID, "AF")
    without = numpy_report(ped, vcf, DEFAULT_GRID)
    assert np.abs(want[0][1:] - without[0][1:]).max() > 100 * BAR  # (the prior matters to the sums)
    compare(rep, want, DEFAULT_GRID, "quad, -afTagAll AF")


def refused(args, tmp_path, pedf=None, code=255):
    ped = fs.synthetic_pedigree("quad")
    vcf = str(tmp_path / "in.vcf")
    if pedf is None:
        pedf = str(tmp_path / "quad.ped")
        pedmod.write_ped(ped, pedf)
    if not os.path.exists(vcf):
        write_family_vcf(ped, vcf, 3)
    out = tmp_path / "o.vcf"
    p = subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == code and not out.exists(), p.stdout + p.stderr
    return p.stdout


def test_cli_rate_scan_refusals(tmp_path):
    """Said before any input is read and before any device is touched (this machine may have none)."""
    from test_gpu_denovo import four_loops

    rep = str(tmp_path / "r.txt")
    missing = str(tmp_path / "no_such_dir" / "report.txt")
    assert "Cannot write %s (the report file of -mRateScan)." % missing in refused(["-mRateScan", missing], tmp_path)
    assert "Cannot write the report file of -mRateScan: it hasn't been set." in refused(["-mRateScan"], tmp_path)
    assert "-mRateGrid gives the rates of -mRateScan FILE, which hasn't been set." in refused(["-mRateGrid", "0,1e-7"], tmp_path)
    assert "the grid is empty" in refused(["-mRateScan", rep, "-mRateGrid"], tmp_path)
    assert "the grid is empty" in refused(["-mRateScan", rep, "-mRateGrid", ""], tmp_path)
    assert "-mRateGrid takes at most 32 rates, not 33." in refused(["-mRateScan", rep, "-mRateGrid", ",".join(["1e-7"] * 33)], tmp_path)
    for bad in ("2", "x", "1e-7x", "nan", "inf", ""):
        assert '-mRateGrid takes mutation rates, numbers in [0, 1], not "%s".' % bad in refused(["-mRateScan", rep, "-mRateGrid", "0,%s,1" % bad], tmp_path)
    assert "the grid is empty" in refused(["-mRateScan", rep, "-mRateGrid", "-0.5,1"], tmp_path)  # (it starts like an option)
    assert not os.path.exists(rep)  # a refused grid leaves no report file behind
    assert "-afTag cannot be combined" in refused(["-mRateScan", rep, "-afTag", "AF"], tmp_path)
    loops = str(tmp_path / "loops.ped")
    pedmod.write_ped(four_loops(), loops)
    assert "-mRateScan cannot serve this pedigree" in refused(["-mRateScan", str(tmp_path / "r2.txt")], tmp_path, loops)
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", str(tmp_path / "quad.ped"), "-mRateScan", str(tmp_path / "r3.txt"),
                        "-output", str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=300)
    assert "-mRateScan applies to vcf mode only; ignored here." in p.stdout and not (tmp_path / "r3.txt").exists()
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-mRateScan FILE\t" in p.stdout + p.stderr and "-mRateGrid r1,r2,..." in p.stdout + p.stderr
