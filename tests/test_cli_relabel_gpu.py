"""`FamSeq vcf -swapCheck FILE`: the report's per-pair sums are the numpy reference's (tests/_maxproduct.py's Z on the rows
rearranged on the host) to the six decimals printed, its site counts are right, the VCF output is the run's without the option
byte for byte, the report does not depend on FAMSEQ_BATCH, a planted exchange of two columns ranks first, -afTagAll brings the
line's prior, and the option's refusals.  The refusals are said before a device is touched: that part is not marked gpu.

The bar for a value: 200 sites of 2e-9 each (alt_loglik and loglik at 1e-9 absolute: test_relabel_host.py) plus the %.6f
rounding, 5e-7."""
import os
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from test_cli_gpu import CLI, run_cli
from test_gpu_evidence import vcf_inputs
from test_pattern_host import _total
from test_relabel_host import rearranged

N_SITES = 200
BAR = N_SITES * 2e-9 + 5e-7
MRATE = 1e-7


def write_family_vcf(ped, path, seed, exchange=None, af=False):
    """About 200 sites of a family whose genotypes follow the pedigree (founders at allele frequency 0.3, children Mendelian),
    written the way test_cli_af_gpu writes its input: PL 0 at the true genotype, 20..60 elsewhere.  The columns stand in the
    reverse of the PED order.  Every fifth site is on X, every seventh has an ID (Known); one site's single posterior fails (a
    column of PLs beyond the table) and one X site makes a female a certain heterozygote, which no male can be handed.
    exchange (a, b): the columns of members a and b change places under unchanged names.  af: an AF= key on two sites in three."""
    mo, fa = ped.relations()
    rng = np.random.RandomState(seed)
    order = list(range(ped.n))[::-1]
    female = [p for p in range(ped.n) if ped.genders[p] != 1][0]
    lines = ["##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names[p] for p in order) + "\n"]
    for s in range(N_SITES):
        g = np.zeros(ped.n, int)
        for p in range(ped.n):  # (parents stand in front of their children in these pedigrees)
            if mo[p] < 0:
                g[p] = rng.binomial(2, 0.3)
            else:
                g[p] = rng.binomial(1, g[mo[p]] / 2.0) + rng.binomial(1, g[fa[p]] / 2.0)
        cols = []
        for p in range(ped.n):
            pl = rng.randint(20, 61, 3)
            pl[g[p]] = 0
            cols.append("%s:%d,%d,%d" % (("0/0", "0/1", "1/1")[g[p]], pl[0], pl[1], pl[2]))
        if s == 50:
            cols[1] = "0/0:9000,9000,9000"
        if s == 55:
            cols[female] = "0/1:9000,0,9000"
        if exchange:
            a, b = exchange
            cols[a], cols[b] = cols[b], cols[a]
        info = "AF=%.3f" % rng.uniform(0.05, 0.6) if af and s % 3 else "DP=%d" % (10 + s)
        lines.append("%s\t%d\t%s\tA\tC\t50\tPASS\t%s\tGT:PL\t%s\n" % ("X" if s % 5 == 0 else "1", 100 + s, "rs%d" % s if s % 7 == 0 else ".", info,
                                                                  "\t".join(cols[p] for p in order)))
    open(path, "w").write("".join(lines))
    return order


def numpy_report(ped, vcf, order, af_key=None):
    """-> (pairs [(name_a, name_b)] in VCF column order, bf[pair], impossible[pair], used, skipped, loglik) from the elimination
    of tests/_maxproduct.py on the rows the driver reads."""
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
    pairs, bf, imp = [], [], []
    for i in range(len(order)):
        for j in range(i + 1, len(order)):
            a = np.arange(ped.n)
            a[order[i]], a[order[j]] = order[j], order[i]
            za = _total(ped, MRATE, rearranged(lk, a), flags, prior)[0][ok]
            with np.errstate(divide="ignore"):
                d = np.log10(za) - np.log10(z[ok])
            total = 0.0
            for x in d[za > 0]:  # in file order
                total += x
            pairs.append((ped.names[order[i]], ped.names[order[j]]))
            bf.append(total)
            imp.append(int((za == 0).sum()))
    return pairs, np.array(bf), imp, int(ok.sum()), int((~ok).sum()), float(np.sum(np.log10(z[ok]) - 7.0))


def read_report(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[1] == "#sample_a\tsample_b\tlog10_BF\tsites_impossible"
    head = dict(kv.split("=") for kv in lines[0][1:].split("\t"))
    assert list(head) == ["sites_used", "sites_skipped", "log10_lik"]
    rows = [l.split("\t") for l in lines[2:-1]]
    for r in rows:
        assert len(r) == 4 and len(r[2].split(".")[1]) == 6  # %.6f
    return head, [(r[0], r[1]) for r in rows], np.array([float(r[2]) for r in rows]), [int(r[3]) for r in rows]


def compare(report, want, what):
    head, pairs, bf, imp = read_report(report)
    w_pairs, w_bf, w_imp, used, skipped, loglik = want
    print("%s: %d pairs, %d sites used, %d skipped, worst |log10_BF error| %.3g (bar %.3g), log10_lik error %.3g" %
          (what, len(pairs), used, skipped, np.abs(bf - w_bf).max(), BAR, abs(float(head["log10_lik"]) - loglik)))
    assert pairs == w_pairs and imp == w_imp
    assert int(head["sites_used"]) == used and int(head["sites_skipped"]) == skipped
    np.testing.assert_allclose(bf, w_bf, rtol=0, atol=BAR)
    assert abs(float(head["log10_lik"]) - loglik) <= BAR
    return pairs, bf


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quad", "ped10", "ped15"])
def test_cli_swap_check(name, tmp_path):
    """ped15: 105 pairs, more than a call takes — two groups, 64 and 41."""
    ped = fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    pedf, vcf, mixed = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf"), str(tmp_path / "m.vcf")
    pedmod.write_ped(ped, pedf)
    order = write_family_vcf(ped, vcf, 11)
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7"]
    plain, with_swap, small = tmp_path / "plain.vcf", tmp_path / "swap.vcf", tmp_path / "small.vcf"
    rep, rep_small = tmp_path / "report.txt", tmp_path / "report_small.txt"
    want = numpy_report(ped, vcf, order)
    assert want[3] == N_SITES - 1 and want[4] == 1 and sum(want[2]) > 0  # one failed site; the certain heterozygote is impossible for a male
    run_cli(base + ["-method", "2"], plain)
    run_cli(base + ["-swapCheck", str(rep)], with_swap)  # (implies -method 2)
    assert open(with_swap, "rb").read() == open(plain, "rb").read()
    p = subprocess.run([CLI] + base + ["-swapCheck", str(rep_small), "-output", str(small)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FAMSEQ_BATCH="7"))
    assert p.returncode == 0, p.stdout + p.stderr
    assert open(rep_small, "rb").read() == open(rep, "rb").read() and open(small, "rb").read() == open(plain, "rb").read()
    pairs, bf = compare(rep, want, name)
    assert len(pairs) == ped.n * (ped.n - 1) // 2
    assert (len(pairs) > fs.MAX_RELABEL) == (name == "ped15")
    if name != "ped15":  # beside every other side option: the same report, and their output unchanged
        others = ["-siteQ", "-dnm", "-loo", "-map"]
        both, alone, rep_both = tmp_path / "both.vcf", tmp_path / "alone.vcf", tmp_path / "report_both.txt"
        run_cli(base + others, alone)
        run_cli(base + others + ["-swapCheck", str(rep_both)], both)
        assert open(both, "rb").read() == open(alone, "rb").read() and open(rep_both, "rb").read() == open(rep, "rb").read()
    # the father's and one child's columns exchanged: that pair first, with a positive value, in the reference and in the report
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    father = fa[child]
    write_family_vcf(ped, mixed, 11, exchange=(father, child))
    want = numpy_report(ped, mixed, order)
    planted = {ped.names[father], ped.names[child]}
    best = int(np.argmax(want[1]))
    assert set(want[0][best]) == planted and want[1][best] > 0 and np.sum(want[1] >= want[1][best]) == 1
    rep_mixed = tmp_path / "report_mixed.txt"
    run_cli(base[:2] + [mixed] + base[3:] + ["-swapCheck", str(rep_mixed)], tmp_path / "mixed_out.vcf")
    pairs, bf = compare(rep_mixed, want, name + ", two columns exchanged")
    assert set(pairs[int(np.argmax(bf))]) == planted and bf.max() > 0 and np.sum(bf >= bf.max()) == 1


@pytest.mark.gpu
def test_cli_swap_check_with_site_priors(tmp_path):
    ped = fs.synthetic_pedigree("quad")
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    order = write_family_vcf(ped, vcf, 12, af=True)
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7", "-afTagAll", "AF"]
    plain, with_swap, rep = tmp_path / "plain.vcf", tmp_path / "swap.vcf", tmp_path / "report.txt"
    run_cli(base, plain)
    run_cli(base + ["-swapCheck", str(rep)], with_swap)
    assert open(with_swap, "rb").read() == open(plain, "rb").read()
    want = numpy_report(ped, vcf, order, "AF")
    without = numpy_report(ped, vcf, order)
    assert np.abs(want[1] - without[1]).max() > 100 * BAR  # (the prior matters to the sums)
    compare(rep, want, "quad, -afTagAll AF")


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


def test_cli_swap_check_refusals(tmp_path):
    """Said before any input is read and before any device is touched (this machine may have none)."""
    from test_gpu_denovo import four_loops

    missing = str(tmp_path / "no_such_dir" / "report.txt")
    assert "Cannot write %s (the report file of -swapCheck)." % missing in refused(["-swapCheck", missing], tmp_path)
    assert "-afTag cannot be combined" in refused(["-swapCheck", str(tmp_path / "r.txt"), "-afTag", "AF"], tmp_path)
    loops = str(tmp_path / "loops.ped")
    pedmod.write_ped(four_loops(), loops)
    assert "-swapCheck cannot serve this pedigree" in refused(["-swapCheck", str(tmp_path / "r2.txt")], tmp_path, loops)
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", str(tmp_path / "quad.ped"), "-swapCheck", str(tmp_path / "r3.txt"),
                        "-output", str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=300)
    assert "-swapCheck applies to vcf mode only; ignored here." in p.stdout and not (tmp_path / "r3.txt").exists()
    p = subprocess.run([CLI, "vcf", "-vcfFile", "x", "-pedFile", "y", "-swapCheck"], capture_output=True, text=True, timeout=300)
    assert "The report file of -swapCheck hasn't been set" in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-swapCheck FILE\t" in p.stdout + p.stderr
