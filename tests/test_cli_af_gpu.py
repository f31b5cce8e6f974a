"""`FamSeq vcf -afEM T [-afStart X]`: FAF / FAL in the INFO column are Context.af_batch's allele frequency and likelihood ratio of
the same sites to the six digits printed, every other byte of every line is the run's without -afEM, it combines with the other
side options (the INFO keys in the order FQ;FLL, PSD;PSR, FAF;FAL), does not depend on FAMSEQ_BATCH, and the option errors.  The
refusals are said before a device is touched: that part is not marked gpu."""
import os
import subprocess

import numpy as np
import pytest

import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from test_cli_gpu import CLI, TD, run_cli
from test_cli_pattern_gpu import SEG
from test_gpu_evidence import vcf_inputs

VCF, PEDF = TD + "/test_subset.vcf", TD + "/fam01.ped"
KEYS = ("FAF=", "FAL=")
STEPS = 4


def split_info(info):
    """-> (the INFO column without FAF / FAL, {key: text})."""
    kept = [kv for kv in info.split(";") if not kv.startswith(KEYS)]
    return (";".join(kept) if kept else "."), {kv[:4]: kv[4:] for kv in info.split(";") if kv.startswith(KEYS)}


@pytest.mark.gpu
@pytest.mark.parametrize("extra,start", [([], None), (SEG + ["-siteQ", "-dnm", "-loo"], 0.2)])
def test_cli_af_em(extra, start, tmp_path):
    ped = pedmod.read_ped(PEDF)
    ped.relations()
    base = ["vcf", "-vcfFile", VCF, "-pedFile", PEDF]
    em = ["-afEM", str(STEPS)] + ([] if start is None else ["-afStart", str(start)])
    plain, with_em, small = tmp_path / "plain.vcf", tmp_path / "em.vcf", tmp_path / "small.vcf"
    run_cli(base + ["-method", "2"] + extra, plain)
    run_cli(base + em + extra, with_em)  # (implies -method 2)
    p = subprocess.run([CLI] + base + em + extra + ["-output", str(small)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FAMSEQ_BATCH="7"))
    assert p.returncode == 0, p.stdout + p.stderr
    assert open(small).read() == open(with_em).read()  # whatever the GPU batches are
    got, want = open(with_em).read().split("\n"), open(plain).read().split("\n")
    head = [l for l in got if l.startswith(("##INFO=<ID=FAF,Number=1,Type=Float", "##INFO=<ID=FAL,Number=1,Type=Float"))]
    assert len(head) == 2 and "%d EM steps from %g" % (STEPS, 0.5 if start is None else start) in head[0]
    got = [l for l in got if l not in head]
    assert len(got) == len(want)
    inputs = vcf_inputs(VCF, ped, None)
    sites = []
    for a, b in zip(got, want):
        t, u = a.split("\t"), b.split("\t")
        if not a or a.startswith("#") or len(t) < 9 or ":GPP:FPP:FGT" not in t[8]:
            assert a == b  # the header, and a line that is no site, as without -afEM
            continue
        info, keys = split_info(t[7])
        assert t[:7] == u[:7] and info == u[7] and t[8:] == u[8:]  # every other byte of the line
        if keys:  # joined at the end, a "." replaced
            assert t[7] == (u[7] + ";" if u[7] != "." else "") + ";".join(k + keys[k] for k in KEYS)
        if keys and extra:  # kSide's order
            order = [kv[:kv.index("=")] for kv in t[7].split(";") if kv.split("=")[0] in ("FQ", "FLL", "PSD", "PSR", "FAF", "FAL")]
            assert order == ["FQ", "FLL", "PSD", "PSR", "FAF", "FAL"]
        sites.append(((t[0], t[1]), keys))
    assert len(sites) >= 12
    lk = np.array([inputs[k][0] for k, _ in sites])
    flags = np.array([inputs[k][1] for k, _ in sites], np.uint8)
    ctx = fs.Context(fs.make_model(ped))
    af, ll, st = ctx.af_batch(0.5 if start is None else start, STEPS, lk=lk, flags=flags)
    ctx.close()
    assert (st == 0).sum() >= 12
    for s, (k, keys) in enumerate(sites):
        if st[s] != 0:
            assert not keys  # -siteQ's rule: a failed site does without the keys
        else:
            assert keys == {"FAF=": "%g" % af[s], "FAL=": "%g" % (ll[s, 0] - ll[s, 1])}, (k, keys, af[s], ll[s])


@pytest.mark.gpu
def test_cli_af_em_excluded_zero_and_a_failed_site(tmp_path):
    ped = fs.synthetic_pedigree("trio")
    mo, _ = ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    founder = [p for p in range(ped.n) if mo[p] < 0][0]
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"
    body = "1\t10\t.\tA\tC\t50\tPASS\t.\tGT:PL\t0/0:0,30,60\t0/1:20,0,40\t0/1:30,0,50\n"
    # a founder that cannot be hom-ref (a PL beyond the table: likelihood 0): the data exclude an allele frequency of 0
    cols = ["0/0:0,25,50"] * 3
    cols[founder] = "0/1:9000,0,40"
    body += "1\t20\t.\tA\tC\t50\tPASS\tDP=2\tGT:PL\t" + "\t".join(cols) + "\n"
    # a site whose single posterior fails: every PL beyond the table for one member
    body += "1\t40\t.\tA\tC\t50\tPASS\tDP=1\tGT:PL\t0/0:9000,9000,9000\t0/1:20,0,40\t0/0:0,25,50\n"
    open(vcf, "w").write(head + body)
    out = tmp_path / "o.vcf"
    run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-afEM", "0", "-afStart", "0.25"], out)
    lines = [l.split("\t") for l in open(out).read().split("\n") if l and not l.startswith("#")]
    assert len(lines) == 3 and lines[0][7].startswith("FAF=0.25;FAL=")  # no steps: the start value
    assert lines[1][7] == "DP=2;FAF=0.25;FAL=inf"
    assert lines[2][7] == "DP=1"  # the failed site keeps its INFO


def refused(args, tmp_path):
    out = tmp_path / "o.vcf"
    p = subprocess.run([CLI, "vcf", "-vcfFile", VCF, "-pedFile", PEDF, "-output", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and not out.exists(), p.stdout + p.stderr
    return p.stdout


def test_cli_af_em_refusals(tmp_path):
    """Said before any device is touched (this machine may have none)."""
    assert "-afEM takes the number of EM steps, 0..64" in refused(["-afEM", "65"], tmp_path)
    assert "-afEM takes the number of EM steps, 0..64" in refused(["-afEM", "1000"], tmp_path)
    assert "-afEM takes the number of EM steps, 0..64" in refused(["-afEM", "four"], tmp_path)
    assert "-afStart takes the allele frequency" in refused(["-afEM", "4", "-afStart", "0"], tmp_path)
    assert "-afStart takes the allele frequency" in refused(["-afEM", "4", "-afStart", "1"], tmp_path)
    assert "-afStart takes the allele frequency" in refused(["-afEM", "4", "-afStart", "x"], tmp_path)
    assert "-afStart belongs to -afEM" in refused(["-afStart", "0.3"], tmp_path)
    assert "-afTag cannot be combined" in refused(["-afEM", "4", "-afTag", "AF"], tmp_path)
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", PEDF, "-afEM", "4", "-output", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=300)
    assert "-afEM applies to vcf mode only; ignored here." in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-afEM T\t" in p.stdout + p.stderr and "-afStart" in p.stdout + p.stderr
