"""`FamSeq vcf -afTag KEY`: the founders' prior of a line from the allele frequency in its INFO column.  The FPP / FGT columns
against Context.bn_prior_batch on the rows the option's rules imply, a file without the tag against plain -method 2, and the
refusal together with -dnm."""
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from famseq_amd import synth
from test_gpu_denovo import CLI

pytestmark = pytest.mark.gpu

# INFO column -> the allele frequency the line runs with (None: the model's rows, by the ID column)
INFOS = (("AF=0.3", 0.3), ("DP=10", None), ("AF=0", None), ("AF=1", None), ("AF=0.2,0.1", 0.2), ("AF=abc", None),
         ("DP=7;AF=0.01;AN=20", 0.01), ("MAF=0.4", None), ("AF=1e-4", 1e-4), (".", None))
N_LINES = 40
HEADER_LINE = "##FS genotype frequency of a site with 0 < AF < 1 in INFO: Hardy-Weinberg at that allele frequency\n"


def phred(p):  # the drivers' |-10 log10 p| with +inf -> 99999 (tests/test_gpu_variants.py)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(-10 * np.log10(p))
    return np.where(np.isinf(q), 99999.0, q)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """A ten-member VCF of N_LINES sites: every INFO form above, chrX lines, known and unknown IDs, mixed line by line."""
    d = tmp_path_factory.mktemp("af")
    ped = fs.synthetic_pedigree("ped10")
    mo, fa = ped.relations()
    pl, _, geno = synth.gen_sites(mo, fa, N_LINES, 5)
    pedf = str(d / "p.ped")
    pedmod.write_ped(ped, pedf)
    gt = ["0/0", "0/1", "1/1"]
    head = ["##fileformat=VCFv4.1", '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="PL">',
            "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + list(ped.names))]
    rows, meta = [], []
    for s in range(N_LINES):
        info, af = INFOS[s % len(INFOS)]
        chrx, known = s % 4 == 3, (s // 2) % 3 == 0  # ten INFO forms against periods of four and six: every combination met
        cols = ["X" if chrx else str(1 + s % 22), str(100 + s), "rs%d" % s if known else ".", "A", "G", "50", "PASS", info, "GT:PL"]
        cols += ["%s:%d,%d,%d" % ((gt[geno[s, p]],) + tuple(int(x) for x in pl[s, p])) for p in range(ped.n)]
        rows.append("\t".join(cols))
        meta.append((af, chrx, known))
    with_tag, without = str(d / "with.vcf"), str(d / "without.vcf")
    open(with_tag, "w").write("\n".join(head + rows) + "\n")
    open(without, "w").write("\n".join(head + [r.replace("\t" + INFOS[i % len(INFOS)][0] + "\t", "\t.\t") if "AF=" in INFOS[i % len(INFOS)][0]
                                               else r for i, r in enumerate(rows)]) + "\n")
    assert "AF=" not in open(without).read()
    return d, ped, pedf, with_tag, without, pl, meta


def run(args, out):
    return subprocess.run([CLI, "vcf"] + args + ["-output", str(out)], capture_output=True, text=True, timeout=300)


def test_fpp_and_fgt_are_bn_prior_batchs(case):
    d, ped, pedf, vcf, _, pl, meta = case
    p = run(["-vcfFile", vcf, "-pedFile", pedf, "-afTag", "AF", "-method", "2"], d / "af.vcf")
    assert p.returncode == 0, p.stdout + p.stderr
    model = fs.make_model(ped)
    flags = np.array([(fs.FLAG_KNOWN if k else 0) | (fs.FLAG_CHRX if x else 0) for _, x, k in meta], np.uint8)
    prior = P.model_rows(model, flags)
    for s, (af, _, _) in enumerate(meta):
        if af is not None:
            prior[s] = fs.hwe_priors([af])[0]
    assert sum(af is not None for af, _, _ in meta) >= 12 and len({tuple(r) for r in prior}) == 6  # four frequencies, the model's N and K rows
    ctx = fs.Context(model, device=0)
    post, _, status = ctx.bn_prior_batch(synth.pl_to_lk(pl), prior, flags)
    ctx.close()
    assert not (status & 3).any()
    text = open(d / "af.vcf").read()
    assert text.count(HEADER_LINE) == 1
    lines = [l for l in text.split("\n") if l and not l.startswith("#")]
    assert len(lines) == N_LINES
    gts = ["0/0", "0/1", "1/1"]
    for s, line in enumerate(lines):
        t = line.split("\t")
        assert t[8] == "GT:PL:GPP:FPP:FGT"
        for p_ in range(ped.n):
            f = t[9 + p_].split(":")
            got = np.array([float(x) for x in f[3].split(",")])
            want = np.array([float("%g" % x) for x in phred(post[s, p_])])
            # six significant digits, and one unit of the sixth for a value that rounds the other way after the last bit of a log10
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=0, err_msg="site %d member %d" % (s, p_))
            assert f[4] == gts[fs.call_genotypes(post[s, p_])[0]], (s, p_)


def test_a_file_without_the_tag_prints_what_plain_method_2_prints(case):
    """Byte for byte, but for the one ##FS header line that names the tag."""
    d, _, pedf, _, vcf, _, _ = case
    a = run(["-vcfFile", vcf, "-pedFile", pedf, "-afTag", "AF", "-method", "2"], d / "tagless_af.vcf")
    b = run(["-vcfFile", vcf, "-pedFile", pedf, "-method", "2"], d / "tagless_plain.vcf")
    assert a.returncode == 0 and b.returncode == 0, a.stdout + a.stderr + b.stdout + b.stderr
    got, plain = open(d / "tagless_af.vcf").read(), open(d / "tagless_plain.vcf").read()
    assert got.count(HEADER_LINE) == 1 and HEADER_LINE not in plain
    assert got.replace(HEADER_LINE, "") == plain
    assert plain.count(":GPP:FPP:FGT") == N_LINES


def test_refusals_and_notices(case, tmp_path):
    d, _, pedf, vcf, _, _, _ = case
    for other in ("-dnm", "-map"):
        p = run(["-vcfFile", vcf, "-pedFile", pedf, "-afTag", "AF", other], tmp_path / "o.vcf")
        assert p.returncode != 0 and "-afTag cannot be combined with -dnm or -map" in p.stdout
        assert len([l for l in p.stdout.split("\n") if l]) == 1 and not (tmp_path / "o.vcf").exists()
    from test_gpu_denovo import four_loops

    loops = str(tmp_path / "loops.ped")
    pedmod.write_ped(four_loops(), loops)
    p = run(["-vcfFile", vcf, "-pedFile", loops, "-afTag", "AF"], tmp_path / "o.vcf")
    assert p.returncode == 255 and "-afTag cannot serve this pedigree" in p.stdout and "more than three" in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-afTag KEY\t" in p.stdout + p.stderr
