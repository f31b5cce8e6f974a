"""`FamSeq vcf -countDist carriers|alleles|homalt [-countOf ID[,ID...]]`: PCD in the INFO column is Context.count_batch's
distribution of the same sites, printed as FLL's value is; every other byte of every line is the run's without the option; the
output does not depend on FAMSEQ_BATCH; -afTagAll runs the site-prior form on the line's rows; a failed site prints "PCD=.";
and the option's refusals, which are said before a device is touched: that part is not marked gpu.

The command line forms its tables and its inverse transform with the C library's cos / sin and the binding with numpy's, which
may differ in the last bit, so the two distributions agree to the entry's own bar, 1e-12 absolute, not to the bit.  A printed
value has six significant digits: it lies within half a unit of the sixth, at most 5e-6 of the value, of what was printed from.
So every value is compared at 5e-6 relative plus 1e-12 absolute; and of the values of 1e-9 and more — a thousand times the
absolute bar: at least three of the six printed digits are the same number's in both — at least 99 in 100 texts are equal (the
others lie on a rounding edge of the sixth digit).  A value below that is rounding around an exact zero and has no digits to
compare."""
import os
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from famseq_amd import prebuild_sets as sets
from test_cli_gpu import CLI, TD, run_cli
from test_gpu_denovo import four_loops
from test_gpu_evidence import vcf_inputs

VCF, PEDF = TD + "/test_subset.vcf", TD + "/fam01.ped"
COUNT_OF = [9, 10, 3, 2]  # PED IDs of fam01.ped (9-11 are the sequenced ones)


def text_of(v):
    return "%g" % v


@pytest.mark.gpu
@pytest.mark.parametrize("kind, of, extra", [("carriers", None, []), ("alleles", COUNT_OF, []),
                                             ("alleles", COUNT_OF, ["-afTagAll", "AF", "-dnm", "-map", "-siteQ", "-mapQ"]),
                                             ("homalt", None, ["-afTagAll", "AF"])])
def test_cli_countdist(kind, of, extra, tmp_path):
    assert "fam01" in sets.CHARFN_PEDIGREES  # (build() has compiled its kernels)
    ped = pedmod.read_ped(PEDF)
    ped.relations()
    base = ["vcf", "-vcfFile", VCF, "-pedFile", PEDF]
    opt = ["-countDist", kind] + (["-countOf", ",".join(map(str, of))] if of else [])
    plain, with_pcd, small = tmp_path / "plain.vcf", tmp_path / "pcd.vcf", tmp_path / "small.vcf"
    run_cli(base + ["-method", "2"] + extra, plain)
    run_cli(base + opt + extra, with_pcd)  # (implies -method 2)
    p = subprocess.run([CLI] + base + opt + extra + ["-output", str(small)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FAMSEQ_BATCH="5"))
    assert p.returncode == 0, p.stdout + p.stderr
    assert open(small).read() == open(with_pcd).read()  # whatever the GPU batches are
    got, want = open(with_pcd).read().split("\n"), open(plain).read().split("\n")
    head = [l for l in got if l.startswith("##INFO=<ID=PCD,Number=.,Type=Float")]
    assert len(head) == 1
    got = [l for l in got if l not in head]
    assert len(got) == len(want)
    inputs = vcf_inputs(VCF, ped, "AF" if extra else None)
    sites = []
    for a, b in zip(got, want):
        t, u = a.split("\t"), b.split("\t")
        if not a or a.startswith("#") or len(t) < 9 or ":GPP:FPP:FGT" not in t[8]:
            assert a == b  # the header, and a line that is no site, as without -countDist
            continue
        kv = t[7].split(";")
        pcd = [x for x in kv if x.startswith("PCD=")]
        assert len(pcd) == 1 and kv[-1] == pcd[0]  # joined at the end
        rest = ";".join(kv[:-1]) if len(kv) > 1 else "."
        assert t[:7] == u[:7] and rest == u[7] and t[8:] == u[8:]  # every other byte of the line
        sites.append(((t[0], t[1]), pcd[0][4:].split(",")))
    assert len(sites) >= 12
    lk = np.array([inputs[k][0] for k, _ in sites])
    flags = np.array([inputs[k][1] for k, _ in sites], np.uint8)
    ids = list(ped.ids)
    scores = fs.count_scores(ped.n, [ids.index(i) for i in of] if of else None, kind)
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    prior = None
    if extra:
        prior = P.model_rows(model, flags)
        for s, (k, _) in enumerate(sites):
            if inputs[k][2] is not None:
                prior[s] = fs.hwe_priors([inputs[k][2]])[0]
        assert sum(inputs[k][2] is not None for k, _ in sites) >= 3
    dist, ll, st = ctx.count_batch(scores, lk=lk, flags=flags, prior=prior)
    if extra:
        assert not np.array_equal(dist, ctx.count_batch(scores, lk=lk, flags=flags)[0])
    ctx.close()
    assert (st == 0).sum() >= 12
    texts = equal = 0
    for s, (k, values) in enumerate(sites):
        if st[s] != 0:
            assert values == ["."], (k, values)  # a failed site: no value
            continue
        assert len(values) == dist.shape[1]
        for text, v in zip(values, dist[s]):
            if v >= 1e-9:
                texts, equal = texts + 1, equal + (text == text_of(v))
            assert abs(float(text) - v) <= 5e-6 * abs(v) + 1e-12, (k, text, v)
        assert abs(sum(float(x) for x in values) - 1.0) < 1e-5 * len(values)
    print("%s: %d of %d printed values of 1e-9 and more are the binding's text" % (kind, equal, texts))
    assert texts >= 3 * len(sites) // 2 and equal >= 0.99 * texts, (equal, texts)


@pytest.mark.gpu
def test_cli_countdist_a_failed_site_and_an_unserved_pedigree(tmp_path):
    ped = fs.synthetic_pedigree("trio")
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"
    body = "1\t10\t.\tA\tC\t50\tPASS\t.\tGT:PL\t0/0:0,30,60\t0/1:20,0,40\t0/1:30,0,50\n"
    # a site whose single posterior fails: every PL beyond the table (likelihood 0) for one member
    body += "1\t40\t.\tA\tC\t50\tPASS\tDP=1\tGT:PL\t0/0:9000,9000,9000\t0/1:20,0,40\t0/0:0,25,50\n"
    open(vcf, "w").write(head + body)
    out = tmp_path / "o.vcf"
    run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-countDist", "alleles"], out)
    text = open(out).read()
    assert "##INFO=<ID=PCD,Number=.,Type=Float" in text and "alternate alleles among all members" in text
    lines = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    assert len(lines) == 2
    values = [float(x) for x in lines[0][7][4:].split(",")]
    assert lines[0][7].startswith("PCD=") and len(values) == 7 and abs(sum(values) - 1.0) < 1e-5 and min(values) >= 0
    assert lines[1][7] == "DP=1;PCD=."  # the failed site: no value


def refused(args, tmp_path, pedf=PEDF):
    out = tmp_path / "o.vcf"
    p = subprocess.run([CLI, "vcf", "-vcfFile", VCF, "-pedFile", pedf, "-output", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and not out.exists(), p.stdout + p.stderr
    return p.stdout


def test_cli_countdist_refusals(tmp_path):
    """Said before any input is read and before any device is touched (this machine may have none)."""
    assert '-countDist takes carriers, alleles or homalt, not "hets".' in refused(["-countDist", "hets"], tmp_path)
    assert '-countDist takes carriers, alleles or homalt, not "".' in refused(["-countDist"], tmp_path)
    assert "-countOf belongs to -countDist carriers|alleles|homalt, which was not given." in refused(["-countOf", "9"], tmp_path)
    assert '-countOf: "99" is not an individual ID of the PED file.' in refused(["-countDist", "carriers", "-countOf", "9,99"], tmp_path)
    assert '-countOf: "x" is not an individual ID of the PED file.' in refused(["-countDist", "homalt", "-countOf", "x"], tmp_path)
    assert "-countOf: individual 9 is named twice." in refused(["-countDist", "alleles", "-countOf", "9,10,9"], tmp_path)
    assert "-countOf takes the members to count" in refused(["-countDist", "alleles", "-countOf"], tmp_path)
    assert "-afTag cannot be combined" in refused(["-countDist", "alleles", "-afTag", "AF"], tmp_path)
    # a count that needs more than 64 frequencies: 70 members' alleles reach 140
    wide = sets.wide_pedigree(70)
    pedf = str(tmp_path / "wide70.ped")
    pedmod.write_ped(wide, pedf)
    said = refused(["-countDist", "alleles"], tmp_path, pedf)
    assert "-countDist alleles: the count reaches D = 140, whose distribution needs 71 frequencies; one call takes at most 64." in said
    # ... which counting fewer members, or carriers, does not need: the next refusal is another one's
    assert "D = " not in refused(["-countDist", "carriers", "-countOf", "1,1"], tmp_path, pedf)
    # a pedigree the engine does not serve
    pedmod.write_ped(four_loops(), pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", VCF, "-pedFile", pedf, "-countDist", "carriers", "-output", str(tmp_path / "r.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-countDist cannot serve this pedigree: " in p.stdout and "more than three" in p.stdout
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", PEDF, "-countDist", "carriers", "-output",
                        str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=300)
    assert "-countDist applies to vcf mode only; ignored here." in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-countDist KIND\t" in p.stdout + p.stderr and "a male's genotype 2 at a chrX site counts 2" in p.stdout + p.stderr
