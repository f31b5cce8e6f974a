"""`FamSeq vcf -map`: the JGT / JP fields against Context.map_batch on the same PLs, the header lines, failed sites, the field
order with -dnm, and — without the flag — the existing goldens."""
import os
import subprocess

import numpy as np
import pytest

import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from test_cli_gpu import REF, TD, assert_same_output, run_cli
from test_gpu_denovo import CLI, four_loops, planted_vcf

pytestmark = pytest.mark.gpu

JGT = {"0/0": 0, "0/1": 1, "1/1": 2}


def strip_fields(text, names):
    """Drop the trailing FORMAT fields `names` (and their ##FORMAT lines) from a result file's text.  (A line without PLs is
    echoed as it came and carries no result fields.)"""
    out = []
    tail = ":" + ":".join(names)
    for line in text.split("\n"):
        if any(line.startswith("##FORMAT=<ID=%s," % nm) for nm in names):
            continue
        if line and not line.startswith("#"):
            t = line.split("\t")
            if ":GPP:FPP:FGT" in t[8]:
                assert t[8].endswith(tail), t[8]
                t[8] = t[8][:-len(tail)]
                for i in range(9, len(t)):
                    if t[i]:
                        t[i] = t[i].rsplit(":", len(names))[0]
                line = "\t".join(t)
        out.append(line)
    return "\n".join(out)


@pytest.mark.parametrize("fam", [1, 4, 6])
def test_testdata_without_and_with_the_flag(fam, tmp_path):
    args = ["vcf", "-vcfFile", TD + "/test_subset.vcf", "-pedFile", "%s/fam%02d.ped" % (TD, fam), "-method", "1"]
    plain, mapped = tmp_path / "plain.vcf", tmp_path / "map.vcf"
    run_cli(args, plain)
    assert assert_same_output(plain, "%s/subset_fam%02d_plain.vcf" % (REF, fam)) >= 12  # what test_cli_gpu.py checks today
    run_cli(args + ["-map"], mapped)
    text = open(mapped).read()
    assert strip_fields(text, ["JGT", "JP"]) == open(plain).read()  # everything else byte for byte
    head = text.split("\n")
    i = [k for k, l in enumerate(head) if l.startswith("##FORMAT=<ID=FGT")][0]
    assert head[i + 1].startswith('##FORMAT=<ID=JGT,Number=1,Type=String,Description="Genotype in the most probable joint')
    assert head[i + 2].startswith('##FORMAT=<ID=JP,Number=1,Type=Float,Description="Posterior probability of that joint')
    n = 0
    for line in head:
        if not line or line.startswith("#"):
            continue
        t = line.split("\t")
        if ":GPP:FPP:FGT" not in t[8]:
            continue
        assert t[8].endswith(":GPP:FPP:FGT:JGT:JP")
        cols = [x for x in t[9:] if x]
        fields = [x.rsplit(":", 2)[1:] for x in cols]
        jps = {f[1] for f in fields}
        assert len(jps) == 1  # the same number in every column of a line
        if jps == {"NA"}:
            assert all(f[0] == "NA" for f in fields)
            continue
        assert all(f[0] in JGT for f in fields) and 0 < float(jps.pop()) <= 1
        n += 1
    assert n >= 12


@pytest.mark.parametrize("name,extra", [("trio", []), ("ped10", []), ("ped10", ["-dnm"])])
def test_synthetic_vcf_against_map_batch(name, extra, tmp_path):
    ped = fs.synthetic_pedigree(name)
    ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    n_sites = 3000
    planted, failed = planted_vcf(ped, n_sites, 23, vcf)
    assert failed
    o1, o2 = str(tmp_path / "plain.vcf"), str(tmp_path / "map.vcf")
    subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", o1] + extra, check=True, capture_output=True, timeout=300)
    subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", o2, "-map"] + extra, check=True, capture_output=True,
                   timeout=300)
    text = open(o2).read()
    assert strip_fields(text, ["JGT", "JP"]) == open(o1).read()  # with -dnm: DNP stays where it was, JGT:JP after it
    lines = text.split("\n")
    title = [l for l in lines if l.startswith("#CHROM")][0].split("\t")
    col = {nm: p for p, nm in enumerate(ped.names)}
    members = np.array([col[nm] for nm in title[9:] if nm], np.int32)
    # the same PLs through the library
    pl = np.zeros((n_sites, len(members), 3), np.uint16)
    src = {}
    for line in open(vcf):
        if line.startswith("#"):
            if line.startswith("#CHROM"):
                src = {nm: k for k, nm in enumerate(line.rstrip("\n").split("\t")[9:])}
            continue
        t = line.rstrip("\n").split("\t")
        for j, p in enumerate(members):
            pl[int(t[1]) - 1, j] = [min(int(x), 0xFFFE) for x in t[9 + src[ped.names[p]]].split(":")[1].split(",")]
    ctx = fs.Context(fs.make_model(ped))
    gt, post, st = ctx.map_batch(pl16=pl, seq_members=members, flags=np.zeros(n_sites, np.uint8))
    ctx.close()
    assert set(np.nonzero(st)[0]) == failed
    want_tag = ":GPP:FPP:FGT" + (":DNP" if extra else "") + ":JGT:JP"
    seen = 0
    for line in lines:
        if not line or line.startswith("#"):
            continue
        t = line.split("\t")
        assert t[8].endswith(want_tag)
        s = int(t[1]) - 1
        fields = [x.rsplit(":", 2)[1:] for x in t[9:9 + len(members)]]
        if s in failed:
            assert all(f == ["NA", "NA"] for f in fields)
            continue
        assert [JGT[f[0]] for f in fields] == gt[s, members].tolist(), s
        assert all(f[1] == "%g" % post[s] for f in fields), (s, fields[0][1], "%g" % post[s])
        seen += 1
    assert seen == n_sites - len(failed)


def test_notice_and_refusal(tmp_path):
    p = subprocess.run([CLI, "LK", "-lkFile", TD + "/loftest.txt", "-pedFile", TD + "/fam04.ped", "-map", "-output", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "-map applies to vcf mode only" in p.stdout
    assert_same_output(tmp_path / "o.txt", REF + "/loftest_fam04.txt")
    pedf = str(tmp_path / "loops.ped")
    pedmod.write_ped(four_loops(), pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", str(tmp_path / "absent.vcf"), "-pedFile", pedf, "-map", "-output", str(tmp_path / "o.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-map cannot serve this pedigree" in p.stdout and "more than three" in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-map\t" in p.stdout + p.stderr
