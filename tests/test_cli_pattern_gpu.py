"""`FamSeq vcf -seg dominant|recessive|both -affected ... [-unaffected ...]`: PSD / PSR in the INFO column are
Context.pattern_batch's posteriors of the same sites to the six digits printed, every other byte of every line is the run's
without -seg, -afTagAll runs the site-prior form on the line's rows, and the option errors.  The refusals are said before a
device is touched: that part is not marked gpu."""
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from test_cli_gpu import CLI, TD, run_cli
from test_gpu_denovo import four_loops
from test_gpu_evidence import vcf_inputs

VCF, PEDF = TD + "/test_subset.vcf", TD + "/fam01.ped"
AFFECTED, UNAFFECTED = [9, 10, 5], [11, 1]  # PED IDs of fam01.ped (9-11 are the sequenced ones)
SEG = ["-seg", "both", "-affected", ",".join(map(str, AFFECTED)), "-unaffected", ",".join(map(str, UNAFFECTED))]
KEYS = ("PSD=", "PSR=")


def split_info(info):
    """-> (the INFO column without PSD / PSR, {key: text})."""
    kept = [kv for kv in info.split(";") if not kv.startswith(KEYS)]
    return (";".join(kept) if kept else "."), {kv[:4]: kv[4:] for kv in info.split(";") if kv.startswith(KEYS)}


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["-afTagAll", "AF", "-dnm", "-map", "-siteQ", "-loo"]])
def test_cli_seg(extra, tmp_path):
    ped = pedmod.read_ped(PEDF)
    ped.relations()
    base = ["vcf", "-vcfFile", VCF, "-pedFile", PEDF]
    plain, seg = tmp_path / "plain.vcf", tmp_path / "seg.vcf"
    run_cli(base + ["-method", "2"] + extra, plain)
    run_cli(base + SEG + extra, seg)  # (implies -method 2)
    got, want = open(seg).read().split("\n"), open(plain).read().split("\n")
    head = [l for l in got if l.startswith(("##INFO=<ID=PSD,Number=1,Type=Float", "##INFO=<ID=PSR,Number=1,Type=Float"))]
    assert len(head) == 2
    got = [l for l in got if l not in head]
    assert len(got) == len(want)
    inputs = vcf_inputs(VCF, ped, "AF" if extra else None)
    sites = []
    for a, b in zip(got, want):
        t, u = a.split("\t"), b.split("\t")
        if not a or a.startswith("#") or len(t) < 9 or ":GPP:FPP:FGT" not in t[8]:
            assert a == b  # the header, and a line that is no site, as without -seg
            continue
        info, keys = split_info(t[7])
        assert t[:7] == u[:7] and info == u[7] and t[8:] == u[8:]  # every other byte of the line
        if keys:  # joined at the end, a "." replaced
            assert t[7] == (u[7] + ";" if u[7] != "." else "") + ";".join(k + keys[k] for k in KEYS if k in keys)
        sites.append(((t[0], t[1]), keys))
    assert len(sites) >= 12
    lk = np.array([inputs[k][0] for k, _ in sites])
    flags = np.array([inputs[k][1] for k, _ in sites], np.uint8)
    ids = list(ped.ids)
    aff, unaff = [ids.index(i) for i in AFFECTED], [ids.index(i) for i in UNAFFECTED]
    masks = np.stack([fs.segregation_masks(ped.n, aff, unaff, m) for m in ("dominant", "recessive")])
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    if extra:
        prior = P.model_rows(model, flags)
        for s, (k, _) in enumerate(sites):
            if inputs[k][2] is not None:
                prior[s] = fs.hwe_priors([inputs[k][2]])[0]
        assert sum(inputs[k][2] is not None for k, _ in sites) >= 3
        pp, _, st = ctx.pattern_prior_batch(prior, masks, lk=lk, flags=flags)
        assert not np.array_equal(pp, ctx.pattern_batch(masks, lk=lk, flags=flags)[0])
    else:
        pp, _, st = ctx.pattern_batch(masks, lk=lk, flags=flags)
    ctx.close()
    assert (st == 0).sum() >= 12
    for s, (k, keys) in enumerate(sites):
        if st[s] != 0:
            assert not keys  # -siteQ's rule: a failed site does without the keys
        else:
            assert keys == {"PSD=": "%g" % pp[s, 0], "PSR=": "%g" % pp[s, 1]}, (k, keys, pp[s])


@pytest.mark.gpu
def test_cli_seg_one_model_and_a_failed_site(tmp_path):
    ped = fs.synthetic_pedigree("trio")
    mo, _ = ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"
    body = "1\t10\t.\tA\tC\t50\tPASS\t.\tGT:PL\t0/0:0,30,60\t0/1:20,0,40\t0/1:30,0,50\n"
    # a site whose single posterior fails: every PL beyond the table (likelihood 0) for one member
    body += "1\t40\t.\tA\tC\t50\tPASS\tDP=1\tGT:PL\t0/0:9000,9000,9000\t0/1:20,0,40\t0/0:0,25,50\n"
    open(vcf, "w").write(head + body)
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    out = tmp_path / "o.vcf"
    for model, key in (("dominant", "PSD"), ("recessive", "PSR")):
        run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-seg", model, "-affected", str(ped.ids[child])], out)
        text = open(out).read()
        assert ("##INFO=<ID=PSD" in text) == (key == "PSD") and ("##INFO=<ID=PSR" in text) == (key == "PSR")
        lines = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
        assert len(lines) == 2 and lines[0][7].startswith(key + "=") and 0.0 <= float(lines[0][7][4:]) <= 1.0
        assert lines[1][7] == "DP=1"  # the failed site keeps its INFO
    pedmod.write_ped(four_loops(), pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-seg", "both", "-affected", "1", "-output", str(tmp_path / "r.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-seg cannot serve this pedigree: " in p.stdout and "more than three" in p.stdout


def refused(args, tmp_path):
    out = tmp_path / "o.vcf"
    p = subprocess.run([CLI, "vcf", "-vcfFile", VCF, "-pedFile", PEDF, "-output", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and not out.exists(), p.stdout + p.stderr
    return p.stdout


def test_cli_seg_refusals(tmp_path):
    """Said before any device is touched (this machine may have none)."""
    assert "-seg needs the affected members" in refused(["-seg", "both"], tmp_path)
    assert "-seg needs the affected members" in refused(["-seg", "dominant", "-unaffected", "1"], tmp_path)
    assert '"99" is not an individual ID of the PED file' in refused(["-seg", "both", "-affected", "9,99"], tmp_path)
    assert '"x" is not an individual ID of the PED file' in refused(["-seg", "both", "-affected", "9", "-unaffected", "x"], tmp_path)
    assert "Individual 9 is listed both as affected and as unaffected" in refused(["-seg", "both", "-affected", "9,10", "-unaffected", "11,9"], tmp_path)
    assert "-seg takes dominant, recessive or both" in refused(["-seg", "additive", "-affected", "9"], tmp_path)
    assert "belong to -seg" in refused(["-affected", "9"], tmp_path)
    assert "-afTag cannot be combined" in refused(["-seg", "both", "-affected", "9", "-afTag", "AF"], tmp_path)
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", PEDF, "-seg", "both", "-affected", "9", "-output",
                        str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=300)
    assert "-seg applies to vcf mode only; ignored here." in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-seg MODEL\t" in p.stdout + p.stderr and "-affected" in p.stdout + p.stderr
