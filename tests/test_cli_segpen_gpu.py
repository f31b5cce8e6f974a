"""`FamSeq vcf -segPen F0,F1,F2[/F0,F1,F2...] -affected ... [-unaffected ...]`: PSL in the INFO column is, per model, the
binding's four-term difference (wt_loglik - loglik) - (wt_loglik0 - loglik0) of the same sites — the second pair the same call
on all-ones rows with the line's flags and prior — to the six digits printed; the numerator of the model 0,1,1 is -seg
dominant's PSD; every other byte of every line is the run's without -segPen; the output does not depend on FAMSEQ_BATCH;
-afTagAll runs the site-prior form on the line's rows; and the option's refusals, which are said before a device is touched:
that part is not marked gpu."""
import os
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
MODELS = [(0.01, 0.8, 0.9), (0.0, 1.0, 1.0), (0.05, 0.5, 0.5)]
WHO = ["-affected", ",".join(map(str, AFFECTED)), "-unaffected", ",".join(map(str, UNAFFECTED))]
PEN = ["-segPen", "/".join(",".join("%g" % f for f in m) for m in MODELS)] + WHO


def text_of(v):
    return "." if np.isnan(v) else "%g" % v


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["-afTagAll", "AF", "-dnm", "-map", "-siteQ", "-loo", "-seg", "dominant"]])
def test_cli_segpen(extra, tmp_path):
    ped = pedmod.read_ped(PEDF)
    ped.relations()
    base = ["vcf", "-vcfFile", VCF, "-pedFile", PEDF]
    others = extra or ["-seg", "dominant"]  # (with or without -seg: the two lists serve both)
    plain, pen, small = tmp_path / "plain.vcf", tmp_path / "pen.vcf", tmp_path / "small.vcf"
    run_cli(base + ["-method", "2"] + ((others + WHO) if "-seg" in others else others), plain)
    run_cli(base + PEN + (extra or ["-seg", "dominant"]), pen)  # (implies -method 2)
    p = subprocess.run([CLI] + base + PEN + (extra or ["-seg", "dominant"]) + ["-output", str(small)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FAMSEQ_BATCH="5"))
    assert p.returncode == 0, p.stdout + p.stderr
    assert open(small).read() == open(pen).read()  # whatever the GPU batches are
    got, want = open(pen).read().split("\n"), open(plain).read().split("\n")
    head = [l for l in got if l.startswith("##INFO=<ID=PSL,Number=.,Type=Float")]
    assert len(head) == 1
    got = [l for l in got if l not in head]
    assert len(got) == len(want)
    inputs = vcf_inputs(VCF, ped, "AF" if extra else None)
    sites = []
    for a, b in zip(got, want):
        t, u = a.split("\t"), b.split("\t")
        if not a or a.startswith("#") or len(t) < 9 or ":GPP:FPP:FGT" not in t[8]:
            assert a == b  # the header, and a line that is no site, as without -segPen
            continue
        kv = t[7].split(";")
        psl = [x for x in kv if x.startswith("PSL=")]
        assert len(psl) == 1 and kv[-1] == psl[0]  # joined at the end
        rest = ";".join(kv[:-1]) if len(kv) > 1 else "."
        assert t[:7] == u[:7] and rest == u[7] and t[8:] == u[8:]  # every other byte of the line
        psd = [x[4:] for x in kv if x.startswith("PSD=")]
        sites.append(((t[0], t[1]), psl[0][4:].split(","), psd[0] if psd else None))
    assert len(sites) >= 12
    lk = np.array([inputs[k][0] for k, _, _ in sites])
    flags = np.array([inputs[k][1] for k, _, _ in sites], np.uint8)
    ids = list(ped.ids)
    aff, unaff = [ids.index(i) for i in AFFECTED], [ids.index(i) for i in UNAFFECTED]
    w = np.stack([fs.penetrance_weights(ped.n, aff, unaff, m) for m in MODELS])
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    ones = np.ones_like(lk)
    if extra:
        prior = P.model_rows(model, flags)
        for s, (k, _, _) in enumerate(sites):
            if inputs[k][2] is not None:
                prior[s] = fs.hwe_priors([inputs[k][2]])[0]
        assert sum(inputs[k][2] is not None for k, _, _ in sites) >= 3
        wl, ll, st = ctx.weight_prior_batch(prior, w, lk=lk, flags=flags)
        wl0, ll0, st0 = ctx.weight_prior_batch(prior, w, lk=ones, flags=flags)
        assert not np.array_equal(wl0, ctx.weight_batch(w, lk=ones, flags=flags)[0])
    else:
        wl, ll, st = ctx.weight_batch(w, lk=lk, flags=flags)
        wl0, ll0, st0 = ctx.weight_batch(w, lk=ones, flags=flags)
    ctx.close()
    assert (st == 0).sum() >= 12 and np.all(st0 == 0)
    np.testing.assert_allclose(ll0, 0.0, rtol=0, atol=1e-9)  # all-ones rows: the priors and the transmissions sum to 1
    with np.errstate(invalid="ignore"):
        null = wl0 - ll0[:, None]
        value = np.where((st != 0)[:, None] | ~np.isfinite(null), np.nan, (wl - ll[:, None]) - null)
    compared = 0
    for s, (k, texts, psd) in enumerate(sites):
        assert texts == [text_of(v) for v in value[s]], (k, texts, value[s])
        if st[s] != 0:
            assert texts == ["."] * len(MODELS) and psd is None  # a failed site: no value
        elif psd is not None and float(psd) > 0:  # the corner 0,1,1: its numerator is -seg dominant's posterior (six digits printed)
            assert abs(10.0 ** (wl[s, 1] - ll[s]) / float(psd) - 1.0) < 1e-5, (k, psd)
            compared += 1
        elif psd is not None:
            assert np.isneginf(wl[s, 1]) and texts[1] == "-inf"
            compared += 1
    assert compared >= 12


@pytest.mark.gpu
def test_cli_segpen_an_impossible_model_a_failed_site_and_an_unserved_pedigree(tmp_path):
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
    # the second model gives the affected child no genotype at all: its numerator and its null are both 0 — no value
    run_cli(["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-segPen", "0,1,1/0,0,0/1,1,1", "-affected", str(ped.ids[child])], out)
    text = open(out).read()
    assert "##INFO=<ID=PSL,Number=.,Type=Float" in text and "##INFO=<ID=PSD" not in text
    lines = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    assert len(lines) == 2
    first = lines[0][7][4:].split(",")
    assert lines[0][7].startswith("PSL=") and np.isfinite(float(first[0])) and first[1] == "." and float(first[2]) == 0.0
    assert lines[1][7] == "DP=1;PSL=.,.,."  # the failed site: no value
    pedmod.write_ped(four_loops(), pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-segPen", "0,1,1", "-affected", "1", "-output", str(tmp_path / "r.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-segPen cannot serve this pedigree: " in p.stdout and "more than three" in p.stdout


def refused(args, tmp_path):
    out = tmp_path / "o.vcf"
    p = subprocess.run([CLI, "vcf", "-vcfFile", VCF, "-pedFile", PEDF, "-output", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and not out.exists(), p.stdout + p.stderr
    return p.stdout


def test_cli_segpen_refusals(tmp_path):
    """Said before any device is touched (this machine may have none)."""
    for bad in ("0,1", "0,1,1,1", "0,1,1.5", "-0.1,1,1", "0,x,1", "0,,1", "nan,0,1"):
        assert '-segPen takes penetrance models F0,F1,F2[/F0,F1,F2...], three numbers in [0, 1] each, not "%s".' % bad in \
            refused(["-segPen", "0.1,0.5,0.9/" + bad, "-affected", "9"], tmp_path)
    assert 'each, not "".' in refused(["-segPen", "0,1,1/", "-affected", "9"], tmp_path)
    assert 'each, not "".' in refused(["-affected", "9", "-segPen"], tmp_path)
    many = "/".join(["0,1,1"] * 33)
    assert "-segPen takes at most 32 models, not 33." in refused(["-segPen", many, "-affected", "9"], tmp_path)
    assert "-segPen needs the affected members: -affected ID[,ID...] (PED IDs)." in refused(["-segPen", "0,1,1"], tmp_path)
    assert "-segPen needs the affected members" in refused(["-segPen", "0,1,1", "-unaffected", "1"], tmp_path)
    assert '-affected: "99" is not an individual ID of the PED file.' in refused(["-segPen", "0,1,1", "-affected", "9,99"], tmp_path)
    assert '-unaffected: "x" is not an individual ID of the PED file.' in refused(["-segPen", "0,1,1", "-affected", "9", "-unaffected", "x"], tmp_path)
    assert "Individual 9 is listed both as affected and as unaffected." in \
        refused(["-segPen", "0,1,1", "-affected", "9,10", "-unaffected", "11,9"], tmp_path)
    assert "-afTag cannot be combined" in refused(["-segPen", "0,1,1", "-affected", "9", "-afTag", "AF"], tmp_path)
    # with neither -seg nor -segPen the message for stray lists is the one it was; with -seg its own refusals come first
    assert "-affected and -unaffected belong to -seg dominant|recessive|both, which was not given." in refused(["-affected", "9"], tmp_path)
    assert "-seg takes dominant, recessive or both" in refused(["-seg", "additive", "-segPen", "0,1,1", "-affected", "9"], tmp_path)
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", PEDF, "-segPen", "0,1,1", "-affected", "9", "-output",
                        str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=300)
    assert "-segPen applies to vcf mode only; ignored here." in p.stdout and "-seg applies" not in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-segPen MODELS\t" in p.stdout + p.stderr
