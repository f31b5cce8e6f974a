"""`FamSeq vcf -phase`: every sample column gains PGT (the genotype phased by transmission, maternal|paternal) and PGP (that pair's
posterior).  They are fs.phased_calls of Context.origin_batch on the rows the driver reads (under -afTagAll: origin_prior_batch on
the line's rows); a founder and a failed site print ".", a son's field at a chrX site is haploid, the header says the order, and
with the two fields taken off again the file is the run's without the option, byte for byte.  The refusals are said before a device
is touched: that part is not marked gpu.

The bar for PGP: the text holds six significant digits (%g), 5e-6 relative, beside the kernel's RTOL.  PGT is compared wherever
the row's two largest entries are further apart than that (a tie within rounding may fall either way between two routes to the
same rows: the driver's table of pow(10, -PL / 10) and numpy's)."""
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from test_cli_gpu import CLI, run_cli
from test_cli_relabel_gpu import write_family_vcf
from test_gpu_evidence import vcf_inputs

MRATE = 1e-7
BAR = 5e-6 + 1e-9


def expected(ped, vcf, af_key=None):
    """-> {(chrom, pos): (index[K], prob[K], origin[K, 4], status, flags)} from origin_batch on the rows the driver reads."""
    inputs = vcf_inputs(vcf, ped, af_key)
    keys = sorted(inputs, key=lambda k: int(k[1]))
    lk = np.array([inputs[k][0] for k in keys])
    flags = np.array([inputs[k][1] for k in keys], np.uint8)
    ctx = fs.Context(fs.make_model(ped, mrate=MRATE))
    if af_key:
        prior = P.model_rows(fs.make_model(ped, mrate=MRATE), flags)
        has = np.array([inputs[k][2] is not None for k in keys])
        assert has.any() and not has.all()
        prior[has] = fs.hwe_priors(np.array([inputs[k][2] for k in keys if inputs[k][2] is not None]))
        origin, _, st = ctx.origin_prior_batch(prior, lk=lk, flags=flags)
    else:
        origin, _, st = ctx.origin_batch(lk=lk, flags=flags)
    ctx.close()
    idx, prob = fs.phased_calls(origin)
    return {k: (idx[i], prob[i], origin[i], st[i], flags[i]) for i, k in enumerate(keys)}


def check_output(ped, out_with, out_plain, want, what):
    """-> (fields compared, haploid fields seen, failed sites seen)."""
    mo, _ = ped.relations()
    kids = [p for p in range(ped.n) if mo[p] >= 0]
    member = {nm: p for p, nm in enumerate(ped.names)}
    text = open(out_with).read()
    head = [l for l in text.splitlines() if l.startswith("##")]
    assert sum(l.startswith("##FORMAT=<ID=PGT,Number=1,Type=String") and "maternal|paternal" in l for l in head) == 1, what
    assert sum(l.startswith("##FORMAT=<ID=PGP,Number=1,Type=Float") for l in head) == 1, what
    stripped, compared, haploid, failed = [], 0, 0, 0
    cols = None
    for line in text.split("\n"):
        t = line.split("\t")
        if line.startswith("##FORMAT=<ID=PGT") or line.startswith("##FORMAT=<ID=PGP"):
            continue
        if line.startswith("#CHROM"):
            cols = [member[nm] for nm in t[9:] if nm]
        if line.startswith("#") or len(t) < 10:
            stripped.append(line)
            continue
        assert t[8].endswith(":PGT:PGP"), what
        idx, prob, origin, st, flags = want[(t[0], t[1])]
        failed += st != 0
        for j, p in enumerate(cols):
            f = t[9 + j].split(":")
            pgt, pgp = f[-2], f[-1]
            if mo[p] < 0 or st != 0:
                assert (pgt, pgp) == (".", "."), (what, line)
                continue
            k = kids.index(p)
            son_x = (flags & fs.FLAG_CHRX) and ped.genders[p] == 1
            haploid += bool(son_x)
            assert len(pgt) == (1 if son_x else 3) and (son_x or pgt[1] == "|"), (what, line)
            top = np.sort(origin[k])[::-1]
            got = 2 * int(pgt[0]) + (0 if son_x else int(pgt[2]))
            if top[0] - top[1] > BAR * top[0]:
                assert got == idx[k] and (not son_x or idx[k] in (0, 2)), (what, line, origin[k])
            assert abs(float(pgp) - origin[k][got]) <= BAR * origin[k][got], (what, line, origin[k])
            compared += 1
        stripped.append("\t".join([t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8][:-len(":PGT:PGP")]] +
                                  [c.rsplit(":", 2)[0] if c else c for c in t[9:]]))
    assert "\n".join(stripped) == open(out_plain).read(), what
    return compared, haploid, failed


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["trio", "ped10"])
def test_cli_phase(name, tmp_path):
    ped = fs.synthetic_pedigree(name)
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    write_family_vcf(ped, vcf, 21)
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7"]
    plain, phased = tmp_path / "plain.vcf", tmp_path / "phased.vcf"
    run_cli(base + ["-method", "2"], plain)
    assert "PGT" not in open(plain).read()
    run_cli(base + ["-phase"], phased)  # (implies -method 2)
    want = expected(ped, vcf)
    compared, haploid, failed = check_output(ped, phased, plain, want, name)
    mo, _ = ped.relations()
    sons = sum(1 for p in range(ped.n) if mo[p] >= 0 and ped.genders[p] == 1)
    assert compared > 150 and failed >= 1 and (haploid > 30 or sons == 0)
    # beside the other per-sample fields: theirs unchanged, PGT:PGP the last
    others = ["-dnm", "-map", "-loo", "-siteQ"]
    alone, both = tmp_path / "alone.vcf", tmp_path / "both.vcf"
    run_cli(base + others, alone)
    run_cli(base + others + ["-phase"], both)
    check_output(ped, both, alone, want, name + ", beside the other side outputs")


@pytest.mark.gpu
def test_cli_phase_with_site_priors(tmp_path):
    ped = fs.synthetic_pedigree("quad")
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    write_family_vcf(ped, vcf, 12, af=True)
    base = ["vcf", "-vcfFile", vcf, "-pedFile", pedf, "-mRate", "1e-7", "-afTagAll", "AF"]
    plain, phased = tmp_path / "plain.vcf", tmp_path / "phased.vcf"
    run_cli(base, plain)
    run_cli(base + ["-phase"], phased)
    want, without = expected(ped, vcf, "AF"), expected(ped, vcf)
    assert max(np.abs(want[k][2] - without[k][2]).max() for k in want if want[k][3] == 0) > 1e-3  # (the prior matters)
    compared, _, _ = check_output(ped, phased, plain, want, "quad, -afTagAll AF")
    assert compared > 150


def test_cli_phase_refusals(tmp_path):
    """Said before any input is read and before any device is touched (this machine may have none)."""
    from test_cli_mutrate_gpu import refused
    from test_gpu_denovo import four_loops

    assert "-afTag cannot be combined" in refused(["-phase", "-afTag", "AF"], tmp_path)
    loops = str(tmp_path / "loops.ped")
    pedmod.write_ped(four_loops(), loops)
    assert "-phase cannot serve this pedigree" in refused(["-phase"], tmp_path, loops)
    p = subprocess.run([CLI, "LK", "-lkFile", str(tmp_path / "none.txt"), "-pedFile", str(tmp_path / "quad.ped"), "-phase",
                        "-output", str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=300)
    assert "-phase applies to vcf mode only; ignored here." in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-phase\t\t(vcf) Add PGT" in p.stdout + p.stderr
