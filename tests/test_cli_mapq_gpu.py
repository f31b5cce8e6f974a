"""`FamSeq vcf -mapQ`: the JGQ field and the JP2 key against Context.maxmarg_batch + joint_call_quality on the same PLs, 99999 for
an infinite quality, NA on failed sites, the header lines, the site-prior form under -afTagAll, the refusal with -afTag, and —
without the flag — the output as it was."""
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from famseq_amd import synth
from test_cli_map_gpu import strip_fields
from test_cli_prior_gpu import N_LINES, case, run  # noqa: F401  (case: that module's fixture, its ten-member VCFs with AF keys)
from test_gpu_denovo import CLI, four_loops, planted_vcf

pytestmark = pytest.mark.gpu

N_SITES = 400
FAILED, CERTAIN = 7, 11  # the planted sites: a sample without any likelihood; a sample whose genotype is certain


def printed(x):
    """What the shared %g formatter prints of a quality: 99999 for +inf."""
    return "99999" if np.isinf(x) else "%g" % x


def strip_info(text, key):
    """Drop `key`=<value> from every INFO column (and its ##INFO line)."""
    out = []
    for line in text.split("\n"):
        if line.startswith("##INFO=<ID=%s," % key):
            continue
        if line and not line.startswith("#"):
            t = line.split("\t")
            kept = [kv for kv in t[7].split(";") if not kv.startswith(key + "=")]
            t[7] = ";".join(kept) if kept else "."
            line = "\t".join(t)
        out.append(line)
    return "\n".join(out)


@pytest.fixture(scope="module")
def vcf_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("mapq")
    ped = fs.synthetic_pedigree("ped10")
    ped.relations()
    pedf, vcf = str(d / "p.ped"), str(d / "s.vcf")
    pedmod.write_ped(ped, pedf)
    _, failed = planted_vcf(ped, N_SITES, 23, vcf)
    lines = open(vcf).read().split("\n")
    first = [k for k, l in enumerate(lines) if l.startswith("#CHROM")][0] + 1
    for site, pls in ((FAILED, "5000,5000,5000"), (CERTAIN, "0,5000,5000")):
        t = lines[first + site].split("\t")
        assert int(t[1]) == site + 1
        t[9 + 2] = "0/1:" + pls
        lines[first + site] = "\t".join(t)
    open(vcf, "w").write("\n".join(lines))
    return d, ped, pedf, vcf, failed | {FAILED}


def library_inputs(ped, vcf, n_sites):
    """The VCF's PLs as the library takes them: (pl16 [S, n_seq, 3], members in VCF column order)."""
    pl, members = None, None
    for line in open(vcf):
        t = line.rstrip("\n").split("\t")
        if line.startswith("#CHROM"):
            col = {nm: p for p, nm in enumerate(ped.names)}
            members = np.array([col[nm] for nm in t[9:]], np.int32)
            pl = np.zeros((n_sites, len(members), 3), np.uint16)
        elif line and not line.startswith("#"):
            for j in range(len(members)):
                pl[int(t[1]) - 1, j] = [min(int(x), 0xFFFE) for x in t[9 + j].split(":")[1].split(",")]
    return pl, members


@pytest.mark.parametrize("extra", [[], ["-map", "-dnm", "-siteQ"]])
def test_jgq_and_jp2_are_the_librarys(vcf_case, extra):
    d, ped, pedf, vcf, failed = vcf_case
    o1, o2 = str(d / ("plain%d.vcf" % len(extra))), str(d / ("mapq%d.vcf" % len(extra)))
    subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", o1, "-method", "2"] + extra, check=True, capture_output=True, timeout=300)
    subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", o2, "-mapQ"] + extra, check=True, capture_output=True, timeout=300)
    text = open(o2).read()
    # (implies -method 2; everything but its own field, key and header lines byte for byte: JGQ stands last in a column, JP2 last in INFO)
    assert strip_info(strip_fields(text, ["JGQ"]), "JP2") == open(o1).read()
    head = [l for l in text.split("\n") if l.startswith("##")]
    assert sum(l.startswith('##FORMAT=<ID=JGQ,Number=1,Type=Float,Description="Quality of the sample\'s genotype in the most probable joint') for l in head) == 1
    assert sum(l.startswith('##INFO=<ID=JP2,Number=1,Type=Float,Description="Posterior probability of the second most probable joint') for l in head) == 1
    pl, members = library_inputs(ped, vcf, N_SITES)
    ctx = fs.Context(fs.make_model(ped))
    mm, top, st = ctx.maxmarg_batch(pl16=pl, seq_members=members, flags=np.zeros(N_SITES, np.uint8))
    jgt_map = ctx.map_batch(pl16=pl, seq_members=members, flags=np.zeros(N_SITES, np.uint8))[0]
    ctx.close()
    assert set(np.nonzero(st)[0]) == failed and FAILED in failed
    jgt, jgq = fs.joint_call_quality(mm)
    assert np.isposinf(jgq[CERTAIN, members[2]]) and np.isfinite(jgq[st == 0]).sum() > 0.9 * (st == 0).sum() * ped.n
    gts = ["0/0", "0/1", "1/1"]
    seen = infinite = 0
    for line in text.split("\n"):
        if not line or line.startswith("#"):
            continue
        t = line.split("\t")
        assert t[8].endswith(":JGQ") and (":JGT:JP" in t[8]) == bool(extra)
        s = int(t[1]) - 1
        fields = [x.split(":") for x in t[9:9 + len(members)]]
        info = dict(kv.split("=") for kv in t[7].split(";") if "=" in kv)
        if s in failed:
            assert all(f[-1] == "NA" for f in fields) and "JP2" not in info
            continue
        for j, p in enumerate(members):
            assert fields[j][-1] == printed(jgq[s, p]), (s, j, fields[j][-1], jgq[s, p])
            infinite += fields[j][-1] == "99999"
            if extra:  # JGT stays the MAP kernel's
                assert fields[j][-3] == gts[jgt_map[s, p]]
        assert info["JP2"] == "%g" % top[s, 1], (s, info["JP2"], top[s, 1])
        seen += 1
    assert seen == N_SITES - len(failed) and infinite >= 1


def test_under_aftagall_the_site_prior_form(case):
    d, ped, pedf, vcf, _, pl, meta = case
    p = run(["-vcfFile", vcf, "-pedFile", pedf, "-afTagAll", "AF", "-mapQ", "-map"], d / "mapq_all.vcf")
    assert p.returncode == 0, p.stdout + p.stderr
    model = fs.make_model(ped)
    flags = np.array([(fs.FLAG_KNOWN if k else 0) | (fs.FLAG_CHRX if x else 0) for _, x, k in meta], np.uint8)
    prior = P.model_rows(model, flags)
    for s, (af, _, _) in enumerate(meta):
        if af is not None:
            prior[s] = fs.hwe_priors([af])[0]
    with_af = np.array([af is not None for af, _, _ in meta])
    lk = synth.pl_to_lk(pl)
    ctx = fs.Context(model, device=0)
    mm, top, st = ctx.maxmarg_prior_batch(prior, lk=lk, flags=flags)
    plain = ctx.maxmarg_batch(lk=lk, flags=flags)
    jp = ctx.map_prior_batch(prior, lk=lk, flags=flags)[1]
    plan = ctx.plan()
    ctx.close()
    assert plan["maxmarg_prior_code_object"].endswith(".hsaco") and not st.any()
    assert np.array_equal(top[:, 0].view(np.uint64), jp.view(np.uint64))
    assert not np.allclose(plain[1][with_af, 1], top[with_af, 1], rtol=1e-3, atol=0)  # (the option matters)
    _, jgq = fs.joint_call_quality(mm)
    lines = [l for l in open(d / "mapq_all.vcf").read().split("\n") if l and not l.startswith("#")]
    assert len(lines) == N_LINES
    for s, line in enumerate(lines):
        t = line.split("\t")
        assert t[8] == "GT:PL:GPP:FPP:FGT:JGT:JP:JGQ"
        info = dict(kv.split("=") for kv in t[7].split(";") if "=" in kv)
        assert info["JP2"] == "%g" % top[s, 1], s
        for m in range(ped.n):
            f = t[9 + m].split(":")
            assert f[-1] == printed(jgq[s, m]) and f[-2] == "%g" % jp[s], (s, m)


def test_refusals_and_notices(case, tmp_path):
    d, _, pedf, vcf, _, _, _ = case
    absent = str(tmp_path / "absent.vcf")  # refused before input is read
    p = run(["-vcfFile", absent, "-pedFile", pedf, "-mapQ", "-afTag", "AF"], tmp_path / "o.vcf")
    assert p.returncode == 255 and "-afTag cannot be combined with -dnm or -map" in p.stdout and not (tmp_path / "o.vcf").exists()
    loops = str(tmp_path / "loops.ped")
    pedmod.write_ped(four_loops(), loops)
    p = run(["-vcfFile", absent, "-pedFile", loops, "-mapQ"], tmp_path / "o.vcf")
    assert p.returncode == 255 and "-mapQ cannot serve this pedigree" in p.stdout and "more than three" in p.stdout
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-mapQ\t" in p.stdout + p.stderr
