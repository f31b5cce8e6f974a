"""`FamSeq vcf -afTagAll KEY`: -afTag's prior of a line, applied to every field the line prints.  DNP, JGT / JP and FPP against
the Python binding's site-prior entries on the rows the option's rules imply, a file without the tag against plain -method 2
-dnm -map, and the refusal together with -afTag."""
import subprocess

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from famseq_amd import synth
from test_cli_prior_gpu import HEADER_LINE, N_LINES, case, phred, run  # noqa: F401  (case: the module's fixture, its VCFs)
from test_gpu_denovo import CLI, TD

pytestmark = pytest.mark.gpu

HEADER_ALL = HEADER_LINE[:-1] + " (-afTagAll: for every field of the line)\n"


def test_every_field_is_the_site_prior_entries(case):
    d, ped, pedf, vcf, _, pl, meta = case
    p = run(["-vcfFile", vcf, "-pedFile", pedf, "-afTagAll", "AF", "-dnm", "-map"], d / "all.vcf")
    assert p.returncode == 0, p.stdout + p.stderr
    model = fs.make_model(ped)
    flags = np.array([(fs.FLAG_KNOWN if k else 0) | (fs.FLAG_CHRX if x else 0) for _, x, k in meta], np.uint8)
    prior = P.model_rows(model, flags)
    for s, (af, _, _) in enumerate(meta):
        if af is not None:
            prior[s] = fs.hwe_priors([af])[0]
    with_af = np.array([af is not None for af, _, _ in meta])
    assert with_af.sum() >= 12 and (~with_af).sum() >= 12  # lines with and without a usable frequency, mixed
    lk = synth.pl_to_lk(pl)
    ctx = fs.Context(model, device=0)
    post, _, status = ctx.bn_prior_batch(lk, prior, flags)
    kids, _, dnm, tst = ctx.trio_prior_batch(prior, lk=lk, flags=flags, want_joint=False)
    jgt, jp, jst = ctx.map_prior_batch(prior, lk=lk, flags=flags)
    plain_dnm = ctx.trio_batch(lk=lk, flags=flags, want_joint=False)[2]
    ctx.close()
    assert not (status & 3).any() and not tst.any() and not jst.any()
    # (the option matters: under the model's rows the de novo posteriors of the lines with a frequency are others)
    assert not np.allclose(plain_dnm[with_af], dnm[with_af], rtol=1e-3, atol=0)
    text = open(d / "all.vcf").read()
    assert text.count(HEADER_ALL) == 1
    lines = [l for l in text.split("\n") if l and not l.startswith("#")]
    assert len(lines) == N_LINES
    gts = ["0/0", "0/1", "1/1"]
    kid_of = {int(c): k for k, c in enumerate(kids)}
    for s, line in enumerate(lines):
        t = line.split("\t")
        assert t[8] == "GT:PL:GPP:FPP:FGT:DNP:JGT:JP"
        for m in range(ped.n):
            f = t[9 + m].split(":")
            got = np.array([float(x) for x in f[3].split(",")])
            # six significant digits, and one unit of the sixth for a value that rounds the other way after the last bit of a log10
            np.testing.assert_allclose(got, [float("%g" % x) for x in phred(post[s, m])], rtol=2e-6, atol=0, err_msg="FPP %d %d" % (s, m))
            assert f[4] == gts[fs.call_genotypes(post[s, m])[0]], (s, m)
            if m in kid_of:
                assert f[5] == "%g" % dnm[s, kid_of[m]], (s, m)  # printed as computed: %g of the same double
            else:
                assert f[5] == "."
            assert f[6] == gts[jgt[s, m]] and f[7] == "%g" % jp[s], (s, m)


def test_a_file_without_the_tag_prints_what_plain_method_2_prints(case):
    """Byte for byte, but for the one ##FS header line that names the option."""
    d, _, pedf, _, vcf, _, _ = case
    a = run(["-vcfFile", vcf, "-pedFile", pedf, "-afTagAll", "AF", "-dnm", "-map"], d / "tagless_all.vcf")
    b = run(["-vcfFile", vcf, "-pedFile", pedf, "-method", "2", "-dnm", "-map"], d / "tagless_plain_joint.vcf")
    assert a.returncode == 0 and b.returncode == 0, a.stdout + a.stderr + b.stdout + b.stderr
    got, plain = open(d / "tagless_all.vcf").read(), open(d / "tagless_plain_joint.vcf").read()
    assert got.count(HEADER_ALL) == 1 and HEADER_LINE[:-1] not in plain
    assert got.replace(HEADER_ALL, "") == plain
    assert plain.count(":GPP:FPP:FGT:DNP:JGT:JP") == N_LINES


def test_refusals_and_notices(case, tmp_path):
    d, _, pedf, vcf, _, _, _ = case
    for args in (["-afTag", "AF", "-afTagAll", "AF"], ["-afTagAll", "AF", "-afTag", "AF"], ["-afTagAll", "AF", "-dnm", "-afTag", "AF"]):
        p = run(["-vcfFile", vcf, "-pedFile", pedf] + args, tmp_path / "o.vcf")
        assert p.returncode != 0 and "-afTag and -afTagAll cannot be combined" in p.stdout
        assert len([l for l in p.stdout.split("\n") if l]) == 1 and not (tmp_path / "o.vcf").exists()
    p = subprocess.run([CLI, "LK", "-lkFile", TD + "/loftest.txt", "-pedFile", TD + "/fam04.ped", "-afTagAll", "AF", "-output", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "-afTagAll applies to vcf mode only; ignored here." in p.stdout
    q = subprocess.run([CLI, "LK", "-lkFile", TD + "/loftest.txt", "-pedFile", TD + "/fam04.ped", "-output", str(tmp_path / "plain.txt")],
                       capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and open(tmp_path / "o.txt").read() == open(tmp_path / "plain.txt").read()
    p = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-afTagAll KEY\t" in p.stdout + p.stderr
