"""`FamSeq vcf` with -dnm, -map, -siteQ, -loo, -sample and -seg together prints what each of them prints alone: every sample
column is the plain run's followed by each option's own fields in the order DNP, JGT:JP, LOP:LOF, SGT, the INFO column the
plain run's followed by -siteQ's and then -seg's keys, the header the plain one plus each option's lines.  The combined run
cuts its blocks at five lines, the others do not: a line's fields (its draws among them) do not depend on the blocks."""
import os
import subprocess

import pytest

from famseq_amd import pedigree as pedmod
import famseq_amd as fs
from test_cli_gpu import CLI, TD
from test_cli_pattern_gpu import SEG

SAMPLE = ["-sample", "3", "-seed", "7"]
FIELD_OPTIONS = ("dnm", "map", "loo", "sample")      # the order of their fields in a sample column
INFO_OPTIONS = ("siteQ", "seg")                      # the order of their keys in the INFO column
HEADER_OPTIONS = ("dnm", "map", "loo", "sample", "seg", "siteQ")  # the order of their header lines


def run(args, out, **env):
    p = subprocess.run([CLI, "vcf"] + args + ["-output", str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stdout + p.stderr
    lines = open(out).read().split("\n")
    assert lines[-1] == ""
    return [l for l in lines[:-1] if l.startswith("#")], [l for l in lines[:-1] if not l.startswith("#")]


def subset_input(tmp_path):
    return ["-vcfFile", TD + "/test_subset.vcf", "-pedFile", TD + "/fam01.ped", "-a"], SEG


def trio_input(tmp_path):
    """test_cli_seg_one_model_and_a_failed_site's file: two lines, founders' columns, the second site's call fails."""
    ped = fs.synthetic_pedigree("trio")
    mo, _ = ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    head = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n"
    body = "1\t10\t.\tA\tC\t50\tPASS\t.\tGT:PL\t0/0:0,30,60\t0/1:20,0,40\t0/1:30,0,50\n"
    body += "1\t40\t.\tA\tC\t50\tPASS\tDP=1\tGT:PL\t0/0:9000,9000,9000\t0/1:20,0,40\t0/0:0,25,50\n"
    open(vcf, "w").write(head + body)
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    return ["-vcfFile", vcf, "-pedFile", pedf], ["-seg", "both", "-affected", str(ped.ids[child])]


def added_keys(info, base):
    """What a run joined to the plain run's INFO column: "" where it left the column as it was."""
    if info == base:
        return ""
    if base == ".":
        return info
    assert info.startswith(base + ";")
    return info[len(base) + 1:]


@pytest.mark.gpu
@pytest.mark.parametrize("make_input", [subset_input, trio_input])
def test_cli_all_side_outputs_together(make_input, tmp_path):
    files, seg = make_input(tmp_path)
    base = files + ["-method", "2"]
    flags = {"dnm": ["-dnm"], "map": ["-map"], "siteQ": ["-siteQ"], "loo": ["-loo"], "sample": SAMPLE, "seg": seg}
    head0, body0 = run(base, tmp_path / "base.vcf")
    solo = {k: run(base + f, tmp_path / (k + ".vcf")) for k, f in flags.items()}
    head, body = run(base + [x for f in flags.values() for x in f], tmp_path / "all.vcf", FAMSEQ_BATCH="5")

    # the header: the plain one, each option's own lines behind the FGT line
    extra = {k: [l for l in solo[k][0] if l not in head0] for k in flags}
    assert all(extra.values())
    at = [i for i, l in enumerate(head0) if l.startswith("##FORMAT=<ID=FGT")][0] + 1
    assert head == head0[:at] + [l for k in HEADER_OPTIONS for l in extra[k]] + head0[at:]

    assert len(body) == len(body0) and all(len(solo[k][1]) == len(body0) for k in flags)
    n_sites = n_failed = n_founder = n_replaced = 0
    for q, (line, line0) in enumerate(zip(body, body0)):
        t, u = line.split("\t"), line0.split("\t")
        if len(u) < 10 or not u[8].endswith(":GPP:FPP:FGT"):
            assert line == line0  # a line that is no site, as without the options
            continue
        one = {k: solo[k][1][q].split("\t") for k in flags}
        n_sites += 1
        assert t[:7] == u[:7]
        assert t[8] == u[8] + ":DNP:JGT:JP:LOP:LOF:SGT"
        assert len(t) == len(u)
        for j in range(9, len(u)):
            want = u[j]
            for k in FIELD_OPTIONS:
                assert one[k][j].startswith(u[j])
                want += one[k][j][len(u[j]):]
            assert t[j] == want, (q, j)
        keys = [x for x in (added_keys(one[k][7], u[7]) for k in INFO_OPTIONS) if x]
        assert t[7] == (";".join(([] if u[7] == "." else [u[7]]) + keys) if keys else u[7]), (q, t[7])
        failed = u[9].endswith(":NA:NA:NA")
        n_failed += failed
        n_replaced += u[7] == "." and bool(keys)
        n_founder += any(one["dnm"][j] == u[j] + ":." for j in range(9, len(u) - 1))
        if failed:  # every field's failed branch, and an INFO column left alone
            assert t[7] == u[7] and all(t[j] == u[j] + ":NA:NA:NA:NA:NA:NA" for j in range(9, len(u) - 1))
    if make_input is trio_input:
        assert (n_sites, n_failed, n_founder, n_replaced) == (2, 1, 1, 1)
    else:
        assert n_sites >= 12
