"""Trio posteriors and de novo mutation posteriors on the device: famseq_trio_batch / famseq_trio_batch_device, and
`FamSeq vcf -dnm`.  The arithmetic is checked against a brute-force enumeration (test_trio_host.brute_joint) and, on the
wide pedigrees, against the sum-product oracle's marginals."""
import os
import subprocess

import numpy as np
import pytest

import famseq_amd as fs
from famseq_amd import pedigree as pedmod
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree
from famseq_amd.synth import random_likelihoods
from test_trio_host import RTOL, brute_joint, check_dnm, check_joint, marginals_from_joint, wide_likelihoods

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "FamSeq")
TD = os.path.join(ROOT, "tests", "golden", "testdata")


def four_loops():
    """Four disjoint sib matings (1 x 2 -> 3, 4; 3 x 4 -> 5), twenty members: every loop needs its own conditioned member,
    one more than the engine takes."""
    ids, mids, fids, gen = [], [], [], []
    for b in range(4):
        o = 10 * b
        ids += [o + 1, o + 2, o + 3, o + 4, o + 5]
        mids += [0, 0, o + 2, o + 2, o + 4]
        fids += [0, 0, o + 1, o + 1, o + 3]
        gen += [1, 2, 1, 2, 1]
    return fs.Pedigree(ids, mids, fids, gen, ["s%d" % i for i in ids])


@pytest.mark.parametrize("seed", range(10))
def test_trio_batch_matches_the_enumeration(seed):
    rng, ped = random_pedigree(seed)
    ped.relations()
    mu = [1e-7, 1e-4, 0.0][seed % 3]
    lk, flags = random_likelihoods(rng, ped, 200)
    ctx = fs.Context(fs.make_model(ped, mrate=mu))
    children, joint, dnm, st = ctx.trio_batch(lk=lk, flags=flags)
    ctx.close()
    ref, ref_st = brute_joint(ped, mu, lk, flags)
    assert np.array_equal(st, ref_st)
    ok = st == 0
    check_joint(joint[ok], ref[ok])
    check_dnm(dnm[ok], ref[ok], children, ped.genders, flags[ok])
    if mu == 0:
        assert np.all(dnm[ok] == 0.0)
    assert np.all(np.isnan(joint[~ok])) and np.all(np.isnan(dnm[~ok]))


def ped10_batch(n, seed=3):
    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(seed)
    lk, flags = random_likelihoods(rng, ped, n)
    return ped, lk, flags


def test_batch_sizes_and_chunks():
    """Every site's result is its own: batches of 1, 63, 64, 65 and one chunk + 1 give the bits of the whole batch."""
    ped, lk, flags = ped10_batch(300)
    ctx = fs.Context(fs.make_model(ped, mrate=1e-4))
    _, j, d, st = ctx.trio_batch(lk=lk, flags=flags)
    for n in (1, 63, 64, 65):
        _, jn, dn, sn = ctx.trio_batch(lk=lk[:n], flags=flags[:n])
        assert np.array_equal(sn, st[:n])
        assert np.array_equal(jn.view(np.uint64), j[:n].view(np.uint64))
        assert np.array_equal(dn.view(np.uint64), d[:n].view(np.uint64))
    ctx.set_option("chunk_sites", 128)
    _, jc, dc, sc = ctx.trio_batch(lk=lk[:129], flags=flags[:129])
    ctx.close()
    assert np.array_equal(sc, st[:129])
    assert np.array_equal(jc.view(np.uint64), j[:129].view(np.uint64))
    assert np.array_equal(dc.view(np.uint64), d[:129].view(np.uint64))


def test_pl16_and_lk_give_the_same_bits():
    ped = fs.synthetic_pedigree("ped10")
    rng = np.random.RandomState(11)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    n = 500
    pl = rng.randint(0, 300, size=(n, len(seq), 3)).astype(np.uint16)
    pl[rng.rand(n, len(seq)) < 0.05] = fs.PL_MISSING
    flags = rng.randint(0, 4, n).astype(np.uint8)
    lk = np.ones((n, ped.n, 3))
    lut = np.array([10.0 ** (-k / 10.0) for k in range(4096)])  # the library's table: pow(10, -k / 10) through libm
    for c, p in enumerate(seq):
        miss = (pl[:, c] == fs.PL_MISSING).all(axis=1)
        lk[:, p] = np.where(miss[:, None], 1.0, lut[np.minimum(pl[:, c], 4095)])
    ctx = fs.Context(fs.make_model(ped))
    _, j1, d1, s1 = ctx.trio_batch(pl16=pl, seq_members=seq, flags=flags)
    _, j2, d2, s2 = ctx.trio_batch(lk=lk, flags=flags)
    ctx.close()
    assert np.array_equal(s1, s2) and (s1 == 0).sum() > 100
    assert np.array_equal(j1.view(np.uint64), j2.view(np.uint64))
    assert np.array_equal(d1.view(np.uint64), d2.view(np.uint64))


def test_device_entry_and_null_outputs():
    import torch

    ped, lk, flags = ped10_batch(1000, seed=5)
    ctx = fs.Context(fs.make_model(ped, mrate=1e-4))
    children, j, d, st = ctx.trio_batch(lk=lk, flags=flags)
    k = len(children)
    _, jo, dnone, so = ctx.trio_batch(lk=lk, flags=flags, want_dnm=False)
    _, jnone, do, _ = ctx.trio_batch(lk=lk, flags=flags, want_joint=False)
    assert dnone is None and jnone is None
    assert np.array_equal(so, st)
    assert np.array_equal(jo.view(np.uint64), j.view(np.uint64))
    assert np.array_equal(do.view(np.uint64), d.view(np.uint64))
    dev = torch.device("cuda")
    t_lk, t_fl = torch.from_numpy(lk).to(dev), torch.from_numpy(flags).to(dev)
    t_j = torch.full((len(lk), k, 27), -1.0, dtype=torch.float64, device=dev)
    t_d = torch.full((len(lk), k), -1.0, dtype=torch.float64, device=dev)
    t_s = torch.zeros(len(lk), dtype=torch.uint8, device=dev)
    ctx.trio_batch_device(len(lk), d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_joint=t_j.data_ptr(), d_dnm=t_d.data_ptr(),
                          d_status=t_s.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(t_s.cpu().numpy(), st)
    assert np.array_equal(t_j.cpu().numpy().view(np.uint64), j.view(np.uint64))
    assert np.array_equal(t_d.cpu().numpy().view(np.uint64), d.view(np.uint64))
    t_d2 = torch.full((len(lk), k), -1.0, dtype=torch.float64, device=dev)  # dnm only, no status
    ctx.trio_batch_device(len(lk), d_lk=t_lk.data_ptr(), d_flags=t_fl.data_ptr(), d_dnm=t_d2.data_ptr())
    torch.cuda.synchronize()
    ctx.close()
    assert np.array_equal(t_d2.cpu().numpy().view(np.uint64), d.view(np.uint64))


def test_four_conditioned_members_are_refused():
    ped = four_loops()
    ctx = fs.Context(fs.make_model(ped))
    lk = np.ones((4, ped.n, 3))
    with pytest.raises(fs.FamseqError, match=r"\(-1\).*three"):
        ctx.trio_batch(lk=lk)
    with pytest.raises(fs.FamseqError, match=r"\(-1\)"):
        ctx.trio_children()
    ctx.close()


@pytest.mark.parametrize("n", [24, 32, 48, 128])
def test_wide_pedigrees_marginals(n):
    import oracle.sum_product as sp

    ped = wide_pedigree(n)
    mo, fa = ped.relations()
    lk, flags = wide_likelihoods(ped, n)
    ctx = fs.Context(fs.make_model(ped))
    children, joint, dnm, st = ctx.trio_batch(lk=lk, flags=flags)
    ctx.close()
    post, _, ref_st = sp.pedigree_posterior(ped, lk, flags, lc=2.0)
    # (a site whose total weight sits at the bottom of the double range — fifty members that each contradict their parents
    # a little — underflows in one order of products and not in another: status 2 on one side only, rare)
    differ = (st == 0) != (ref_st == 0)
    assert differ.sum() <= 0.02 * len(st) and np.all(st[differ & (st != 0)] == 2)
    ok = (ref_st == 0) & (st == 0)
    assert ok.sum() > 100
    for p, rows in marginals_from_joint(joint[ok], children, mo, fa, ped.n).items():
        for r in rows:
            sel = post[ok, p] >= 1e-280
            np.testing.assert_allclose(r[sel], post[ok, p][sel], rtol=RTOL, atol=0)


# ---- the command line -------------------------------------------------------------------------------------------------

def planted_vcf(ped, n_sites, seed, path):
    """Mendelian sites with sharp PLs (the true genotype 0, the others 60 / 120), ~1 % of them with a planted de novo
    mutation (every member 0,120,250 except one child 200,0,200) and a few failed sites (a sample with an all-zero
    likelihood row).  -> (planted {site: member}, failed sites)."""
    rng = np.random.RandomState(seed)
    mo, fa = ped.relations()
    kids = [p for p in range(ped.n) if mo[p] >= 0]
    planted, failed = {}, set()
    lines = []
    for s in range(n_sites):
        g = np.zeros(ped.n, int)
        for p in parents_first(mo, fa):
            if mo[p] < 0:
                g[p] = rng.choice(3, p=[0.6, 0.3, 0.1])
            else:
                a = (0, 0, 1)[g[mo[p]]] if g[mo[p]] != 1 else rng.randint(2)
                b = (0, 0, 1)[g[fa[p]]] if g[fa[p]] != 1 else rng.randint(2)
                g[p] = a + b
        pls = []
        for p in range(ped.n):
            row = [60 * abs(h - g[p]) for h in range(3)]
            pls.append(row)
        r = rng.rand()
        if r < 0.01:
            c = kids[rng.randint(len(kids))]
            planted[s] = c
            pls = [[0, 120, 250] for _ in range(ped.n)]
            pls[c] = [200, 0, 200]
        elif r < 0.013:
            failed.add(s)
            pls[rng.randint(ped.n)] = [5000, 5000, 5000]
        cols = ["1", str(1 + s), ".", "A", "G", "50", "PASS", ".", "GT:PL"] + ["0/1:%d,%d,%d" % tuple(x) for x in pls]
        lines.append("\t".join(cols))
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.1\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"PL\">\n##INFO=<ID=X,Number=0,Type=Flag,Description=\"x\">\n"
                "##contig=<ID=1,length=1000000>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(ped.names) + "\n")
        f.write("\n".join(lines) + "\n")
    return planted, failed


def parents_first(mo, fa):
    order, done = [], set()
    while len(order) < len(mo):
        for p in range(len(mo)):
            if p not in done and (mo[p] < 0 or (mo[p] in done and fa[p] in done)):
                order.append(p)
                done.add(p)
    return order


def strip_dnp(text):
    out = []
    for line in text.split("\n"):
        if line.startswith("##FORMAT=<ID=DNP"):
            continue
        if line and not line.startswith("#"):
            t = line.split("\t")
            assert t[8].endswith(":DNP")
            t[8] = t[8][:-4]
            for i in range(9, len(t)):
                if t[i]:
                    t[i] = t[i].rsplit(":", 1)[0]
            line = "\t".join(t)
        out.append(line)
    return "\n".join(out)


@pytest.mark.parametrize("name", ["trio", "ped10"])
def test_cli_dnm(name, tmp_path):
    ped = fs.synthetic_pedigree(name)
    ped.relations()
    pedf, vcf = str(tmp_path / "p.ped"), str(tmp_path / "s.vcf")
    pedmod.write_ped(ped, pedf)
    planted, failed = planted_vcf(ped, 3000, 17, vcf)
    assert len(planted) > 10 and failed
    o1, o2 = str(tmp_path / "plain.vcf"), str(tmp_path / "dnm.vcf")
    subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", o1], check=True, capture_output=True, timeout=300)
    subprocess.run([CLI, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", o2, "-dnm"], check=True, capture_output=True, timeout=300)
    plain, dnm = open(o1).read(), open(o2).read()
    assert strip_dnp(dnm) == plain
    head = dnm.split("\n")
    i = [k for k, l in enumerate(head) if l.startswith("##FORMAT=<ID=FGT")][0]
    assert head[i + 1].startswith('##FORMAT=<ID=DNP,Number=1,Type=Float,Description="Posterior probability of a de novo mutation')
    mo, _ = ped.relations()
    col = {nm: p for p, nm in enumerate(ped.names)}
    title = [l for l in head if l.startswith("#CHROM")][0].split("\t")
    members = [col[nm] for nm in title[9:] if nm]
    low = total = 0
    for line in head:
        if not line or line.startswith("#"):
            continue
        t = line.split("\t")
        s = int(t[1]) - 1
        vals = [x.rsplit(":", 1)[1] for x in t[9:9 + len(members)]]
        if s in failed:
            assert all(v == "NA" for v in vals)
            continue
        for p, v in zip(members, vals):
            if mo[p] < 0:
                assert v == "."
            elif planted.get(s) == p:
                assert float(v) > 0.9, (s, p, v)
            else:
                total += 1
                low += float(v) < 1e-3
    assert low >= 0.99 * total


def test_cli_dnm_notice_and_refusal(tmp_path):
    p = subprocess.run([CLI, "LK", "-lkFile", TD + "/loftest.txt", "-pedFile", TD + "/fam04.ped", "-dnm", "-output", str(tmp_path / "o.txt")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "-dnm applies to vcf mode only" in p.stdout
    ped = four_loops()
    pedf = str(tmp_path / "loops.ped")
    pedmod.write_ped(ped, pedf)
    p = subprocess.run([CLI, "vcf", "-vcfFile", str(tmp_path / "absent.vcf"), "-pedFile", pedf, "-dnm", "-output", str(tmp_path / "o.vcf")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 255 and "-dnm cannot serve this pedigree" in p.stdout
