"""Trio / de novo posteriors on the device: famseq_trio_batch_device next to famseq_bn_batch_device (sum-product engine) on
the same resident batch, in one process; then whole-process `FamSeq vcf` with and without -dnm.

    python tools/denovo_rate.py [n_sites=10000000] [cli_sites=3000000]

Per pedigree (ped10, trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the kernels timed with HIP events,
alternating (elim, trio dnm-only, trio joint) and repeated.  Algorithmic bytes per site: 24 N + 1 in (likelihood rows and the
flags byte), out 8 K (dnm) or 216 K (joint) + 1 (status); the fraction is of 8 TB/s.  The first-call compile time of the trio
kernel is measured on an empty kernel cache (a scratch FAMSEQ_KERNEL_CACHE, in a child process).
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import famseq_amd as fs  # noqa: E402
from famseq_amd import pedigree, synth  # noqa: E402

PEAK = 8e12
args = [a for a in sys.argv[1:]]
n = int(args[0]) if args else 10_000_000
cli_n = int(args[1]) if len(args) > 1 else 3_000_000
REPS = 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def compile_time(name):
    code = ("import time, numpy as np, famseq_amd as fs\n"
            "ctx = fs.Context(fs.make_model(fs.synthetic_pedigree(%r)))\n"
            "t0 = time.time(); ctx.set_option('trio_kernels', 1); print('%%.2f' %% (time.time() - t0))\n" % name)
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FAMSEQ_KERNEL_CACHE=d, PYTHONPATH=ROOT),
                             capture_output=True, text=True, timeout=600, check=True)
    return float(out.stdout.split()[-1])


def device_rates(name):
    ped = fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    model = fs.make_model(ped)
    elim = fs.Context(model, engine=fs.ENGINE_ELIM)
    trio = fs.Context(model)
    k = len(trio.trio_children())
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    post = torch.empty_like(lk)
    single = torch.empty_like(lk)
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    dnm = torch.empty((n, k), dtype=torch.float64, device="cuda")
    joint = torch.empty((n, k, 27), dtype=torch.float64, device="cuda")
    runs = {
        "elim (post + single)": (lambda: elim.bn_batch_device(n, lk.data_ptr(), flags.data_ptr(), post.data_ptr(), single.data_ptr(), st.data_ptr()),
                                 24 * ped.n + 1 + 48 * ped.n + 1),
        "trio dnm-only": (lambda: trio.trio_batch_device(n, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_dnm=dnm.data_ptr(),
                                                         d_status=st.data_ptr()), 24 * ped.n + 1 + 8 * k + 1),
        "trio joint": (lambda: trio.trio_batch_device(n, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_joint=joint.data_ptr(),
                                                      d_status=st.data_ptr()), 24 * ped.n + 1 + 216 * k + 1),
    }
    for f, _ in runs.values():  # warm-up (loads the kernels)
        timed(f)
    best = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            best[key].append(timed(f))
    print("%s: N = %d, K = %d, %d sites (elim variant %s, trio variant %s)" % (name, ped.n, k, n, elim.plan()["elim_variant"],
                                                                             trio.plan()["trio_variant"]))
    for key, (_, b) in runs.items():
        t = sorted(best[key])
        print("  %-22s median %.3f ms  (min %.3f, max %.3f)  %4d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * t[len(t) // 2], 1e3 * t[0], 1e3 * t[-1], b, b * n / t[len(t) // 2] / PEAK))
    med = {key: sorted(v)[len(v) // 2] for key, v in best.items()}
    print("  trio dnm-only / elim = %.2f   trio joint / elim = %.2f" % (med["trio dnm-only"] / med["elim (post + single)"],
                                                                       med["trio joint"] / med["elim (post + single)"]))
    elim.close()
    trio.close()
    del lk, flags, post, single, st, dnm, joint
    torch.cuda.empty_cache()


def cli_rates():
    ped = pedigree.synthetic_pedigree("ped10")
    mo, fa = ped.relations()
    with tempfile.TemporaryDirectory() as d:
        pedf, vcf = os.path.join(d, "p.ped"), os.path.join(d, "s.vcf")
        pedigree.write_ped(ped, pedf)
        pl, known, geno = synth.gen_sites(mo, fa, cli_n, synth.SEED_BASE + 2)  # the sites of tools/cli_throughput.py
        synth.write_vcf(vcf, ped.names, pl, known, geno)
        cli = os.path.join(ROOT, "bin", "FamSeq")
        for rep in range(2):
            for extra in ([], ["-dnm"]):
                out = os.path.join(d, "o.vcf")
                if os.path.exists(out):
                    os.unlink(out)
                t0 = time.time()
                subprocess.run([cli, "vcf", "-vcfFile", vcf, "-pedFile", pedf, "-output", out] + extra, check=True,
                               stdout=subprocess.DEVNULL, timeout=600)
                t = time.time() - t0
                print("FamSeq vcf %-5s %d sites: %.2f s  %.2f M sites/s%s" % (" ".join(extra) or "", cli_n, t, cli_n / t / 1e6,
                                                                            "   [first run]" if rep == 0 else ""), flush=True)


if __name__ == "__main__":
    print("trio kernel, first call on an empty cache: ped10 %.2f s, trio %.2f s" % (compile_time("ped10"), compile_time("trio")), flush=True)
    for name in ("ped10", "trio"):
        device_rates(name)
        sys.stdout.flush()
    if cli_n:
        cli_rates()
