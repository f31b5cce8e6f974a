"""The site-prior forms of the trio and MAP kernels on the device: famseq_trio_prior_batch_device / famseq_map_prior_batch_device
next to famseq_trio_batch_device / famseq_map_batch_device on the same resident batch, in one process.

    python tools/prior_joint_rate.py [ped10_sites=10000000] [trio_sites=8000000]

Per pedigree (ped10, trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, Hardy-Weinberg prior rows for
allele frequencies drawn once; per output (the dnm-only trio form, the joint form, MAP) the plain and the site-prior kernel
timed with HIP events, alternating, warmed up, REPS repetitions each; medians, and the time ratio next to the byte ratio.
Algorithmic bytes per site: 24 N + 2 in (likelihood rows, flags; status out) plus the outputs — 8 K de novo posteriors, 216 K
joint posteriors, N + 8 for the MAP genotypes and their posterior — and 48 more for the site-prior forms (the prior row).  No
figure is expected in advance: nobody has timed a site-prior form of these kernels.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import famseq_amd as fs  # noqa: E402
from famseq_amd import synth  # noqa: E402

PEAK = 8e12
REPS = 7
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 10_000_000, "trio": int(args[1]) if len(args) > 1 else 8_000_000}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def device_rates(name, n):
    ped = fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    ctx = fs.Context(fs.make_model(ped))
    k = len(ctx.trio_children())
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    prior = torch.from_numpy(fs.hwe_priors(10.0 ** np.random.RandomState(1).uniform(-6, -0.001, n))).cuda()
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    base = 24 * ped.n + 2
    print("%s: N = %d, K = %d, %d sites, %d repetitions each, alternating" % (name, ped.n, k, n, REPS))
    for what, b_out in (("dnm", 8 * k), ("joint", 216 * k), ("map", ped.n + 8)):
        if what == "map":
            gt = torch.empty((n, ped.n), dtype=torch.int8, device="cuda")
            post = torch.empty(n, dtype=torch.float64, device="cuda")
            out = dict(d_map_gt=gt.data_ptr(), d_map_post=post.data_ptr())
            plain, site = ctx.map_batch_device, ctx.map_prior_batch_device
        else:
            buf = torch.empty((n, k * (1 if what == "dnm" else 27)), dtype=torch.float64, device="cuda")
            out = {"d_dnm" if what == "dnm" else "d_joint": buf.data_ptr()}
            plain, site = ctx.trio_batch_device, ctx.trio_prior_batch_device
        common = dict(d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_status=st.data_ptr(), **out)
        runs = {what: (lambda: plain(n, **common), base + b_out),
                what + "_prior": (lambda: site(n, prior.data_ptr(), **common), base + b_out + 48)}
        for _ in range(2):  # warm-up (the first loads the kernels)
            for f, _ in runs.values():
                timed(f)
        times = {key: [] for key in runs}
        for _ in range(REPS):
            for key, (f, _) in runs.items():
                times[key].append(timed(f))
        med = {}
        for key, (_, b) in runs.items():
            t = sorted(times[key])
            med[key] = t[len(t) // 2]
            print("  %-11s median %.3f ms  (min %.3f, max %.3f)  %4d B/site  %.3f of 8 TB/s" %
                  (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
        plan = ctx.plan()
        key = "map" if what == "map" else "trio"
        print("  %s_prior / %s (medians) = %.3f, bytes %.3f   (variants: plain %d, site-prior %d; status != 0 on %d sites)" %
              (what, what, med[what + "_prior"] / med[what], (base + b_out + 48) / (base + b_out), plan[key + "_variant"],
               plan[key + "_prior_variant"], int((st != 0).sum())))
        sys.stdout.flush()
        del out, common, runs
        if what == "map":
            del gt, post
        else:
            del buf
        torch.cuda.empty_cache()
    ctx.close()
    del lk, flags, prior, st
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "trio"):
        device_rates(name, SITES[name])
