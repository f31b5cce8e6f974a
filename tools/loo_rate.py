"""The leave-one-out kernel on the device: famseq_loo_batch_device next to famseq_bn_batch_device (sum-product engine) on the
same resident batch, in one process; then the site-prior pair, famseq_loo_prior against famseq_elim_prior.

    python tools/loo_rate.py [ped10_sites=10000000] [wide32_sites=2000000]

Per pedigree (ped10, 32 members): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the kernels timed with HIP
events, alternating, warmed up, REPS repetitions each; min, median and max.  famseq_elim is timed twice: in the variant a
context takes for the pedigree (rows staged through LDS) and in its lane-shell variant of the same fence level (8-11: rows
straight from and to global memory in 8-byte per-lane accesses, the shell famseq_loo has), which is the closer comparison.
Algorithmic bytes per site: 24 N + 1 in (likelihood rows and the flags byte); out 32 N + 1 (loo rows, fit, status) or 48 N + 1
(famseq_elim: posterior and single posterior rows, status); the site-prior forms read 48 B more; the fraction is of 8 TB/s.
The yardstick is famseq_elim in the same run.  By bytes famseq_loo should take (56 N + 2) / (72 N + 2) of its time, about 0.78;
the time ratios are printed next to that.  At ten members the route users had before is timed too: N calls of
famseq_bn_batch_device, one per masked member (the rows' values do not move the kernel's time, so the batch is passed as it
is).
"""
import os
import sys
import tempfile
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import famseq_amd as fs  # noqa: E402
from famseq_amd import synth  # noqa: E402
from famseq_amd.prebuild_sets import wide_pedigree  # noqa: E402

PEAK = 8e12
REPS = 7
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 10_000_000, "wide32": int(args[1]) if len(args) > 1 else 2_000_000}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def race(title, runs, n, byte_ratio, subject, yardsticks):
    for _ in range(2):  # warm-up (the first loads the kernels)
        for f, _ in runs.values():
            timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            times[key].append(timed(f))
    print(title)
    med = {}
    for key, (_, b) in runs.items():
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-34s median %.3f ms  (min %.3f, max %.3f)  %4d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
    for y in yardsticks:
        ratio = med[subject] / med[y]
        print("  %s / %s (medians) = %.3f, by bytes %.3f   -> %s" %
              (subject, y, ratio, byte_ratio, "not above the yardstick by more than 5 %" if ratio <= 1.05 else "MORE than 5 % above the yardstick"))
    return med


def device_rates(name, n):
    ped = wide_pedigree(32) if name == "wide32" else fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    model = fs.make_model(ped)
    elim = fs.Context(model, engine=fs.ENGINE_ELIM)
    v = elim.plan()["elim_variant"]
    # famseq_elim's lane-shell variant of the same fence level, from a cache of its own (no note of it is left for later contexts)
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=tempfile.mkdtemp(prefix="loo_rate_"), FAMSEQ_VARIANT_ONLY=str(8 + (v & 3)))):
        lane = fs.Context(model, engine=fs.ENGINE_ELIM)
    assert lane.plan()["elim_variant"] == 8 + (v & 3)
    ctx = fs.Context(model)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    post = torch.empty_like(lk)
    single = torch.empty_like(lk)
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    loo = torch.empty_like(lk)
    fit = torch.empty((n, ped.n), dtype=torch.float64, device="cuda")
    io, nn = dict(d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_status=st.data_ptr()), ped.n
    b_loo, b_elim = 24 * nn + 1 + 32 * nn + 1, 24 * nn + 1 + 48 * nn + 1
    bn = lambda c: c.bn_batch_device(n, lk.data_ptr(), flags.data_ptr(), post.data_ptr(), single.data_ptr(), st.data_ptr())
    runs = {
        "loo (loo + fit)": (lambda: ctx.loo_batch_device(n, d_loo=loo.data_ptr(), d_fit=fit.data_ptr(), **io), b_loo),
        "elim v%d (post + single)" % v: (lambda: bn(elim), b_elim),
        "elim v%d, lane shell" % (8 + (v & 3)): (lambda: bn(lane), b_elim),
    }
    keys = list(runs)
    if nn == 10:
        def masked_route():
            for _ in range(nn):
                bn(elim)
        runs["elim, %d calls (masked rows)" % nn] = (masked_route, nn * b_elim)
    med = race("%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS), runs, n, b_loo / b_elim, keys[0], keys[1:])
    if nn == 10:
        print("  the masked-row route / loo (medians) = %.2f" % (med["elim, %d calls (masked rows)" % nn] / med[keys[0]]))
    ctx.loo_batch_device(n, d_loo=loo.data_ptr(), d_fit=fit.data_ptr(), **io)
    torch.cuda.synchronize()
    ok = st == 0
    print("  variants: loo %s, elim %s / %s; status != 0 on %d sites; mean fit %.6g" %
          (ctx.plan()["loo_variant"], v, lane.plan()["elim_variant"], int((~ok).sum()), float(fit[ok].mean())))
    # the site-prior pair: Hardy-Weinberg rows at allele frequencies log-uniform in (1e-4, 0.5)
    af = np.exp(np.random.RandomState(1).uniform(np.log(1e-4), np.log(0.5), 1 << 16))
    prior = torch.from_numpy(fs.hwe_priors(af)).to("cuda").repeat((n + (1 << 16) - 1) >> 16, 1)[:n].contiguous()
    runs = {
        "loo_prior": (lambda: ctx.loo_prior_batch_device(n, prior.data_ptr(), d_loo=loo.data_ptr(), d_fit=fit.data_ptr(), **io), b_loo + 48),
        "elim_prior": (lambda: elim.bn_prior_batch_device(n, lk.data_ptr(), flags.data_ptr(), prior.data_ptr(), post.data_ptr(), single.data_ptr(),
                                                          st.data_ptr()), b_elim + 48),
    }
    race("%s, founder priors per site:" % name, runs, n, (b_loo + 48) / (b_elim + 48), "loo_prior", ["elim_prior"])
    for c in (elim, lane, ctx):
        c.close()
    del lk, flags, post, single, st, loo, fit, prior
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
