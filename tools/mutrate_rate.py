"""The mutation-rate kernel on the device: famseq_mutrate_batch_device at R = 8 and R = 32 rates next to the route users had before —
R contexts, one made at each rate, each one famseq_evidence_batch_device launch on the same resident rows — on the same resident
batch, in one process.

    python tools/mutrate_rate.py [ped10_sites=10000000] [wide32_sites=2000000]

Per pedigree (ped10; 32 members): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the two routes timed with HIP
events, alternating, warmed up, REPS repetitions each; min, median and max.  Per route and R: the time, the bytes per site the
route has to move (rows and flags in once per launch, the outputs out), that over the median as a share of 8 TB/s; the cost of
one further pass of the fused kernel, (t(32) - t(8)) / 24; and the worst |difference| of the two routes' numbers over every site
and rate (the contract says 0: the same bits).  Nobody has fixed a ratio: the times are written down as they come.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import famseq_amd as fs  # noqa: E402
from famseq_amd import synth  # noqa: E402
from famseq_amd.prebuild_sets import wide_pedigree  # noqa: E402

REPS = 7
COUNTS = (8, 32)
HBM = 8e12  # bytes per second
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 10_000_000, "wide32": int(args[1]) if len(args) > 1 else 2_000_000}


def rate_grid(n):
    """n rates: 0 and log-spaced from 1e-9 to 1e-3."""
    return np.concatenate([[0.0], 10.0 ** np.linspace(-9, -3, n - 1)])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def device_rates(name, n):
    ped = wide_pedigree(32) if name == "wide32" else fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    nn = ped.n
    rates = rate_grid(max(COUNTS))
    ctx = fs.Context(fs.make_model(ped))
    ctx.set_option("mutrate_kernels", 1)
    per_rate = [fs.Context(fs.make_model(ped, mrate=float(r))) for r in rates]
    for c in per_rate:
        c.set_option("evidence_kernels", 1)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    tables = torch.from_numpy(ctx.rate_tables(rates)).to("cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    rl = torch.empty((n, max(COUNTS)), dtype=torch.float64, device="cuda")
    ev = torch.empty((max(COUNTS), n), dtype=torch.float64, device="cuda")  # the route's outputs, one array per context

    def fused(r):
        return lambda: ctx.mutrate_device(n, tables.data_ptr(), r, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_rate_loglik=rl.data_ptr(),
                                          d_loglik=ll.data_ptr(), d_status=st.data_ptr())

    def route(r):
        def run():
            for k in range(r):
                per_rate[k].evidence_batch_device(n, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_loglik=ev[k].data_ptr(), d_status=st.data_ptr())
        return run

    runs = {}
    for r in COUNTS:
        runs["mutrate, R = %d" % r] = fused(r)
        runs["evidence, %d contexts" % r] = route(r)
    for f in runs.values():  # warm-up (the first loads the kernels)
        timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, f in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS))
    row_in = 24 * nn + 1  # the site's rows and its flags
    moved = {}
    for r in COUNTS:
        moved["mutrate, R = %d" % r] = row_in + 8 * r + 8 + 1          # one read; R columns, loglik and status out
        moved["evidence, %d contexts" % r] = r * (row_in + 8 + 1)      # R reads; loglik and status out per launch
    med = {}
    for key in runs:
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-24s median %9.3f ms  (min %.3f, max %.3f)  %5d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], moved[key], moved[key] * n / med[key] / HBM))
    for r in COUNTS:
        print("  R = %2d: the fused kernel takes %.3f of the %d launches" % (r, med["mutrate, R = %d" % r] / med["evidence, %d contexts" % r], r))
    print("  one further pass: (t(32) - t(8)) / 24 = %.3f ms; one evidence launch: %.3f ms" %
          (1e3 * (med["mutrate, R = 32"] - med["mutrate, R = 8"]) / 24, 1e3 * med["evidence, 32 contexts"] / 32))
    # the two routes' numbers, every site and rate
    fused(max(COUNTS))()
    route(max(COUNTS))()
    torch.cuda.synchronize()
    good = st == 0
    a, b = rl[good], ev.t()[good]
    both = torch.isfinite(a) & torch.isfinite(b)
    same_inf = bool((torch.isfinite(a) == torch.isfinite(b)).all())
    worst = float((a[both] - b[both]).abs().max()) if bool(both.any()) else 0.0
    bits = bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all())
    plan = ctx.plan()
    print("  variants: mutrate %s, evidence %s; %d sites with status 0: worst |difference| of the two routes %.3g, -inf in the same places: %s, "
          "the same bits: %s" % (plan["mutrate_variant"], per_rate[0].plan()["evidence_variant"], int(good.sum()), worst, same_inf, bits))
    ctx.close()
    for c in per_rate:
        c.close()
    del lk, flags, tables, st, ll, rl, ev
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
