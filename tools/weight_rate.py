"""The weight kernel on the device: famseq_weight_batch_device at M = 8 and M = 32 weight tables next to the route users had
before — M famseq_evidence_batch_device launches, each on a copy of the rows premultiplied by one table ahead of the timed region —
on the same resident batch, in one process.

    python tools/weight_rate.py [ped10_sites=4000000] [wide32_sites=1000000] [variant]

Per pedigree (ped10; 32 members): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the two routes timed with HIP
events, alternating, warmed up, REPS repetitions each; min, median and max.  Per route and M: the time, the bytes per site the
route has to move (rows and flags in once per launch, the outputs out; the old route's premultiplication, one read and one write
of the rows per table, is NOT in its time or its bytes), that over the median as a share of 8 TB/s; the cost of one further pass
of the fused kernel, (t(32) - t(8)) / 24; and whether the two routes give the same bits (the contract says they do).  The
premultiplied copies are M x the batch, which sets the site counts: 32 copies of 4 M ten-member sites are 31 GB.  Nobody has
fixed a ratio: the times are written down as they come.  variant: that fence level of both kernels instead of the contest's
(a site count of 0 leaves a pedigree out).
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
SITES = {"ped10": int(args[0]) if args else 4_000_000, "wide32": int(args[1]) if len(args) > 1 else 1_000_000}
VARIANT = args[2] if len(args) > 2 else None


def tables(n_members, m):
    """m weight tables: penetrance models on the first members, soft clamps, one with weights above 1."""
    rng = np.random.RandomState(5)
    w = np.ones((m, n_members, 3))
    for k in range(m):
        who = rng.permutation(n_members)[:6]
        if k % 3 == 0:
            w[k] = fs.penetrance_weights(n_members, who[:3], who[3:], (0.01 * (k + 1) / m, 0.8, 0.9))
        elif k % 3 == 1:
            w[k, who] = 10.0 ** rng.uniform(-3, 0, (6, 3))
        else:
            w[k, who[0]] = (2.0, 3.5, 0.25)
    return w


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
    mmax = max(COUNTS)
    w = tables(nn, mmax)
    ctx = fs.Context(fs.make_model(ped))
    if VARIANT is not None:
        os.environ["FAMSEQ_VARIANT_ONLY"] = VARIANT
    ctx.set_option("weight_kernels", 1)
    ctx.set_option("evidence_kernels", 1)
    os.environ.pop("FAMSEQ_VARIANT_ONLY", None)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    t_w = torch.from_numpy(w).to("cuda")
    pre = torch.empty((mmax,) + tuple(lk.shape), dtype=torch.float64, device="cuda")  # the old route's rows, made ahead
    for k in range(mmax):
        torch.mul(lk.view(n, nn, 3), t_w[k], out=pre[k].view(n, nn, 3))
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    st_ev = torch.empty(n, dtype=torch.uint8, device="cuda")
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    wl = torch.empty((n, mmax), dtype=torch.float64, device="cuda")
    ev = torch.empty((mmax, n), dtype=torch.float64, device="cuda")  # the route's outputs, one array per launch

    def fused(m):
        return lambda: ctx.weight_device(n, t_w.data_ptr(), m, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_wt_loglik=wl.data_ptr(),
                                         d_loglik=ll.data_ptr(), d_status=st.data_ptr())

    def route(m):
        def run():
            for k in range(m):
                ctx.evidence_batch_device(n, d_lk=pre[k].data_ptr(), d_flags=flags.data_ptr(), d_loglik=ev[k].data_ptr(), d_status=st_ev.data_ptr())
        return run

    runs = {}
    for m in COUNTS:
        runs["weight, M = %d" % m] = fused(m)
        runs["evidence, %d launches" % m] = route(m)
    for f in runs.values():  # warm-up (the first loads the kernels)
        timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, f in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS))
    row_in = 24 * nn + 1  # the site's rows and its flags
    moved = {}
    for m in COUNTS:
        moved["weight, M = %d" % m] = row_in + 8 * m + 8 + 1          # one read; M columns, loglik and status out
        moved["evidence, %d launches" % m] = m * (row_in + 8 + 1)     # M reads; loglik and status out per launch
    med = {}
    for key in runs:
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-24s median %9.3f ms  (min %.3f, max %.3f)  %5d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], moved[key], moved[key] * n / med[key] / HBM))
    for m in COUNTS:
        print("  M = %2d: the fused kernel takes %.3f of the %d launches" % (m, med["weight, M = %d" % m] / med["evidence, %d launches" % m], m))
    print("  one further pass: (t(32) - t(8)) / 24 = %.3f ms; one evidence launch: %.3f ms" %
          (1e3 * (med["weight, M = 32"] - med["weight, M = 8"]) / 24, 1e3 * med["evidence, 32 launches"] / 32))
    # the two routes' numbers, every site and table
    fused(mmax)()
    route(mmax)()
    torch.cuda.synchronize()
    good = st == 0
    a, b = wl[good], ev.t()[good]
    both = torch.isfinite(a) & torch.isfinite(b)
    worst = float((a[both] - b[both]).abs().max()) if bool(both.any()) else 0.0
    # (where the route's call fails on a good site Z_m is 0: -inf here, NaN there — not among the compared)
    comparable = ~torch.isnan(b)
    bits = bool((a.contiguous().view(torch.int64)[comparable] == b.contiguous().view(torch.int64)[comparable]).all())
    zeros = bool(torch.isneginf(a[~comparable]).all())
    plan = ctx.plan()
    print("  variants: weight %s, evidence %s; %d sites with status 0: worst |difference| of the two routes %.3g, the same bits: %s "
          "(%d entries the old route fails on: all -inf here: %s)" % (plan["weight_variant"], plan["evidence_variant"], int(good.sum()), worst, bits,
                                                                      int((~comparable).sum()), zeros))
    ctx.close()
    del lk, flags, t_w, pre, st, st_ev, ll, wl, ev
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        if SITES[name] > 0:
            device_rates(name, SITES[name])
        sys.stdout.flush()
