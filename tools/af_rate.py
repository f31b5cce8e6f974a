"""The allele-frequency kernel on the device: famseq_af_batch_device with T = 4 and T = 16 EM steps next to the route users had
before — T launches of famseq_bn_prior_batch_device, each followed by the update as torch elementwise operations on the founders'
rows, and one launch of famseq_evidence_prior_batch_device for the log-likelihood — on the same resident batch, in one process.
The route's T + 1 launches are also timed alone (the prior rows formed, no update): its floor, whoever writes the update.

    python tools/af_rate.py [ped10_sites=10000000] [wide32_sites=2000000]

Per pedigree (ped10, 32 members): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the routes timed with HIP
events, alternating, warmed up, REPS repetitions each; min, median and max.  Algorithmic bytes per site: the fused kernel reads
24 N + 9 once (rows, flag, start value) and writes 25 (af, loglik[2], status); a step of the route reads 24 N + 49 (rows, flag,
prior rows) and writes 48 N + 1 (posterior and single-posterior rows, status), T times over, and the evidence launch reads
24 N + 49 and writes 9.  The fraction is of 8 TB/s.  Reported beside the medians: the cost of one further pass of the fused
kernel, (t(16) - t(4)) / 12, and the two routes' largest relative difference in af.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import famseq_amd as fs  # noqa: E402
from famseq_amd import synth  # noqa: E402
from famseq_amd.prebuild_sets import wide_pedigree  # noqa: E402

PEAK = 8e12
REPS = 7
START = 0.5
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 10_000_000, "wide32": int(args[1]) if len(args) > 1 else 2_000_000}


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
    # (lc = 2: no site takes the posterior kernel's -LRC shortcut, whose rows are not the network's; the fused kernel has none)
    ctx = fs.Context(fs.make_model(ped, lc=2.0), engine=fs.ENGINE_ELIM)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    q0 = torch.full((n,), START, **f64)
    af, ll = torch.empty(n, **f64), torch.empty((n, 2), **f64)
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    # today's route: the prior rows, the posterior rows, the update on the founders' rows
    prior, post = torch.empty((n, 6), **f64), torch.empty((n, nn, 3), **f64)
    q, ll_r = torch.empty(n, **f64), torch.empty(n, **f64)
    founders = [p for p in range(nn) if mo[p] < 0]
    male = torch.tensor([ped.genders[f] == 1 for f in founders], device="cuda")
    idx = torch.tensor(founders, device="cuda")
    chrx = (flags & fs.FLAG_CHRX) != 0
    n_male = int(male.sum())
    c = torch.where(chrx, 2.0 * (len(founders) - n_male) + n_male, 2.0 * len(founders)).to(torch.float64)

    def rows(x):
        p = 1 - x
        prior[:, 0], prior[:, 1], prior[:, 2] = p * p, 2 * x * p, x * x
        prior[:, 3], prior[:, 4], prior[:, 5] = p, 0.0, x

    def fused(t):
        return lambda: ctx.af_batch_device(n, q0.data_ptr(), t, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_af=af.data_ptr(),
                                           d_loglik=ll.data_ptr(), d_status=st.data_ptr())

    def route(t, update=True):
        def run():
            q.copy_(q0)
            for _ in range(t):
                rows(q)
                ctx.bn_prior_batch_device(n, lk.data_ptr(), flags.data_ptr(), prior.data_ptr(), post.data_ptr(), 0, st.data_ptr())
                if not update:  # (the library's launches alone: what the route costs whoever writes the update as a kernel of its own)
                    continue
                m = post[:, idx]  # [n, founders, 3]
                num = torch.where(chrx[:, None] & male[None, :], m[:, :, 2], m[:, :, 1] + 2 * m[:, :, 2])
                q.copy_(torch.clamp((num / m.sum(dim=2)).sum(dim=1) / c, max=1.0))
            rows(q)
            ctx.evidence_prior_batch_device(n, prior.data_ptr(), d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_loglik=ll_r.data_ptr(),
                                            d_status=st.data_ptr())
        return run

    b_step, b_ev = 24 * nn + 49 + 48 * nn + 1, 24 * nn + 49 + 9
    runs = {}
    for t in (4, 16):
        runs["af, T = %d" % t] = (fused(t), 24 * nn + 9 + 25)
        runs["posteriors x %d + update + evidence" % t] = (route(t), t * b_step + b_ev)
        runs["  ... its %d launches alone" % (t + 1)] = (route(t, False), t * b_step + b_ev)
    for _ in range(2):  # warm-up (the first loads the kernels)
        for f, _ in runs.values():
            timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d (%d founders), %d sites, start %g, %d repetitions each, alternating" % (name, nn, len(founders), n, START, REPS))
    med = {}
    for key, (_, b) in runs.items():
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-38s median %.3f ms  (min %.3f, max %.3f)  %6d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
    for t in (4, 16):
        r = med["af, T = %d" % t] / med["posteriors x %d + update + evidence" % t]
        print("  af, T = %d / the route (medians) = %.3f   -> %s;  / its launches alone = %.3f" %
              (t, r, "below the route" if r < 1 else "NOT below the route", med["af, T = %d" % t] / med["  ... its %d launches alone" % (t + 1)]))
    print("  one further pass of the fused kernel, (t(16) - t(4)) / 12: %.3f ms" % (1e3 * (med["af, T = 16"] - med["af, T = 4"]) / 12))
    # the two routes' numbers, T = 4
    route(4)()
    fused(4)()
    torch.cuda.synchronize()
    ok = st == 0
    plan = ctx.plan()
    print("  variants: af %s, posteriors (site priors) %s, evidence (site priors) %s; status != 0 on %d sites; mean af %.6g; worst relative "
          "difference of the two routes in af %.3g, worst |difference| in loglik %.3g" %
          (plan["af_variant"], plan["prior_variant"], plan["evidence_prior_variant"], int((~ok).sum()), float(af[ok].mean()),
           float(((af[ok] - q[ok]).abs() / q[ok].clamp(min=1e-300)).max()), float((ll[ok, 0] - ll_r[ok]).abs().max())))
    ctx.close()
    del lk, flags, prior, post, q, af, ll, st
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
