"""The relabelling kernel on the device: famseq_relabel_batch_device with n_assign = 1, 10 and 45 (the exchanges of two of ten
samples) next to the route users had before — n_assign + 1 launches of famseq_evidence_batch_device, one on the batch as it is and
one on a row-permuted copy per hypothesis, the copy made with torch on the device — on the same resident batch, in one process.

    python tools/relabel_rate.py [ped10_sites=10000000] [wide32_sites=2000000]

Per pedigree (ped10; 32 members, the first 45 pairs): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the routes
timed with HIP events, alternating, warmed up, REPS repetitions each; min, median and max.  The relabelling kernel is timed in
both of its forms where both exist (below forty members): the rows in the lanes' LDS rows (the default there) and the lean form,
which reads the site's row in global memory at each use (FAMSEQ_RELABEL_LEAN=1, a second context).  Today's route is timed whole
(a permuted copy into one scratch buffer, then the launch, per hypothesis: what a caller without 45 spare copies of the batch
does) and as its launches alone (on the unpermuted batch: what it would cost if the copies were free).  Nobody has fixed a ratio:
both are written down.  The two routes' numbers are compared bit for bit on the last hypothesis.
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

REPS = 5
COUNTS = (1, 10, 45)
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
    assign = fs.swap_assignments(nn)[0][:max(COUNTS)]
    ctx = fs.Context(fs.make_model(ped))
    os.environ["FAMSEQ_RELABEL_LEAN"] = "1"
    lean = fs.Context(fs.make_model(ped))
    lean.set_option("relabel_kernels", 1)  # (generated under the variable: the lean form's text, a code object of its own)
    del os.environ["FAMSEQ_RELABEL_LEAN"]
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    scratch = torch.empty_like(lk)
    t_assign = torch.from_numpy(assign).to("cuda")
    perms = [torch.from_numpy(a.astype(np.int64)).to("cuda") for a in assign]
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    lla = torch.empty(n, dtype=torch.float64, device="cuda")
    alt = torch.empty((n, len(assign)), dtype=torch.float64, device="cuda")
    one = lambda rows: ctx.evidence_batch_device(n, d_lk=rows.data_ptr(), d_flags=flags.data_ptr(), d_loglik=lla.data_ptr(), d_status=st.data_ptr())

    def relabel(c, m):
        return lambda: c.relabel_device(n, t_assign.data_ptr(), m, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_alt=alt.data_ptr(),
                                              d_loglik=ll.data_ptr(), d_status=st.data_ptr())

    def route(m, copies):
        def run():
            one(lk)
            for p in perms[:m]:
                if copies:
                    torch.index_select(lk, 1, p, out=scratch)
                one(scratch if copies else lk)
        return run

    runs = {"evidence, 1 launch": lambda: one(lk)}
    for m in COUNTS:
        runs["relabel, n_assign = %d (LDS rows)" % m] = relabel(ctx, m)
        runs["relabel, n_assign = %d (lean)" % m] = relabel(lean, m)
        runs["evidence, %d launches + copies" % (m + 1)] = route(m, True)
        runs["evidence, %d launches alone" % (m + 1)] = route(m, False)
    for f in runs.values():  # warm-up (the first loads the kernels)
        timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, f in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS))
    med = {}
    for key in runs:
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-38s median %8.3f ms  (min %.3f, max %.3f)" % (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1]))
    for m in COUNTS:
        for form in ("LDS rows", "lean"):
            t = med["relabel, n_assign = %d (%s)" % (m, form)]
            print("  n_assign = %2d, %-8s: %.3f of today's route with its copies, %.3f of its launches alone, %.2f launches of famseq_evidence" %
                  (m, form, t / med["evidence, %d launches + copies" % (m + 1)], t / med["evidence, %d launches alone" % (m + 1)],
                   t / med["evidence, 1 launch"]))
    # the two routes' numbers on the last hypothesis, and the two forms'
    relabel(ctx, max(COUNTS))()
    torch.cuda.synchronize()
    kept = alt.clone()
    torch.index_select(lk, 1, perms[-1], out=scratch)
    one(scratch)
    torch.cuda.synchronize()
    both = st == 0
    same = bool((kept[both, len(assign) - 1].view(torch.int64) == lla[both].view(torch.int64)).all())
    relabel(lean, max(COUNTS))()
    torch.cuda.synchronize()
    forms = bool((kept.view(torch.int64) == alt.view(torch.int64)).all())
    plan, lplan = ctx.plan(), lean.plan()
    print("  variants: relabel %s (lean %s), evidence %s; the last hypothesis equals famseq_evidence on the permuted "
          "copy bit for bit on %d sites: %s; the two forms give the same bits: %s" %
          (plan["relabel_variant"], lplan["relabel_variant"], plan["evidence_variant"], int(both.sum()), same, forms))
    ctx.close()
    lean.close()
    del lk, flags, scratch, st, ll, lla, alt, kept
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
