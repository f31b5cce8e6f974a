"""The pattern kernel on the device: famseq_pattern_batch_device with M = 2 (the `-seg both` case) and M = 8 patterns next to the
route users had before — M + 1 launches of famseq_evidence_batch_device, one on the batch as it is and one on a pre-masked copy
per pattern — on the same resident batch, in one process.

    python tools/pattern_rate.py [ped10_sites=10000000] [wide32_sites=2000000]

Per pedigree (ped10, 32 members): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM and its M masked copies, the
routes timed with HIP events, alternating, warmed up, REPS repetitions each; min, median and max.  Algorithmic bytes per site:
the pattern kernel reads 24 N + 1 once and writes 8 M + 9 (posteriors, loglik, status); a launch of famseq_evidence reads 24 N + 1
and writes 17, M + 1 times over.  The fraction is of 8 TB/s.  The yardstick is famseq_evidence in the same run: the pattern kernel
does the arithmetic of its M + 1 launches on one read of the rows, so it should not take more than 1.05 of their time, and
approaches one launch's where the passes hide under the memory time; more than 1.05 wants an explanation from
profiles/pattern/resources.txt.  The masks: a dominant and a recessive row for a random 40 % affected, and for M = 8
six rows that constrain up to six random members.
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


def make_masks(n, rng):
    aff = rng.permutation(n)[:max(1, int(round(0.4 * n)))]
    unaff = [p for p in range(n) if p not in set(aff)]
    rows = [fs.segregation_masks(n, aff, unaff, "dominant"), fs.segregation_masks(n, aff, unaff, "recessive")]
    for _ in range(6):
        row = np.full(n, 7, np.uint8)
        who = rng.permutation(n)[:rng.randint(1, 7)]
        row[who] = rng.randint(1, 8, len(who))
        rows.append(row)
    return np.stack(rows)


def device_rates(name, n):
    ped = wide_pedigree(32) if name == "wide32" else fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    nn = ped.n
    ctx = fs.Context(fs.make_model(ped))
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    masks = make_masks(nn, np.random.RandomState(7))
    keep = ((masks[:, :, None] >> np.arange(3)) & 1).astype(np.float64)
    copies = [lk * torch.from_numpy(k).to("cuda") for k in keep]  # the pre-masked rows of today's route
    t_masks = torch.from_numpy(masks).to("cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    llm = torch.empty(n, dtype=torch.float64, device="cuda")
    pp = torch.empty((n, len(masks)), dtype=torch.float64, device="cuda")
    one = lambda rows: ctx.evidence_batch_device(n, d_lk=rows.data_ptr(), d_flags=flags.data_ptr(), d_loglik=llm.data_ptr(), d_status=st.data_ptr())
    b_ev = 24 * nn + 1 + 9

    def pattern(m):
        return lambda: ctx.pattern_batch_device(n, t_masks.data_ptr(), m, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_pat_post=pp.data_ptr(),
                                                d_loglik=ll.data_ptr(), d_status=st.data_ptr())

    def route(m):
        def run():
            one(lk)
            for c in copies[:m]:
                one(c)
        return run

    runs = {"evidence, 1 launch": (lambda: one(lk), b_ev)}
    for m in (2, 8):
        runs["pattern, M = %d" % m] = (pattern(m), 24 * nn + 1 + 8 * m + 9)
        runs["evidence, %d launches (masked)" % (m + 1)] = (route(m), (m + 1) * b_ev)
    for _ in range(2):  # warm-up (the first loads the kernels)
        for f, _ in runs.values():
            timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS))
    med = {}
    for key, (_, b) in runs.items():
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-34s median %.3f ms  (min %.3f, max %.3f)  %5d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
    for m in (2, 8):
        r = med["pattern, M = %d" % m] / med["evidence, %d launches (masked)" % (m + 1)]
        print("  pattern, M = %d / evidence, %d launches (medians) = %.3f   -> %s;  / one launch = %.3f" %
              (m, m + 1, r, "not above the yardstick by more than 5 %" if r <= 1.05 else "MORE than 5 % above the yardstick",
               med["pattern, M = %d" % m] / med["evidence, 1 launch"]))
    # the two routes' numbers, M = 8: Z_m / Z against 10 ** (loglik_m - loglik)
    pattern(8)()
    torch.cuda.synchronize()
    ok = st == 0
    worst = 0.0
    for m, c in enumerate(copies):
        one(c)
        torch.cuda.synchronize()
        both = ok & (st == 0)
        want = 10.0 ** (llm[both] - ll[both])
        worst = max(worst, float(((pp[both, m] - want).abs() / want).max()))
    pattern(8)()
    torch.cuda.synchronize()
    plan = ctx.plan()
    print("  variants: pattern %s, evidence %s; status != 0 on %d sites; mean PSD %.6g, mean PSR %.6g; worst relative difference of the "
          "two routes %.3g" % (plan["pattern_variant"], plan["evidence_variant"], int((st != 0).sum()), float(pp[st == 0, 0].mean()),
                               float(pp[st == 0, 1].mean()), worst))
    ctx.close()
    del lk, flags, copies, st, ll, llm, pp
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
