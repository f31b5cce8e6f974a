"""The characteristic-function kernel on the device: famseq_charfn_batch_device on the ten-member benchmark pedigree with the 11
tables of its allele count (count_tables: D = 20), next to famseq_weight_batch_device with 11 real tables on the same resident
batch, in one process.

    python tools/charfn_rate.py [sites=4000000] [variant]

The seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the two entries timed with HIP events, alternating, warmed up,
REPS repetitions each; min, median and max, the sites per second of the median, and the ratio of the two medians.  A complex
pass is about four real multiplications per real one, so a small multiple of the weight kernel's time is what to expect; nobody
has fixed a ratio: the times are written down as they come.  Then the count's distribution of the first 1000 sites through
count_from_cf: the largest |sum - 1| and the smallest entry.  variant: that fence level of both kernels instead of the contest's.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import famseq_amd as fs  # noqa: E402
from famseq_amd import synth  # noqa: E402

REPS = 7
args = sys.argv[1:]
SITES = int(args[0]) if args else 4_000_000
VARIANT = args[1] if len(args) > 1 else None


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def main():
    ped = fs.synthetic_pedigree("ped10")
    mo, fa = ped.relations()
    n, nn = SITES, ped.n
    tables, D = fs.count_tables(fs.count_scores(nn, kind="alleles"))
    m = len(tables)
    assert (D, m) == (20, 11)
    real = 0.5 ** (np.arange(1, m + 1)[:, None, None] * fs.count_scores(nn, kind="alleles")[None] / m)  # t^count at 11 points t
    ctx = fs.Context(fs.make_model(ped))
    if VARIANT is not None:
        os.environ["FAMSEQ_VARIANT_ONLY"] = VARIANT
    ctx.set_option("charfn_kernels", 1)
    ctx.set_option("weight_kernels", 1)
    os.environ.pop("FAMSEQ_VARIANT_ONLY", None)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    t_cw = torch.from_numpy(np.ascontiguousarray(tables).view(np.float64).reshape(m, nn, 3, 2)).to("cuda")
    t_w = torch.from_numpy(np.ascontiguousarray(real)).to("cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    cf = torch.empty((n, m, 2), dtype=torch.float64, device="cuda")
    wl = torch.empty((n, m), dtype=torch.float64, device="cuda")
    runs = {
        "charfn, 11 tables": lambda: ctx.charfn_device(n, t_cw.data_ptr(), m, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_cf=cf.data_ptr(),
                                                       d_loglik=ll.data_ptr(), d_status=st.data_ptr()),
        "weight, 11 tables": lambda: ctx.weight_device(n, t_w.data_ptr(), m, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_wt_loglik=wl.data_ptr(),
                                                       d_loglik=ll.data_ptr(), d_status=st.data_ptr()),
    }
    for f in runs.values():  # warm-up (the first loads the kernels)
        timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, f in runs.items():
            times[key].append(timed(f))
    print("ped10: N = %d, %d sites, %d repetitions each, alternating" % (nn, n, REPS))
    med = {}
    for key in runs:
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-18s median %9.3f ms  (min %.3f, max %.3f)  %.3g sites/s" % (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], n / med[key]))
    print("  charfn / weight: %.2f; one complex pass about %.3f ms, one real pass about %.3f ms" %
          (med["charfn, 11 tables"] / med["weight, 11 tables"], 1e3 * med["charfn, 11 tables"] / (m + 1), 1e3 * med["weight, 11 tables"] / (m + 1)))
    runs["charfn, 11 tables"]()
    torch.cuda.synchronize()
    k = min(n, 1000)
    good = st[:k].cpu().numpy() == 0
    dist = fs.count_from_cf(cf[:k].cpu().numpy()[good], D)
    plan = ctx.plan()
    print("  variants: charfn %s, weight %s; %d of the first %d sites with status 0: largest |sum of the distribution - 1| %.3g, smallest entry %.3g"
          % (plan["charfn_variant"], plan["weight_variant"], int(good.sum()), k, np.abs(dist.sum(axis=1) - 1).max(), dist.min()))
    ctx.close()


if __name__ == "__main__":
    main()
