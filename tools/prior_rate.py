"""The site-prior kernel on the device: famseq_bn_prior_batch_device next to famseq_bn_batch_device (sum-product engine) on
the same resident batch, in one process.

    python tools/prior_rate.py [ped10_sites=10000000] [trio_sites=8000000]

Per pedigree (ped10, trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, Hardy-Weinberg prior rows for
allele frequencies drawn once, the two kernels timed with HIP events, alternating, warmed up, REPS repetitions each; min and
median.  Algorithmic bytes per site: famseq_elim 72 N + 2 (likelihood rows, flags; posterior and single posterior rows,
status), famseq_elim_prior 48 more (its prior row).  The plain kernel's code object is the parent commit's, so its median is
the parent's number taken in the same run.  The expectation under test: the time ratio does not exceed the byte ratio by more
than 5 %.
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
    model = fs.make_model(ped)
    elim = fs.Context(model, engine=fs.ENGINE_ELIM)
    pri = fs.Context(model)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    prior = torch.from_numpy(fs.hwe_priors(10.0 ** np.random.RandomState(1).uniform(-6, -0.001, n))).cuda()
    post = torch.empty_like(lk)
    single = torch.empty_like(lk)
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    b_plain = 72 * ped.n + 2
    runs = {
        "elim": (lambda: elim.bn_batch_device(n, lk.data_ptr(), flags.data_ptr(), post.data_ptr(), single.data_ptr(), st.data_ptr()), b_plain),
        "elim_prior": (lambda: pri.bn_prior_batch_device(n, lk.data_ptr(), flags.data_ptr(), prior.data_ptr(), post.data_ptr(),
                                                         single.data_ptr(), st.data_ptr()), b_plain + 48),
    }
    for _ in range(2):  # warm-up (the first loads the kernels)
        for f, _ in runs.values():
            timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d sites (elim variant %s, prior variant %s), %d repetitions each, alternating" %
          (name, ped.n, n, elim.plan()["elim_variant"], pri.plan()["prior_variant"], REPS))
    med = {}
    for key, (_, b) in runs.items():
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-11s median %.3f ms  (min %.3f, max %.3f)  %4d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
    ratio, bytes_ratio = med["elim_prior"] / med["elim"], (b_plain + 48) / b_plain
    print("  elim_prior / elim (medians) = %.3f, bytes %.3f   -> the expectation (time ratio <= 1.05 x byte ratio = %.3f) %s" %
          (ratio, bytes_ratio, 1.05 * bytes_ratio, "holds" if ratio <= 1.05 * bytes_ratio else "is MISSED"))
    print("  status != 0 on %d sites" % int(((st & 3) != 0).sum()))
    elim.close()
    pri.close()
    del lk, flags, prior, post, single, st
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "trio"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
