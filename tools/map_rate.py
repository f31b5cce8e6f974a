"""The joint MAP kernel on the device: famseq_map_batch_device next to famseq_bn_batch_device (sum-product engine) on the same
resident batch, in one process.

    python tools/map_rate.py [ped10_sites=10000000] [trio_sites=8000000]

Per pedigree (ped10, trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the two kernels timed with HIP
events, alternating, warmed up, REPS repetitions each; min and median.  Algorithmic bytes per site: 24 N + 1 in (likelihood
rows and the flags byte); out N + 9 (MAP: genotype row, posterior, status) or 48 N + 1 (famseq_elim: posterior and single
posterior rows, status); the fraction is of 8 TB/s.  The expectation under test: the MAP kernel's median does not exceed
famseq_elim's from the same run by more than 5 %.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    mapc = fs.Context(model)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    post = torch.empty_like(lk)
    single = torch.empty_like(lk)
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    gt = torch.empty((n, ped.n), dtype=torch.int8, device="cuda")
    jp = torch.empty(n, dtype=torch.float64, device="cuda")
    runs = {
        "elim (post + single)": (lambda: elim.bn_batch_device(n, lk.data_ptr(), flags.data_ptr(), post.data_ptr(), single.data_ptr(), st.data_ptr()),
                                 24 * ped.n + 1 + 48 * ped.n + 1),
        "map (gt + post)": (lambda: mapc.map_batch_device(n, d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_map_gt=gt.data_ptr(),
                                                          d_map_post=jp.data_ptr(), d_status=st.data_ptr()), 24 * ped.n + 1 + ped.n + 9),
    }
    for _ in range(2):  # warm-up (the first loads the kernels)
        for f, _ in runs.values():
            timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d sites (elim variant %s, map variant %s), %d repetitions each, alternating" %
          (name, ped.n, n, elim.plan()["elim_variant"], mapc.plan()["map_variant"], REPS))
    med = {}
    for key, (_, b) in runs.items():
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-22s median %.3f ms  (min %.3f, max %.3f)  %4d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
    ratio = med["map (gt + post)"] / med["elim (post + single)"]
    print("  map / elim (medians) = %.3f   -> the 5 %% expectation %s" % (ratio, "holds" if ratio <= 1.05 else "is MISSED"))
    bad = int((st != 0).sum())
    print("  status != 0 on %d sites; MAP posterior mean %.4f" % (bad, float(jp[st == 0].mean())))
    elim.close()
    mapc.close()
    del lk, flags, post, single, st, gt, jp
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "trio"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
