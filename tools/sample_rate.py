"""The sampling kernel on the device: famseq_sample_batch_device at K = 1, 8 and 32 draws per site next to
famseq_map_batch_device — the same rows in, at K = 1 the same bytes out — on the same resident batch, in one process; then the
site-prior pair (famseq_sample_prior at K = 8 next to famseq_map_prior).

    python tools/sample_rate.py [ped10_sites=10000000] [wide32_sites=2000000] [trio_sites=8000000]

Per pedigree (ped10, 32 members, trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the kernels timed with
HIP events, alternating, warmed up, REPS repetitions each; min, median and max.  Algorithmic bytes per site: 24 N + 1 in (+ 48
with prior rows); out K N + 8 K + 1 (drawn configurations, their posteriors, status) or N + 9 (MAP).  The fraction is of 8 TB/s.
famseq_map is the yardstick: at K = 1 a median more than 5 % above its median wants an explanation from
profiles/sample/resources.txt; the cost of a further draw, (t(32) - t(1)) / 31, is reported, not judged.
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
DRAWS = (1, 8, 32)
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 10_000_000, "wide32": int(args[1]) if len(args) > 1 else 2_000_000,
         "trio": int(args[2]) if len(args) > 2 else 8_000_000}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def race(runs, title):
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
        print("  %-26s median %8.3f ms  (min %.3f, max %.3f)  %5d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b[0], b[0] * b[1] / med[key] / PEAK))
    return med


def device_rates(name, n):
    ped = wide_pedigree(32) if name == "wide32" else fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    nn = ped.n
    model = fs.make_model(ped)
    ctx = fs.Context(model)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    gt = torch.empty((n, max(DRAWS), nn), dtype=torch.int8, device="cuda")
    jp = torch.empty((n, max(DRAWS)), dtype=torch.float64, device="cuda")
    rows_in = 24 * nn + 1
    common = dict(d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_status=st.data_ptr())

    def sample(k):
        return lambda: ctx.sample_batch_device(n, k, seed=1, d_samp_gt=gt.data_ptr(), d_samp_post=jp.data_ptr(), **common)

    runs = {"map (gt + post)": (lambda: ctx.map_batch_device(n, d_map_gt=gt.data_ptr(), d_map_post=jp.data_ptr(), **common), (rows_in + nn + 9, n))}
    for k in DRAWS:
        runs["sample, K = %d" % k] = (sample(k), (rows_in + k * nn + 8 * k + 1, n))
    med = race(runs, "%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS))
    t_map = med["map (gt + post)"]
    for k in DRAWS:
        print("  sample, K = %-2d / map (medians) = %.3f" % (k, med["sample, K = %d" % k] / t_map))
    r1 = med["sample, K = 1"] / t_map
    print("  K = 1 is %s" % ("not above the yardstick by more than 5 %" if r1 <= 1.05 else "MORE than 5 % above the yardstick"))
    per_draw = (med["sample, K = 32"] - med["sample, K = 1"]) / 31
    print("  a further draw: (t(32) - t(1)) / 31 = %.4f ms per %d sites = %.3f ns per site and draw" % (1e3 * per_draw, n, 1e9 * per_draw / n))
    # the site-prior pair: the model's own rows, as the host entries would be given them
    known = (flags & fs.FLAG_KNOWN) != 0
    n_row = torch.tensor(list(model.genoProbN) + list(model.genoProbXN), dtype=torch.float64, device="cuda")
    k_row = torch.tensor(list(model.genoProbK) + list(model.genoProbXK), dtype=torch.float64, device="cuda")
    prior = torch.where(known[:, None], k_row[None], n_row[None]).contiguous()
    runs = {
        "map_prior": (lambda: ctx.map_prior_batch_device(n, prior.data_ptr(), d_map_gt=gt.data_ptr(), d_map_post=jp.data_ptr(), **common),
                      (rows_in + 48 + nn + 9, n)),
        "sample_prior, K = 8": (lambda: ctx.sample_prior_batch_device(n, prior.data_ptr(), 8, seed=1, d_samp_gt=gt.data_ptr(),
                                                                      d_samp_post=jp.data_ptr(), **common), (rows_in + 48 + 8 * nn + 65, n)),
    }
    medp = race(runs, "  ... with the founders' prior per site:")
    print("  sample_prior, K = 8 / map_prior = %.3f;  sample_prior, K = 8 / sample, K = 8 = %.3f" %
          (medp["sample_prior, K = 8"] / medp["map_prior"], medp["sample_prior, K = 8"] / med["sample, K = 8"]))
    sample(8)()
    torch.cuda.synchronize()
    ok = st == 0
    plan = ctx.plan()
    print("  variants: sample %s, map %s; status != 0 on %d sites; mean samp_post %.4f; mean alt-allele count per member %.4f" %
          (plan["sample_variant"], plan["map_variant"], int((~ok).sum()), float(jp[ok][:, :8].mean()), float(gt[ok][:, :8].float().mean())))
    ctx.close()
    del lk, flags, st, gt, jp, prior
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32", "trio"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
