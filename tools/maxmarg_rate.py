"""The max-marginal kernel on the device: famseq_maxmarg_batch_device next to famseq_loo_batch_device and
famseq_map_batch_device on the same resident batch, in one process.

    python tools/maxmarg_rate.py [ped10_sites=2000000] [wide32_sites=1000000]

Per pedigree (ped10, 32 members): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the kernels timed with HIP
events, alternating, warmed up, REPS repetitions each; min, median and max, and sites per second at the median.
Algorithmic bytes per site: 24 N + 1 in (likelihood rows and the flags byte); out 24 N + 16 + 1 (famseq_maxmarg: rows, top,
status), 32 N + 1 (famseq_loo: rows, fit, status), N + 8 + 1 (famseq_map: genotypes, posterior, status); the fraction is of
8 TB/s.  The yardstick is famseq_loo — the same messages in both directions and nearly the same output bytes; famseq_map is
the kernel whose max pass this one runs both ways.  The spread of a kernel's own repetitions (max / min) is printed beside
the ratios: a ratio inside it says nothing.
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
REPS = 9
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 2_000_000, "wide32": int(args[1]) if len(args) > 1 else 1_000_000}


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
    ctx = fs.Context(fs.make_model(ped))
    nn = ped.n
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    rows = torch.empty_like(lk)
    top = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    fit = torch.empty((n, nn), dtype=torch.float64, device="cuda")
    gt = torch.empty((n, nn), dtype=torch.int8, device="cuda")
    post = torch.empty(n, dtype=torch.float64, device="cuda")
    io = dict(d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_status=st.data_ptr())
    b_in = 24 * nn + 1
    runs = {
        "maxmarg (rows + top)": (lambda: ctx.maxmarg_device(n, d_maxmarg=rows.data_ptr(), d_top=top.data_ptr(), **io), b_in + 24 * nn + 17),
        "loo (rows + fit)": (lambda: ctx.loo_batch_device(n, d_loo=rows.data_ptr(), d_fit=fit.data_ptr(), **io), b_in + 32 * nn + 1),
        "map (genotypes + posterior)": (lambda: ctx.map_batch_device(n, d_map_gt=gt.data_ptr(), d_map_post=post.data_ptr(), **io), b_in + nn + 9),
    }
    for _ in range(2):  # warm-up (the first loads the kernels)
        for f, _ in runs.values():
            timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, (f, _) in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, %d resident sites, %d repetitions each, alternating" % (name, nn, n, REPS))
    med, spread = {}, {}
    for key, (_, b) in runs.items():
        t = sorted(times[key])
        med[key], spread[key] = t[len(t) // 2], t[-1] / t[0]
        print("  %-28s median %.3f ms  (min %.3f, max %.3f: spread %.3f)  %.3g sites/s  %4d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], spread[key], n / med[key], b, b * n / med[key] / PEAK))
    keys = list(runs)
    for y in keys[1:]:
        print("  %s / %s (medians) = %.3f   (the two kernels' own spreads: %.3f, %.3f)" % (keys[0], y, med[keys[0]] / med[y], spread[keys[0]], spread[y]))
    ctx.maxmarg_device(n, d_maxmarg=rows.data_ptr(), d_top=top.data_ptr(), **io)
    ctx.map_batch_device(n, d_map_gt=gt.data_ptr(), d_map_post=post.data_ptr(), **io)
    torch.cuda.synchronize()
    ok = st == 0
    same = bool((top[ok][:, 0].view(torch.int64) == post[ok].view(torch.int64)).all())
    plan = ctx.plan()
    print("  variants: maxmarg %s, loo %s, map %s; status != 0 on %d sites; top[0] has map_post's bits: %s; mean top %.6g / %.6g" %
          (plan["maxmarg_variant"], plan["loo_variant"], plan["map_variant"], int((~ok).sum()), same, float(top[ok][:, 0].mean()),
           float(top[ok][:, 1].mean())))
    ctx.close()
    del lk, flags, st, rows, top, fit, gt, post
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "wide32"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
