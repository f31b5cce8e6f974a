"""The evidence kernel on the device: famseq_evidence_batch_device next to famseq_map_batch_device and famseq_bn_batch_device
(sum-product engine) on the same resident batch, in one process; then the site-prior pair, famseq_evidence_prior against
famseq_map_prior.

    python tools/evidence_rate.py [ped10_sites=10000000] [trio_sites=8000000]

Per pedigree (ped10, trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the kernels timed with HIP events,
alternating, warmed up, REPS repetitions each; min and median.  Algorithmic bytes per site: 24 N + 1 in (likelihood rows and
the flags byte); out 17 (evidence: loglik, pref, status), N + 9 (MAP: genotype row, posterior, status) or 48 N + 1
(famseq_elim: posterior and single posterior rows, status); the site-prior forms read 48 B more; the fraction is of 8 TB/s.
The yardstick is famseq_map in the same run: the evidence kernel reads the same rows, runs a subset of its arithmetic and
writes less, so its median should not exceed famseq_map's; same-run alternation leaves a few percent of noise, and more than
5 % above it wants an explanation.
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


def race(title, runs, n, yardstick, subject):
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
        print("  %-28s median %.3f ms  (min %.3f, max %.3f)  %4d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], b, b * n / med[key] / PEAK))
    ratio = med[subject] / med[yardstick]
    print("  %s / %s (medians) = %.3f   -> %s" % (subject, yardstick, ratio,
                                               "not above the yardstick by more than 5 %" if ratio <= 1.05 else "MORE than 5 % above the yardstick"))


def device_rates(name, n):
    ped = fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    model = fs.make_model(ped)
    elim = fs.Context(model, engine=fs.ENGINE_ELIM)
    ctx = fs.Context(model)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    post = torch.empty_like(lk)
    single = torch.empty_like(lk)
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    gt = torch.empty((n, ped.n), dtype=torch.int8, device="cuda")
    jp = torch.empty(n, dtype=torch.float64, device="cuda")
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    p0 = torch.empty(n, dtype=torch.float64, device="cuda")
    io, nn = dict(d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_status=st.data_ptr()), ped.n
    runs = {
        "evidence (loglik + pref)": (lambda: ctx.evidence_batch_device(n, d_loglik=ll.data_ptr(), d_pref=p0.data_ptr(), **io), 24 * nn + 1 + 17),
        "map (gt + post)": (lambda: ctx.map_batch_device(n, d_map_gt=gt.data_ptr(), d_map_post=jp.data_ptr(), **io), 24 * nn + 1 + nn + 9),
        "elim (post + single)": (lambda: elim.bn_batch_device(n, lk.data_ptr(), flags.data_ptr(), post.data_ptr(), single.data_ptr(), st.data_ptr()),
                                 24 * nn + 1 + 48 * nn + 1),
    }
    race("%s: N = %d, %d sites, %d repetitions each, alternating" % (name, nn, n, REPS), runs, n, "map (gt + post)", "evidence (loglik + pref)")
    ctx.evidence_batch_device(n, d_loglik=ll.data_ptr(), d_pref=p0.data_ptr(), **io)
    torch.cuda.synchronize()
    ok = st == 0
    print("  variants: evidence %s, map %s, elim %s; status != 0 on %d sites; mean loglik %.4f, mean pref %.4f" %
          (ctx.plan()["evidence_variant"], ctx.plan()["map_variant"], elim.plan()["elim_variant"], int((~ok).sum()), float(ll[ok].mean()),
           float(p0[ok].mean())))
    # the site-prior pair: Hardy-Weinberg rows at allele frequencies log-uniform in (1e-4, 0.5)
    af = np.exp(np.random.RandomState(1).uniform(np.log(1e-4), np.log(0.5), 1 << 16))
    prior = torch.from_numpy(fs.hwe_priors(af)).to("cuda").repeat((n + (1 << 16) - 1) >> 16, 1)[:n].contiguous()
    runs = {
        "evidence_prior": (lambda: ctx.evidence_prior_batch_device(n, prior.data_ptr(), d_loglik=ll.data_ptr(), d_pref=p0.data_ptr(), **io),
                           24 * nn + 1 + 17 + 48),
        "map_prior": (lambda: ctx.map_prior_batch_device(n, prior.data_ptr(), d_map_gt=gt.data_ptr(), d_map_post=jp.data_ptr(), **io),
                      24 * nn + 1 + nn + 9 + 48),
    }
    race("%s, founder priors per site:" % name, runs, n, "map_prior", "evidence_prior")
    elim.close()
    ctx.close()
    del lk, flags, post, single, st, gt, jp, ll, p0, prior
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "trio"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
