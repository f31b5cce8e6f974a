"""The origin kernel on the device: famseq_origin_batch_device next to the two forms of famseq_trio_batch_device — the joint
form, the route users had before (27 K doubles per site, split on the host afterwards), and the dnm form (K doubles) — on the
same resident batch, in one process.

    python tools/origin_rate.py [ped10_sites=10000000] [trio_sites=8000000]

Per pedigree (ped10; trio): the seeded synthetic batch (famseq_amd.synth, config 1) in HBM, the three kernels timed with HIP
events, alternating, warmed up, REPS repetitions each; min, median and max.  Per kernel: the time, the bytes per site it has to
move (24 N + 1 in; out 64 K + 1, 216 K + 1 and 8 K + 1), that over the median as a share of 8 TB/s.  By the bytes the origin
kernel belongs between the other two.  Nobody has fixed a ratio: the times are written down as they come.  Last, the origin
kernel's rows against the joint's split on the host by the allele-level factor (numpy, on the first sites of the batch).
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
HBM = 8e12  # bytes per second
CHECK_SITES = 4096
args = sys.argv[1:]
SITES = {"ped10": int(args[0]) if args else 10_000_000, "trio": int(args[1]) if len(args) > 1 else 8_000_000}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def host_split(joint, ped, children, al, flags):
    """The joint [S, K, 27] split by tm tf / sum tm tf -> origin [S, K, 4] (al: Context.allele_tables())."""
    out = np.zeros(joint.shape[:2] + (4,))
    chrx = ((flags & 2) != 0).astype(int)
    for k, c in enumerate(children):
        sex = 0 if ped.genders[c] == 1 else 1
        w = np.zeros((2, 4, 3, 3, 3))
        for x in range(2):
            for a in range(2):
                for b in range(2):
                    w[x, 2 * a + b, 2 * a if (x and sex == 0) else a + b] = al[x, sex, 0, a][:, None] * al[x, sex, 1, b][None, :]
            tot = w[x].sum(axis=0)
            with np.errstate(invalid="ignore", divide="ignore"):
                w[x] = np.where(tot > 0, w[x] / tot, 0.0)
        out[:, k] = (w.reshape(2, 4, 27)[chrx] * joint[:, k][:, None, :]).sum(axis=2)
    return out


def device_rates(name, n):
    ped = fs.synthetic_pedigree(name)
    mo, fa = ped.relations()
    nn = ped.n
    ctx = fs.Context(fs.make_model(ped))
    for key, form in (("origin_kernels", 1), ("trio_kernels", 1), ("trio_kernels", 2)):
        ctx.set_option(key, form)
    children = ctx.trio_children()
    k = len(children)
    lk, flags = synth.gen_batch_torch(mo, fa, n, 1, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    og = torch.empty((n, k, 4), dtype=torch.float64, device="cuda")
    hg = torch.empty((n, k, 4), dtype=torch.float64, device="cuda")
    jt = torch.empty((n, k, 27), dtype=torch.float64, device="cuda")
    dn = torch.empty((n, k), dtype=torch.float64, device="cuda")
    io = dict(d_lk=lk.data_ptr(), d_flags=flags.data_ptr(), d_status=st.data_ptr())
    runs = {
        "origin (origin + hettx)": lambda: ctx.origin_device(n, d_origin=og.data_ptr(), d_hettx=hg.data_ptr(), **io),
        "trio, joint form": lambda: ctx.trio_batch_device(n, d_joint=jt.data_ptr(), **io),
        "trio, dnm form": lambda: ctx.trio_batch_device(n, d_dnm=dn.data_ptr(), **io),
    }
    row_in = 24 * nn + 1  # the site's rows and its flags
    moved = {"origin (origin + hettx)": row_in + 64 * k + 1, "trio, joint form": row_in + 216 * k + 1, "trio, dnm form": row_in + 8 * k + 1}
    for f in runs.values():  # warm-up (the first loads the kernels)
        timed(f)
    times = {key: [] for key in runs}
    for _ in range(REPS):
        for key, f in runs.items():
            times[key].append(timed(f))
    print("%s: N = %d, K = %d, %d sites, %d repetitions each, alternating" % (name, nn, k, n, REPS))
    med = {}
    for key in runs:
        t = sorted(times[key])
        med[key] = t[len(t) // 2]
        print("  %-26s median %9.3f ms  (min %.3f, max %.3f)  %5d B/site  %.3f of 8 TB/s" %
              (key, 1e3 * med[key], 1e3 * t[0], 1e3 * t[-1], moved[key], moved[key] * n / med[key] / HBM))
    print("  origin / joint form: %.3f;  origin / dnm form: %.3f" %
          (med["origin (origin + hettx)"] / med["trio, joint form"], med["origin (origin + hettx)"] / med["trio, dnm form"]))
    # the kernel's rows against the joint's split on the host
    m = min(n, CHECK_SITES)
    good = (st[:m] == 0).cpu().numpy()
    want = host_split(jt[:m].cpu().numpy(), ped, children, ctx.allele_tables(), flags[:m].cpu().numpy())
    got = og[:m].cpu().numpy()
    plan = ctx.plan()
    print("  variants: origin %s, trio %s; first %d sites, %d with status 0: worst |origin - split of the joint| %.3g, worst |row sum - 1| %.3g"
          % (plan["origin_variant"], plan["trio_variant"], m, int(good.sum()), np.abs(got[good] - want[good]).max(),
             np.abs(got[good].sum(axis=-1) - 1).max()))
    ctx.close()
    del lk, flags, st, og, hg, jt, dn
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for name in ("ped10", "trio"):
        device_rates(name, SITES[name])
        sys.stdout.flush()
