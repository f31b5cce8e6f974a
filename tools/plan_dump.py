#!/usr/bin/env python3
"""Which generated kernels does a plan-only context build for a fixed list of pedigrees, and under which names?

A refactor of the library's host side must leave the generated sources (hence the content-hashed code-object names) and
the variants taken as they were.  This writes, per pedigree, the keys of famseq_plan_json that name a code object, a
variant or an error after every kernel family has been asked for, the SHA-256 of the full plans, and the sorted listing
of the (fresh) kernel cache.  Run it on both commits and compare the files byte for byte.  No GPU needed.

    python tools/plan_dump.py OUT.json [--compile] [--root CHECKOUT]

Default: FAMSEQ_JIT_SOURCE_ONLY (nothing is compiled; the variant contest takes its first candidate) over trio, ped5,
ped10, ped15, random_pedigree(0..5), a 32-member wide pedigree and four disjoint sib matings (four loops: one more than
the sum-product engine conditions on, so every kernel of its family is refused).  --compile: compile for real, so that the spill
contest and the shipped picks decide, over ped10, ped15, random_pedigree(3) (a loop) and a 48-member wide pedigree.
--root: the checkout whose library is loaded (default: this one)."""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--compile", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

cache = tempfile.mkdtemp(prefix="famseq_plan_dump_")
os.environ.update(FAMSEQ_KERNEL_CACHE=cache, FAMSEQ_QUIET="1")
if not args.compile:
    os.environ.update(FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_KEEP_SRC="1")

import famseq_amd as fs  # noqa: E402  (after the environment is set)
from famseq_amd.prebuild_sets import random_pedigree, wide_pedigree  # noqa: E402

if args.compile:
    peds = [(n, fs.synthetic_pedigree(n)) for n in ("ped10", "ped15")] + [("random3", random_pedigree(3)[1]), ("wide48", wide_pedigree(48))]
else:
    peds = [(n, fs.synthetic_pedigree(n)) for n in ("trio", "ped5", "ped10", "ped15")]
    peds += [("random%d" % s, random_pedigree(s)[1]) for s in range(6)] + [("wide32", wide_pedigree(32))]
    o = [10 * b for b in range(4) for _ in range(5)]  # 1 x 2 -> 3, 4; 3 x 4 -> 5, four times over
    ids = [x + k for x, k in zip(o, [1, 2, 3, 4, 5] * 4)]
    peds.append(("loops4", fs.Pedigree(ids, [x + k if k else 0 for x, k in zip(o, [0, 0, 2, 2, 4] * 4)],
                                       [x + k if k else 0 for x, k in zip(o, [0, 0, 1, 1, 3] * 4)], [1, 2, 1, 2, 1] * 4, ["s%d" % i for i in ids])))


def kept(key):
    return any(w in key for w in ("code_object", "variant", "error", "reads_rows", "enum_group_digits")) or key in ("engine", "tune")


out = {}
for name, ped in peds:
    ctx = fs.Context(fs.make_model(ped), device=-1)
    steps = [("enum_impl", 1), ("group_digits", 1), ("group_digits", 2), ("engine", fs.ENGINE_ELIM), ("trio_kernels", 1),
             ("trio_kernels", 3), ("map_kernels", 1), ("call_kernels", 1), ("prior_kernels", 1), ("trio_prior_kernels", 3),
             ("map_prior_kernels", 1), ("evidence_kernels", 1), ("evidence_prior_kernels", 1), ("loo_kernels", 1),
             ("loo_prior_kernels", 1)]
    refused = []
    for k, v in steps:  # (a pedigree without that many looped members, or one the sum-product engine does not serve, says so)
        try:
            ctx.set_option(k, v)
        except fs.FamseqError as e:
            refused.append("%s=%d: %s" % (k, v, str(e).replace(cache + "/", "")[:200]))
    full = json.dumps(ctx.plan(), sort_keys=True).replace(cache + "/", "")
    ctx.close()
    out[name] = {k: v for k, v in json.loads(full).items() if kept(k)}
    out[name]["refused"] = refused
    out[name]["plan_sha256"] = hashlib.sha256(full.encode()).hexdigest()
out["cache_files"] = sorted(os.listdir(cache))
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
shutil.rmtree(cache)
print("%s: %d pedigrees, %d cache files" % (args.out, len(peds), len(out["cache_files"])))
