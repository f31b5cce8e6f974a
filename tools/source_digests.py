#!/usr/bin/env python3
"""SHA-256 of the source text of every generated kernel, for a fixed matrix of pedigrees, kernel families, variants and
tuning switches.  No GPU needed.

Code objects are cached by the hash of their source and famseq_amd/tuned_picks.json is keyed by it, so a change of the
generators (csrc/elim_codegen.cpp, enum_codegen.cpp, kernel_shell.cpp) that is meant to leave the kernels alone must leave
every one of these digests alone.  tests/golden/generated_sources.json is the record; tests/test_generated_sources.py
regenerates the matrix and compares.

    python tools/source_digests.py OUT.json              # write the manifest (to record a deliberate change of emitted text)
    python tools/source_digests.py OUT.json --dump DIR   # ... and every source text, one file per case: run it on two commits
                                                         # and `diff -r` the directories to see what changed
    python tools/source_digests.py --later OUT.json      # the manifest of the products added since (LATER_STEMS, below)
    python tools/source_digests.py --newer OUT.json      # ... and of those added since that one was written (NEWER_STEMS)

The sources are obtained the way the host tests obtain them: a plan-only context with FAMSEQ_JIT_SOURCE_ONLY,
FAMSEQ_KEEP_SRC and a scratch FAMSEQ_KERNEL_CACHE; FAMSEQ_VARIANT_ONLY forces the variant; the .hip file is read next to
the code object the plan names."""
import hashlib
import json
import os
import re
import shutil
import sys
import tempfile
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import famseq_amd as fs  # noqa: E402
from famseq_amd.prebuild_sets import (EDGE_PEDIGREES, SIDE_PRODUCTS, SIDE_PRODUCTS_LATER, SIDE_PRODUCTS_NEWER, SIDE_PRODUCTS_SINCE,  # noqa: E402
                                      SIDE_VARIANTS,
                                      edge_pedigree, random_pedigree, wide_pedigree)

TWO_CUT_SEED = 99  # the first random_pedigree seed whose loops need exactly two conditioned members (seeds 0..117 searched)


def _named(name):
    if name == "cousins":  # a first-cousin marriage: one conditioned member
        ids, mids, fids = [1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 0, 2, 2, 0, 0, 5, 4, 8], [0, 0, 1, 1, 0, 0, 3, 6, 7]
        return fs.Pedigree(ids, mids, fids, [1, 2, 1, 2, 2, 1, 1, 2, 1], ["s%d" % i for i in ids])
    if name == "lone":  # a trio and a member of no nuclear family (trio_body's lone-founder branch)
        return fs.Pedigree([1, 2, 3, 4], [0, 0, 2, 0], [0, 0, 1, 0], [1, 2, 1, 2], ["s1", "s2", "s3", "s4"])
    if name in EDGE_PEDIGREES:
        return edge_pedigree(name)
    if name.startswith("random"):
        return random_pedigree(int(name[6:]))[1]
    if name.startswith("wide"):
        return wide_pedigree(int(name[4:]))
    return fs.synthetic_pedigree(name)


# trio .. ped15:12, cousins (one conditioned member) and random15 (three): the variant matrices' pedigrees (tests/_variants.py);
# random0 / random3: the MAP host tests'; random99: two conditioned members; wide24 / 48 / 64: the staged form, the lean forms
# (from forty members) and the LDS-row members (from fifty-six); lone: a component without a family.
# The lane kernel's once-per-site form (lane/4..7 differ from lane/0..3) is taken by ped10 (a looped member unrolled ahead of
# the block, one prefix digit in the tables rebuilt per step), random99 (two such digits) and random34 (every prefix table
# constant: none); for every other pedigree lane/4..7 are recorded as the text of lane/0..3.
PEDIGREES = ("trio", "quad", "ped5", "ped10", "ped15:12", "cousins", "random15", "random0", "random3", "random%d" % TWO_CUT_SEED,
             "wide24", "wide48", "wide64", "lone", "random34")

# The matrix has two layers, so that a manifest written before the second existed still checks against the first alone.
# The base layer is the above with SWITCHES: the main engines, the lane kernels, trio and map (digests(name)).  The side layer
# (digests(name, side=True)) is the base layer plus every other row of side_table() (csrc/kernels.cpp), as (stem, has a site-prior
# sibling): cases "<stem>/<v>" and "<stem>_prior/<v>", v < SIDE_VARIANTS, SIDE_SWITCHES, and four more pedigrees, edge37 ..
# edge40 (prebuild_sets.EDGE_PEDIGREES), the side products around their size edges — relabel_source's three forms (LDS rows up to
# 37 members, global rows under an emitter that is not lean at 38 and 39, both lean from 40) and every side product's switch
# to the lean form between 39 and 40.  tests/golden/generated_sources.json holds the side layer.
SIDE_PEDIGREES = PEDIGREES + ("edge37", "edge38", "edge39", "edge40")
SIDE_STEMS = tuple((stem, has_prior) for stem, _, has_prior in SIDE_PRODUCTS + SIDE_PRODUCTS_SINCE if stem not in ("trio", "map"))
# A third layer, in a manifest of its own (a manifest that exists is a test's yardstick and is not rewritten for a new product):
# the rows side_table() has gained since the side layer's manifest was written (prebuild_sets.SIDE_PRODUCTS_LATER), on
# SIDE_PEDIGREES, cases "<stem>/<v>" and "<stem>_prior/<v>" as in the side layer and nothing else (later_digests(name)).
# tests/golden/generated_sources_later.json holds it; tests/test_generated_sources_later.py compares.
LATER_STEMS = tuple((stem, has_prior) for stem, _, has_prior in SIDE_PRODUCTS_LATER)
# A fourth layer, for the same reason in a manifest of its own: the rows gained since the third layer's manifest was written
# (prebuild_sets.SIDE_PRODUCTS_NEWER), the same cases on the same pedigrees (later_digests(name, NEWER_STEMS)).
# tests/golden/generated_sources_newer.json holds it; tests/test_generated_sources_newer.py compares.
NEWER_STEMS = tuple((stem, has_prior) for stem, _, has_prior in SIDE_PRODUCTS_NEWER)
REFUSED = "refused"  # recorded in the digest's place where the generator declines the pedigree (sample_source: LDS rows)

# One case per tuning switch at a value that is not its default, in a kernel family that reads it: (switch, value, pedigree,
# cases).  ped10, and wide48 for the form without LDS staging.  A case is "<family>/<variant>" as _one_variant names it.
SWITCHES = (
    ("FAMSEQ_ELIM_BT", "1", "ped10", ("elim/1",)),
    ("FAMSEQ_DIV_GROUP", "1", "ped10", ("elim/0",)),
    ("FAMSEQ_DIV_FAST", "0", "ped10", ("elim/1",)),
    ("FAMSEQ_PREFETCH_MAXN", "0", "ped10", ("elim/1",)),
    ("FAMSEQ_PREFETCH_EARLY_MAXN", "10", "ped10", ("elim/1",)),
    ("FAMSEQ_CHUNK_STRIDE", "1", "ped10", ("elim/1",)),
    ("FAMSEQ_PHASE_CLOCK", "1", "ped10", ("elim/1", "elim_call/1")),  # the plain form and the call form
    ("FAMSEQ_CALL_PHRED_GROUP", "1", "ped10", ("elim_call/1",)),
    ("FAMSEQ_CALL_FLAT", "0", "ped10", ("elim_call/1",)),
    ("FAMSEQ_CALL_LUT_LDS", "512", "ped10", ("elim_call/1",)),
    ("FAMSEQ_ELIM_MINWAVES", "2", "ped10", ("elim/1",)),
    ("FAMSEQ_ELIM_MINWAVES", "2", "wide48", ("elim/9",)),
    ("FAMSEQ_ELIM_REGS", "0", "ped10", ("elim/4",)),
    ("FAMSEQ_ELIM_REGS", "1", "ped10", ("elim/1",)),
    ("FAMSEQ_ELIM_CALL_REGS", "1", "ped10", ("elim_call/1",)),
    ("FAMSEQ_ELIM_LEAN", "1", "wide48", ("elim/9",)),
    ("FAMSEQ_ELIM_LDSL", "12", "wide48", ("elim/9",)),
    ("FAMSEQ_PRIOR_LATE", "1", "ped10", ("trio_prior3/1", "map_prior/1")),
    ("FAMSEQ_LANE_BT", "1", "ped10", ("lane/1", "lane_group1/1")),
    ("FAMSEQ_LANE_LATE", "1", "ped10", ("lane/1", "lane_call/1")),
    # the lane generator's other switches read beside its shell calls
    ("FAMSEQ_LANE_CAP", "5", "ped10", ("lane/1",)),
    ("FAMSEQ_LANE_MINWAVES", "2", "ped10", ("lane/1",)),
    ("FAMSEQ_LANE_ST", "0", "ped10", ("lane/1",)),
    ("FAMSEQ_LANE_PRE", "0", "ped10", ("lane/1",)),
    # ... and what the once-per-site form (lane/4..7) reads
    ("FAMSEQ_LANE_HOIST", "0", "ped10", ("lane/5",)),
    ("FAMSEQ_LANE_PRE", "0", "ped10", ("lane/5",)),
    ("FAMSEQ_LANE_PRE", "1", "ped10", ("lane/1", "lane/5")),
    ("FAMSEQ_LANE_CAP", "5", "ped10", ("lane/5",)),
    ("FAMSEQ_LANE_TABLE_BUDGET", "40", "ped10", ("lane/1",)),
)
# ... and the side layer's: the switches the side products read
SIDE_SWITCHES = (
    ("FAMSEQ_PRIOR_LATE", "1", "ped10", ("evidence_prior/1", "weight_prior/1")),
    ("FAMSEQ_RELABEL_LEAN", "1", "ped10", ("relabel/1",)),
    ("FAMSEQ_SAMPLE_ROWS", "1", "ped10", ("sample/1",)),
)


TEXTS = None  # a dict: the source texts are kept in it by digest (--dump, and the test's report of a mismatch)


def _digest(plan, key, index=None):
    path = plan[key] if index is None else plan[key][index]
    assert path.endswith(".hsaco"), (key, index, path)
    with open(path[:-6] + ".hip", "rb") as f:
        text = f.read()
    digest = hashlib.sha256(text).hexdigest()
    if TEXTS is not None:
        TEXTS[digest] = text
    return digest


def _side_digest(ctx, key):
    """The source of side product `key` ("<stem>" or "<stem>_prior"), or REFUSED where its generator throws for the pedigree."""
    try:
        ctx.set_option(key + "_kernels", 1)
    except fs.FamseqError as e:
        if "_source: " not in str(e):  # (not the generator's own word: a failure, not a refusal)
            raise
        if TEXTS is not None:
            TEXTS[REFUSED] = ("%s\n" % e).encode()
        return REFUSED
    return _digest(ctx.plan(), key + "_code_object")


def _one_variant(ped, v, env, side=False, later=None):
    """Every kernel family's source in variant v (the families that have that many variants), under `env`; side: the side
    layer's families too; later: the families of that layer (LATER_STEMS or NEWER_STEMS) and no others."""
    out = {}
    cache = tempfile.mkdtemp(prefix="famseq_digests_")
    base = dict(FAMSEQ_KERNEL_CACHE=cache, FAMSEQ_JIT_SOURCE_ONLY="1", FAMSEQ_KEEP_SRC="1", FAMSEQ_QUIET="1", FAMSEQ_VARIANT_ONLY=str(v))
    try:
        with mock.patch.dict(os.environ, dict(base, **env)):
            model = fs.make_model(ped)
            if later:
                ctx = fs.Context(model, device=-1)
                for stem, has_prior in later:
                    for key in [stem] + ([stem + "_prior"] if has_prior else []):
                        out["%s/%d" % (key, v)] = _side_digest(ctx, key)
                ctx.close()
                return out
            if ped.n <= fs.MAXN and v < 8:  # the enumeration's lane kernel, its lanes-per-site forms and its call form
                ctx = fs.Context(model, device=-1)
                ctx.set_option("enum_impl", 1)
                out["lane/%d" % v] = _digest(ctx.plan(), "enum_lane_code_object")
                # (variants 4-7, the once-per-site form: the plain kernel only — their lanes-per-site forms are the text of
                # 0-3 and the call path has variants 0-3)
                for d in range(1, ctx.plan()["enum_group_digits_max"] + 1 if v < 4 else 0):
                    ctx.set_option("group_digits", d)
                    out["lane_group%d/%d" % (d, v)] = _digest(ctx.plan(), "enum_group_code_objects", d - 1)
                if v < 4:
                    ctx.set_option("call_kernels", 2)
                    out["lane_call/%d" % v] = _digest(ctx.plan(), "enum_lane_call_code_object")
                ctx.close()
            ctx = fs.Context(model, device=-1)
            ctx.set_option("engine", fs.ENGINE_ELIM)
            out["elim/%d" % v] = _digest(ctx.plan(), "elim_code_object")
            ctx.set_option("prior_kernels", 1)
            out["prior/%d" % v] = _digest(ctx.plan(), "prior_code_object")
            if ped.n <= fs.MAXN and v < 8:  # (no call-path form of a wide pedigree's kernel)
                ctx.set_option("call_kernels", 2)
                out["elim_call/%d" % v] = _digest(ctx.plan(), "elim_call_code_object")
            if v < 4:
                for form in (1, 2, 3):
                    ctx.set_option("trio_kernels", form)
                    out["trio%d/%d" % (form, v)] = _digest(ctx.plan(), "trio_code_object")
                    ctx.set_option("trio_prior_kernels", form)
                    out["trio_prior%d/%d" % (form, v)] = _digest(ctx.plan(), "trio_prior_code_object")
                ctx.set_option("map_kernels", 1)
                out["map/%d" % v] = _digest(ctx.plan(), "map_code_object")
                ctx.set_option("map_prior_kernels", 1)
                out["map_prior/%d" % v] = _digest(ctx.plan(), "map_prior_code_object")
            if side and v < SIDE_VARIANTS:
                for stem, has_prior in SIDE_STEMS:
                    for key in [stem] + ([stem + "_prior"] if has_prior else []):
                        out["%s/%d" % (key, v)] = _side_digest(ctx, key)
            ctx.close()
    finally:
        shutil.rmtree(cache, ignore_errors=True)
    return out


def digests(name, side=False):
    """{case: sha256} of pedigree `name`: every family in every variant, and the cases of SWITCHES on that pedigree; side: with
    the side layer's families and the cases of SIDE_SWITCHES."""
    ped = _named(name)
    ped.relations()
    out = {}
    for v in range(12):
        for k, d in _one_variant(ped, v, {}, side).items():
            out["%s %s" % (name, k)] = d
    for key, value, where, cases in SWITCHES + (SIDE_SWITCHES if side else ()):
        if where == name:
            for case in cases:
                got = _one_variant(ped, int(case.split("/")[1]), {key: value}, side)
                out["%s %s %s=%s" % (name, case, key, value)] = got[case]
    return out


def later_digests(name, stems=LATER_STEMS):
    """{case: sha256} of pedigree `name` in the third layer (stems = NEWER_STEMS: the fourth): the families of `stems` in every
    fence level."""
    ped = _named(name)
    ped.relations()
    return {"%s %s" % (name, k): d for v in range(SIDE_VARIANTS) for k, d in _one_variant(ped, v, {}, later=stems).items()}


def main():
    global TEXTS
    if len(sys.argv) == 3 and sys.argv[1] in ("--later", "--newer"):
        out = {}
        for name in SIDE_PEDIGREES:
            out.update(later_digests(name, LATER_STEMS if sys.argv[1] == "--later" else NEWER_STEMS))
        with open(sys.argv[2], "w") as f:
            f.write(json.dumps(out, indent=0, sort_keys=True) + "\n")
        print("%s: %d cases over %d pedigrees" % (sys.argv[2], len(out), len(SIDE_PEDIGREES)))
        return
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4 and sys.argv[2] != "--dump"):
        sys.exit(__doc__)
    if len(sys.argv) == 4:
        TEXTS = {}
        os.makedirs(sys.argv[3], exist_ok=True)
    out = {}
    for name in SIDE_PEDIGREES:
        mine = digests(name, side=True)
        out.update(mine)
        if TEXTS is not None:
            for case, digest in mine.items():
                with open(os.path.join(sys.argv[3], re.sub(r"[^A-Za-z0-9_=.]+", "_", case) + ".hip"), "wb") as f:
                    f.write(TEXTS[digest])
            TEXTS.clear()
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(out, indent=0, sort_keys=True) + "\n")
    print("%s: %d cases over %d pedigrees" % (sys.argv[1], len(out), len(SIDE_PEDIGREES)))


if __name__ == "__main__":
    main()
