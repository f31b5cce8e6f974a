"""The relabelling kernel's arithmetic (famseq_relabel / famseq_relabel_prior: per site and assignment a the log10 of the
network's total weight Z_a with member p given row a[p] of the site, and the site's own log10 likelihood), checked without a GPU.

As in test_pattern_host.py, the kernel is generated for a one-lane workgroup on a plan-only context and its source compiled
with g++ -ffp-contract=off.  References: tests/_maxproduct.py's Z (max_product(...)[2]) on the rows rearranged on the host
(-1 -> ones), up to ten members also the 3^N enumeration of test_map_host.brute_weights; under per-site priors
tests/_prior_joint.py's factors through the same elimination.

Wanted: status exact (the rows as given decide it); alt_loglik and loglik at an ABSOLUTE 1e-9 (test_evidence_host's derivation:
a relative 1e-9 on Z is 4.3e-10 in log10); -inf exactly where the reference's Z_a is exactly 0; and the bit contracts of
include/famseq_hip.h against the host-compiled famseq_evidence of the same variant on the rearranged rows: alt_loglik[s][j] is
that kernel's loglik wherever it has status 0, an identity row gives loglik's bits, loglik is famseq_evidence's on the rows as
given, a column does not depend on n_assign or on the other rows, the prior form on the model's rows gives the plain form's bits.

No site is left out of a comparison: every batch asserts, on the reference alone and before the kernel runs, status 0 everywhere
and Z and every non-zero Z_a >= 1e-200.
"""
import ctypes as C
import mmap
import os
import subprocess
from unittest import mock

import numpy as np
import pytest

import _prior as P
import famseq_amd as fs
from test_evidence_host import build_evidence_host, run_evidence
from test_generated_host import factor_tables, host_source
from test_map_host import brute_weights, clear_likelihoods
from test_pattern_host import _total, pedigree, same_bits

LL_ATOL = 1e-9  # absolute, on log10 Z (see the module's docstring)
MRATES = [1e-7, 1e-4, 0.0]
N_VARIANTS = 4  # kRelabelVariants
FLOOR = 1e-200
N_SITES = 64
PED_NAMES = ["random0", "random1", "random2", "random3", "random99", "wide24", "wide48"]  # random99: two conditioned members


def build_relabel_host(model, where, variant=None, prior=False, lean=False):
    """Generate famseq_relabel (prior: famseq_relabel_prior) for a one-lane workgroup on a plan-only context, compile it for
    the host.  lean: the form that reads the site's row in global memory at each use, at every size.  -> (fn, plan, source)."""
    where.mkdir(parents=True, exist_ok=True)
    env = dict(FAMSEQ_KERNEL_CACHE=str(where), FAMSEQ_KEEP_SRC="1", FAMSEQ_ELIM_BT="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    if variant is not None:
        env["FAMSEQ_VARIANT_ONLY"] = str(variant)
    if lean:
        env["FAMSEQ_RELABEL_LEAN"] = "1"
    key, entry = ("relabel_prior", "famseq_relabel_prior") if prior else ("relabel", "famseq_relabel")
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1)
        ctx.set_option(key + "_kernels", 1)
        plan = ctx.plan()
        ctx.close()
    src = open(plan[key + "_code_object"][:-6] + ".hip").read()
    assert "#define BT 1\n" in src and (entry + "(") in src
    assert ("founder priors per site" in src.splitlines()[0]) == prior
    assert variant is None or plan[key + "_variant"] == variant
    tag = key + ("" if variant is None else "_%d" % variant) + ("_lean" if lean else "")
    cpp, so = str(where / (tag + ".cpp")), str(where / (tag + ".so"))
    open(cpp, "w").write(host_source(src))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-shared", "-fPIC", "-o", so, cpp])
    fn = getattr(C.CDLL(so), entry)
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_double, C.c_void_p, C.c_int] + ([C.c_void_p] if prior else [])
    return fn, plan, src


def run_relabel(fn, model, lk, flags, assign, prior=None, want=(True, True, True), lk_at=None):
    """lk_at: the address the kernel reads the rows from (default: a contiguous copy of lk)."""
    s, m = lk.shape[0], assign.shape[0]
    a = np.ascontiguousarray(lk, dtype=np.float64)
    alt, ll, st = np.full((s, m), -5.0), np.full(s, -5.0), np.full(s, 77, np.uint8)
    fl = np.ascontiguousarray(flags, np.uint8)
    at = np.ascontiguousarray(assign, np.int32)
    tc = np.ascontiguousarray(factor_tables(model))
    args = [lk_at if lk_at is not None else a.ctypes.data, fl.ctypes.data, alt.ctypes.data if want[0] else None,
            ll.ctypes.data if want[1] else None, st.ctypes.data if want[2] else None, s, tc.ctypes.data, 1.0, at.ctypes.data, m]
    if prior is not None:
        raw = np.zeros(prior.size + 2)
        pr = raw[(raw.ctypes.data % 16) // 8:][:prior.size].reshape(prior.shape)
        pr[...] = prior
        args.append(pr.ctypes.data)
    fn(*args)
    return alt, ll, st


def rearranged(lk, a):
    """The site's rows as assignment a [N] hands them out: member p gets row a[p], -1 the row (1, 1, 1)."""
    a = np.asarray(a)
    out = lk[:, np.where(a < 0, 0, a), :].copy()
    out[:, a < 0, :] = 1.0
    return out


def reference(ped, mrate, lk, flags, assign, prior=None, brute=True):
    """-> (z[S], za[S, M], status[S]): the total weight as given, every assignment's (both with the reference's 1e7), and the
    status of the rows as given.  Up to ten members (brute) the 3^N enumeration is checked against the elimination here."""
    z, fail = _total(ped, mrate, lk, flags, prior)
    za = np.stack([_total(ped, mrate, rearranged(lk, a), flags, prior)[0] for a in assign], axis=1)
    if brute and ped.n <= 10 and prior is None:
        for j in [-1] + list(range(len(assign))):
            _, W, bst = brute_weights(ped, mrate, lk if j < 0 else rearranged(lk, assign[j]), flags)
            # (its NaN rows: a member whose row times its prior is all zeros, or no configuration with weight — a total of 0)
            W = np.where(bst != 0, 0.0, np.nansum(W, axis=1))
            have = z if j < 0 else za[:, j]
            assert np.array_equal(W == 0, have == 0)
            np.testing.assert_allclose(have, W, rtol=1e-12, atol=0)
    st = np.where(fail, 1, np.where(~((z > 0) & np.isfinite(z)), 2, 0)).astype(np.uint8)
    return z, za, st


def batch_assign(rng, n):
    """The assignments of one batch: the identity, three random transpositions, a random full permutation, a row with two -1,
    a row that uses one member's row twice."""
    ident = np.arange(n, dtype=np.int32)
    rows = [ident.copy()]
    for _ in range(3):
        i, j = rng.permutation(n)[:2]
        row = ident.copy()
        row[i], row[j] = j, i
        rows.append(row)
    rows.append(rng.permutation(n).astype(np.int32))
    gone = ident.copy()
    gone[rng.permutation(n)[:2]] = -1
    rows.append(gone)
    twice = ident.copy()
    i, j = rng.permutation(n)[:2]
    twice[i] = j
    rows.append(twice)
    return np.stack(rows)


def clear(ref, what=""):
    """On the reference alone: nothing is left out of a comparison."""
    z, za, st = ref
    assert np.all(st == 0) and np.all(z >= FLOOR) and np.all((za == 0) | (za >= FLOOR)), what


def check(out, ref, what=""):
    """The module docstring's rules; every site and assignment compared.  Prints the worst errors before it asserts."""
    alt, ll, st = out
    z, za, ref_st = ref
    assert np.array_equal(st, ref_st), what
    ok = ref_st == 0
    assert np.all(np.isnan(ll[~ok])) and np.all(np.isnan(alt[~ok])), what
    zero = za[ok] == 0
    with np.errstate(divide="ignore"):
        want = np.log10(za[ok]) - 7.0
    got = alt[ok]
    err_a = np.abs(got[~zero] - want[~zero])
    err = np.abs(ll[ok] - (np.log10(z[ok]) - 7.0))
    print("%s: %d sites x %d assignments, %d exact zeros, worst |alt_loglik error| %.3g, worst |loglik error| %.3g, smallest Z %.3g, "
          "smallest non-zero Z_a %.3g" % (what, ok.sum(), za.shape[1], zero.sum(), err_a.max(initial=0), err.max(initial=0),
                                          z[ok].min(initial=1), za[ok][~zero].min(initial=1)))
    assert np.array_equal(np.isneginf(got), zero), what
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=0, atol=LL_ATOL, err_msg=what)
    np.testing.assert_allclose(ll[ok], np.log10(z[ok]) - 7.0, rtol=0, atol=LL_ATOL, err_msg=what)


def evidence_bits(ev, model, lk, flags, assign, out, prior=None):
    """The bit contracts against the host-compiled famseq_evidence: loglik on the rows as given, every column on the rows
    rearranged wherever that call has status 0 (where it has status 2 on a good site, Z_a is 0 and the column holds -inf).
    -> the number of column entries compared bit for bit."""
    alt, ll, st = out
    e_ll, _, e_st = run_evidence(ev, model, lk, flags, prior)
    assert np.array_equal(st, e_st) and same_bits([ll], [e_ll])
    compared = 0
    for j, a in enumerate(assign):
        a_ll, _, a_st = run_evidence(ev, model, rearranged(lk, a), flags, prior)
        good = (a_st == 0) & (st == 0)
        assert same_bits([alt[good, j]], [a_ll[good]])
        assert np.all(np.isneginf(alt[(a_st == 2) & (st == 0), j]))
        compared += int(good.sum())
        if np.array_equal(a, np.arange(len(a))):
            assert same_bits([alt[:, j]], [ll])
    return compared


def batch(name, seed=0):
    ped = pedigree(name)
    rng = np.random.RandomState(300 + 7 * ped.n + seed)
    lk, flags = clear_likelihoods(rng, ped, N_SITES)  # flags 0..3 mixed
    return ped, lk, flags, batch_assign(rng, ped.n)


@pytest.mark.parametrize("name", PED_NAMES)
def test_the_kernel_matches_the_reference(name, tmp_path):
    ped, lk, flags, assign = batch(name)
    assert {0, 1, 2, 3} <= set(flags.tolist())
    refs = {mrate: reference(ped, mrate, lk, flags, assign) for mrate in MRATES}
    for mrate in MRATES:
        clear(refs[mrate], "%s mrate %g" % (name, mrate))
    fn, plan, src = build_relabel_host(fs.make_model(ped), tmp_path)
    assert ("#define l0_0 lgv[0]" in src) == (ped.n >= 40)  # the rows in the lane's LDS row below forty members, lean from there
    assert src.count("for (int ps_ = 0;") == 1 and src.count("const double Zp_") == 1  # the pass's text stands once
    assert "#pragma unroll 1\n      for (int ps_ = 0; ps_ <= last_; ++ps_)" in src
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", plan["relabel_variant"])[0]
    forms = [fn] if ped.n >= 40 else [fn, build_relabel_host(fs.make_model(ped), tmp_path / "lean", plan["relabel_variant"], lean=True)[0]]
    zeros = 0
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        out = run_relabel(fn, model, lk, flags, assign)
        check(out, refs[mrate], "%s mrate %g" % (name, mrate))
        assert evidence_bits(ev, model, lk, flags, assign, out) > N_SITES  # (the identity column alone gives that many)
        for other in forms[1:]:  # where the rows live changes no bit
            assert same_bits(run_relabel(other, model, lk, flags, assign), out)
        zeros += int((refs[mrate][1] == 0).sum())
    print("%s: %d exact zeros over the three mutation rates" % (name, zeros))


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_the_four_variants_give_the_same_bits(name, tmp_path):
    ped, lk, flags, assign = batch(name, 1)
    model = fs.make_model(ped, mrate=1e-4)
    outs = [run_relabel(build_relabel_host(model, tmp_path, v)[0], model, lk, flags, assign) for v in range(N_VARIANTS)]
    assert np.all(outs[0][2] == 0)
    for out in outs[1:]:
        assert same_bits(out, outs[0])


@pytest.mark.parametrize("name", ["random0", "random1", "wide48"])
def test_site_prior_form(name, tmp_path):
    """Fed the model's rows: the plain form's bits.  Under Hardy-Weinberg rows: tests/_prior_joint.py's factors on the rearranged
    rows, and famseq_evidence_prior's bits."""
    ped, lk, flags, assign = batch(name, 2)
    hwe = fs.hwe_priors(np.random.RandomState(3).uniform(0.01, 0.5, len(lk)))
    refs = {mrate: reference(ped, mrate, lk, flags, assign, hwe) for mrate in MRATES}
    for mrate in MRATES:
        clear(refs[mrate], "%s mrate %g, HWE rows" % (name, mrate))
    plain = build_relabel_host(fs.make_model(ped), tmp_path / "plain", 1)[0]
    fn, _, src = build_relabel_host(fs.make_model(ped), tmp_path / "prior", 1, prior=True)
    assert "PRIOR_LOAD(site);" in src and "tcf[0] * l" not in src and "tcf[27] * l" not in src
    assert "int n_assign, const double *__restrict__ prior_g) {" in src  # the assignments stand in front of the prior rows
    ev = build_evidence_host(fs.make_model(ped), tmp_path / "ev", 1, prior=True)[0]
    for mrate in MRATES:
        model = fs.make_model(ped, mrate=mrate)
        want = run_relabel(plain, model, lk, flags, assign)
        assert np.all(want[2] == 0)
        assert same_bits(run_relabel(fn, model, lk, flags, assign, P.model_rows(model, flags)), want)
        out = run_relabel(fn, model, lk, flags, assign, hwe)
        check(out, refs[mrate], "%s mrate %g, HWE rows" % (name, mrate))
        assert evidence_bits(ev, model, lk, flags, assign, out, hwe) > 0


def test_planted_exact_zeros(tmp_path):
    """A trio at mutation rate 0 whose swap of father and child is Mendel-impossible; a chrX site where a male is handed (0, 1, 0)."""
    ped = pedigree("trio")
    mo, fa = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    father, mother = fa[child], mo[child]
    lk = np.zeros((4, ped.n, 3))
    lk[:, mother] = (1.0, 0.0, 0.0)
    lk[:, father] = (1.0, 0.0, 0.0)
    lk[:, child] = (1.0, 0.0, 0.0)
    lk[:2, father] = (0.0, 0.0, 1.0)  # sites 0, 1: hom-alt father, het child — handed to each other, a hom-alt child of a het father
    lk[:2, child] = (0.0, 1.0, 0.0)   # and a hom-ref mother, which no transmission without mutation gives
    flags = np.zeros(4, np.uint8)
    swap = np.arange(ped.n, dtype=np.int32)
    swap[father], swap[child] = child, father
    assign = np.stack([np.arange(ped.n, dtype=np.int32), swap])
    ref = reference(ped, 0.0, lk, flags, assign)
    clear(ref)
    assert np.all(ref[1][:2, 1] == 0) and np.all(ref[1][2:, 1] > 0) and np.all(ref[1][:, 0] > 0)
    model = fs.make_model(ped, mrate=0.0)
    fn = build_relabel_host(model, tmp_path)[0]
    out = run_relabel(fn, model, lk, flags, assign)
    check(out, ref, "Mendel-impossible swap")
    assert np.all(np.isneginf(out[0][:2, 1])) and np.all(np.isfinite(out[0][2:])) and np.all(out[2] == 0)
    # chrX: the mother's row (0, 1, 0) handed to the father, a male
    rng = np.random.RandomState(5)
    lkx, _ = clear_likelihoods(rng, ped, 4)
    lkx[:, mother] = (0.0, 1.0, 0.0)
    fx = np.full(4, 2, np.uint8)
    give = np.arange(ped.n, dtype=np.int32)
    give[father] = mother
    assign = np.stack([give, np.arange(ped.n, dtype=np.int32)])
    for mrate in (1e-7, 0.0):
        ref = reference(ped, mrate, lkx, fx, assign)
        clear(ref)
        assert np.all(ref[1][:, 0] == 0) and np.all(ref[1][:, 1] > 0)
        model = fs.make_model(ped, mrate=mrate)
        out = run_relabel(build_relabel_host(model, tmp_path)[0], model, lkx, fx, assign)
        check(out, ref, "male handed a heterozygote's row on chrX")
        assert np.all(np.isneginf(out[0][:, 0])) and np.all(out[2] == 0)


def test_failure_statuses(tmp_path):
    """An all-zero likelihood row: status 1.  The quad_mu0 shape (both parents hom-ref for certain, a child hom-alt for certain,
    mutation rate 0): status 2.  1e160 rows: status 2.  Every output of such a site is NaN."""
    ped = pedigree("quad")
    mo, _ = ped.relations()
    child = [p for p in range(ped.n) if mo[p] >= 0][0]
    lk, _ = clear_likelihoods(np.random.RandomState(3), ped, 32)
    flags = np.zeros(32, np.uint8)
    lk[5, 1, :] = 0.0
    lk[9] = (1.0, 0.0, 0.0)
    lk[9, child] = (0.0, 0.0, 1.0)
    assign = batch_assign(np.random.RandomState(4), ped.n)
    model = fs.make_model(ped, mrate=0.0)
    ref = reference(ped, 0.0, lk, flags, assign)
    assert ref[2][5] == 1 and ref[2][9] == 2 and np.all(np.delete(ref[2], [5, 9]) == 0)
    for prior in (None, P.model_rows(model, flags)):
        for variant in (0, 3):
            fn = build_relabel_host(model, tmp_path, variant, prior=prior is not None)[0]
            alt, ll, st = out = run_relabel(fn, model, lk, flags, assign, prior)
            check(out, ref, "planted failures")
            assert st[5] == 1 and st[9] == 2 and np.all(np.isnan(alt[[5, 9]])) and np.all(np.isnan(ll[[5, 9]]))
            assert not np.any(np.isnan(alt[np.delete(np.arange(32), [5, 9])]))
    big = np.full((2, ped.n, 3), 1e160)
    alt, ll, st = run_relabel(build_relabel_host(model, tmp_path, 0)[0], model, big, np.zeros(2, np.uint8), assign)
    assert np.all(st == 2) and np.all(np.isnan(ll)) and np.all(np.isnan(alt))


def test_each_output_may_be_null(tmp_path):
    ped, lk, flags, assign = batch("random1", 4)
    model = fs.make_model(ped)
    for prior in (None, P.model_rows(model, flags)):
        fn = build_relabel_host(model, tmp_path, prior=prior is not None)[0]
        full = run_relabel(fn, model, lk, flags, assign, prior)
        for want in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            got = run_relabel(fn, model, lk, flags, assign, prior, want=want)
            untouched = (np.full(full[0].shape, -5.0), np.full(N_SITES, -5.0), np.full(N_SITES, 77, np.uint8))
            for k in range(3):
                assert same_bits([got[k]], [full[k] if want[k] else untouched[k]])


@pytest.mark.parametrize("name", ["random0", "wide48"])
def test_one_assignment_and_sixty_four(name, tmp_path):
    """n_assign = 1 and FAMSEQ_MAX_RELABEL: a column's value does not depend on how many others the call holds or what they are."""
    ped, lk, flags, assign = batch(name, 5)
    rng = np.random.RandomState(6)
    many = np.concatenate([assign, rng.randint(-1, ped.n, size=(fs.MAX_RELABEL - len(assign), ped.n)).astype(np.int32)])
    assert many.shape[0] == 64
    ref = reference(ped, 1e-4, lk, flags, many)
    clear(ref)
    model = fs.make_model(ped, mrate=1e-4)
    fn = build_relabel_host(model, tmp_path)[0]
    out = run_relabel(fn, model, lk, flags, many)
    check(out, ref, "%s, 64 assignments" % name)
    for m in (0, 2, 40, 63):
        one = run_relabel(fn, model, lk, flags, many[m:m + 1])
        assert same_bits([one[0][:, 0], one[1], one[2]], [out[0][:, m], out[1], out[2]])
    shuffled = many[::-1]
    assert same_bits([run_relabel(fn, model, lk, flags, shuffled)[0][:, ::-1]], [out[0]])


@pytest.mark.parametrize("lean", [False, True])
def test_an_out_of_range_entry_reads_nothing_outside_the_row(lean, tmp_path):
    """The kernel itself (what the device entries reach unchecked) takes every entry outside 0 .. N-1 as -1: the site's row ends
    at the last byte before a page nobody may read, entries far outside are given, and the outputs are those of -1."""
    ped = pedigree("random1")
    n = ped.n
    lk, flags = clear_likelihoods(np.random.RandomState(8), ped, 1)
    page = mmap.PAGESIZE
    mem = mmap.mmap(-1, 2 * page)
    base = C.addressof(C.c_char.from_buffer(mem))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    assert libc.mprotect(base + page, page, 0) == 0  # PROT_NONE behind the row
    row = np.frombuffer(mem, dtype=np.float64, count=3 * n, offset=page - 24 * n)
    row[:] = lk.reshape(-1)
    wild = np.tile(np.arange(n, dtype=np.int32), (6, 1))
    tame = wild.copy()
    for j, v in enumerate((n, n + 5, -2, -7, 2 ** 31 - 1, -2 ** 31)):
        wild[j, (j * 3) % n] = v
        wild[j, n - 1 - j] = v
        tame[j, (j * 3) % n] = tame[j, n - 1 - j] = -1
    model = fs.make_model(ped)
    fn = build_relabel_host(model, tmp_path, lean=lean)[0]
    want = run_relabel(fn, model, lk, flags, tame)
    got = run_relabel(fn, model, lk, flags, wild, lk_at=base + page - 24 * n)
    assert np.all(want[2] == 0) and same_bits(got, want)
    del row
    assert libc.mprotect(base + page, page, 3) == 0
    mem.close()


def test_generating_the_relabel_kernel_leaves_the_other_sources_alone(tmp_path):
    """The new body and the shell's new field must not reach the text of the existing kernels (their code objects are cached by
    content hash)."""
    ped = pedigree("random0")
    model = fs.make_model(ped)
    env = dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_KEEP_SRC="1", FAMSEQ_JIT_SOURCE_ONLY="1")
    stems = ("map", "map_prior", "evidence", "evidence_prior", "loo", "loo_prior", "prior", "pattern", "pattern_prior", "sample",
             "sample_prior", "af")
    keys = ("elim_code_object", "trio_code_object") + tuple(s + "_code_object" for s in stems)
    with mock.patch.dict(os.environ, env):
        ctx = fs.Context(model, device=-1, engine=fs.ENGINE_ELIM)
        ctx.set_option("trio_kernels", 3)
        for stem in stems:
            ctx.set_option(stem + "_kernels", 1)
        before = ctx.plan()
        texts = {k: open(before[k][:-6] + ".hip").read() for k in keys}
        assert before["relabel_code_object"] == "" and before["relabel_variant"] == -1
        ctx.set_option("relabel_kernels", 1)
        ctx.set_option("relabel_prior_kernels", 1)
        after = ctx.plan()
        ctx.close()
    for k in keys:
        assert before[k] == after[k] and open(after[k][:-6] + ".hip").read() == texts[k]
    assert after["relabel_code_object"] not in [before[k] for k in keys]
    assert after["relabel_prior_code_object"] not in [before[k] for k in keys] + [after["relabel_code_object"]]


def test_plan_only_behaviour(tmp_path):
    from test_gpu_denovo import four_loops

    ctx = fs.Context(fs.make_model(four_loops()), device=-1)
    for key in ("relabel_kernels", "relabel_prior_kernels"):
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*more than three"):
            ctx.set_option(key, 1)
    ctx.close()
    ped = pedigree("random0")
    ones = np.ones((1, ped.n, 3))
    with mock.patch.dict(os.environ, dict(FAMSEQ_KERNEL_CACHE=str(tmp_path), FAMSEQ_JIT_SOURCE_ONLY="1")):
        ctx = fs.Context(fs.make_model(ped), device=-1)
        plan = ctx.plan()
        assert plan["relabel_code_object"] == "" and plan["relabel_variant"] == -1
        assert plan["relabel_prior_code_object"] == "" and plan["relabel_prior_variant"] == -1
        with pytest.raises(fs.FamseqError, match="takes 1"):
            ctx.set_option("relabel_kernels", 2)
        ctx.set_option("relabel_kernels", 1)
        ctx.set_option("relabel_prior_kernels", 1)
        plan = ctx.plan()
        assert plan["relabel_code_object"].endswith(".hsaco") and 0 <= plan["relabel_variant"] < N_VARIANTS
        assert plan["relabel_prior_code_object"].endswith(".hsaco") and plan["relabel_prior_variant"] == plan["relabel_variant"]
        assert plan["relabel_prior_code_object"] != plan["relabel_code_object"] and plan["evidence_code_object"] == ""
        # the ABI's refusals of the assignments come before anything else, so a context without a device gives them too
        good = np.arange(ped.n, dtype=np.int32)[None, :]
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_assign must be 1\.\.64"):
            ctx.relabel_batch(np.tile(good, (65, 1)), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-1\).*n_assign must be 1\.\.64"):
            ctx.relabel_batch(np.zeros((0, ped.n), np.int32), lk=ones)
        for value in (ped.n, -2):
            bad = np.tile(good, (3, 1))
            bad[1, ped.n - 1] = value
            bad[2, 0] = value  # (the first is named)
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*assignment 1, member %d is %d" % (ped.n - 1, value)):
                ctx.relabel_batch(bad, lk=ones)
            with pytest.raises(fs.FamseqError, match=r"\(-1\).*assignment 1, member %d is %d" % (ped.n - 1, value)):
                ctx.relabel_prior_batch(np.ones((1, 6)), bad, lk=ones)
        for fn, more in (("famseq_relabel_batch", ()), ("famseq_relabel_prior_batch", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 1, None, None, None)
            assert rc == -1 and "assign must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        for fn, more in (("famseq_relabel_batch_device", ()), ("famseq_relabel_prior_batch_device", (None,))):
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 0, None, None, None, None)
            assert rc == -1 and "n_assign must be 1..64" in fs.lib().famseq_last_error(ctx._h).decode()
            rc = getattr(fs.lib(), fn)(ctx._h, 1, None, None, None, 0, None, *more, None, 2, None, None, None, None)
            assert rc == -1 and "assign must be given" in fs.lib().famseq_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match="shape"):
            ctx.relabel_batch(np.zeros((1, ped.n + 1), np.int32), lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.relabel_batch(good, lk=ones)
        with pytest.raises(fs.FamseqError, match=r"\(-4\)|without a device"):
            ctx.relabel_prior_batch(np.ones((1, 6)), good, lk=ones)
        ctx.close()


def test_swap_assignments():
    a, pairs = fs.swap_assignments(3)
    assert pairs == [(0, 1), (0, 2), (1, 2)] and a.dtype == np.int32
    assert a.tolist() == [[1, 0, 2], [2, 1, 0], [0, 2, 1]]
    a, pairs = fs.swap_assignments(5, [3, 0, 4])
    assert pairs == [(3, 0), (3, 4), (0, 4)]
    assert a.tolist() == [[3, 1, 2, 0, 4], [0, 1, 2, 4, 3], [4, 1, 2, 3, 0]]
    a, pairs = fs.swap_assignments(4, [2])
    assert pairs == [] and a.shape == (0, 4)
    assert len(fs.swap_assignments(11)[1]) == 55 <= fs.MAX_RELABEL
    for args in ((3, [3]), (3, [-1]), (3, [0, 0])):
        with pytest.raises(ValueError):
            fs.swap_assignments(*args)
