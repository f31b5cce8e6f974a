"""famseq_amd — MI355X-native FamSeq `-method 1` pedigree posterior (host-side Python binding).

The product is ``famseq_amd/lib/libfamseq_hip.so`` (HIP, gfx950; C ABI in
``include/famseq_hip.h``).  This module is a thin ctypes layer over that ABI whose
``Family`` class mirrors the slice of the reference's ``class family`` that the path
uses (/root/reference/src/family.h:225-375): construct from PED members, ``set_LK`` /
``calPostProbBN`` / ``get_postProb`` / ``get_postProbSingle`` / ``get_postRlt`` — except
that ``set_LK`` takes a batch of sites, because the boundary is batched.

There is no CPU compute path: if the shared library is missing, or no gfx950 device is
usable, the calls raise.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

from . import shard, synth  # noqa: F401
from .pedigree import Pedigree, read_ped, synthetic_pedigree  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libfamseq_hip.so")
MAXN = 20
TEXT_STRIDE = 80  # FAMSEQ_TEXT_STRIDE

ST_OK, ST_SINGLE_FAIL, ST_BN_FAIL, ST_SHORTCUT = 0, 1, 2, 0x80
FLAG_KNOWN, FLAG_CHRX = 1, 2
ENGINE_ENUM, ENGINE_ELIM = 0, 1


class FamseqError(RuntimeError):
    pass


class CModel(C.Structure):
    """famseq_model (include/famseq_hip.h)."""
    _fields_ = [
        ("n_members", C.c_int32),
        ("mother", C.c_int32 * MAXN),
        ("father", C.c_int32 * MAXN),
        ("gender", C.c_int32 * MAXN),
        ("sequenced", C.c_uint8 * MAXN),
        ("pcp2", C.c_double * 27),
        ("pcp2Xf", C.c_double * 27),
        ("pcp2Xm", C.c_double * 27),
        ("genoProbN", C.c_double * 3),
        ("genoProbK", C.c_double * 3),
        ("genoProbXN", C.c_double * 3),
        ("genoProbXK", C.c_double * 3),
        ("lc", C.c_double),
    ]


class CPedigree(C.Structure):
    """famseq_pedigree (include/famseq_hip.h): the size-independent model; the per-member arrays are numpy arrays
    kept alive in ``_keep``."""
    _fields_ = [
        ("n_members", C.c_int32),
        ("mother", C.POINTER(C.c_int32)),
        ("father", C.POINTER(C.c_int32)),
        ("gender", C.POINTER(C.c_int32)),
        ("sequenced", C.POINTER(C.c_uint8)),
        ("pcp2", C.c_double * 27),
        ("pcp2Xf", C.c_double * 27),
        ("pcp2Xm", C.c_double * 27),
        ("genoProbN", C.c_double * 3),
        ("genoProbK", C.c_double * 3),
        ("genoProbXN", C.c_double * 3),
        ("genoProbXK", C.c_double * 3),
        ("lc", C.c_double),
    ]


# every symbol include/famseq_hip.h declares
ABI_SYMBOLS = [
    "famseq_transmission_tables", "famseq_model_init", "famseq_pedigree_init", "famseq_device_count", "famseq_create",
    "famseq_create_pedigree",
    "famseq_destroy", "famseq_last_error", "famseq_set_option", "famseq_plan_json",
    "famseq_bn_batch", "famseq_bn_batch_sharded", "famseq_bn_batch_device", "famseq_bn_batch_device_sharded",
    "famseq_bn_call_batch", "famseq_bn_call_text_batch", "famseq_bn_call_batch_device", "famseq_format_probe", "famseq_alloc_pinned", "famseq_free_pinned", "famseq_stream_probe",
    "famseq_call_genotypes", "famseq_trio_children", "famseq_trio_batch", "famseq_trio_batch_device",
    "famseq_map_batch", "famseq_map_batch_device",
    "famseq_bn_prior_batch", "famseq_bn_prior_batch_device", "famseq_bn_prior_call_batch", "famseq_hwe_priors",
    "famseq_trio_prior_batch", "famseq_trio_prior_batch_device", "famseq_map_prior_batch", "famseq_map_prior_batch_device",
    "famseq_evidence_batch", "famseq_evidence_batch_device", "famseq_evidence_prior_batch", "famseq_evidence_prior_batch_device",
    "famseq_loo_batch", "famseq_loo_batch_device", "famseq_loo_prior_batch", "famseq_loo_prior_batch_device",
    "famseq_pattern_batch", "famseq_pattern_batch_device", "famseq_pattern_prior_batch", "famseq_pattern_prior_batch_device",
    "famseq_sample_batch", "famseq_sample_batch_device", "famseq_sample_prior_batch", "famseq_sample_prior_batch_device",
    "famseq_af_batch", "famseq_af_batch_device",
    "famseq_relabel_batch", "famseq_relabel_batch_device", "famseq_relabel_prior_batch", "famseq_relabel_prior_batch_device",
    "famseq_rate_tables",
    "famseq_mutrate_batch", "famseq_mutrate_batch_device", "famseq_mutrate_prior_batch", "famseq_mutrate_prior_batch_device",
    "famseq_allele_tables",
    "famseq_origin_batch", "famseq_origin_batch_device", "famseq_origin_prior_batch", "famseq_origin_prior_batch_device",
    "famseq_weight_batch", "famseq_weight_batch_device", "famseq_weight_prior_batch", "famseq_weight_prior_batch_device",
    "famseq_maxmarg_batch", "famseq_maxmarg_batch_device", "famseq_maxmarg_prior_batch", "famseq_maxmarg_prior_batch_device",
    "famseq_charfn_batch", "famseq_charfn_batch_device", "famseq_charfn_prior_batch", "famseq_charfn_prior_batch_device",
]
# (and famseq_philox4x32_10, the one name with digits in it: philox4x32 below)
PL_MISSING = 0xFFFF

_lib = None


def lib():
    """Load libfamseq_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FamseqError("%s not found: run `make` (or __graft_entry__.build()) first; "
                          "there is no fallback implementation" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so, and ours is
    # linked against the unversioned name so that it binds to whichever is already loaded
    # (see Makefile).  Import torch first so a later `import torch` cannot bring a second one.
    if "torch" not in sys.modules and not os.environ.get("FAMSEQ_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    mp = C.POINTER(CModel)
    L.famseq_transmission_tables.argtypes = [C.c_double, dp, dp, dp]
    L.famseq_transmission_tables.restype = None
    L.famseq_model_init.argtypes = [mp, C.c_int32, ip, ip, ip, ip, bp, C.c_double, C.c_double]
    L.famseq_model_init.restype = C.c_int
    L.famseq_pedigree_init.argtypes = [C.POINTER(CPedigree), C.c_int32, ip, ip, ip, ip, bp, C.c_double, C.c_double, ip, ip]
    L.famseq_pedigree_init.restype = C.c_int
    L.famseq_create_pedigree.argtypes = [C.POINTER(CPedigree), C.c_int, C.c_char_p, C.c_size_t]
    L.famseq_create_pedigree.restype = C.c_void_p
    L.famseq_device_count.restype = C.c_int
    L.famseq_create.argtypes = [mp, C.c_int, C.c_char_p, C.c_size_t]
    L.famseq_create.restype = C.c_void_p
    L.famseq_destroy.argtypes = [C.c_void_p]
    L.famseq_destroy.restype = None
    L.famseq_last_error.argtypes = [C.c_void_p]
    L.famseq_last_error.restype = C.c_char_p
    L.famseq_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.famseq_set_option.restype = C.c_int
    L.famseq_plan_json.argtypes = [C.c_void_p]
    L.famseq_plan_json.restype = C.c_char_p
    L.famseq_bn_batch.argtypes = [C.c_void_p, C.c_int64, dp, bp, dp, dp, bp]
    L.famseq_bn_batch.restype = C.c_int
    L.famseq_bn_batch_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int64, dp, bp, dp, dp, bp]
    L.famseq_bn_batch_sharded.restype = C.c_int
    vp = C.c_void_p
    L.famseq_bn_batch_device.argtypes = [C.c_void_p, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.famseq_bn_batch_device.restype = C.c_int
    pp = C.POINTER(C.c_void_p)
    L.famseq_bn_batch_device_sharded.argtypes = [pp, C.c_int, C.POINTER(C.c_int64), pp, pp, pp, pp, pp]
    L.famseq_bn_batch_device_sharded.restype = C.c_int
    L.famseq_bn_call_batch.argtypes = [C.c_void_p, C.c_int64, dp, C.POINTER(C.c_uint16), bp, ip, C.c_int32, dp, dp,
                                       C.POINTER(C.c_int8), bp]
    L.famseq_bn_call_batch.restype = C.c_int
    L.famseq_bn_call_text_batch.argtypes = [C.c_void_p, C.c_int64, dp, C.POINTER(C.c_uint16), bp, ip, C.c_int32, C.c_char_p, bp]
    L.famseq_bn_call_text_batch.restype = C.c_int
    L.famseq_bn_call_batch_device.argtypes = [C.c_void_p, C.c_int64, vp, vp, vp, ip, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.famseq_bn_call_batch_device.restype = C.c_int
    L.famseq_format_probe.argtypes = [C.c_void_p, C.c_int64, dp, C.c_char_p]
    L.famseq_format_probe.restype = C.c_int
    L.famseq_stream_probe.argtypes = [C.c_void_p, C.c_int64, vp, vp, vp, vp]
    L.famseq_stream_probe.restype = C.c_int
    L.famseq_alloc_pinned.argtypes = [C.c_size_t]
    L.famseq_alloc_pinned.restype = C.c_void_p
    L.famseq_free_pinned.argtypes = [C.c_void_p]
    L.famseq_free_pinned.restype = None
    L.famseq_call_genotypes.argtypes = [dp, C.c_int64, C.POINTER(C.c_int8)]
    L.famseq_call_genotypes.restype = None
    L.famseq_trio_children.argtypes = [C.c_void_p, ip]
    L.famseq_trio_children.restype = C.c_int
    L.famseq_bn_prior_batch.argtypes = [C.c_void_p, C.c_int64, dp, bp, dp, dp, dp, bp]
    L.famseq_bn_prior_batch.restype = C.c_int
    L.famseq_bn_prior_batch_device.argtypes = [C.c_void_p, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
    L.famseq_bn_prior_batch_device.restype = C.c_int
    L.famseq_bn_prior_call_batch.argtypes = [C.c_void_p, C.c_int64, dp, C.POINTER(C.c_uint16), bp, dp, C.POINTER(C.c_int32), C.c_int32, dp, dp,
                                             C.POINTER(C.c_int8), C.c_char_p, bp]
    L.famseq_bn_prior_call_batch.restype = C.c_int
    L.famseq_hwe_priors.argtypes = [C.c_int64, dp, dp]
    L.famseq_hwe_priors.restype = None
    # the side products' entries: famseq_<name>[_prior]_batch[_device]
    u16p = C.POINTER(C.c_uint16)
    # (more: what an entry takes between the prior rows and its outputs, as the host and the device entry declare it)
    masks = ([bp, C.c_int32], [vp, C.c_int32])
    draws = ([C.c_uint64, C.c_int64, C.c_int32],) * 2  # seed, site_base, n_draws
    assigns = ([ip, C.c_int32], [vp, C.c_int32])
    rates = ([dp, C.c_int32], [vp, C.c_int32])  # the host entries take the rates (weights), the device entries the resident tables
    for name, out_a, more in (("trio", dp, ([], [])), ("map", C.POINTER(C.c_int8), ([], [])), ("evidence", dp, ([], [])), ("loo", dp, ([], [])),
                              ("pattern", dp, masks), ("sample", C.POINTER(C.c_int8), draws),
                              ("relabel", dp, assigns), ("mutrate", dp, rates), ("origin", dp, ([], [])), ("weight", dp, rates),
                              ("maxmarg", dp, ([], [])), ("charfn", dp, rates)):
        for prior in (0, 1):
            host = getattr(L, "famseq_%s%s_batch" % (name, "_prior" * prior))
            dev = getattr(L, "famseq_%s%s_batch_device" % (name, "_prior" * prior))
            host.argtypes = [C.c_void_p, C.c_int64, dp, u16p, ip, C.c_int32, bp] + [dp] * prior + more[0] + [out_a, dp, bp]
            dev.argtypes = [C.c_void_p, C.c_int64, vp, vp, ip, C.c_int32, vp] + [vp] * prior + more[1] + [vp, vp, vp, vp]
            host.restype = dev.restype = C.c_int
    # (the allele-frequency entries: no site-prior form; af0 and n_iter stand where the others' `more` does)
    L.famseq_af_batch.argtypes = [C.c_void_p, C.c_int64, dp, u16p, ip, C.c_int32, bp, dp, C.c_int32, dp, dp, bp]
    L.famseq_af_batch_device.argtypes = [C.c_void_p, C.c_int64, vp, vp, ip, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp]
    L.famseq_af_batch.restype = L.famseq_af_batch_device.restype = C.c_int
    L.famseq_rate_tables.argtypes = [C.c_void_p, dp, C.c_int32, dp]
    L.famseq_rate_tables.restype = C.c_int
    L.famseq_allele_tables.argtypes = [C.c_void_p, dp]
    L.famseq_allele_tables.restype = C.c_int
    u32p = C.POINTER(C.c_uint32)
    L.famseq_philox4x32_10.argtypes = [u32p, u32p, u32p]
    L.famseq_philox4x32_10.restype = None
    _lib = L
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


_POINTER = {np.dtype(t): C.POINTER(c) for t, c in ((np.float64, C.c_double), (np.uint16, C.c_uint16), (np.int32, C.c_int32),
                                                  (np.uint8, C.c_uint8), (np.int8, C.c_int8))}


def _opt(a):
    """An optional array as the pointer to its element type (None: NULL)."""
    return None if a is None else a.ctypes.data_as(_POINTER[a.dtype])


def _inputs(n, lk, pl16, seq_members, flags, n_seq_required):
    """What the entries that take likelihood rows or packed PLs are given: exactly one of lk [S,n,3] and pl16 [S,n_seq,3], the
    sequenced members and the flags, as contiguous arrays.  -> (lk, pl16, S, seq, n_seq, flags).  n_seq_required: the call
    path, which takes seq_members with either input (and leaves the flags' shape to the library); otherwise they are read with
    pl16 only, and the flags must have one byte per site."""
    seq, n_seq = None, 0
    if n_seq_required:
        seq = np.ascontiguousarray(seq_members, dtype=np.int32)
        n_seq = len(seq)
    if (lk is None) == (pl16 is None):
        raise ValueError("give exactly one of lk / pl16")
    if lk is not None:
        lk = np.ascontiguousarray(lk, dtype=np.float64).reshape(-1, n, 3)
        s = lk.shape[0]
    else:
        if seq is None:
            seq = np.ascontiguousarray(seq_members, dtype=np.int32)
            n_seq = len(seq)
        pl16 = np.ascontiguousarray(pl16, dtype=np.uint16).reshape(-1, n_seq, 3)
        s = pl16.shape[0]
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    if not n_seq_required and fl is not None and fl.shape != (s,):
        raise ValueError("flags must have one byte per site")
    return lk, pl16, s, seq, n_seq, fl


def transmission_tables(mrate):
    a, b, c = (np.zeros(27) for _ in range(3))
    lib().famseq_transmission_tables(float(mrate), _p(a, C.c_double), _p(b, C.c_double), _p(c, C.c_double))
    return a, b, c


def device_count():
    return lib().famseq_device_count()


def _prior_rows(prior, s):
    prior = np.ascontiguousarray(prior, dtype=np.float64)
    if prior.shape != (s, 6):
        raise ValueError("prior must be [n_sites, 6]")
    return prior


def hwe_priors(af):
    """Hardy-Weinberg founder priors from allele frequencies (famseq_hwe_priors): -> prior[S, 6] for bn_prior_batch.
    Row s is ((1-q)^2, 2q(1-q), q^2) — female founders, and every founder off chrX — then (1-q, 0, q), male founders on chrX."""
    af = np.ascontiguousarray(af, dtype=np.float64).ravel()
    prior = np.empty((len(af), 6))
    lib().famseq_hwe_priors(len(af), _p(af, C.c_double), _p(prior, C.c_double))
    return prior


def philox4x32(counter, key):
    """One block of Philox4x32-10, the generator of Context.sample_batch (famseq_philox4x32_10): counter (4 words), key (2 words)
    -> uint32[4].  Word w of the stream of site i's draw k under `seed` is element w % 4 of
    philox4x32((i & 0xffffffff, i >> 32, k, w // 4), (seed & 0xffffffff, seed >> 32))."""
    c = np.ascontiguousarray(counter, dtype=np.uint32)
    k = np.ascontiguousarray(key, dtype=np.uint32)
    if c.shape != (4,) or k.shape != (2,):
        raise ValueError("counter must have 4 words and key 2")
    out = np.empty(4, np.uint32)
    lib().famseq_philox4x32_10(_p(c, C.c_uint32), _p(k, C.c_uint32), _p(out, C.c_uint32))
    return out


SEGREGATION_MASKS = {"dominant": (6, 1), "recessive": (4, 3)}  # model -> (affected, unaffected); anyone else 7


def segregation_masks(n, affected, unaffected=(), model="dominant"):
    """The mask row [n] uint8 of a segregation pattern for Context.pattern_batch; affected / unaffected: member indices (PED
    order).  dominant: the affected carry the variant (genotypes 1, 2: mask 6), the unaffected are hom-ref (1).  recessive: the
    affected are hom-alt (4), the unaffected are not (3).  A member in neither list is unconstrained (7)."""
    if model not in SEGREGATION_MASKS:
        raise ValueError("model must be 'dominant' or 'recessive', got %r" % (model,))
    aff, unaff = [int(i) for i in affected], [int(i) for i in unaffected]
    for i in aff + unaff:
        if not 0 <= i < n:
            raise ValueError("member index %d is outside 0..%d" % (i, n - 1))
    if set(aff) & set(unaff):
        raise ValueError("members %s are listed as affected and as unaffected" % sorted(set(aff) & set(unaff)))
    row = np.full(n, 7, np.uint8)
    row[aff], row[unaff] = SEGREGATION_MASKS[model]
    return row


def penetrance_weights(n, affected, unaffected=(), pen=(0.0, 1.0, 1.0)):
    """The weight table [n, 3] float64 of a penetrance model for Context.weight_batch; affected / unaffected: member indices (PED
    order); pen = (f0, f1, f2), the probability of being affected given 0, 1, 2 alt alleles.  An affected member's row is pen, an
    unaffected member's 1 - pen, anyone else's ones (phenotype unknown).  pen = (0, 1, 1) is segregation_masks' dominant model,
    (0, 0, 1) its recessive one."""
    f = np.asarray(pen, dtype=np.float64)
    if f.shape != (3,) or not np.all((f >= 0) & (f <= 1)):
        raise ValueError("pen must be three probabilities (f0, f1, f2) in [0, 1], got %r" % (pen,))
    aff, unaff = [int(i) for i in affected], [int(i) for i in unaffected]
    for i in aff + unaff:
        if not 0 <= i < n:
            raise ValueError("member index %d is outside 0..%d" % (i, n - 1))
    if set(aff) & set(unaff):
        raise ValueError("members %s are listed as affected and as unaffected" % sorted(set(aff) & set(unaff)))
    w = np.ones((n, 3))
    w[aff], w[unaff] = f, 1.0 - f
    return w


MAX_RELABEL = 64
MAX_RATES = 32
MAX_WEIGHTS = 32
MAX_CWEIGHTS = 64
COUNT_KINDS = {"carriers": (0, 1, 1), "alleles": (0, 1, 2), "homalt": (0, 0, 1)}
COUNT_CLIP = 1e-12  # count_from_cf: a probability in [-COUNT_CLIP, 0) is rounding below an exact 0 (charfn_batch's absolute bar)


def count_scores(n, members=None, kind="carriers"):
    """The per-member genotype scores [n, 3] int64 of an additive count for count_tables / Context.count_batch: the members
    named (indices in PED order; default all n) score (0, 1, 1) per genotype for kind "carriers", (0, 1, 2) for "alleles" — the
    genotype index as coded: a male's genotype 2 at a chrX site counts 2 — and (0, 0, 1) for "homalt"; everyone else scores 0."""
    if kind not in COUNT_KINDS:
        raise ValueError("kind must be 'carriers', 'alleles' or 'homalt', got %r" % (kind,))
    mem = list(range(n)) if members is None else [int(i) for i in members]
    for i in mem:
        if not 0 <= i < n:
            raise ValueError("member index %d is outside 0..%d" % (i, n - 1))
    if len(set(mem)) != len(mem):
        raise ValueError("members are listed twice: %s" % sorted(i for i in set(mem) if mem.count(i) > 1))
    scores = np.zeros((n, 3), np.int64)
    scores[mem] = COUNT_KINDS[kind]
    return scores


def count_tables(scores):
    """The complex weight tables of the count sum_p scores[p][g_p] for Context.charfn_batch: -> (tables [M // 2 + 1, N, 3]
    complex128, D).  D = sum_p max_g scores[p][g] is the count's largest value, M = D + 1 the length of its distribution, and
    table j is omega^(j * scores), omega = exp(2 pi i / M), for j = 0 .. M // 2: the other frequencies are these ones' conjugates
    (count_from_cf).  scores: non-negative integers [N, 3]."""
    sc = np.asarray(scores)
    if sc.ndim != 2 or sc.shape[1] != 3 or sc.dtype.kind not in "iu" or np.any(sc < 0):
        raise ValueError("scores must be non-negative integers [N, 3]")
    D = int(sc.max(axis=1).sum())
    M = D + 1
    if M // 2 + 1 > MAX_CWEIGHTS:
        raise ValueError("a count that reaches D = %d needs %d tables, more than the %d of one call" % (D, M // 2 + 1, MAX_CWEIGHTS))
    j = np.arange(M // 2 + 1)[:, None, None]
    # (the exponent reduced mod M in integers, so that omega^(j s) is exact at the quarter turns and equal where j s mod M is)
    return np.exp(2j * np.pi * ((j * sc[None].astype(np.int64)) % M) / M), D


def count_from_cf(cf, D):
    """The count's distribution from its characteristic function at the frequencies count_tables gives: cf [S, D // 2 + 1]
    complex (or [S, D // 2 + 1, 2] float64, charfn_batch's own) -> dist [S, D + 1] float64, dist[s, k] = P(count = k | data) =
    (1 / M) sum_j phi_j omega^(-j k) with M = D + 1, the missing frequencies the conjugates of those given; the real part.
    Values in [-1e-12, 0), rounding below an exact 0, become 0.0; nothing is renormalised; a failed site's row (NaN) stays NaN."""
    phi = np.asarray(cf)
    if not np.iscomplexobj(phi):
        phi = phi[..., 0] + 1j * phi[..., 1]
    M = int(D) + 1
    if phi.ndim != 2 or phi.shape[1] != M // 2 + 1:
        raise ValueError("cf must hold %d frequencies per site for D = %d, got %s" % (M // 2 + 1, D, list(phi.shape)))
    full = np.empty((phi.shape[0], M), np.complex128)
    full[:, :M // 2 + 1] = phi
    j = np.arange(M // 2 + 1, M)
    full[:, j] = np.conj(phi[:, M - j])
    jk = (np.arange(M)[:, None] * np.arange(M)[None, :]) % M
    with np.errstate(invalid="ignore"):
        dist = (full @ np.exp(-2j * np.pi * jk / M)).real / M
        dist[(dist < 0) & (dist >= -COUNT_CLIP)] = 0.0
    return dist
RATE_TABLE_DOUBLES = 432
ALLELE_TABLE_DOUBLES = 48


def swap_assignments(n, members=None):
    """The assignment rows of every transposition of two of `members` (member indices in PED order; default all n) for
    Context.relabel_batch: -> (assign [M, n] int32, pairs), pairs[k] = (i, j) the two members row k exchanges, i before j in the
    order of `members`, the pairs ordered (first, second) in that order.  Everybody else keeps their own row."""
    mem = list(range(n)) if members is None else [int(i) for i in members]
    for i in mem:
        if not 0 <= i < n:
            raise ValueError("member index %d is outside 0..%d" % (i, n - 1))
    if len(set(mem)) != len(mem):
        raise ValueError("members are listed twice: %s" % sorted(i for i in set(mem) if mem.count(i) > 1))
    pairs = [(mem[a], mem[b]) for a in range(len(mem)) for b in range(a + 1, len(mem))]
    assign = np.tile(np.arange(n, dtype=np.int32), (len(pairs), 1))
    for k, (i, j) in enumerate(pairs):
        assign[k, i], assign[k, j] = j, i
    return assign, pairs


def make_model(ped: Pedigree, mrate=1e-7, lc=1.0, genoProbN=None, genoProbK=None, genoProbXN=None,
               genoProbXK=None, sequenced=None, size_independent=False):
    """family(mem, mRate) + set_genoProb* + set_lc + init()  (file.cpp:1888-1927).  Up to 20 members: the fixed
    famseq_model; beyond (or size_independent=True): famseq_pedigree, which only the sum-product engine serves."""
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    ids, mids, fids, gen = i32(ped.ids), i32(ped.mids), i32(ped.fids), i32(ped.genders)
    seq = np.ascontiguousarray(ped.sequenced if sequenced is None else sequenced, dtype=np.uint8)
    if ped.n > MAXN or size_independent:
        m = CPedigree()
        mo, fa = np.zeros(ped.n, np.int32), np.zeros(ped.n, np.int32)
        m._keep = (gen, seq, mo, fa)  # the struct points into these
        rc = lib().famseq_pedigree_init(C.byref(m), ped.n, _p(ids, C.c_int32), _p(mids, C.c_int32), _p(fids, C.c_int32),
                                        _p(gen, C.c_int32), _p(seq, C.c_uint8), float(mrate), float(lc), _p(mo, C.c_int32),
                                        _p(fa, C.c_int32))
    else:
        m = CModel()
        rc = lib().famseq_model_init(C.byref(m), ped.n, _p(ids, C.c_int32), _p(mids, C.c_int32), _p(fids, C.c_int32),
                                     _p(gen, C.c_int32), _p(seq, C.c_uint8), float(mrate), float(lc))
    if rc != 0:
        msg = {-10: "This is not a fulfill family. Please check the ped file.",
               -11: "a mother is not female or a father is not male"}.get(rc, "bad pedigree arguments")
        raise FamseqError("famseq_model_init: %s (%d)" % (msg, rc))
    for name, v in (("genoProbN", genoProbN), ("genoProbK", genoProbK), ("genoProbXN", genoProbXN),
                    ("genoProbXK", genoProbXK)):
        if v is not None:
            for g in range(3):
                getattr(m, name)[g] = float(v[g])
    return m


class Context:
    """famseq_ctx: one model bound to one GPU (device=-1: plan only, no compute)."""

    def __init__(self, model, device=0, **options):
        self.n = model.n_members
        self._model = model
        err = C.create_string_buffer(512)
        create = lib().famseq_create_pedigree if isinstance(model, CPedigree) else lib().famseq_create
        self._h = create(C.byref(model), int(device), err, len(err))
        if not self._h:
            raise FamseqError("famseq_create: " + err.value.decode())
        for k, v in options.items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "_h", None):
            lib().famseq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise FamseqError("%s failed (%d): %s" % (what, rc, lib().famseq_last_error(self._h).decode()))

    def set_option(self, key, value):
        self._check(lib().famseq_set_option(self._h, key.encode(), int(value)), "famseq_set_option(%s)" % key)

    def plan(self):
        return json.loads(lib().famseq_plan_json(self._h).decode())

    def bn_batch(self, lk, flags=None, want_single=True, want_status=True):
        """Host arrays in, host arrays out: (post, single, status)."""
        lk = np.ascontiguousarray(lk, dtype=np.float64).reshape(-1, self.n, 3)
        s = lk.shape[0]
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        if fl is not None and fl.shape != (s,):
            raise ValueError("flags must have one byte per site")
        post = np.empty_like(lk)
        single = np.empty_like(lk) if want_single else None
        status = np.zeros(s, np.uint8) if want_status else None
        rc = lib().famseq_bn_batch(self._h, s, _p(lk, C.c_double), None if fl is None else _p(fl, C.c_uint8),
                                   _p(post, C.c_double), None if single is None else _p(single, C.c_double),
                                   None if status is None else _p(status, C.c_uint8))
        self._check(rc, "famseq_bn_batch")
        return post, single, status

    def bn_prior_batch(self, lk, prior, flags=None, want_single=True, want_status=True):
        """bn_batch with the founders' genotype prior given per site: -> (post, single, status).
        prior [S, 6] float64: doubles 0-2 the prior of female founders and of every founder at an autosomal site, doubles 3-5
        the prior of male founders at a chrX site (hwe_priors makes such rows from allele frequencies).  Of the flags only
        FLAG_CHRX is read.  Always the sum-product kernel, whatever this context's engine is."""
        lk = np.ascontiguousarray(lk, dtype=np.float64).reshape(-1, self.n, 3)
        s = lk.shape[0]
        prior = np.ascontiguousarray(prior, dtype=np.float64)
        if prior.shape != (s, 6):
            raise ValueError("prior must have six doubles per site")
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        if fl is not None and fl.shape != (s,):
            raise ValueError("flags must have one byte per site")
        post = np.empty_like(lk)
        single = np.empty_like(lk) if want_single else None
        status = np.zeros(s, np.uint8) if want_status else None
        rc = lib().famseq_bn_prior_batch(self._h, s, _p(lk, C.c_double), None if fl is None else _p(fl, C.c_uint8),
                                         _p(prior, C.c_double), _p(post, C.c_double),
                                         None if single is None else _p(single, C.c_double),
                                         None if status is None else _p(status, C.c_uint8))
        self._check(rc, "famseq_bn_prior_batch")
        return post, single, status

    def bn_prior_batch_device(self, n_sites, d_lk, d_flags, d_prior, d_post, d_single=0, d_status=0, stream=0):
        """bn_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        rc = lib().famseq_bn_prior_batch_device(self._h, int(n_sites), d_lk or None, d_flags or None, d_prior or None, d_post or None,
                                                d_single or None, d_status or None, stream or None)
        self._check(rc, "famseq_bn_prior_batch_device")

    def bn_call_batch(self, seq_members, lk=None, pl16=None, flags=None):
        """Fused call path: -> (gpp[S,n_seq,3], fpp[S,n_seq,3], fgt[S,n_seq], status[S]).
        Input is either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16 (VCF column order)."""
        lk, pl16, s, seq, k, fl = _inputs(self.n, lk, pl16, seq_members, flags, True)
        gpp, fpp = np.empty((s, k, 3)), np.empty((s, k, 3))
        fgt, status = np.empty((s, k), np.int8), np.zeros(s, np.uint8)
        rc = lib().famseq_bn_call_batch(self._h, s, _opt(lk), _opt(pl16), _opt(fl), _p(seq, C.c_int32), k,
                                        _p(gpp, C.c_double), _p(fpp, C.c_double), _p(fgt, C.c_int8), _p(status, C.c_uint8))
        self._check(rc, "famseq_bn_call_batch")
        return gpp, fpp, fgt, status

    def bn_prior_call_batch(self, seq_members, prior, lk=None, pl16=None, flags=None):
        """bn_call_batch with the founders' prior given per site (prior [S,6] as for bn_prior_batch): separate stages around the
        site-prior kernel.  -> (gpp, fpp, fgt, status)."""
        lk, pl16, s, seq, k, fl = _inputs(self.n, lk, pl16, seq_members, flags, True)
        prior = np.ascontiguousarray(prior, dtype=np.float64)
        if prior.shape != (s, 6):
            raise ValueError("prior must be [n_sites, 6]")
        gpp, fpp = np.empty((s, k, 3)), np.empty((s, k, 3))
        fgt, status = np.empty((s, k), np.int8), np.zeros(s, np.uint8)
        rc = lib().famseq_bn_prior_call_batch(self._h, s, _opt(lk), _opt(pl16), _opt(fl), _p(prior, C.c_double), _p(seq, C.c_int32), k,
                                              _p(gpp, C.c_double), _p(fpp, C.c_double), _p(fgt, C.c_int8), None, _p(status, C.c_uint8))
        self._check(rc, "famseq_bn_prior_call_batch")
        return gpp, fpp, fgt, status

    def bn_call_text_batch(self, seq_members, lk=None, pl16=None, flags=None):
        """The call path with its outputs as text: -> (records, status).  records[s][j] is the bytes the reference's drivers
        append to sample column j of site s, b"g0,g1,g2:f0,f1,f2:0/1\\t" (file.cpp:696-745), formatted on the device."""
        lk, pl16, s, seq, k, fl = _inputs(self.n, lk, pl16, seq_members, flags, True)
        text = np.zeros((s, k, TEXT_STRIDE), np.uint8)
        status = np.zeros(s, np.uint8)
        rc = lib().famseq_bn_call_text_batch(self._h, s, _opt(lk), _opt(pl16), _opt(fl), _p(seq, C.c_int32), k,
                                             text.ctypes.data_as(C.c_char_p), _p(status, C.c_uint8))
        self._check(rc, "famseq_bn_call_text_batch")
        return text, status

    def bn_call_batch_device(self, n_sites, seq_members, d_lk=0, d_pl16=0, d_flags=0, d_gpp=0, d_fpp=0, d_fgt=0, d_status=0, d_text=0,
                             stream=0):
        """The call path on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        seq = np.ascontiguousarray(seq_members, dtype=np.int32)
        rc = lib().famseq_bn_call_batch_device(self._h, int(n_sites), d_lk or None, d_pl16 or None, d_flags or None, _p(seq, C.c_int32),
                                               len(seq), d_gpp or None, d_fpp or None, d_fgt or None, d_status or None, d_text or None,
                                               stream or None)
        self._check(rc, "famseq_bn_call_batch_device")

    def trio_children(self):
        """Member indices of the children (the members with parents, PED order): child k of trio_batch is member children[k]."""
        k = lib().famseq_trio_children(self._h, None)
        self._check(min(k, 0), "famseq_trio_children")
        idx = np.zeros(k, np.int32)
        if k:
            lib().famseq_trio_children(self._h, _p(idx, C.c_int32))
        return idx

    def _side_host(self, name, prior, lk, pl16, seq_members, flags, outs, more=()):
        """The host entry of a side product, famseq_<name>_batch or (prior given) famseq_<name>_prior_batch.  outs(S) makes its two
        output arrays (None: not wanted); more: the arguments the entry takes between the prior rows and its outputs.
        -> (out_a, out_b, status)."""
        lk, pl16, s, seq, n_seq, fl = _inputs(self.n, lk, pl16, seq_members, flags, False)
        out_a, out_b = outs(s)
        status = np.zeros(s, np.uint8)
        fn = "famseq_%s%s_batch" % (name, "" if prior is None else "_prior")
        rows = () if prior is None else (_p(_prior_rows(prior, s), C.c_double),)
        self._check(getattr(lib(), fn)(self._h, s, _opt(lk), _opt(pl16), _opt(seq), n_seq, _opt(fl), *rows, *more, _opt(out_a), _opt(out_b),
                                       _opt(status)), fn)
        return out_a, out_b, status

    def _side_device(self, name, n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior, d_a, d_b, d_status, stream, more=()):
        """The device entry of a side product on raw device pointers, famseq_<name>_batch_device or (d_prior not None: an int, 0
        = not given) famseq_<name>_prior_batch_device.  more: as _side_host's."""
        seq = np.ascontiguousarray(seq_members, dtype=np.int32)
        fn = "famseq_%s%s_batch_device" % (name, "" if d_prior is None else "_prior")
        rows = () if d_prior is None else (d_prior or None,)
        self._check(getattr(lib(), fn)(self._h, int(n_sites), d_lk or None, d_pl16 or None, _p(seq, C.c_int32) if len(seq) else None, len(seq),
                                       d_flags or None, *rows, *more, d_a or None, d_b or None, d_status or None, stream or None), fn)

    def trio_batch(self, lk=None, pl16=None, seq_members=None, flags=None, want_joint=True, want_dnm=True):
        """Trio posteriors: -> (children[K], joint[S,K,27] or None, dnm[S,K] or None, status[S]).
        joint[s, k, 9 gc + 3 gm + gf] is the posterior of child k's and its parents' genotypes; dnm[s, k] the mass of the
        entries the mutation-free transmission table rules out.  Input is either lk [S,N,3] float64 or pl16 [S,n_seq,3]
        uint16 in VCF column order (seq_members: their PED indices)."""
        return self._trio(None, lk, pl16, seq_members, flags, want_joint, want_dnm)

    def trio_prior_batch(self, prior, lk=None, pl16=None, seq_members=None, flags=None, want_joint=True, want_dnm=True):
        """trio_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give trio_batch's bits."""
        return self._trio(prior, lk, pl16, seq_members, flags, want_joint, want_dnm)

    def _trio(self, prior, lk, pl16, seq_members, flags, want_joint, want_dnm):
        children = self.trio_children() if (lk is None) != (pl16 is None) else ()  # (else _inputs says what is wrong)
        k = len(children)
        outs = lambda s: (np.empty((s, k, 27)) if want_joint else None, np.empty((s, k)) if want_dnm else None)
        return (children,) + self._side_host("trio", prior, lk, pl16, seq_members, flags, outs)

    def trio_batch_device(self, n_sites, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_joint=0, d_dnm=0, d_status=0, stream=0):
        """Trio posteriors on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("trio", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_joint, d_dnm, d_status, stream)

    def trio_prior_batch_device(self, n_sites, d_prior, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_joint=0, d_dnm=0, d_status=0, stream=0):
        """trio_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("trio", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_joint, d_dnm, d_status, stream)

    def map_batch(self, lk=None, pl16=None, seq_members=None, flags=None, want_gt=True, want_post=True):
        """The joint MAP configuration: -> (map_gt[S,N] int8, map_post[S] float64, status[S] uint8).
        map_gt[s] is the most probable genotype assignment of the whole pedigree at site s (0 / 1 / 2 per member, PED order; -1
        where status != 0), map_post[s] its posterior probability (NaN where status != 0).  Input as trio_batch: either lk
        [S,N,3] float64 or pl16 [S,n_seq,3] uint16 in VCF column order (seq_members: their PED indices).  want_gt / want_post
        False: that output is not computed and returned as None."""
        outs = lambda s: (np.empty((s, self.n), np.int8) if want_gt else None, np.empty(s) if want_post else None)
        return self._side_host("map", None, lk, pl16, seq_members, flags, outs)

    def map_prior_batch(self, prior, lk=None, pl16=None, seq_members=None, flags=None, want_gt=True, want_post=True):
        """map_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give map_batch's bits."""
        outs = lambda s: (np.empty((s, self.n), np.int8) if want_gt else None, np.empty(s) if want_post else None)
        return self._side_host("map", prior, lk, pl16, seq_members, flags, outs)

    def map_batch_device(self, n_sites, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_map_gt=0, d_map_post=0, d_status=0, stream=0):
        """The joint MAP configuration on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream`
        and returns."""
        self._side_device("map", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_map_gt, d_map_post, d_status, stream)

    def map_prior_batch_device(self, n_sites, d_prior, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_map_gt=0, d_map_post=0, d_status=0,
                               stream=0):
        """map_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("map", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_map_gt, d_map_post, d_status, stream)

    def evidence_batch(self, lk=None, pl16=None, seq_members=None, flags=None, want_loglik=True, want_pref=True):
        """The evidence: -> (loglik[S] float64, pref[S] float64, status[S] uint8).
        loglik[s] is log10 of the data's likelihood under the pedigree at site s, pref[s] the posterior probability that every
        member is hom-ref (both NaN where status != 0).  Input as map_batch: either lk [S,N,3] float64 or pl16 [S,n_seq,3]
        uint16 in VCF column order (seq_members: their PED indices).  want_loglik / want_pref False: that output is not
        computed and returned as None."""
        outs = lambda s: (np.empty(s) if want_loglik else None, np.empty(s) if want_pref else None)
        return self._side_host("evidence", None, lk, pl16, seq_members, flags, outs)

    def evidence_prior_batch(self, prior, lk=None, pl16=None, seq_members=None, flags=None, want_loglik=True, want_pref=True):
        """evidence_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags
        only FLAG_CHRX is read).  Rows equal to the model's constants give evidence_batch's bits."""
        outs = lambda s: (np.empty(s) if want_loglik else None, np.empty(s) if want_pref else None)
        return self._side_host("evidence", prior, lk, pl16, seq_members, flags, outs)

    def evidence_batch_device(self, n_sites, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_loglik=0, d_pref=0, d_status=0, stream=0):
        """The evidence on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("evidence", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_loglik, d_pref, d_status, stream)

    def evidence_prior_batch_device(self, n_sites, d_prior, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_loglik=0, d_pref=0, d_status=0,
                                    stream=0):
        """evidence_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("evidence", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_loglik, d_pref, d_status, stream)

    def loo_batch(self, lk=None, pl16=None, seq_members=None, flags=None, want_loo=True, want_fit=True):
        """Leave-one-out posteriors and per-member fit: -> (loo[S,N,3] float64, fit[S,N] float64, status[S] uint8).
        loo[s, i] is member i's genotype distribution given the likelihood rows of every member but i (for a member whose row
        is all ones, its posterior); fit[s, i] = sum_a loo[s, i, a] * lk[s, i, a], the predictive likelihood of i's row given
        its relatives, linear and in the row's own units (0.0: the row is impossible given the relatives).  Both NaN where
        status != 0.  Input as map_batch: either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16 in VCF column order
        (seq_members: their PED indices).  want_loo / want_fit False: that output is not computed and returned as None."""
        outs = lambda s: (np.empty((s, self.n, 3)) if want_loo else None, np.empty((s, self.n)) if want_fit else None)
        return self._side_host("loo", None, lk, pl16, seq_members, flags, outs)

    def loo_prior_batch(self, prior, lk=None, pl16=None, seq_members=None, flags=None, want_loo=True, want_fit=True):
        """loo_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give loo_batch's bits."""
        outs = lambda s: (np.empty((s, self.n, 3)) if want_loo else None, np.empty((s, self.n)) if want_fit else None)
        return self._side_host("loo", prior, lk, pl16, seq_members, flags, outs)

    def loo_batch_device(self, n_sites, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_loo=0, d_fit=0, d_status=0, stream=0):
        """Leave-one-out posteriors and fit on resident buffers (raw device pointers as ints; 0 = not given); enqueues on
        `stream` and returns."""
        self._side_device("loo", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_loo, d_fit, d_status, stream)

    @staticmethod
    def _masks(masks, n):
        """masks [M, N] (or one row [N]) as a contiguous uint8 array."""
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.ndim == 1:
            m = m[None, :]
        if m.ndim != 2 or m.shape[1] != n:
            raise ValueError("masks must have shape [n_patterns, %d]" % n)
        return m

    def pattern_batch(self, masks, lk=None, pl16=None, seq_members=None, flags=None, want_post=True, want_loglik=True):
        """Genotype-pattern posteriors: -> (pat_post[S,M] float64, loglik[S] float64, status[S] uint8).
        masks [M, N] uint8 (PED order): bit g of masks[m, i] set = pattern m allows member i genotype g (7: unconstrained).
        pat_post[s, m] = P(every member's genotype is allowed by pattern m | data) in the full network; loglik is
        evidence_batch's.  segregation_masks() makes the dominant and recessive rows.  Input is either lk [S,N,3] float64 or
        pl16 [S,n_seq,3] uint16 in VCF column order (seq_members: their PED indices).  want_* False: not computed, None."""
        m = self._masks(masks, self.n)
        outs = lambda s: (np.empty((s, m.shape[0])) if want_post else None, np.empty(s) if want_loglik else None)
        return self._side_host("pattern", None, lk, pl16, seq_members, flags, outs, (_p(m, C.c_uint8), m.shape[0]))

    def pattern_prior_batch(self, prior, masks, lk=None, pl16=None, seq_members=None, flags=None, want_post=True, want_loglik=True):
        """pattern_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give pattern_batch's bits."""
        m = self._masks(masks, self.n)
        outs = lambda s: (np.empty((s, m.shape[0])) if want_post else None, np.empty(s) if want_loglik else None)
        return self._side_host("pattern", prior, lk, pl16, seq_members, flags, outs, (_p(m, C.c_uint8), m.shape[0]))

    def _draw_args(self, n_draws, seed, site_base):
        return (int(seed) & 0xFFFFFFFFFFFFFFFF, int(site_base), int(n_draws))

    def _draw_outs(self, n_draws, want_gt, want_post):
        k = max(int(n_draws), 0)  # (what the library refuses must reach it: no array is made too small)
        return lambda s: (np.empty((s, k, self.n), np.int8) if want_gt else None, np.empty((s, k)) if want_post else None)

    def sample_batch(self, n_draws, seed=0, site_base=0, lk=None, pl16=None, seq_members=None, flags=None, want_gt=True, want_post=True):
        """Exact joint posterior draws: -> (gt[S,K,N] int8, post[S,K] float64, status[S] uint8), K = n_draws (1 .. 256).
        gt[s, k] is a genotype configuration of the whole pedigree (PED order) drawn with probability w(g) / Z, post[s, k] that
        probability; -1 / NaN where status != 0.  Distinct (site, draw) pairs are independent.  A draw depends on the pedigree, the
        site's rows, seed, the site's absolute index site_base + s and k only: a batch cut into parts, each sampled with its
        first site's index as site_base, gives the rows of the whole batch.  Input as map_batch."""
        return self._side_host("sample", None, lk, pl16, seq_members, flags, self._draw_outs(n_draws, want_gt, want_post),
                               self._draw_args(n_draws, seed, site_base))

    def sample_prior_batch(self, prior, n_draws, seed=0, site_base=0, lk=None, pl16=None, seq_members=None, flags=None, want_gt=True,
                           want_post=True):
        """sample_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give sample_batch's bits."""
        return self._side_host("sample", prior, lk, pl16, seq_members, flags, self._draw_outs(n_draws, want_gt, want_post),
                               self._draw_args(n_draws, seed, site_base))

    def sample_batch_device(self, n_sites, n_draws, seed=0, site_base=0, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_samp_gt=0,
                            d_samp_post=0, d_status=0, stream=0):
        """sample_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("sample", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_samp_gt, d_samp_post, d_status, stream,
                          self._draw_args(n_draws, seed, site_base))

    def sample_prior_batch_device(self, n_sites, d_prior, n_draws, seed=0, site_base=0, d_lk=0, d_pl16=0, seq_members=(), d_flags=0,
                                  d_samp_gt=0, d_samp_post=0, d_status=0, stream=0):
        """sample_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("sample", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_samp_gt, d_samp_post, d_status, stream,
                          self._draw_args(n_draws, seed, site_base))

    def pattern_batch_device(self, n_sites, d_masks, n_patterns, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_pat_post=0, d_loglik=0,
                             d_status=0, stream=0):
        """pattern_batch on resident buffers (raw device pointers as ints; 0 = not given), d_masks [n_patterns, N] uint8 among
        them; enqueues on `stream` and returns."""
        self._side_device("pattern", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_pat_post, d_loglik, d_status, stream,
                          (d_masks or None, int(n_patterns)))

    def pattern_prior_batch_device(self, n_sites, d_prior, d_masks, n_patterns, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_pat_post=0,
                                   d_loglik=0, d_status=0, stream=0):
        """pattern_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("pattern", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_pat_post, d_loglik, d_status, stream,
                          (d_masks or None, int(n_patterns)))

    @staticmethod
    def _assign(assign, n):
        """assign [M, N] (or one row [N]) as a contiguous int32 array."""
        a = np.ascontiguousarray(assign, dtype=np.int32)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != n:
            raise ValueError("assign must have shape [n_assign, %d]" % n)
        return a

    def relabel_batch(self, assign, lk=None, pl16=None, seq_members=None, flags=None, want_alt=True, want_loglik=True):
        """Relabelling evidence: -> (alt_loglik[S,M] float64, loglik[S] float64, status[S] uint8).
        assign [M, N] int32 (PED order): assign[m, p] is the member whose likelihood row member p is given under hypothesis m,
        -1 for no data (the row (1, 1, 1)); a row need not be a permutation.  alt_loglik[s, m] = log10 of the site's likelihood
        under the pedigree with the rows so assigned (evidence_batch's bits on the rows rearranged; -inf where it is exactly 0);
        loglik is evidence_batch's.  alt_loglik - loglik summed over sites is the log10 Bayes factor of the relabelling.
        swap_assignments() makes the rows of every transposition.  Input is either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16
        in VCF column order (seq_members: their PED indices).  want_* False: not computed, None."""
        a = self._assign(assign, self.n)
        outs = lambda s: (np.empty((s, a.shape[0])) if want_alt else None, np.empty(s) if want_loglik else None)
        return self._side_host("relabel", None, lk, pl16, seq_members, flags, outs, (_p(a, C.c_int32), a.shape[0]))

    def relabel_prior_batch(self, prior, assign, lk=None, pl16=None, seq_members=None, flags=None, want_alt=True, want_loglik=True):
        """relabel_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give relabel_batch's bits."""
        a = self._assign(assign, self.n)
        outs = lambda s: (np.empty((s, a.shape[0])) if want_alt else None, np.empty(s) if want_loglik else None)
        return self._side_host("relabel", prior, lk, pl16, seq_members, flags, outs, (_p(a, C.c_int32), a.shape[0]))

    def relabel_device(self, n_sites, d_assign, n_assign, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_alt=0, d_loglik=0,
                             d_status=0, stream=0):
        """relabel_batch on resident buffers (raw device pointers as ints; 0 = not given), d_assign [n_assign, N] int32 among
        them (an entry outside 0 .. N-1 is taken as -1); enqueues on `stream` and returns."""
        self._side_device("relabel", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_alt, d_loglik, d_status, stream,
                          (d_assign or None, int(n_assign)))

    def relabel_prior_device(self, n_sites, d_prior, d_assign, n_assign, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_alt=0,
                                   d_loglik=0, d_status=0, stream=0):
        """relabel_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("relabel", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_alt, d_loglik, d_status, stream,
                          (d_assign or None, int(n_assign)))

    @staticmethod
    def _rates(rates):
        """rates (a scalar or [R]) as a contiguous float64 array."""
        r = np.ascontiguousarray(rates, dtype=np.float64)
        if r.ndim == 0:
            r = r[None]
        if r.ndim != 1:
            raise ValueError("rates must be a list of mutation rates")
        return r

    def rate_tables(self, rates):
        """The factor tables of `rates` for mutrate_device: -> [R, 432] float64, block r this context's own table with the
        transmission tables of rates[r] (bit for bit the table of a context made with mrate = rates[r]).  Needs no device."""
        r = self._rates(rates)
        tables = np.empty((len(r), RATE_TABLE_DOUBLES))
        self._check(lib().famseq_rate_tables(self._h, _p(r, C.c_double), len(r), _p(tables, C.c_double)), "famseq_rate_tables")
        return tables

    def mutrate_batch(self, rates, lk=None, pl16=None, seq_members=None, flags=None, want_rates=True, want_loglik=True):
        """The mutation-rate likelihood profile: -> (rate_loglik[S,R] float64, loglik[S] float64, status[S] uint8).
        rates [R] (1 .. MAX_RATES numbers in [0, 1]).  rate_loglik[s, r] = log10 of the site's likelihood under the pedigree with
        the mutation rate rates[r] (evidence_batch's bits on a context made with that mrate; -inf where it is exactly 0, as at
        rate 0 on a Mendel-impossible site); loglik is evidence_batch's under this context's own rate.  Summed over sites a column
        is the log10 likelihood of its rate; rate_loglik[:, r] - rate_loglik[:, r0] with rates[r0] = 0 is the log10 Bayes factor
        "the site needs a mutation".  Input is either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16 in VCF column order
        (seq_members: their PED indices).  want_* False: not computed, None."""
        r = self._rates(rates)
        outs = lambda s: (np.empty((s, len(r))) if want_rates else None, np.empty(s) if want_loglik else None)
        return self._side_host("mutrate", None, lk, pl16, seq_members, flags, outs, (_p(r, C.c_double), len(r)))

    def mutrate_prior_batch(self, prior, rates, lk=None, pl16=None, seq_members=None, flags=None, want_rates=True, want_loglik=True):
        """mutrate_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give mutrate_batch's bits."""
        r = self._rates(rates)
        outs = lambda s: (np.empty((s, len(r))) if want_rates else None, np.empty(s) if want_loglik else None)
        return self._side_host("mutrate", prior, lk, pl16, seq_members, flags, outs, (_p(r, C.c_double), len(r)))

    def mutrate_device(self, n_sites, d_tables, n_rates, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_rate_loglik=0, d_loglik=0,
                       d_status=0, stream=0):
        """mutrate_batch on resident buffers (raw device pointers as ints; 0 = not given), d_tables [n_rates, 432] float64 among
        them (rate_tables() makes them; they must stay unchanged until the kernel has run); enqueues on `stream` and returns."""
        self._side_device("mutrate", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_rate_loglik, d_loglik, d_status, stream,
                          (d_tables or None, int(n_rates)))

    def mutrate_prior_device(self, n_sites, d_prior, d_tables, n_rates, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_rate_loglik=0,
                             d_loglik=0, d_status=0, stream=0):
        """mutrate_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("mutrate", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_rate_loglik, d_loglik, d_status, stream,
                          (d_tables or None, int(n_rates)))

    def _weights(self, weights):
        """weights ([N, 3] or [M, N, 3]) as a contiguous float64 array [M, N, 3]."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1:] != (self.n, 3):
            raise ValueError("weights must be [M, %d, 3] (or one table [%d, 3]), got %s" % (self.n, self.n, list(w.shape)))
        return w

    def weight_batch(self, weights, lk=None, pl16=None, seq_members=None, flags=None, want_wt=True, want_loglik=True):
        """Per-member genotype weights: -> (wt_loglik[S,M] float64, loglik[S] float64, status[S] uint8).
        weights [M, N, 3] (1 .. MAX_WEIGHTS tables; a single [N, 3] table is accepted; finite numbers >= 0, above 1 included):
        wt_loglik[s, m] = log10 Z(lk * weights[m]), evidence_batch's bits on the rows lk[s] * weights[m] formed in double (-inf
        where that is exactly 0); loglik is evidence_batch's on the rows as they are.  wt_loglik[:, m] - loglik is
        log10 E[prod_p w_p(g_p) | data] under the exact joint posterior: with penetrance_weights() the phenotypes' probability
        given the reads, with w = t ** count a moment generating function.  Every member has a row of weights, sequenced or not.
        Input is either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16 in VCF column order (seq_members: their PED indices).
        want_* False: not computed, None."""
        w = self._weights(weights)
        outs = lambda s: (np.empty((s, w.shape[0])) if want_wt else None, np.empty(s) if want_loglik else None)
        return self._side_host("weight", None, lk, pl16, seq_members, flags, outs, (_p(w, C.c_double), w.shape[0]))

    def weight_prior_batch(self, prior, weights, lk=None, pl16=None, seq_members=None, flags=None, want_wt=True, want_loglik=True):
        """weight_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give weight_batch's bits."""
        w = self._weights(weights)
        outs = lambda s: (np.empty((s, w.shape[0])) if want_wt else None, np.empty(s) if want_loglik else None)
        return self._side_host("weight", prior, lk, pl16, seq_members, flags, outs, (_p(w, C.c_double), w.shape[0]))

    def weight_device(self, n_sites, d_weights, n_weights, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_wt_loglik=0, d_loglik=0,
                      d_status=0, stream=0):
        """weight_batch on resident buffers (raw device pointers as ints; 0 = not given), d_weights [n_weights, N, 3] float64
        among them (unchecked; it must stay unchanged until the kernel has run); enqueues on `stream` and returns."""
        self._side_device("weight", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_wt_loglik, d_loglik, d_status, stream,
                          (d_weights or None, int(n_weights)))

    def weight_prior_device(self, n_sites, d_prior, d_weights, n_weights, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_wt_loglik=0,
                            d_loglik=0, d_status=0, stream=0):
        """weight_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("weight", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_wt_loglik, d_loglik, d_status, stream,
                          (d_weights or None, int(n_weights)))

    def _cweights(self, cweights):
        """cweights (complex [N, 3] / [M, N, 3], or real [M, N, 3, 2]) as a contiguous float64 array [M, N, 3, 2]."""
        w = np.asarray(cweights)
        if np.iscomplexobj(w):
            w = np.ascontiguousarray(w, dtype=np.complex128)
            if w.ndim == 2:
                w = w[None]
            w = w.view(np.float64).reshape(w.shape + (2,))
        else:
            w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim != 4 or w.shape[1:] != (self.n, 3, 2):
            raise ValueError("cweights must be complex [M, %d, 3] (or real [M, %d, 3, 2]), got %s" % (self.n, self.n, list(np.shape(cweights))))
        return w

    def charfn_batch(self, cweights, lk=None, pl16=None, seq_members=None, flags=None, want_cf=True, want_loglik=True):
        """Complex per-member weights: -> (cf[S,M] complex128, loglik[S] float64, status[S] uint8).
        cweights complex [M, N, 3] (1 .. MAX_CWEIGHTS tables; a single [N, 3] table, or real [M, N, 3, 2] = (re, im), is
        accepted; finite): cf[s, m] = E[prod_p w_m[p][g_p] | data] = Z(lk * w_m) / Z(lk) under the exact joint posterior, to
        1e-12 ABSOLUTE times Z(lk * |w_m|) / Z(lk) (1 for unit-modulus weights); loglik is evidence_batch's.  With
        count_tables() the characteristic function of a count, which count_from_cf() turns into its distribution
        (count_batch does both).  Input is either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16 in VCF column order
        (seq_members: their PED indices).  want_* False: not computed, None."""
        return self._charfn(None, cweights, lk, pl16, seq_members, flags, want_cf, want_loglik)

    def charfn_prior_batch(self, prior, cweights, lk=None, pl16=None, seq_members=None, flags=None, want_cf=True, want_loglik=True):
        """charfn_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give charfn_batch's bits."""
        return self._charfn(prior, cweights, lk, pl16, seq_members, flags, want_cf, want_loglik)

    def _charfn(self, prior, cweights, lk, pl16, seq_members, flags, want_cf, want_loglik):
        w = self._cweights(cweights)
        outs = lambda s: (np.empty((s, w.shape[0], 2)) if want_cf else None, np.empty(s) if want_loglik else None)
        cf, ll, st = self._side_host("charfn", prior, lk, pl16, seq_members, flags, outs, (_p(w, C.c_double), w.shape[0]))
        return (None if cf is None else cf.view(np.complex128)[..., 0]), ll, st

    def charfn_device(self, n_sites, d_cweights, n_tables, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_cf=0, d_loglik=0, d_status=0,
                      stream=0):
        """charfn_batch on resident buffers (raw device pointers as ints; 0 = not given), d_cweights [n_tables, N, 3, 2] float64
        among them (unchecked; it must stay unchanged until the kernel has run), d_cf [n_sites, n_tables, 2]; enqueues on
        `stream` and returns."""
        self._side_device("charfn", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_cf, d_loglik, d_status, stream,
                          (d_cweights or None, int(n_tables)))

    def charfn_prior_device(self, n_sites, d_prior, d_cweights, n_tables, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_cf=0,
                            d_loglik=0, d_status=0, stream=0):
        """charfn_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("charfn", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_cf, d_loglik, d_status, stream,
                          (d_cweights or None, int(n_tables)))

    def count_batch(self, scores, lk=None, pl16=None, seq_members=None, flags=None, prior=None):
        """The exact posterior distribution of the count sum_p scores[p][g_p] (count_scores()): -> (dist[S, D + 1] float64,
        loglik[S], status[S]), dist[s, k] = P(count = k | data), each to 1e-12 absolute (count_from_cf's rules: not
        renormalised, NaN where status != 0).  One charfn_batch call (prior [S, 6] given: charfn_prior_batch) at the
        D // 2 + 1 frequencies of count_tables(scores) and an inverse DFT on the host."""
        tables, D = count_tables(scores)
        cf, ll, st = self._charfn(prior, tables, lk, pl16, seq_members, flags, True, True)
        return count_from_cf(cf, D), ll, st

    def allele_tables(self):
        """The allele-level transmission rows origin_batch uses: -> [2 chrX, 2 child sex (0 son, 1 daughter), 2 parent (0 mother,
        1 father), 2 allele, 3 parent's genotype] float64, for the mutation rate the model's tables were made with (plan()
        ["origin_mrate"]).  FamseqError for a model with custom transmission tables.  Needs no device."""
        t = np.empty((2, 2, 2, 2, 3))
        self._check(lib().famseq_allele_tables(self._h, _p(t, C.c_double)), "famseq_allele_tables")
        return t

    def _origin(self, prior, lk, pl16, seq_members, flags, want_origin, want_hettx):
        k = len(self.trio_children()) if (lk is None) != (pl16 is None) else 0  # (else _inputs says what is wrong)
        outs = lambda s: (np.empty((s, k, 4)) if want_origin else None, np.empty((s, k, 4)) if want_hettx else None)
        return self._side_host("origin", prior, lk, pl16, seq_members, flags, outs)

    def origin_batch(self, lk=None, pl16=None, seq_members=None, flags=None, want_origin=True, want_hettx=True):
        """Phase by transmission: -> (origin[S,K,4] float64, hettx[S,K,4] float64, status[S] uint8), child k being member
        trio_children()[k].  origin[s, k, 2 a + b] is the posterior that the child received allele a (0 ref, 1 alt) from its
        mother and b from its father, given everybody's data (a row sums to 1; a son at a chrX site has no paternal allele:
        entries 1 and 3 are 0).  hettx[s, k] = (P(g_m = 1, a = 1), P(g_m = 1, a = 0), P(g_f = 1, b = 1), P(g_f = 1, b = 0)): the
        expected transmissions from heterozygous parents, what a transmission test sums over families.  Both NaN where status
        != 0.  Input as evidence_batch: either lk [S,N,3] float64 or pl16 [S,n_seq,3] uint16 in VCF column order (seq_members:
        their PED indices).  want_* False: not computed, None.  phased_calls(origin) makes the a|b call."""
        return self._origin(None, lk, pl16, seq_members, flags, want_origin, want_hettx)

    def origin_prior_batch(self, prior, lk=None, pl16=None, seq_members=None, flags=None, want_origin=True, want_hettx=True):
        """origin_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give origin_batch's bits."""
        return self._origin(prior, lk, pl16, seq_members, flags, want_origin, want_hettx)

    def origin_device(self, n_sites, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_origin=0, d_hettx=0, d_status=0, stream=0):
        """origin_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("origin", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_origin, d_hettx, d_status, stream)

    def origin_prior_device(self, n_sites, d_prior, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_origin=0, d_hettx=0, d_status=0,
                            stream=0):
        """origin_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("origin", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_origin, d_hettx, d_status, stream)

    def af_batch(self, af0, n_iter, lk=None, pl16=None, seq_members=None, flags=None, want_af=True, want_loglik=True):
        """The founders' allele frequency by maximum likelihood: -> (af[S] float64, loglik[S,2] float64, status[S] uint8).
        n_iter (0 .. 64) EM steps from af0 ([S], or a scalar for every site; each in [0, 1]) on the allele frequency q of the
        founders' Hardy-Weinberg prior, hwe_priors' rows: af[s] is q after the steps (n_iter = 0: af0's bits), loglik[s, 0] the
        site's log10 likelihood at that q on evidence_batch's scale, loglik[s, 1] the same at q = 0 (-inf where the data exclude
        it); their difference is the log10 likelihood ratio for "the allele is present among the founders".  All NaN where
        status != 0 (1: the single-posterior rule under af0's rows; 2: a total weight or a founder's row sum that is not a
        positive finite number).  No early exit: n_iter = a, then n_iter = b from the returned af, gives the bits of one call
        with n_iter = a + b.  Of the flags only FLAG_CHRX is read.  Input as evidence_batch.  want_* False: not computed, None."""
        n = np.asarray(lk).size // (3 * self.n) if lk is not None else (len(pl16) if pl16 is not None else 0)
        q = np.ascontiguousarray(np.full(n, af0) if np.ndim(af0) == 0 else af0, dtype=np.float64)
        if q.shape != (n,):
            raise ValueError("af0 must be a scalar or have one value per site")
        outs = lambda s: (np.empty(s) if want_af else None, np.empty((s, 2)) if want_loglik else None)
        return self._side_host("af", None, lk, pl16, seq_members, flags, outs, (_p(q, C.c_double), int(n_iter)))

    def af_batch_device(self, n_sites, d_af0, n_iter, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_af=0, d_loglik=0, d_status=0, stream=0):
        """af_batch on resident buffers (raw device pointers as ints; 0 = not given), d_af0 [n_sites] float64 among them;
        enqueues on `stream` and returns."""
        self._side_device("af", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_af, d_loglik, d_status, stream,
                          (d_af0 or None, int(n_iter)))

    def maxmarg_batch(self, lk=None, pl16=None, seq_members=None, flags=None, want_maxmarg=True, want_top=True):
        """Max-marginals and the runner-up of the joint MAP call: -> (maxmarg[S,N,3] float64, top[S,2] float64, status[S] uint8).
        maxmarg[s, p, a] is the posterior of the best configuration in which member p has genotype a (exactly 0.0 where none
        has positive weight); top[s] = (map_batch's map_post, bit for bit; the second-largest configuration's posterior).
        Status as for map_batch; failed sites are NaN.  joint_call_quality() makes the per-member call and its quality of
        maxmarg.  Inputs as for map_batch.  want_maxmarg / want_top False: that output is not computed and returned as None."""
        outs = lambda s: (np.empty((s, self.n, 3)) if want_maxmarg else None, np.empty((s, 2)) if want_top else None)
        return self._side_host("maxmarg", None, lk, pl16, seq_members, flags, outs)

    def maxmarg_prior_batch(self, prior, lk=None, pl16=None, seq_members=None, flags=None, want_maxmarg=True, want_top=True):
        """maxmarg_batch with the founders' genotype prior given per site (prior [S, 6] as for bn_prior_batch; of the flags only
        FLAG_CHRX is read).  Rows equal to the model's constants give maxmarg_batch's bits."""
        outs = lambda s: (np.empty((s, self.n, 3)) if want_maxmarg else None, np.empty((s, 2)) if want_top else None)
        return self._side_host("maxmarg", prior, lk, pl16, seq_members, flags, outs)

    def maxmarg_device(self, n_sites, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_maxmarg=0, d_top=0, d_status=0, stream=0):
        """maxmarg_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("maxmarg", n_sites, d_lk, d_pl16, seq_members, d_flags, None, d_maxmarg, d_top, d_status, stream)

    def maxmarg_prior_device(self, n_sites, d_prior, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_maxmarg=0, d_top=0, d_status=0,
                                   stream=0):
        """maxmarg_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("maxmarg", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_maxmarg, d_top, d_status, stream)

    def loo_prior_batch_device(self, n_sites, d_prior, d_lk=0, d_pl16=0, seq_members=(), d_flags=0, d_loo=0, d_fit=0, d_status=0, stream=0):
        """loo_prior_batch on resident buffers (raw device pointers as ints; 0 = not given); enqueues on `stream` and returns."""
        self._side_device("loo", n_sites, d_lk, d_pl16, seq_members, d_flags, d_prior or 0, d_loo, d_fit, d_status, stream)

    def g6_probe(self, values):
        """The device formatter alone (famseq_format_probe): -> list of bytes, one per value."""
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        out = np.zeros((len(v), 16), np.uint8)
        self._check(lib().famseq_format_probe(self._h, len(v), _p(v, C.c_double), out.ctypes.data_as(C.c_char_p)), "famseq_format_probe")
        return [bytes(r[:r[15]]) for r in out]

    def bn_batch_device(self, n_sites, d_lk, d_flags, d_post, d_single=0, d_status=0, stream=0):
        """Raw device pointers (ints); enqueues on `stream` and returns."""
        rc = lib().famseq_bn_batch_device(self._h, int(n_sites), d_lk, d_flags or None, d_post, d_single or None,
                                          d_status or None, stream or None)
        self._check(rc, "famseq_bn_batch_device")


def stream_probe(ctx, n_doubles, d_in, d_out1, d_out2, stream=0):
    """famseq_stream_probe: the kernels' traffic shape as a bare elementwise kernel (diagnostic)."""
    ctx._check(lib().famseq_stream_probe(ctx._h, int(n_doubles), d_in, d_out1, d_out2, stream or None), "famseq_stream_probe")


def bn_batch_sharded(contexts, lk, flags=None):
    """famseq_bn_batch over several contexts (one per GPU) from this process: contiguous site ranges,
    one host thread per context.  -> (post, single, status)."""
    n = contexts[0].n
    lk = np.ascontiguousarray(lk, dtype=np.float64).reshape(-1, n, 3)
    s = lk.shape[0]
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    post, single, status = np.empty_like(lk), np.empty_like(lk), np.zeros(s, np.uint8)
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = lib().famseq_bn_batch_sharded(arr, len(contexts), s, _p(lk, C.c_double), None if fl is None else _p(fl, C.c_uint8),
                                       _p(post, C.c_double), _p(single, C.c_double), _p(status, C.c_uint8))
    if rc != 0:
        msgs = [lib().famseq_last_error(c._h).decode() for c in contexts]
        raise FamseqError("famseq_bn_batch_sharded failed (%d): %s" % (rc, "; ".join(m for m in msgs if m)))
    return post, single, status


def bn_batch_device_sharded(contexts, n_sites, d_lk, d_flags, d_post, d_single=None, d_status=None):
    """famseq_bn_batch_device_sharded: shard g = n_sites[g] sites resident on contexts[g]'s device, given as
    raw device pointers (ints; 0 / None = absent).  Blocking; one host thread per context."""
    g = len(contexts)

    def ptrs(v):
        if v is None:
            return None
        return (C.c_void_p * g)(*[(x or None) for x in v])

    arr = (C.c_void_p * g)(*[c._h for c in contexts])
    ns = (C.c_int64 * g)(*[int(x) for x in n_sites])
    rc = lib().famseq_bn_batch_device_sharded(arr, g, ns, ptrs(d_lk), ptrs(d_flags), ptrs(d_post), ptrs(d_single),
                                              ptrs(d_status))
    if rc != 0:
        msgs = [lib().famseq_last_error(c._h).decode() for c in contexts]
        raise FamseqError("famseq_bn_batch_device_sharded failed (%d): %s" % (rc, "; ".join(m for m in msgs if m)))


def phased_calls(origin):
    """The phased call of origin_batch's rows: origin [..., 4] -> (index [...] int8, probability [...] float64), index = 2 a + b
    of the largest entry (a the maternal, b the paternal allele; the lowest index among equals), probability that entry; -1 and
    NaN for a NaN row."""
    o = np.asarray(origin, dtype=np.float64)
    bad = np.isnan(o).any(axis=-1)
    idx = np.argmax(np.where(bad[..., None], 0.0, o), axis=-1)  # (np.argmax: the first of equals)
    prob = np.take_along_axis(o, idx[..., None], axis=-1)[..., 0]
    return np.where(bad, -1, idx).astype(np.int8), np.where(bad, np.nan, prob)


def joint_call_quality(maxmarg):
    """The per-member joint call of maxmarg_batch's rows and its quality: maxmarg [..., 3] -> (jgt [...] int8, jgq [...] float64).
    jgt is the row's largest entry (the lowest genotype among equals); jgq = -10 log10(second largest of the row / largest), the
    Phred-scaled ratio between the best configuration and the best one in which the member is called differently: +inf where
    the second largest is 0, 0 under an exact tie.  -1 and NaN for a NaN row."""
    m = np.asarray(maxmarg, dtype=np.float64)
    bad = np.isnan(m).any(axis=-1)
    rows = np.where(bad[..., None], 1.0, m)
    jgt = np.argmax(rows, axis=-1)  # (np.argmax: the first of equals)
    ordered = np.sort(rows, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        jgq = np.abs(-10.0 * np.log10(ordered[..., 1] / ordered[..., 2]))
    jgq = np.where(ordered[..., 1] == 0, np.inf, jgq)
    return np.where(bad, -1, jgt).astype(np.int8), np.where(bad, np.nan, jgq)


def call_genotypes(post):
    post = np.ascontiguousarray(post, dtype=np.float64).reshape(-1, 3)
    out = np.empty(post.shape[0], np.int8)
    lib().famseq_call_genotypes(_p(post, C.c_double), post.shape[0], _p(out, C.c_int8))
    return out


class Family:
    """Batched mirror of the reference's `family` for the BN path.

    ref = family(mem, mRate); ref.set_lc(lc); ref.init(); ref.set_mapV2P(...)
    then per site set_LK(lk) / calPostProbBN(Known, chrType) / get_postProb() ...
    Here set_LK takes [S,N,3] (PED order) and calPostProbBN takes per-site arrays."""

    def __init__(self, ped: Pedigree, mrate=1e-7, lc=1.0, device=0, **priors):
        self.ped = ped
        self.model = make_model(ped, mrate, lc, **priors)
        self.ctx = Context(self.model, device)
        self._seq_idx = np.nonzero(ped.sequenced)[0]
        self._lk = None
        self._post = self._single = self._status = None

    def get_numInd(self):
        return self.ped.n

    def get_realNumInd(self):
        return len(self._seq_idx)

    def set_mapV2P(self, v2p):
        """VCF column -> PED index (or -1); fixes the order of the get_* rows (family.cpp:364-376)."""
        self._seq_idx = np.array([p for p in v2p if p >= 0], dtype=np.int64)

    def set_LK(self, lk):
        lk = np.asarray(lk, dtype=np.float64)
        if lk.ndim == 2:
            lk = lk[None]
        if lk.shape[1:] != (self.ped.n, 3):
            print("The dimention of likelihood matrix is wrong. Cannot set likelihood.")
            return False
        self._lk = lk
        self._post = self._single = self._status = None
        return True

    def calPostProbBN(self, Known=False, chrType=0):
        """-> bool array per site (True where the reference would return true)."""
        if self._lk is None:
            print("Likelihood has not been set. Please set likelihood first.")
            return False
        s = self._lk.shape[0]
        flags = (np.broadcast_to(np.asarray(Known, dtype=bool), (s,)).astype(np.uint8) * FLAG_KNOWN
                 | np.broadcast_to(np.asarray(chrType) == 1, (s,)).astype(np.uint8) * FLAG_CHRX)
        self._post, self._single, self._status = self.ctx.bn_batch(self._lk, flags)
        return (self._status & 3) == 0

    def get_status(self):
        return self._status

    def get_postProb(self, flag=True):
        return self._post[:, self._seq_idx, :] if flag else self._post

    def get_postProbSingle(self, flag=True):
        return self._single[:, self._seq_idx, :] if flag else self._single

    def get_postRlt(self):
        p = self.get_postProb(True)
        return call_genotypes(p).reshape(p.shape[0], p.shape[1])
