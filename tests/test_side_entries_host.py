"""The argument checks of the twelve side-product entries (trio, MAP, evidence; plain and site-prior; host and device buffers) and
of their prebuild options, on plan-only contexts: what a caller can observe without a GPU.  Every entry is called through
fs.lib() directly; return codes and famseq_last_error texts are literals.

Two pedigrees: the trio, and four disjoint sib matings (`loops4` of tools/plan_dump.py, whose `refused` entries in
profiles/side_table/plan_dump_*.json are the engine's refusals quoted below).  On a context without a device no entry gets as
far as loading a kernel, so both pedigrees answer the entries alike; the options tell them apart.

The order pinned, first complaint wins: a site-prior device entry asks for d_prior before anything else; then exactly one of
lk / pl16 (a negative site count says the same); then the device.  A site-prior host entry asks for its prior rows only after
the device, so without one its "prior must be given" cannot be seen: the missing device is what it says (the GPU suite sees
the other).  With no sites there is nothing to complain about before the device."""
import ctypes as C

import numpy as np
import pytest

import famseq_amd as fs
from test_gpu_denovo import four_loops

E_ARG, E_NODEVICE = -1, -2
ONE_OF = b"exactly one of lk / pl16 must be given"
D_PRIOR = b"d_prior must be given (six doubles per site)"
NO_DEVICE = b"context was created without a device; there is no CPU path"
REFUSAL = "the pedigree's loops need more than three conditioning members; use the enumeration engine"
TAKES = {"trio_kernels": "trio_kernels takes 1 (dnm), 2 (joint) or 3 (both)",
         "trio_prior_kernels": "trio_prior_kernels takes 1 (dnm), 2 (joint) or 3 (both)",
         "map_kernels": "map_kernels takes 1", "map_prior_kernels": "map_prior_kernels takes 1",
         "evidence_kernels": "evidence_kernels takes 1", "evidence_prior_kernels": "evidence_prior_kernels takes 1"}
REFUSED = {"trio_kernels": "trio posteriors (sum-product engine): " + REFUSAL,
           "trio_prior_kernels": "site priors, trio posteriors (sum-product engine): " + REFUSAL,
           "map_kernels": "joint MAP call (sum-product engine): " + REFUSAL,
           "map_prior_kernels": "site priors, joint MAP call (sum-product engine): " + REFUSAL,
           "evidence_kernels": "site evidence (sum-product engine): " + REFUSAL,
           "evidence_prior_kernels": "site priors, site evidence (sum-product engine): " + REFUSAL}

ENTRIES = [(name, prior, device) for name in ("trio", "map", "evidence") for prior in (False, True) for device in (False, True)]
PEDS = {"trio": lambda: fs.synthetic_pedigree("trio"), "loops4": four_loops}


@pytest.fixture(scope="module", params=sorted(PEDS))
def ctx(request):
    c = fs.Context(fs.make_model(PEDS[request.param]()), device=-1)
    yield c
    c.close()


def call(ctx, entry, n_sites=1, lk=True, pl16=False, prior=True):
    """-> (return code, famseq_last_error) of one entry on arrays for one site; lk / pl16 / prior False: that pointer NULL."""
    name, site_prior, device = entry
    fn = getattr(fs.lib(), "famseq_%s%s_batch%s" % (name, "_prior" if site_prior else "", "_device" if device else ""))
    n = ctx.n
    args = [np.ones((1, n, 3)) if lk else None, np.zeros((1, n, 3), np.uint16) if pl16 else None, np.arange(n, dtype=np.int32), n,
            np.zeros(1, np.uint8)]
    if site_prior:
        args.append(np.full((1, 6), 0.25) if prior else None)
    args += [np.zeros((1, n), np.int8) if name == "map" else np.zeros(27 * n), np.zeros(n), np.zeros(1, np.uint8)]
    args = [ctx._h, n_sites] + args + ([None] if device else [])
    assert len(args) == len(fn.argtypes)
    keep = [a for a in args if isinstance(a, np.ndarray)]  # (alive over the call)
    rc = fn(*[a.ctypes.data_as(t) if isinstance(a, np.ndarray) else a for a, t in zip(args, fn.argtypes)])
    del keep
    return rc, fs.lib().famseq_last_error(ctx._h)


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: "%s%s%s" % (e[0], "_prior" if e[1] else "", "_device" if e[2] else ""))
def test_argument_checks_in_their_order(ctx, entry):
    _, site_prior, device = entry
    first = D_PRIOR if device else ONE_OF  # what a site-prior entry without a prior says when its input is wrong as well
    # neither lk nor pl16, both of them
    assert call(ctx, entry, lk=False, pl16=False) == (E_ARG, ONE_OF)
    assert call(ctx, entry, lk=True, pl16=True) == (E_ARG, ONE_OF)
    if site_prior:
        assert call(ctx, entry, lk=False, pl16=False, prior=False) == (E_ARG, first)
        assert call(ctx, entry, lk=True, pl16=True, prior=False) == (E_ARG, first)
        # no prior: a device entry says so before it asks for the device, a host entry after, lk or packed input alike
        no_prior = (E_ARG, D_PRIOR) if device else (E_NODEVICE, NO_DEVICE)
        assert call(ctx, entry, prior=False) == no_prior
        assert call(ctx, entry, lk=False, pl16=True, prior=False) == no_prior
    # no device
    assert call(ctx, entry) == (E_NODEVICE, NO_DEVICE)
    assert call(ctx, entry, lk=False, pl16=True) == (E_NODEVICE, NO_DEVICE)
    # no sites: nothing to give, the device is what is missing
    assert call(ctx, entry, n_sites=0) == (E_NODEVICE, NO_DEVICE)
    assert call(ctx, entry, n_sites=0, lk=False, pl16=False, prior=False) == (E_NODEVICE, NO_DEVICE)
    assert call(ctx, entry, n_sites=0, lk=True, pl16=True) == (E_NODEVICE, NO_DEVICE)
    # a negative site count: said as a bad input, whatever else is given or missing
    assert call(ctx, entry, n_sites=-1) == (E_ARG, ONE_OF)
    assert call(ctx, entry, n_sites=-1, lk=False, pl16=False, prior=False) == (E_ARG, ONE_OF)


def test_a_null_context_is_refused():
    for name, site_prior, device in ENTRIES:
        fn = getattr(fs.lib(), "famseq_%s%s_batch%s" % (name, "_prior" if site_prior else "", "_device" if device else ""))
        assert fn(None, 1, *[None if t is not C.c_int32 else 0 for t in fn.argtypes[2:]]) == E_ARG


def set_option(ctx, key, value):
    rc = fs.lib().famseq_set_option(ctx._h, key.encode(), value)
    return rc, fs.lib().famseq_last_error(ctx._h).decode()


@pytest.mark.parametrize("key", sorted(TAKES))
def test_prebuild_options_refuse_values_out_of_range(ctx, key):
    top = 3 if key.startswith("trio") else 1
    for value in (0, -1, top + 1):
        assert set_option(ctx, key, value) == (E_ARG, TAKES[key])
    if ctx.n == 20:  # the pedigree the engine refuses: said for every value in range, with the product's name in front
        for value in range(1, top + 1):
            assert set_option(ctx, key, value) == (E_ARG, REFUSED[key])


def test_prior_kernels_option(ctx):
    assert set_option(ctx, "prior_kernels", 0) == (E_ARG, "prior_kernels takes 1")
    if ctx.n == 20:
        assert set_option(ctx, "prior_kernels", 1) == (E_ARG, "site priors (sum-product engine): " + REFUSAL)
