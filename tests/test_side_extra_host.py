"""The argument checks of the side-product entries that tests/test_side_entries_host.py leaves out (loo, pattern, sample, af,
relabel, mutrate, origin, weight; plain and site-prior where the product has that form; host and device buffers), on plan-only
contexts of the trio: what a caller can observe without a GPU.  Every entry is called through fs.lib() directly; return codes and
famseq_last_error texts are literals.

What these entries take beside the common arguments (their "extra": a count, a table, the sampling entries' site_base; the origin
entries' demand on the model) is checked before anything else: a bad extra is what is said even when neither lk nor pl16 is given,
the prior rows are missing and the context has no device.  Within one entry the count is looked at before the table.  A host entry
checks the table's values as well and names the first bad one by its indices; a device entry cannot read its table and goes on.
With a good extra the order is the one test_side_entries_host.py pins: a site-prior device entry asks for d_prior, then exactly one
of lk / pl16 (a negative site count says the same), then the device."""
import ctypes as C

import numpy as np
import pytest

import famseq_amd as fs

E_ARG, E_NODEVICE = -1, -2
ONE_OF = b"exactly one of lk / pl16 must be given"
D_PRIOR = b"d_prior must be given (six doubles per site)"
NO_DEVICE = b"context was created without a device; there is no CPU path"
NO_ALLELE = (b"phase by transmission: there is no allele-level model for custom transmission tables (the model's pcp2, pcp2Xf and "
             b"pcp2Xm are not famseq_transmission_tables of one mutation rate)")
N, S = 3, 2  # the trio's members; the sites the arrays of a call hold

# name -> (has a site-prior form, dtype of the first output, the count's name and bounds or None, does it take a table)
PRODUCTS = {"loo": (True, np.float64, None, False), "pattern": (True, np.float64, ("n_patterns", 1, 32), True),
            "sample": (True, np.int8, ("n_draws", 1, 256), False), "af": (False, np.float64, ("n_iter", 0, 64), True),
            "relabel": (True, np.float64, ("n_assign", 1, 64), True), "mutrate": (True, np.float64, ("n_rates", 1, 32), True),
            "origin": (True, np.float64, None, False), "weight": (True, np.float64, ("n_weights", 1, 32), True)}
ENTRIES = [(name, prior, device) for name in PRODUCTS for prior in ((False, True) if PRODUCTS[name][0] else (False,))
           for device in (False, True)]
entry_id = lambda e: "%s%s%s" % (e[0], "_prior" if e[1] else "", "_device" if e[2] else "")
# what an entry says of a table that is NULL: (host, device)
NO_TABLE = {"pattern": (b"masks must be given (n_patterns rows of one byte per member)",) * 2,
            "af": (b"af0 must be given (one start value per site)",) * 2,
            "relabel": (b"assign must be given (n_assign rows of one int32 per member)",) * 2,
            "mutrate": (b"rates must be given (n_rates mutation rates)", b"d_tables must be given (n_rates factor tables of 432 doubles)"),
            "weight": (b"weights must be given (n_weights tables of three doubles per member)",
                       b"d_weights must be given (n_weights tables of three doubles per member)")}


def good_table(name, count, device):
    return {"pattern": lambda: np.full((count, N), 7, np.uint8), "af": lambda: np.full(S, 0.1),
            "relabel": lambda: np.tile(np.arange(N, dtype=np.int32), (count, 1)),
            "mutrate": lambda: np.zeros((count, 432)) if device else np.full(count, 1e-7),
            "weight": lambda: np.ones((count, N, 3)), "sample": lambda: None}[name]()


# one bad value per case: (product, label) -> (the table of a call with count 2, what a host entry says of it)
def _spoil(name, at, value):
    t = good_table(name, 2, False)
    t[at] = value
    return t


BAD_VALUES = {
    ("pattern", "mask 8"): (_spoil("pattern", (1, 2), 8), b"masks: pattern 1, member 2 is 8; a mask is 0..7 (bit g: genotype g allowed)"),
    ("relabel", "assignment N"): (_spoil("relabel", (1, 0), N),
                                  b"assign: assignment 1, member 0 is 3; an entry is -1 (no data) or a member index 0..2"),
    ("relabel", "assignment -2"): (_spoil("relabel", (0, 1), -2),
                                   b"assign: assignment 0, member 1 is -2; an entry is -1 (no data) or a member index 0..2"),
    ("mutrate", "rate 1.5"): (_spoil("mutrate", 1, 1.5), b"rates[1] must be a finite number in [0, 1]"),
    ("mutrate", "rate NaN"): (_spoil("mutrate", 0, np.nan), b"rates[0] must be a finite number in [0, 1]"),
    ("weight", "weight -1"): (_spoil("weight", (1, 2, 1), -1.0),
                              b"a weight is a finite number >= 0: weight table 1, member 2, genotype 1 is -1"),
    ("weight", "weight inf"): (_spoil("weight", (0, 1, 2), np.inf),
                               b"a weight is a finite number >= 0: weight table 0, member 1, genotype 2 is inf"),
    ("af", "af0 1.5"): (_spoil("af", 1, 1.5), b"af0 entries must be finite numbers in [0, 1] (site 1)"),
}


def trio_model(spoiled=False):
    model = fs.make_model(fs.synthetic_pedigree("trio"), mrate=1e-4)
    if spoiled:  # tables of two different rates: nobody's famseq_transmission_tables
        other = fs.make_model(fs.synthetic_pedigree("trio"), mrate=1e-5)
        for i in range(27):
            model.pcp2Xf[i] = other.pcp2Xf[i]
    return model


@pytest.fixture(scope="module")
def ctx():
    c = fs.Context(trio_model(), device=-1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def spoiled():
    c = fs.Context(trio_model(spoiled=True), device=-1)
    yield c
    c.close()


def entry_fn(entry):
    name, site_prior, device = entry
    return getattr(fs.lib(), "famseq_%s%s_batch%s" % (name, "_prior" if site_prior else "", "_device" if device else ""))


def call(ctx, entry, n_sites=S, lk=True, pl16=False, prior=True, count=2, table="good", site_base=1000):
    """-> (return code, famseq_last_error) of one entry on arrays for S sites; lk / pl16 / prior False, table None: that pointer
    NULL.  count, table, site_base: the entry's extra, where it takes one (table "good": a valid one for a count of 2)."""
    name, site_prior, device = entry
    _, out_a, counted, has_table = PRODUCTS[name]
    fn = entry_fn(entry)
    args = [np.ones((S, N, 3)) if lk else None, np.zeros((S, N, 3), np.uint16) if pl16 else None, np.arange(N, dtype=np.int32), N,
            np.zeros(S, np.uint8)]
    if site_prior:
        args.append(np.full((S, 6), 0.25) if prior else None)
    if name == "sample":
        args += [7, site_base, count]
    elif counted:
        args += [good_table(name, 2, device) if isinstance(table, str) else table, count]
    args += [np.zeros(4096, out_a), np.zeros(4096), np.zeros(S, np.uint8)]
    args = [ctx._h, n_sites] + args + ([None] if device else [])
    assert len(args) == len(fn.argtypes)
    keep = [a for a in args if isinstance(a, np.ndarray)]  # (alive over the call)
    rc = fn(*[a.ctypes.data_as(t) if isinstance(a, np.ndarray) else a for a, t in zip(args, fn.argtypes)])
    del keep
    return rc, fs.lib().famseq_last_error(ctx._h)


def everything_else_wrong(ctx, entry, want, any_site_count=True, **extra):
    """The complaint about the extra wins: with the rest in order, and with neither lk nor pl16, no prior rows (and no device);
    any_site_count: with a negative site count and with none as well (af0 has one value per site: none to complain about there)."""
    assert call(ctx, entry, **extra) == (E_ARG, want)
    assert call(ctx, entry, lk=False, pl16=False, prior=False, **extra) == (E_ARG, want)
    if not any_site_count:
        return
    assert call(ctx, entry, lk=True, pl16=True, prior=False, n_sites=-1, **extra) == (E_ARG, want)
    assert call(ctx, entry, lk=False, pl16=False, prior=False, n_sites=0, **extra) == (E_ARG, want)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if PRODUCTS[e[0]][2]], ids=entry_id)
def test_a_bad_count_is_said_first(ctx, entry):
    name, lo, hi = PRODUCTS[entry[0]][2]
    for bad in (lo - 1, hi + 1):
        want = ("%s must be %d..%d, got %d" % (name, lo, hi, bad)).encode()
        everything_else_wrong(ctx, entry, want, count=bad)
        everything_else_wrong(ctx, entry, want, count=bad, table=None)  # the count before the table
    if entry[0] == "sample":  # ... and before site_base
        everything_else_wrong(ctx, entry, b"n_draws must be 1..256, got 0", count=0, site_base=-1)
    for good in (lo, hi):
        assert call(ctx, entry, count=good, table=good_table(entry[0], hi, entry[2])) == (E_NODEVICE, NO_DEVICE)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if PRODUCTS[e[0]][3]], ids=entry_id)
def test_a_null_table_is_said_first(ctx, entry):
    everything_else_wrong(ctx, entry, NO_TABLE[entry[0]][entry[2]], table=None)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e[0] == "sample"], ids=entry_id)
def test_a_negative_site_base_is_said_first(ctx, entry):
    everything_else_wrong(ctx, entry, b"site_base must be >= 0, got -1", site_base=-1)
    everything_else_wrong(ctx, entry, b"site_base must be >= 0, got -5000000000", site_base=-5000000000)
    assert call(ctx, entry, site_base=0) == (E_NODEVICE, NO_DEVICE)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e[0] == "origin"], ids=entry_id)
def test_origin_asks_for_an_allele_level_model_first(spoiled, entry):
    everything_else_wrong(spoiled, entry, NO_ALLELE)


@pytest.mark.parametrize("case", sorted(BAD_VALUES), ids=lambda c: "%s: %s" % c)
def test_host_entries_name_the_first_bad_value(ctx, case):
    table, want = BAD_VALUES[case]
    for entry in (e for e in ENTRIES if e[0] == case[0]):
        _, site_prior, device = entry
        if not device:
            everything_else_wrong(ctx, entry, want, any_site_count=case[0] != "af", table=table)
            continue
        # a device entry cannot read its table: it goes on to the next complaint
        assert call(ctx, entry, table=table) == (E_NODEVICE, NO_DEVICE)
        assert call(ctx, entry, table=table, lk=False, pl16=False) == (E_ARG, ONE_OF)
        if site_prior:
            assert call(ctx, entry, table=table, prior=False) == (E_ARG, D_PRIOR)
            assert call(ctx, entry, table=table, lk=False, pl16=False, prior=False) == (E_ARG, D_PRIOR)


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_with_a_good_extra_the_order_is_the_trio_entries(ctx, entry):
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
    for entry in ENTRIES:
        fn = entry_fn(entry)
        assert fn(None, 1, *[0 if t in (C.c_int32, C.c_int64, C.c_uint64) else None for t in fn.argtypes[2:]]) == E_ARG
