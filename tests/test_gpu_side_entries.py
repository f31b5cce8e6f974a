"""The twelve entries of the side products (trio, MAP, evidence; plain and site-prior; host and device buffers) against one
another on the device, bit for bit: they share one body in the library (side_entry), and this is what it must keep.

Shapes, the smallest that can still go wrong: the trio and ped5, 1 site and one site more than a workgroup takes per trip of its
loop (evidence_block_threads + 1), and 7 sites through the host pipeline at 3 sites per chunk (three chunks over two buffer
slots, the last one partial).  Every combination of the two outputs that has one (for the trio these are its three kernels: dnm
only, joint only, both), likelihood rows and packed PLs.  The reference of every comparison is the plain host entry asked for
both outputs, computed once per pedigree, site count and kind of input."""
import numpy as np
import pytest

import _prior as P
import famseq_amd as fs

pytestmark = pytest.mark.gpu

FORMS = ((False, True), (True, False), (True, True))  # (first output, second output): the trio's forms 1, 2, 3
SENTINEL = {np.dtype(np.float64): -1.0, np.dtype(np.int8): 55, np.dtype(np.uint8): 77}


def host(ctx, product, prior, inp, want):
    """-> (out_a, out_b, status) of the host entry; prior None: the plain one."""
    call = getattr(ctx, product + ("_batch" if prior is None else "_prior_batch"))
    names = {"trio": ("want_joint", "want_dnm"), "map": ("want_gt", "want_post"), "evidence": ("want_loglik", "want_pref")}[product]
    out = call(*(() if prior is None else (prior,)), **inp, **dict(zip(names, want)))
    return out[-3:]


def device(ctx, product, prior, inp, want, like):
    """The device entry on resident copies of the same arrays -> (out_a, out_b, status), each as the caller's buffer holds it
    afterwards: an output that is not asked for is not passed, and must have kept its sentinel."""
    import torch

    dev = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for k, v in inp.items() if k != "seq_members"}
    outs = [torch.full(x.shape, SENTINEL[x.dtype], dtype=getattr(torch, x.dtype.name), device="cuda") for x in like]
    names = {"trio": ("d_joint", "d_dnm"), "map": ("d_map_gt", "d_map_post"), "evidence": ("d_loglik", "d_pref")}[product]
    args = {"d_" + k: t.data_ptr() for k, t in dev.items()}
    args.update({n: t.data_ptr() for n, t, w in zip(names, outs, want) if w}, d_status=outs[2].data_ptr(), seq_members=inp.get("seq_members", ()))
    call = getattr(ctx, product + ("_batch_device" if prior is None else "_prior_batch_device"))
    n = len(like[2])
    if prior is None:
        call(n, **args)
    else:
        d_prior = torch.from_numpy(prior).cuda()
        call(n, d_prior.data_ptr(), **args)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in outs)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def inputs(ped, n, packed, rng):
    flags = (np.arange(n) % 4).astype(np.uint8)
    if not packed:
        return dict(lk=10.0 ** (-rng.randint(0, 30, size=(n, ped.n, 3)) / 10.0), flags=flags)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()  # a column order of its own
    return dict(pl16=rng.randint(0, 60, size=(n, len(seq), 3)).astype(np.uint16), seq_members=seq, flags=flags)


def check_plan(ctx, form, prior, seen):
    """The plan's trio keys follow the form asked for last, plain and site-prior each on its own."""
    plan = ctx.plan()
    if prior is None:
        assert plan["trio_code_object"] == plan["trio_code_objects"][form - 1] != "" and plan["trio_variant"] >= 0
    else:
        assert plan["trio_prior_code_object"].endswith(".hsaco") and plan["trio_prior_variant"] == plan["trio_variant"] >= 0
    now = plan["trio_code_object" if prior is None else "trio_prior_code_object"]
    assert seen.setdefault((form, prior is None), now) == now


@pytest.mark.parametrize("product", ["trio", "map", "evidence"])
def test_every_entry_gives_the_plain_host_entrys_bits(product):
    for name in ("trio", "ped5"):
        ped = fs.synthetic_pedigree(name)
        ped.relations()
        model = fs.make_model(ped)
        ctx = fs.Context(model, device=0)
        bt = ctx.plan()["evidence_block_threads"]
        rng = np.random.RandomState(ped.n)
        seen = {}
        for n, chunk in ((1, 0), (bt + 1, 0), (7, 3)):
            for packed in (False, True):
                inp = inputs(ped, n, packed, rng)
                rows = P.model_rows(model, inp["flags"])  # the model's own constants, site by site: the plain entries' bits
                ctx.set_option("chunk_sites", 0)
                ref = host(ctx, product, None, inp, (True, True))
                assert (ref[2] == 0).all()
                ctx.set_option("chunk_sites", chunk)
                for form, want in enumerate(FORMS, 1):
                    for prior in (None, rows):
                        what = "%s, %s, %d sites, %s, outputs %s, %s" % (product, name, n, "pl16" if packed else "lk", want,
                                                                         "plain" if prior is None else "site prior")
                        got = host(ctx, product, prior, inp, want)
                        if product == "trio":
                            check_plan(ctx, form, prior, seen)
                        for k in range(3):
                            if k < 2 and not want[k]:
                                assert got[k] is None, what
                            else:
                                assert same_bits(got[k], ref[k]), what
                        if chunk:
                            continue  # (the chunked pipeline is the host entries')
                        got = device(ctx, product, prior, inp, want, ref)
                        if product == "trio":
                            check_plan(ctx, form, prior, seen)
                        for k in range(3):
                            if k < 2 and not want[k]:
                                assert (got[k] == SENTINEL[got[k].dtype]).all(), what
                            else:
                                assert same_bits(got[k], ref[k]), what
        if product == "trio":  # six kernels, six code objects
            assert len(seen) == 6 and len(set(seen.values())) == 6
        ctx.close()


@pytest.mark.parametrize("product", ["trio", "map", "evidence"])
def test_no_sites_still_loads_the_kernel(product):
    ped = fs.synthetic_pedigree("trio")
    ctx = fs.Context(fs.make_model(ped), device=0)
    key = product + "_code_object"
    assert ctx.plan()[key] == "" and ctx.plan()[product + "_prior_code_object"] == ""
    out = host(ctx, product, None, dict(lk=np.ones((0, ped.n, 3))), (True, True))
    assert [len(x) for x in out] == [0, 0, 0] and ctx.plan()[key].endswith(".hsaco")
    getattr(ctx, product + "_prior_batch_device")(0, 0)  # (no sites: no prior rows to ask for)
    assert ctx.plan()[product + "_prior_code_object"].endswith(".hsaco")
    ctx.close()
