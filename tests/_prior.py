"""Shared by the site-prior tests (tests/test_prior_host.py on the CPU, tests/test_gpu_prior.py and tests/test_cli_prior_gpu.py
on the device): pedigrees, batches, and the reference — the existing oracles with one model per site, whose genoProbN /
genoProbXN are that site's prior row and whose flags carry the chrX bit only."""
import numpy as np

import famseq_amd as fs
from famseq_amd.prebuild_sets import wide_pedigree
from famseq_amd.synth import random_likelihoods

RTOL = 1e-9  # the project's bar for posteriors
N_SITES = 200


def pedigree(name):
    if name == "cousins":  # a first-cousin marriage: one loop, one conditioned member (tests/_variants.py)
        ids, mids, fids = [1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 0, 2, 2, 0, 0, 5, 4, 8], [0, 0, 1, 1, 0, 0, 3, 6, 7]
        ped = fs.Pedigree(ids, mids, fids, [1, 2, 1, 2, 2, 1, 1, 2, 1], ["s%d" % i for i in ids])
    elif name.startswith("wide"):
        ped = wide_pedigree(int(name[4:]))
    else:
        ped = fs.synthetic_pedigree(name)
    ped.relations()
    return ped


def batch(ped, n_sites=N_SITES, seed=11):
    """(lk, flags, prior): random_likelihoods' rows (hard zeros, sharp sites, flags 0..3 mixed site by site; PLs below 40 from
    twenty members on, as every wide-pedigree test draws them), allele frequencies uniform in log space over (1e-6, 0.999).
    Beyond 24 members the sharp sites' 1e-40 becomes 1e-18 — still sharp enough for the -LRC shortcut, 1 / (1 + 2e-18) being
    1 — because thirty members that contradict their parents at 1e-40 a piece put messages below the normal range of a
    double, where the oracle's own digits depend on its order of products (assert_well_conditioned finds such sites)."""
    rng = np.random.RandomState(seed + ped.n)
    lk, flags = random_likelihoods(rng, ped, n_sites, max_pl=300 if ped.n <= 20 else 40)
    if ped.n > 24:
        lk[lk == 1e-40] = 1e-18
    af = 10.0 ** rng.uniform(-6, np.log10(0.999), n_sites)
    assert af.min() > 1e-6 and af.max() < 0.999
    return lk, flags, fs.hwe_priors(af)


def reference(ped, lk, flags, prior, mrate=1e-7, lc=1.0):
    """-> (post, single, status): per site the oracle of a model built for that site."""
    import oracle
    import oracle.sum_product as sp

    post, single, status = np.empty_like(lk), np.empty_like(lk), np.zeros(len(lk), np.uint8)
    chrx = (np.asarray(flags) & fs.FLAG_CHRX).astype(np.uint8)
    for s in range(len(lk)):
        r = prior[s]
        if ped.n <= 20:
            m = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders, ped.sequenced, mrate=mrate, lc=lc,
                                   genoProbN=r[0:3], genoProbXN=r[3:6])
            out = m.bn_batch(lk[s:s + 1], chrx[s:s + 1])
        else:
            out = sp.pedigree_posterior(ped, lk[s:s + 1], chrx[s:s + 1], mrate=mrate, lc=lc, gN=tuple(r[0:3]), gXN=tuple(r[3:6]))
        post[s], single[s], status[s] = out[0][0], out[1][0], out[2][0]
    return post, single, status


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_well_conditioned(ped, lk, flags, prior, ref, **consts):
    """The reference's own digits can be trusted on every site: with every likelihood row scaled by 2^8 — which scales every
    weight of the network by the same power of two, exactly, unless a product has left the normal range on the way — it
    returns the same bits."""
    again = reference(ped, lk * 256.0, flags, prior, **consts)
    assert np.array_equal(again[2], ref[2])
    for a, b in zip(again[:2], ref[:2]):
        assert np.array_equal(bits(a), bits(b))


def check(out, ref, what=""):
    """status and single posterior bit-exact, posteriors at RTOL, failed rows NaN; no site left out."""
    post, single, status = out
    assert np.array_equal(status, ref[2]), what
    ok, s_ok = (status & 3) == 0, (status & 3) != 1
    assert np.array_equal(bits(single[s_ok]), bits(ref[1][s_ok])), what
    np.testing.assert_allclose(post[ok], ref[0][ok], rtol=RTOL, atol=0, err_msg=what)
    cut = status == 0x80
    assert np.array_equal(bits(post[cut]), bits(ref[0][cut])), what
    assert np.all(np.isnan(post[~ok])) and np.all(np.isnan(single[~s_ok])), what


def model_rows(model, flags):
    """The rows the model itself would have used at each site: genoProbK / genoProbXK where the Known bit is set, genoProbN /
    genoProbXN elsewhere."""
    known = (np.asarray(flags) & fs.FLAG_KNOWN) != 0
    n_row = np.array(list(model.genoProbN) + list(model.genoProbXN))
    k_row = np.array(list(model.genoProbK) + list(model.genoProbXK))
    return np.ascontiguousarray(np.where(known[:, None], k_row[None], n_row[None]))
