"""The weight entries on a caller's stream: famseq_weight_batch_device / famseq_weight_prior_batch_device (Python
Context.weight_device / weight_prior_device) promise, like every device entry, to enqueue on `stream` and return without
synchronising.  The method and the machinery are test_gpu_streams.py's test A: the stream is a torch.cuda.Stream() that is BUSY
behind a measured delay while the library is called, the entry's input buffers hold poison at that moment and the real inputs
arrive by copies enqueued in front of it, the host must come back while the stream is still busy, and the copies of the outputs
enqueued behind the entry carry the host entry's bits.  With d_lk and with d_pl16 (the unpack stage, the column maps and the
kept scratch rows), plain and with site priors, ped5 (N % 4 != 0) and ped10, evidence_block_threads + 1 sites.

Unlike the masks of the pattern entries and the tables of the mutation-rate entries, the weight table is staged by the caller
among the inputs: the entry is given a table of 0.5s and the real one arrives by a copy on the stream in front of it — the device
entries read nothing of the table on the host and keep no copy of it."""
import numpy as np
import pytest

import famseq_amd as fs
import test_gpu_streams as S
from test_gpu_streams import PEDIGREES, Entry, Job, Pending, context, delay_unit_ms, report, warm_up  # noqa: F401 (the fixtures)
from test_gpu_side_entries import same_bits

pytestmark = pytest.mark.gpu

N_WEIGHTS = 3
POISON = dict(S.POISON, d_weights=0.5)  # (a legal table: the poisoned call answers, with other numbers)


class WeightEntry(Entry):
    """One way of calling Context.weight_device / weight_prior_device."""

    def __init__(self, prior, packed):
        self.method = "weight_prior_device" if prior else "weight_device"
        self.packed, self.text, self.called, self.prior, self.product = packed, False, True, prior, "weight"
        self.id = "%s-%s" % (self.method, "pl16" if packed else "lk")

    def arrays(self, ped, n, rng, seq):
        a = super().arrays(ped, n, rng, seq)  # (the flags, the rows or the packed PLs with their columns, the prior rows)
        w = np.ones((N_WEIGHTS, ped.n, 3))
        w[0] = fs.penetrance_weights(ped.n, [ped.n - 1], [0], (0.01, 0.8, 0.9))
        w[1] = 10.0 ** rng.uniform(-3, 0.5, (ped.n, 3))
        w[2, rng.randint(ped.n)] = (2.0, 3.5, 0.25)
        a.update(d_weights=w, n_weights=N_WEIGHTS)
        return a

    def host(self, ctx, a):
        io = {"flags": a["d_flags"], ("pl16" if self.packed else "lk"): a["d_pl16" if self.packed else "d_lk"]}
        if self.packed:
            io["seq_members"] = a["seq_members"]
        out = ctx.weight_prior_batch(a["d_prior"], a["d_weights"], **io) if self.prior else ctx.weight_batch(a["d_weights"], **io)
        return dict(zip(("d_wt_loglik", "d_loglik", "d_status"), out))


class WeightJob(Job):
    """test_gpu_streams.Job with the weight table among the poisoned inputs that issue() stages on the stream."""

    def poisoned(self):
        a = dict(self.a)
        for k, v in POISON.items():
            if k in a:
                a[k] = np.full_like(a[k], v)
        return self.entry.host(self.ctx, a)

    def reset(self):
        super().reset()
        self.buf["d_weights"].fill_(POISON["d_weights"])

    def issue(self, stream):
        import torch

        with torch.cuda.stream(stream):
            self.buf["d_weights"].copy_(self.src["d_weights"], non_blocking=True)
        super().issue(stream)


ENTRIES = [WeightEntry(prior, packed) for prior in (False, True) for packed in (False, True)]


def test_both_device_methods_are_here():
    """Context's device methods of the weight entries, by the names this file calls them."""
    assert {e.method for e in ENTRIES} == {m for m in dir(fs.Context) if m.startswith("weight") and m.endswith("_device")}


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("entry", ENTRIES, ids=[e.id for e in ENTRIES])
def test_the_weight_device_entries_follow_their_stream(entry, name, context, delay_unit_ms):
    ctx, ped, n = context(name, "default")
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()
    what = "%s, %s, %d sites" % (entry.id, name, n)
    job = WeightJob(ctx, entry, ped, n, seq, what)
    poison = job.poisoned()
    for k in job.ref:
        assert k == "d_status" or not same_bits(poison[k], job.ref[k]), "%s: %s is the same on the poison" % (what, k)
    # ... and the table alone on poison, the rows real: what an entry that read the table before the stream reached it would give
    late = entry.host(ctx, dict(job.a, d_weights=np.full_like(job.a["d_weights"], POISON["d_weights"])))
    assert not same_bits(late["d_wt_loglik"], job.ref["d_wt_loglik"]), "%s: wt_loglik is the same on the poisoned table" % what
    p = Pending(delay_unit_ms, warm_up([job]))
    problems = []
    job.issue(p.stream)
    p.still_busy(what, problems)
    p.stream.synchronize()
    report(what, p)
    assert not problems + job.wrong(what), "\n".join(problems + job.wrong(what))
