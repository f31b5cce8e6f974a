"""The mutation-rate entries on a caller's stream: famseq_mutrate_batch_device / famseq_mutrate_prior_batch_device (Python
Context.mutrate_device / mutrate_prior_device) promise, like every device entry, to enqueue on `stream` and return without
synchronising.  The method and the machinery are test_gpu_streams.py's test A, unchanged: the stream is a torch.cuda.Stream() that
is BUSY behind a measured delay while the library is called, the entry's input buffers hold poison at that moment and the real
inputs arrive by copies enqueued in front of it, the host must come back while the stream is still busy, and the copies of the
outputs enqueued behind the entry carry the host entry's bits.  With d_lk and with d_pl16 (the unpack stage, the column maps and
the kept scratch rows), plain and with site priors, ped5 (N % 4 != 0) and ped10, evidence_block_threads + 1 sites.  The tables
are resident and are no test of the stream (as the masks of the pattern entries are not)."""
import numpy as np
import pytest

import famseq_amd as fs
from test_gpu_streams import PEDIGREES, Entry, Job, Pending, context, delay_unit_ms, report, warm_up  # noqa: F401 (the fixtures)
from test_gpu_side_entries import same_bits

pytestmark = pytest.mark.gpu

RATES = (0.0, 1e-7, 1e-3)


class MutrateEntry(Entry):
    """One way of calling Context.mutrate_device / mutrate_prior_device."""

    def __init__(self, prior, packed):
        self.method = "mutrate_prior_device" if prior else "mutrate_device"
        self.packed, self.text, self.called, self.prior, self.product = packed, False, True, prior, "mutrate"
        self.id = "%s-%s" % (self.method, "pl16" if packed else "lk")

    def arrays(self, ped, n, rng, seq):
        a = super().arrays(ped, n, rng, seq)  # (the flags, the rows or the packed PLs with their columns, the prior rows)
        plan_only = fs.Context(fs.make_model(ped), device=-1)  # (the fixture's model: the tables are the context's own but for the rate)
        a.update(d_tables=plan_only.rate_tables(RATES), n_rates=len(RATES))
        plan_only.close()
        return a

    def host(self, ctx, a):
        io = {"flags": a["d_flags"], ("pl16" if self.packed else "lk"): a["d_pl16" if self.packed else "d_lk"]}
        if self.packed:
            io["seq_members"] = a["seq_members"]
        out = ctx.mutrate_prior_batch(a["d_prior"], RATES, **io) if self.prior else ctx.mutrate_batch(RATES, **io)
        return dict(zip(("d_rate_loglik", "d_loglik", "d_status"), out))


ENTRIES = [MutrateEntry(prior, packed) for prior in (False, True) for packed in (False, True)]


def test_both_device_methods_are_here():
    """Context's device methods of the mutation-rate entries, by the names this file calls them."""
    assert {e.method for e in ENTRIES} == {m for m in dir(fs.Context) if m.startswith("mutrate") and m.endswith("_device")}


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("entry", ENTRIES, ids=[e.id for e in ENTRIES])
def test_the_mutrate_device_entries_follow_their_stream(entry, name, context, delay_unit_ms):
    ctx, ped, n = context(name, "default")
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()
    what = "%s, %s, %d sites" % (entry.id, name, n)
    job = Job(ctx, entry, ped, n, seq, what)
    poison = job.poisoned()
    for k in job.ref:
        assert k == "d_status" or not same_bits(poison[k], job.ref[k]), "%s: %s is the same on the poison" % (what, k)
    p = Pending(delay_unit_ms, warm_up([job]))
    problems = []
    job.issue(p.stream)
    p.still_busy(what, problems)
    p.stream.synchronize()
    report(what, p)
    assert not problems + job.wrong(what), "\n".join(problems + job.wrong(what))
