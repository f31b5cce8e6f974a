"""The relabelling entries on a caller's stream: famseq_relabel_batch_device / famseq_relabel_prior_batch_device (Python
Context.relabel_device / relabel_prior_device) promise, like every device entry, to enqueue on `stream` and return without
synchronising.  The method and the machinery are test_gpu_streams.py's test A, unchanged: the stream is a torch.cuda.Stream() that
is BUSY behind a measured delay while the library is called, the entry's input buffers hold poison at that moment and the real
inputs arrive by copies enqueued in front of it, the host must come back while the stream is still busy, and the copies of the
outputs enqueued behind the entry carry the host entry's bits.  With d_lk and with d_pl16 (the unpack stage and the column maps),
plain and with site priors, ped5 (N % 4 != 0) and ped10, evidence_block_threads + 1 sites.  The assignment table is resident and
is no test of the stream (as the masks of the pattern entries are not)."""
import numpy as np
import pytest

import famseq_amd as fs
from test_gpu_streams import PEDIGREES, Entry, Job, Pending, context, delay_unit_ms, report, warm_up  # noqa: F401 (the fixtures)
from test_gpu_side_entries import same_bits

pytestmark = pytest.mark.gpu

N_ASSIGN = 3


class RelabelEntry(Entry):
    """One way of calling Context.relabel_device / relabel_prior_device."""

    def __init__(self, prior, packed):
        self.method = "relabel_prior_device" if prior else "relabel_device"
        self.packed, self.text, self.called, self.prior, self.product = packed, False, True, prior, "relabel"
        self.id = "%s-%s" % (self.method, "pl16" if packed else "lk")

    def arrays(self, ped, n, rng, seq):
        a = super().arrays(ped, n, rng, seq)  # (the flags, the rows or the packed PLs with their columns, the prior rows)
        a.update(d_assign=rng.randint(-1, ped.n, size=(N_ASSIGN, ped.n)).astype(np.int32), n_assign=N_ASSIGN)
        return a

    def host(self, ctx, a):
        io = {"flags": a["d_flags"], ("pl16" if self.packed else "lk"): a["d_pl16" if self.packed else "d_lk"]}
        if self.packed:
            io["seq_members"] = a["seq_members"]
        out = ctx.relabel_prior_batch(a["d_prior"], a["d_assign"], **io) if self.prior else ctx.relabel_batch(a["d_assign"], **io)
        return dict(zip(("d_alt", "d_loglik", "d_status"), out))


ENTRIES = [RelabelEntry(prior, packed) for prior in (False, True) for packed in (False, True)]


def test_both_device_methods_are_here():
    """Context's device methods of the relabelling entries, by the names this file calls them."""
    assert {e.method for e in ENTRIES} == {m for m in dir(fs.Context) if m.startswith("relabel") and m.endswith("_device")}


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("entry", ENTRIES, ids=[e.id for e in ENTRIES])
def test_the_relabel_device_entries_follow_their_stream(entry, name, context, delay_unit_ms):
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
