"""The device entries on a caller's stream: include/famseq_hip.h promises of every one that it "enqueues on `stream` and returns
without synchronising".  The rest of the suite passes torch.cuda.current_stream() — the null stream, on which a blocking copy inside
the library is ordered with the kernels by accident — and compares after torch.cuda.synchronize().  Here the stream is one a
PyTorch pipeline uses, torch.cuda.Stream() (created non-blocking), and it is BUSY while the library is called:

  * a delay of ordinary torch work goes on the stream first and an event `done` behind it;
  * the library calls follow with no host synchronisation between them;
  * straight after they return, `done.query()` must still be false: the host came back while the stream was busy (the documented
    "returns without synchronising"), and whatever the calls did on the host — a blocking copy into the context's column maps,
    a rewritten argument block — happened while everything they enqueued was still waiting.  A test whose window was not
    open fails; none skips or passes on luck;
  * then the stream is synchronised and every output is compared bit for bit with the host entry's (one kernel behind both: no
    tolerance).

The delay is not a constant: one unit of it (torch.cuda._sleep(UNIT_CYCLES)) is timed once per session with events, the host side
of the warmed-up calls with time.perf_counter, and the delay is MULTIPLE times the larger of the two (profiles/streams/README.md
has the figures measured on an MI355X).  The warm-up is the same sequence of calls on the same stream, twice, then synchronised:
it loads the kernels and grows the context's scratch, so the calls under test do neither (both may wait, and say so in the header).

Shapes, the smallest at which this layer can go wrong: ped5 (N % 4 != 0) and ped10; evidence_block_threads + 1 sites for the
generated kernels, 300 for the compiled-in team kernel and its separate stages (two whole tiles and a ragged one, as in
test_gpu_call.py); flags 0..3 in turn; likelihood rows and packed PLs drawn as in test_gpu_side_entries.inputs.

What these tests never do: grow scratch while another stream's call is pending, free a buffer behind a pending call, or loop until
a race shows."""
import math
import time
import zlib

import numpy as np
import pytest

import famseq_amd as fs
from test_gpu_call import CALL_ENGINES
from test_gpu_side_entries import SENTINEL, inputs, same_bits

pytestmark = pytest.mark.gpu

MULTIPLE = 20          # the delay, in units of the larger of (one unit of the delay, the host side of the calls under test)
UNIT_CYCLES = 200_000  # one unit of the delay: torch.cuda._sleep of this many ticks (timed once per session, not assumed)
ENGINES = dict([("default", {})] + CALL_ENGINES)
PEDIGREES = ("ped5", "ped10")
POISON = {"d_lk": 0.0, "d_pl16": 3, "d_flags": 0, "d_prior": 0.0}  # all-zero rows; flat PLs, none missing; flags 0; zero priors
# the side products: the names of their two outputs and what each takes beside the common arguments
SIDE = {"trio": ("d_joint", "d_dnm"), "map": ("d_map_gt", "d_map_post"), "evidence": ("d_loglik", "d_pref"), "loo": ("d_loo", "d_fit"),
        "pattern": ("d_pat_post", "d_loglik"), "sample": ("d_samp_gt", "d_samp_post"), "af": ("d_af", "d_loglik")}
N_PATTERNS, N_DRAWS, SEED, SITE_BASE, N_ITER = 3, 3, 12345, 1000, 4


class Entry:
    """One way of calling one *_batch_device method of famseq_amd.Context."""

    def __init__(self, method, packed=False, text=False, called=True):
        self.method, self.packed, self.text, self.called = method, packed, text, called
        stem = method[:-len("_batch_device")]
        self.prior = stem.endswith("_prior")
        self.product = stem[:-len("_prior")] if self.prior else stem  # bn, bn_call, or a key of SIDE
        self.id = "%s-%s%s" % (method, "pl16" if packed else "lk", "-text" if text and called else "-text_only" if text else "")

    def arrays(self, ped, n, rng, seq):
        """The call's arguments by the names the device method gives them: numpy arrays for what is resident, the rest as it is."""
        inp = inputs(ped, n, self.packed, rng)
        a = {"d_flags": inp["flags"], ("d_pl16" if self.packed else "d_lk"): inp["pl16" if self.packed else "lk"]}
        if self.packed or self.product == "bn_call":
            a["seq_members"] = seq
        if self.prior:
            a["d_prior"] = fs.hwe_priors(rng.uniform(0.01, 0.5, n))
        if self.product == "pattern":
            a.update(d_masks=rng.randint(1, 8, size=(N_PATTERNS, ped.n)).astype(np.uint8), n_patterns=N_PATTERNS)
        if self.product == "sample":
            a.update(n_draws=N_DRAWS, seed=SEED, site_base=SITE_BASE)
        if self.product == "af":
            a.update(d_af0=rng.uniform(0.05, 0.5, n), n_iter=N_ITER)
        return a

    def host(self, ctx, a):
        """The host entry's answer on the same arguments -> {name of the device method's output: array}."""
        io = {"flags": a["d_flags"], ("pl16" if self.packed else "lk"): a["d_pl16" if self.packed else "d_lk"]}
        if self.product == "bn":
            out = ctx.bn_prior_batch(io["lk"], a["d_prior"], io["flags"]) if self.prior else ctx.bn_batch(io["lk"], io["flags"])
            return dict(zip(("d_post", "d_single", "d_status"), out))
        if self.product == "bn_call":
            out = dict(zip(("d_gpp", "d_fpp", "d_fgt", "d_status"), ctx.bn_call_batch(a["seq_members"], **io))) if self.called else {}
            if self.text:
                out["d_text"], out["d_status"] = ctx.bn_call_text_batch(a["seq_members"], **io)
            return out
        if self.packed:
            io["seq_members"] = a["seq_members"]
        lead = ((a["d_prior"],) if self.prior else ()) + {"pattern": lambda: (a["d_masks"],), "sample": lambda: (N_DRAWS, SEED, SITE_BASE),
                                                          "af": lambda: (a["d_af0"], N_ITER)}.get(self.product, lambda: ())()
        out = getattr(ctx, self.method[:-len("_device")])(*lead, **io)[-3:]
        return dict(zip(SIDE[self.product] + ("d_status",), out))


class Job:
    """One call of an entry on resident buffers of its own: `src` holds the real inputs, `buf` — what the entry is given — poison
    until issue() copies the real ones into it on the stream, `out` the suite's sentinels until the entry writes it."""

    def __init__(self, ctx, entry, ped, n, seq, key, arrays=None):
        import torch

        self.ctx, self.entry, self.n = ctx, entry, n
        self.a = arrays or entry.arrays(ped, n, np.random.RandomState(zlib.crc32(key.encode())), seq)
        self.ref = entry.host(ctx, self.a)
        dev = lambda v: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda()
        self.src = {k: dev(v) for k, v in self.a.items() if isinstance(v, np.ndarray) and k != "seq_members"}
        self.buf = {k: torch.empty_like(t) for k, t in self.src.items()}
        self.out = {k: torch.empty(v.shape, dtype=getattr(torch, v.dtype.name), device="cuda") for k, v in self.ref.items()}
        self.reset()

    def poisoned(self):
        """The host entry's answer on the poison: what an entry that read its buffers before the stream reached them would give."""
        a = dict(self.a)
        for k, v in POISON.items():
            if k in a:
                a[k] = np.full_like(a[k], v)
        return self.entry.host(self.ctx, a)

    def reset(self):
        for k, t in self.buf.items():
            t.fill_(POISON[k]) if k in POISON else t.copy_(self.src[k])  # (masks and start values are no test of the stream)
        for t in self.out.values():
            t.fill_(SENTINEL[np.dtype(str(t.dtype).split(".")[1])])
        self.got = None

    def issue(self, stream):
        """On `stream`: the real inputs into the entry's buffers, the entry, a copy of every output.  No host synchronisation."""
        import torch

        with torch.cuda.stream(stream):
            for k in POISON:
                if k in self.buf:
                    self.buf[k].copy_(self.src[k], non_blocking=True)
            kw = {k: v for k, v in self.a.items() if k not in self.buf}
            kw.update({k: t.data_ptr() for k, t in self.buf.items()})
            kw.update({k: t.data_ptr() for k, t in self.out.items()})
            getattr(self.ctx, self.entry.method)(self.n, stream=stream.cuda_stream, **kw)
            self.got = {k: t.clone() for k, t in self.out.items()}

    def wrong(self, what):
        """(after a synchronise) the outputs whose copy does not carry the reference's bits, as messages."""
        return ["%s: %s differs from the host entry's (%d of %d bytes)" % (what, k, np.count_nonzero(g.view(np.uint8) != self.ref[k].view(np.uint8)), g.nbytes)
                for k, g in ((k, t.cpu().numpy()) for k, t in self.got.items()) if not same_bits(g, self.ref[k])]


@pytest.fixture(scope="session")
def delay_unit_ms():
    """One unit of the delay, timed with events (the median of three, after one to load the kernel)."""
    import torch

    torch.cuda._sleep(UNIT_CYCLES)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(UNIT_CYCLES)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    assert sorted(ms)[1] > 0
    return sorted(ms)[1]


@pytest.fixture(scope="module")
def context():
    """context(pedigree name, engine label) -> (Context, Pedigree, sites): one context per pair for the whole file."""
    made = {}

    def get(name, label="default"):
        if (name, label) not in made:
            ped = fs.synthetic_pedigree(name)
            ped.relations()
            ctx = fs.Context(fs.make_model(ped), device=0, **ENGINES[label])
            n = 300 if ENGINES[label].get("enum_impl") == 0 else ctx.plan()["evidence_block_threads"] + 1
            made[name, label] = (ctx, ped, n)
        return made[name, label]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


class Pending:
    """A side stream with the delay on it and the event `done` behind the delay."""

    def __init__(self, unit_ms, host_ms, delayed=True, settle=True):
        import torch

        self.stream = torch.cuda.Stream()
        self.unit_ms, self.host_ms = unit_ms, host_ms
        self.units = max(1, math.ceil(MULTIPLE * max(unit_ms, host_ms) / unit_ms))
        self.done = torch.cuda.Event()
        if settle:  # what the null stream did to the buffers is done: the side streams do not wait for it.  (Not behind another
            torch.cuda.synchronize()  # Pending: that would wait for its delay.)
        self.t0 = time.perf_counter()
        if delayed:
            with torch.cuda.stream(self.stream):
                torch.cuda._sleep(UNIT_CYCLES * self.units)
                self.done.record()

    def still_busy(self, what, problems):
        """The precondition: to be called straight after the library calls have returned."""
        busy, now_ms = not self.done.query(), (time.perf_counter() - self.t0) * 1e3
        if not busy:
            problems.append("%s: the stream was idle when the host came back — the entry waited for its stream, or the delay was too short: delay "
                            "%.3f ms (%d units of %.3f ms, %d times the larger of a unit and the warmed-up calls' %.3f ms of host time), the host "
                            "took %.3f ms this time" % (what, self.units * self.unit_ms, self.units, self.unit_ms, MULTIPLE, self.host_ms, now_ms))
        return busy


def warm_up(jobs, stream=None):
    """The calls under test, in their order, on one stream, twice; -> the host side of the second pass in ms.  Leaves the
    buffers poisoned again."""
    import torch

    stream = stream or torch.cuda.Stream()
    for timed in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for job in jobs:
            job.issue(stream)
        host_ms = (time.perf_counter() - t0) * 1e3
        stream.synchronize()
    for job in jobs:
        wrong = job.wrong("warm-up")
        assert not wrong, wrong  # (one call at a time, synchronised: what the rest of the suite pins)
        job.reset()
    return host_ms


def report(what, p):
    print("streams: %-60s delay unit %.3f ms, host side of the calls %.3f ms, delay %d units = %.2f ms" % (what, p.unit_ms, p.host_ms, p.units, p.units * p.unit_ms))


def every_entry():
    out = [(Entry("bn_batch_device"), "default"), (Entry("bn_prior_batch_device"), "default")]
    for product in SIDE:
        for prior in (("", "_prior") if product != "af" else ("",)):
            out += [(Entry("%s%s_batch_device" % (product, prior), packed), "default") for packed in (False, True)]
    for label, _ in CALL_ENGINES:
        out += [(Entry("bn_call_batch_device", packed, text), label) for packed in (False, True) for text in (False, True)]
    return out


EVERY = every_entry()


def test_the_table_names_every_device_entry():
    """Whoever adds a *_batch_device method to Context adds it to the table of test A."""
    assert {e.method for e, _ in EVERY} == {m for m in dir(fs.Context) if m.endswith("_batch_device")}


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("entry,label", EVERY, ids=["%s-%s" % (e.id, label.split(",")[0].split(" ")[0]) for e, label in EVERY])
def test_every_device_entry_follows_its_stream(entry, label, name, context, delay_unit_ms):
    """A. Every *_batch_device method (bn_call with d_lk and d_pl16, with and without d_text; each side entry with d_lk and d_pl16)
    is given buffers that hold poison when it is called: the real inputs arrive by copies enqueued on the side stream in front of it,
    behind the delay.  The copies of the outputs, enqueued behind it, carry the host entry's bits — so every stage of the entry
    ran on that stream, between the two.  A stage on another stream, or on the null stream, reads the poison, whose answer differs
    (asserted on the host entry)."""
    ctx, ped, n = context(name, label)
    seq = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()
    what = "%s, %s, %s, %d sites" % (entry.id, label, name, n)
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


def pair(context, name, label, entry, tag):
    """Two calls of one entry on one context, each with inputs and outputs of its own: the first in column order A (the
    sequenced members from the last to the first), the second in the reverse."""
    ctx, ped, n = context(name, label)
    a = np.nonzero(ped.sequenced)[0].astype(np.int32)[::-1].copy()
    what = "%s, %s, %s, %d sites" % (entry.id, label, name, n)
    return [Job(ctx, entry, ped, n, a, tag + what + " call 1"), Job(ctx, entry, ped, n, a[::-1].copy(), tag + what + " call 2")], what


PAIRS = [(Entry("bn_call_batch_device", True), label) for label, _ in CALL_ENGINES]
PAIRS += [(Entry("bn_call_batch_device", True, text=True, called=False), CALL_ENGINES[1][0])]  # the text alone: the numbers go through the scratch
PAIRS += [(Entry("evidence_batch_device", True), "default"), (Entry("sample_batch_device", True), "default")]  # the unpack stage and d_col
PAIR_IDS = ["%s-%s" % (e.id, label.split(",")[0].split(" ")[0]) for e, label in PAIRS]


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("entry,label", PAIRS, ids=PAIR_IDS)
def test_a_later_call_leaves_an_earlier_one_alone(entry, label, name, context, delay_unit_ms):
    """B. On one side stream, behind the delay: call 1 in column order A, call 2 in the reverse order, each with its own inputs and
    outputs; each carries its own reference's bits.  A context that rewrites its column maps or its argument block when call 2 is
    ISSUED, not where call 2 stands in the stream, gives call 1 in call 2's column order."""
    jobs, what = pair(context, name, label, entry, "B ")
    p = Pending(delay_unit_ms, warm_up(jobs))
    problems = []
    for k, job in enumerate(jobs):
        job.issue(p.stream)
        p.still_busy("%s, after call %d" % (what, k + 1), problems)
    p.stream.synchronize()
    report(what, p)
    problems += [m for k, job in enumerate(jobs) for m in job.wrong("%s, call %d" % (what, k + 1))]
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", PEDIGREES)
def test_a_host_entry_leaves_an_earlier_device_call_alone(name, context, delay_unit_ms):
    """B, with call 2 made as the HOST entry bn_call_batch in the reverse column order while the device call in order A is pending.
    The host entry may wait (it is blocking anyway), so the precondition is checked between the two; it must not change the maps
    under the pending call, and must itself be right."""
    entry, label = PAIRS[1]
    jobs, what = pair(context, name, label, entry, "B host ")
    p = Pending(delay_unit_ms, warm_up(jobs[:1]))
    problems = []
    jobs[0].issue(p.stream)
    p.still_busy(what + ", after the device call", problems)
    got = entry.host(jobs[1].ctx, jobs[1].a)
    p.stream.synchronize()
    report(what, p)
    problems += jobs[0].wrong(what + ", the device call") + ["%s, the host call: %s differs" % (what, k) for k in got if not same_bits(got[k], jobs[1].ref[k])]
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("entry,label", [PAIRS[0], PAIRS[4]], ids=[PAIR_IDS[0], PAIR_IDS[4]])
def test_two_streams_one_context(entry, label, name, context, delay_unit_ms):
    """C. The same pair with call 2 on a second side stream that has no delay: calls that touch the context's state take effect in
    the order issued, whatever streams they are on.  An update that is merely asynchronous on the caller's own stream lands
    before call 1 runs, and fails here."""
    jobs, what = pair(context, name, label, entry, "C ")
    p = Pending(delay_unit_ms, warm_up(jobs))
    other = Pending(delay_unit_ms, p.host_ms, delayed=False, settle=False)
    problems = []
    jobs[0].issue(p.stream)
    jobs[1].issue(other.stream)
    p.still_busy(what + ", after both calls", problems)
    p.stream.synchronize()
    other.stream.synchronize()
    report(what, p)
    problems += [m for k, job in enumerate(jobs) for m in job.wrong("%s, call %d" % (what, k + 1))]
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", PEDIGREES)
def test_entries_without_context_state_run_on_any_stream(name, context, delay_unit_ms):
    """D. bn_batch_device on one side stream and evidence_batch_device on d_lk on another, both behind delays: neither waits, both
    are right.  (Their kernels may overlap; these entries use nothing of the context's that changes, and get no cross-stream wait.)"""
    ctx, ped, n = context(name)
    what = "bn_batch_device and evidence_batch_device-lk, %s, %d sites" % (name, n)
    jobs = [Job(ctx, Entry(m), ped, n, None, "D " + what + m) for m in ("bn_batch_device", "evidence_batch_device")]
    host_ms = warm_up(jobs)
    pending = [Pending(delay_unit_ms, host_ms), Pending(delay_unit_ms, host_ms, settle=False)]
    problems = []
    for job, p in zip(jobs, pending):
        job.issue(p.stream)
    for job, p in zip(jobs, pending):
        p.still_busy("%s, stream of %s" % (what, job.entry.method), problems)
    for p in pending:
        p.stream.synchronize()
    report(what, pending[0])
    problems += [m for job in jobs for m in job.wrong("%s, %s" % (what, job.entry.method))]
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", PEDIGREES)
@pytest.mark.parametrize("label", [e[0] for e in CALL_ENGINES])
def test_repeated_calls_do_not_wait(label, name, context, delay_unit_ms):
    """E. Three calls of bn_call_batch_device behind one delay: the call the warm-up ended with once more, the same with other
    output buffers, and one in another column order.  The host comes back from each while the stream is busy: neither a
    comparison of argument blocks that sees their padding, nor changed pointers, nor a changed column order makes the entry wait."""
    entry = Entry("bn_call_batch_device", True)
    (first, third), what = pair(context, name, label, entry, "E ")
    ctx, ped, n = context(name, label)
    second = Job(ctx, entry, ped, n, first.a["seq_members"], "", arrays=first.a)
    host_ms = warm_up([second, third, first])  # (ends with the first call)
    p = Pending(delay_unit_ms, host_ms)
    problems = []
    for k, job in enumerate((first, second, third)):
        job.issue(p.stream)
        p.still_busy("%s, after call %d (%s)" % (what, k + 1, ("the warm-up's last call again", "other output buffers", "another column order")[k]), problems)
    p.stream.synchronize()
    report(what, p)
    problems += [m for k, job in enumerate((first, second, third)) for m in job.wrong("%s, call %d" % (what, k + 1))]
    assert not problems, "\n".join(problems)
