// pipeline.cpp — host batches through the device: per chunk H2D -> kernels -> D2H, each stage on its own stream and
// chained by events, so that chunk k+1 is copied in while chunk k is copied out (two chunk-sized streams running the
// whole sequence each fell into lockstep and used one direction of the link at a time).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "ctx.h"
#include "io_kernels.h"

namespace famseq {
namespace {

// One host array of `row` bytes per site and the slot buffer it is staged through.
struct Staged {
  int buf;
  size_t row;
  char *host;
};
// What a call moves: the arrays copied in before a chunk's kernels and those copied out after them, in that order.
struct ChunkJob {
  int64_t n_sites = 0, chunk = 0;
  Staged in[3], out[7];
  int n_in = 0, n_out = 0;
  void copy_in(int buf, size_t row, const void *host) {
    if (host && row) in[n_in++] = {buf, row, static_cast<char *>(const_cast<void *>(host))};  // (read only)
  }
  void copy_out(int buf, size_t row, void *host) {
    if (host && row) out[n_out++] = {buf, row, static_cast<char *>(host)};
  }
};
// Enqueues a chunk's kernels — n sites in slot s — on the compute stream; 0 or the error code (message set).
// (lo: the chunk's first site in the call)
using Stage = std::function<int(int s, int64_t n, hipStream_t stream, int64_t lo)>;

// Default chunk: at most 64 MiB per array of `row` bytes per site, at least four chunks per call so that the stages
// overlap, but not below the batch size the lane-per-site kernel needs to fill the chip.
int64_t chunk_for(const famseq_ctx *c, int64_t n_sites, size_t row) {
  int64_t chunk = c->chunk_sites;
  if (chunk <= 0) {
    chunk = std::max<int64_t>(1, (int64_t(64) << 20) / int64_t(row));
    chunk = std::min(chunk, std::max<int64_t>(c->lane_min_sites, (n_sites + 3) / 4));
  }
  return std::min(chunk, n_sites);
}

// Make every buffer b of the set hold `sites` sites of want[b] bytes each (0: not needed by this call).
int reserve(famseq_ctx *c, SlotSet &t, int64_t sites, const size_t (&want)[B_COUNT]) {
  bool fits = t.sites >= sites;
  for (int b = 0; b < B_COUNT; ++b) fits = fits && t.row[b] >= want[b];
  if (fits) return 0;
  const int64_t cap = std::max(sites, t.sites);
  t.release();
  for (int b = 0; b < B_COUNT; ++b) t.row[b] = std::max(t.row[b], want[b]);
  for (int s = 0; s < kSlots; ++s)
    for (int b = 0; b < B_COUNT; ++b)
      if (t.row[b]) HIP_TRY(c, t.buf[s][b].alloc(size_t(cap) * t.row[b]));
  t.sites = cap;
  return 0;
}

int run_chunks(famseq_ctx *c, SlotSet &t, const ChunkJob &job, const Stage &stage) {
  hipStream_t s_in = c->stream[0], s_k = c->stream[1], s_out = c->stream[2];
  int k = 0;
  for (int64_t lo = 0; lo < job.n_sites; lo += job.chunk, ++k) {
    const int s = k % kSlots;
    const int64_t n = std::min(job.chunk, job.n_sites - lo);
    // copy in: the slot is free once the chunk that used it last has been copied out
    if (k >= kSlots) HIP_TRY(c, hipStreamWaitEvent(s_in, c->ev_out[s], 0));
    for (int i = 0; i < job.n_in; ++i) {
      const Staged &a = job.in[i];
      HIP_TRY(c, hipMemcpyAsync(t.buf[s][a.buf].p, a.host + lo * a.row, n * a.row, hipMemcpyHostToDevice, s_in));
    }
    HIP_TRY(c, hipEventRecord(c->ev_in[s], s_in));
    // compute
    HIP_TRY(c, hipStreamWaitEvent(s_k, c->ev_in[s], 0));
    const int rc = stage(s, n, s_k, lo);
    if (rc != 0) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_done[s], s_k));
    // copy out
    HIP_TRY(c, hipStreamWaitEvent(s_out, c->ev_done[s], 0));
    for (int i = 0; i < job.n_out; ++i) {
      const Staged &a = job.out[i];
      HIP_TRY(c, hipMemcpyAsync(a.host + lo * a.row, t.buf[s][a.buf].p, n * a.row, hipMemcpyDeviceToHost, s_out));
    }
    HIP_TRY(c, hipEventRecord(c->ev_out[s], s_out));
  }
  return 0;
}

// The chunk loop of every host-buffer entry point.  Once it has started, copies into the caller's buffers may be in
// flight: an error does not return before all three streams have drained.
int run_pipeline(famseq_ctx *c, SlotSet &t, const ChunkJob &job, const Stage &stage) {
  const int rc = run_chunks(c, t, job, stage);
  for (int s = 0; s < kStages; ++s) {
    const hipError_t e = hipStreamSynchronize(c->stream[s]);
    if (e != hipSuccess && rc == 0) return fail(c, FAMSEQ_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  }
  return rc;
}

}  // namespace

int upload_lut(famseq_ctx *c) {
  if (c->d_lut) return 0;
  std::vector<double> lut(kPlLutSize);  // pow(10,-k/10) through the host's libm, as file.cpp:589 computes it
  for (int k = 0; k < kPlLutSize; ++k) lut[k] = std::pow(10.0, -std::fabs(double(k)) / 10.0);
  HIP_TRY(c, c->d_lut.alloc(lut.size() * sizeof(double)));
  HIP_TRY(c, hipMemcpy(c->d_lut.p, lut.data(), lut.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

CallIO make_call_io(const famseq_ctx *c, const uint16_t *d_pl, double *d_gpp, double *d_fpp, int8_t *d_fgt, int32_t n_seq,
                    unsigned long long *d_phase_clk) {
  CallIO cio;
  cio.pl = d_pl;
  cio.lut = c->d_lut.as<double>();
  cio.col = c->d_col.as<int32_t>();
  cio.slot = c->d_slot.as<int32_t>();
  cio.gpp = d_gpp, cio.fpp = d_fpp, cio.fgt = d_fgt;
  cio.n_seq = n_seq;
  // e / d for e < 2^16, d <= 60 as the high word of e * (2^32 / d + 1): exact (io_kernels.hip)
  cio.magic_w = 0xFFFFFFFFu / uint32_t(3 * n_seq) + 1;
  cio.magic_n = n_seq > 1 ? 0xFFFFFFFFu / uint32_t(n_seq) + 1 : 0;  // one column: the kernel divides by 1 itself
  cio.phase_clk = d_phase_clk;
  return cio;
}

// The posterior and call entries: per chunk the fused call-path launch, or [unpack] -> posterior kernel -> [Phred / call]
// -> [text].  With io.prior (famseq_bn_prior_batch, famseq_bn_prior_call_batch) the posterior kernel is the site-prior one.
int run_host(famseq_ctx *c, int64_t n_sites, const HostIO &io, int n_seq) {
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, "context was created without a device; there is no CPU path");
  if (n_sites == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const int N = c->model.n_members;
  const size_t row = size_t(3) * N * sizeof(double), seq = (io.pl16 || io.gpp || io.fpp || io.fgt || io.text) ? std::max(n_seq, 1) : 0;
  const size_t call_row = 3 * seq * sizeof(double);
  const bool called = io.gpp || io.fpp || io.fgt || io.text;
  ChunkJob job;
  job.n_sites = n_sites;
  job.chunk = chunk_for(c, n_sites, row);
  SlotSet &t = c->slots;
  const size_t prior_row = io.prior ? 6 * sizeof(double) : 0;
  const size_t want[B_COUNT] = {row, 1, 1, seq * 3 * sizeof(uint16_t), row, row, call_row, call_row, seq, seq * size_t(kTextStride), prior_row};
  int rc = reserve(c, t, job.chunk, want);
  if (rc != 0) return rc;
  if (io.pl16 && (rc = upload_lut(c)) != 0) return rc;
  if (called) {
    // The generated kernels' call-path arguments (struct fs_call_args) depend on the slot only, not on the
    // chunk: written once per call, synchronously (nothing of an earlier call is in flight any more), so
    // that no asynchronous copy ever reads host memory that has gone out of scope.
    if (std::getenv("FAMSEQ_PHASE_CLOCK")) {
      if (!c->d_phase) HIP_TRY(c, c->d_phase.alloc(kPhases * sizeof(unsigned long long)));
      HIP_TRY(c, hipMemset(c->d_phase.p, 0, kPhases * sizeof(unsigned long long)));
    }
    for (int s = 0; s < kSlots; ++s) {
      const bool text = io.text != nullptr;
      const CallIO cio = make_call_io(c, io.pl16 ? t.buf[s][B_PL].as<uint16_t>() : nullptr, io.gpp || text ? t.buf[s][B_GPP].as<double>() : nullptr,
                                      io.fpp || text ? t.buf[s][B_FPP].as<double>() : nullptr, io.fgt || text ? t.buf[s][B_FGT].as<int8_t>() : nullptr,
                                      n_seq, std::getenv("FAMSEQ_PHASE_CLOCK") ? c->d_phase.as<unsigned long long>() : nullptr);
      if (!c->d_call[s]) HIP_TRY(c, c->d_call[s].alloc(sizeof(CallIO)));
      HIP_TRY(c, hipMemcpy(c->d_call[s].p, &cio, sizeof cio, hipMemcpyHostToDevice));
    }
  }
  job.copy_in(B_PL, size_t(n_seq) * 3 * sizeof(uint16_t), io.pl16);
  if (!io.pl16) job.copy_in(B_LK, row, io.lk);
  job.copy_in(B_FLAGS, 1, io.flags);
  job.copy_in(B_PRIOR, prior_row, io.prior);  // a chunk's 48 n bytes travel with its likelihoods
  const size_t cr = size_t(3) * n_seq * sizeof(double);
  job.copy_out(B_GPP, cr, io.gpp);
  job.copy_out(B_FPP, cr, io.fpp);
  job.copy_out(B_FGT, size_t(n_seq), io.fgt);
  job.copy_out(B_TEXT, size_t(n_seq) * kTextStride, io.text);
  job.copy_out(B_POST, row, io.post);
  job.copy_out(B_SINGLE, row, io.single);
  job.copy_out(B_STATUS, 1, io.status);
  rc = run_pipeline(c, t, job, [&](int s, int64_t n, hipStream_t s_k, int64_t) -> int {
    DevBuf *d = t.buf[s];
    const double *d_prior = d[B_PRIOR].as<double>();
    double *d_lk = d[B_LK].as<double>(), *d_post = d[B_POST].as<double>(), *d_single = d[B_SINGLE].as<double>();
    double *d_gpp = d[B_GPP].as<double>(), *d_fpp = d[B_FPP].as<double>();
    const uint8_t *d_flags = io.flags ? d[B_FLAGS].as<uint8_t>() : nullptr;
    uint8_t *d_status = io.status || called ? d[B_STATUS].as<uint8_t>() : nullptr;
    const bool need_single = io.single || io.gpp || io.text;
    bool fused = false;
    // site priors: the sum-product kernel of that form, whatever the engine (the entry has loaded it), between the separate
    // stages; there is no fused call-path form of it
    if (called && !io.post && !io.single && !io.prior) {
      hipError_t e = hipSuccess;
      fused = launch_engine_fused(c, n, io.pl16 ? nullptr : d_lk, d_flags, d_status, io.pl16 != nullptr, c->d_call[s].as<CallIO>(), s_k, &e);
      if (fused) HIP_TRY(c, e);
    }
    if (!fused) {
      if (io.pl16)
        HIP_TRY(c, launch_unpack_pl16(d[B_PL].as<uint16_t>(), c->d_col.as<int32_t>(), c->d_lut.as<double>(), N, n_seq, n, d_lk, s_k));
      if (io.prior)
        HIP_TRY(c, launch_generated(c, c->kern[K_PRIOR], n, d_lk, d_flags, d_post, need_single ? d_single : nullptr, d_status, s_k, 0,
                                    {&d_prior}));
      else
        HIP_TRY(c, launch_engine(c, n, d_lk, d_flags, d_post, need_single ? d_single : nullptr, d_status, s_k, n_sites));
      if (called)
        HIP_TRY(c, launch_phred_call(d_post, d_single, d_status, c->d_seq.as<int32_t>(), N, n_seq, n, d_gpp, d_fpp, d[B_FGT].as<int8_t>(), s_k));
    }
    // the called outputs as text, while they are in HBM anyway: one record per (site, sample) pair
    if (io.text) HIP_TRY(c, launch_text_call(d_gpp, d_fpp, d[B_FGT].as<int8_t>(), n * n_seq, d[B_TEXT].as<char>(), s_k));
    return 0;
  });
  if (called && c->d_phase && rc == 0) {  // measuring aid: where the call-path kernel's waves spend their cycles
    unsigned long long ph[kPhases];
    HIP_TRY(c, hipMemcpy(ph, c->d_phase.p, sizeof ph, hipMemcpyDeviceToHost));
    unsigned long long tot = 0;
    for (int i = 0; i < kPhases; ++i) tot += ph[i];
    std::fprintf(stderr, "famseq phase clock (wave cycles, %lld sites):", (long long)n_sites);
    for (int i = 0; i < kPhases; ++i) std::fprintf(stderr, " [%d] %.1f%%", i, tot ? 100.0 * double(ph[i]) / double(tot) : 0.0);
    std::fprintf(stderr, "  total %llu\n", tot);
  }
  return rc;
}

// ... and every side product's host entries (side_table(); plain and site-prior): per chunk [unpack] -> kernel, on the product's own
// set of slots.  out_a / out_b: the two per-site outputs (NULL: not wanted), a_row / b_row their bytes per site (0: the pedigree
// has none).  What a product's kernel takes beside the common arguments arrives as `lead`, made by the caller; `per` names the
// arguments a chunk gets its own value of: the device copy of what is staged with the chunk in B_PRIOR, and site_base.
int side_batch(famseq_ctx *c, SlotSet &t, const GenKernel &g, int64_t n_sites, const double *lk, const uint16_t *pl16, int32_t n_seq,
               const uint8_t *flags, void *out_a, size_t a_row, void *out_b, size_t b_row, uint8_t *status, const MoreArgs &lead,
               const PerChunk &per) {
  const int N = c->model.n_members;
  const size_t row = size_t(3) * N * sizeof(double), pl_row = pl16 ? size_t(n_seq) * 3 * sizeof(uint16_t) : 0;
  const size_t staged_row = per.staged ? per.row : 0;
  ChunkJob job;
  job.n_sites = n_sites;
  job.chunk = chunk_for(c, n_sites, std::max(row, a_row + 1));
  size_t want[B_COUNT] = {};
  want[B_LK] = row, want[B_FLAGS] = want[B_STATUS] = 1, want[B_PL] = pl_row, want[B_OUT_A] = a_row, want[B_OUT_B] = b_row;
  want[B_PRIOR] = staged_row;
  const int rc = reserve(c, t, job.chunk, want);
  if (rc != 0) return rc;
  job.copy_in(B_PL, pl_row, pl16);
  if (!pl16) job.copy_in(B_LK, row, lk);
  job.copy_in(B_FLAGS, 1, flags);
  job.copy_in(B_PRIOR, staged_row, per.staged);
  job.copy_out(B_OUT_A, a_row, out_a);
  job.copy_out(B_OUT_B, b_row, out_b);
  job.copy_out(B_STATUS, 1, status);
  return run_pipeline(c, t, job, [&](int s, int64_t n, hipStream_t s_k, int64_t lo) -> int {
    DevBuf *d = t.buf[s];
    if (pl16)
      HIP_TRY(c, launch_unpack_pl16(d[B_PL].as<uint16_t>(), c->d_col.as<int32_t>(), c->d_lut.as<double>(), N, n_seq, n, d[B_LK].as<double>(), s_k));
    const void *d_staged = per.staged ? d[B_PRIOR].p : nullptr;
    MoreArgs more = lead;
    const long chunk_base = long(per.site_base + lo);  // (read when the launch is enqueued)
    if (per.base_at >= 0) more.at[per.base_at] = const_cast<long *>(&chunk_base);
    if (per.at >= 0) more.at[per.at] = &d_staged;
    else more.add(&d_staged);  // (behind the last parameter of a plain form: not read)
    HIP_TRY(c, launch_generated(c, g, n, d[B_LK].as<double>(), flags ? d[B_FLAGS].as<uint8_t>() : nullptr, out_a ? d[B_OUT_A].p : nullptr,
                                out_b ? d[B_OUT_B].p : nullptr, status ? d[B_STATUS].as<uint8_t>() : nullptr, s_k, 0, more));
    return 0;
  });
}

}  // namespace famseq
