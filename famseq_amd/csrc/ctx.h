// ctx.h — what the host translation units of libfamseq_hip.so share: the context behind the C ABI, the record of a
// generated kernel, the device buffers a context owns and the table of the side products (SideProduct: their kernels, and what
// their entries take beside the common arguments).  capi.cpp is the extern "C" surface and its argument checks, kernels.cpp
// holds side_table() and loads, launches and tunes the generated kernels, pipeline.cpp moves host batches through the device.
#ifndef FAMSEQ_CTX_H_
#define FAMSEQ_CTX_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "bn_kernel.h"
#include "enum_codegen.h"
#include "famseq_hip.h"
#include "jit.h"
#include "plan.h"

// The fused call path's side of a generated kernel's argument list (kCallArgs): packed PLs in, GPP / FPP /
// FGT out.  All null on the plain path.
struct CallIO {  // = struct fs_call_args of the generated source (kernel_shell.cpp kCallHelpers)
  const uint16_t *pl = nullptr;
  const double *lut = nullptr;
  const int32_t *col = nullptr, *slot = nullptr;
  double *gpp = nullptr, *fpp = nullptr;
  int8_t *fgt = nullptr;
  int32_t n_seq = 0;
  uint32_t magic_w = 0, magic_n = 0;
  unsigned long long *phase_clk = nullptr;  // FAMSEQ_PHASE_CLOCK (measuring aid): cycles per phase of the call-path kernel, summed over waves
};
constexpr int kPhases = 8;

namespace famseq {

// Device memory with an owner: freed when the owner goes, or when it is asked for again at another size.
struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  hipError_t alloc(size_t bytes) {
    release();
    return hipMalloc(&p, bytes);
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
  explicit operator bool() const { return p != nullptr; }
};

// A generated (per-pedigree) kernel a context may hold.  The kinds, and how each is made: kernel_spec in kernels.cpp; the side
// products' kinds (K_TRIO .. K_CHARFN_PRIOR) are the rows of side_table() below.
enum KernelKind {
  K_LANE = 0,  // K_LANE + d: the enumeration with 3^d lanes per site; d = 0 (one lane per site) serves large batches,
               // d = 1..kEnumMaxGroupDigits batches too small to give every lane of the chip a site (compiled on first use of each d)
  K_LANE_CALL = K_LANE + kEnumMaxGroupDigits + 1,  // the fused call-path form of the one-lane-per-site kernel (famseq_bn_call_batch)
  K_ELIM,                                          // sum-product kernel (engine = FAMSEQ_ENGINE_ELIM)
  K_ELIM_CALL,                                     // ... and its call-path form
  K_TRIO,                                          // K_TRIO + form - 1: trio posteriors per output form (1 dnm, 2 joint, 3 both)
  K_MAP = K_TRIO + 3,                              // the joint MAP configuration
  K_PRIOR,                                         // the sum-product kernel with the founders' prior per site (famseq_bn_prior_batch)
  K_TRIO_PRIOR,                                    // K_TRIO_PRIOR + form - 1: the trio kernels with the founders' prior per site
  K_MAP_PRIOR = K_TRIO_PRIOR + 3,                  // ... and the MAP kernel
  K_EVID,                                          // the evidence: log10 likelihood of the site and the hom-ref posterior
  K_EVID_PRIOR,                                    // ... with the founders' prior per site
  K_LOO,                                           // leave-one-out posteriors and the per-member fit
  K_LOO_PRIOR,                                     // ... with the founders' prior per site
  K_PATTERN,                                       // genotype-pattern posteriors: the sum pass once per pattern
  K_PATTERN_PRIOR,                                 // ... with the founders' prior per site
  K_SAMPLE,                                        // exact joint posterior draws
  K_SAMPLE_PRIOR,                                  // ... with the founders' prior per site
  K_AF,                                            // the founders' allele frequency by maximum likelihood (no site-prior form)
  K_RELABEL,                                       // relabelling evidence: the sum pass once per assignment of rows to members
  K_RELABEL_PRIOR,                                 // ... with the founders' prior per site
  K_MUTRATE,                                       // mutation-rate likelihood profile: the sum pass once per transmission table
  K_MUTRATE_PRIOR,                                 // ... with the founders' prior per site
  K_ORIGIN,                                        // phase by transmission: each child's alleles by parent of origin
  K_ORIGIN_PRIOR,                                  // ... with the founders' prior per site
  K_WEIGHT,                                        // per-member genotype weights: the sum pass once per weight table
  K_WEIGHT_PRIOR,                                  // ... with the founders' prior per site
  K_MAXMARG,                                       // max-marginals and the runner-up: the max pass in both directions
  K_MAXMARG_PRIOR,                                 // ... with the founders' prior per site
  K_CHARFN,                                        // count characteristic function: the real sum pass, then a complex one per weight table
  K_CHARFN_PRIOR,                                  // ... with the founders' prior per site
  K_LANE_BULK,  // the one-lane-per-site enumeration in the outer-leaf plan (lane variant 8 + K_LANE's block shape and fencing): serves
                // large batches where that text differs from K_LANE's (kernels.cpp, bulk_serves); no pick, no contest of its own
  K_COUNT
};

struct GenKernel {
  JitKernel k;  // on a plan-only context (device < 0) only the path of the compiled code object
  int block_threads = 0, blocks_per_cu = 0;
  int variant = -1;  // which generator variant the tuner's note or jit_pick_variant took
  // the lane kinds and the call-path forms remember that they could not be built (no compiler at run time, ...) and say
  // so once; each keeps its own verdict: a call-path form that does not build must not take the plain kernels down with
  // it, nor the other way round.  (The lanes-per-site kinds leave their message with K_LANE, which keeps its own in preference.)
  bool failed = false;
  std::string error;
  void drop() {  // unloaded and forgotten: the next use generates it again
    jit_unload(k);
    k.path.clear();
    variant = -1;
  }
};

constexpr int kSlots = 2;
constexpr int kStages = 3;
constexpr int kStageRing = 16;  // pinned staging slots of the device entries' small uploads (famseq_ctx::stage_mem)

// The device side of the chunked host pipeline: kSlots copies of every array a chunk passes through.  A set only grows
// (in sites and in bytes per site), so that varying batch sizes do not thrash.
enum SlotBuf { B_LK, B_FLAGS, B_STATUS, B_PL, B_POST, B_SINGLE, B_GPP, B_FPP, B_FGT, B_TEXT, B_PRIOR, B_COUNT,
               B_OUT_A = B_POST, B_OUT_B = B_SINGLE };  // (the side products' two outputs)
struct SlotSet {
  DevBuf buf[kSlots][B_COUNT];
  size_t row[B_COUNT] = {};  // bytes per site of each buffer (0: not allocated)
  int64_t sites = 0;
  void release() {
    for (auto &slot : buf)
      for (DevBuf &b : slot) b.release();
    sites = 0;
  }
};

// What a side entry takes beside the common arguments: at most one table and one count, and the sampling entries' seed and
// site_base.  What each of them is for a product, how it is checked and how it reaches the kernel: the product's ExtraSpec.
struct SideExtra {
  const void *table = nullptr;  // host entries: the caller's host array; device entries: resident
  int32_t count = 1;
  uint64_t seed = 0;
  int64_t site_base = 0;  // the absolute index of the call's first site
  SideExtra() = default;
  SideExtra(const void *table_, int32_t count_) : table(table_), count(count_) {}
  SideExtra(uint64_t seed_, int64_t site_base_, int32_t n_draws) : count(n_draws), seed(seed_), site_base(site_base_) {}
};
// How a host entry's table reaches the device (a device entry's is resident):
enum ExtraVia {
  X_NONE,   // no table: the entries take nothing beside, or scalars only (ExtraSpec::params)
  X_CALL,   // one table per call: staged at its size from the context's copy into a buffer allocated once at the largest count
  X_SITE,   // one element per site: staged chunk by chunk where the site-prior forms stage their rows
  X_CONST,  // no table of the caller's: rows made from the context's model, uploaded on their first use and never changed
};
// The argument side of a product: one column of side_table().  Plain data and functions; the generic code is capi.cpp's
// check_extra, stage_extra and side_entry.
struct ExtraSpec {
  ExtraVia via = X_NONE;
  // the kernel's parameters between the common ones and the prior rows, in order: 't' the table, 'n' the count, 's' the seed,
  // 'b' site_base (a host entry's chunks: plus the chunk's first index)
  const char *params = "";
  // the count: "<count> must be <lo>..<hi>, got <v>" (NULL: the entries take none)
  const char *count = nullptr;
  int lo = 1, hi = 1;
  // the table: "<name> must be given (<given>)" (name NULL: none to give)
  const char *name = nullptr, *given = nullptr;
  // host entries: the first value of the table that is out of range (fail()'s code), or 0
  int (*check)(famseq_ctx *, const void *table, int32_t count, int64_t n_sites) = nullptr;
  // X_CALL: bytes of the device table per count; X_SITE: per site; X_CONST: in all
  size_t (*bytes)(const Model &) = nullptr;
  // X_CALL, X_CONST: fills the context's copy of the device table (NULL: the caller's table as it is)
  void (*build)(const famseq_ctx *, const void *table, int32_t count, void *staged) = nullptr;
  // where the device entries call the table otherwise, or say otherwise what is to be given
  const char *device_name = nullptr, *device_given = nullptr;
  // asked of the context before anything else, whatever the arguments (the origin kernels' origin_model)
  int (*precondition)(famseq_ctx *) = nullptr;
};

// A side product of the sum-product engine: a generated kernel that takes the common argument list and writes two outputs per
// site and a status byte, in a plain form and in one that reads the founders' prior per site.  Everything its ABI entries, its
// prebuild options, its plan keys and its loader differ in is one row of side_table() (kernels.cpp).
enum SideId { SIDE_TRIO, SIDE_MAP, SIDE_EVID, SIDE_LOO, SIDE_PATTERN, SIDE_SAMPLE, SIDE_AF, SIDE_RELABEL, SIDE_MUTRATE, SIDE_ORIGIN, SIDE_WEIGHT, SIDE_MAXMARG, SIDE_CHARFN, SIDE_COUNT };  // (also the index of its staging buffers, famseq_ctx::side_slots)
struct SideProduct {
  const char *stem;   // "trio": the entry points famseq_trio[_prior], the options trio[_prior]_kernels, the plan keys trio[_prior]_*
  const char *what;   // load_or_fail's message starts "[site priors, ]<what> (sum-product engine): "
  const char *takes;  // the values of its prebuild options, as their refusal names them
  int kind, prior_kind, n_forms;  // output form f = 1 .. n_forms is kind + f - 1, its site-prior form prior_kind + f - 1
                                  // (prior_kind < 0: the product has no site-prior form — no <stem>_prior_* name exists anywhere)
  int n_variants;
  std::string (*source)(const Model &, int variant, int form, bool site_prior);
  // bytes per site of the two outputs; count: the call's SideExtra::count (1 where the entries take none), for the rows that read it
  void (*rows)(const Model &, int count, size_t row[2]);
  ExtraSpec extra;
  int kind_of(int form, bool site_prior) const { return (site_prior ? prior_kind : kind) + form - 1; }
  bool has_prior() const { return prior_kind >= 0; }
};
using SideTable = const SideProduct[SIDE_COUNT];
SideTable &side_table();

}  // namespace famseq

struct famseq_ctx {
  famseq::Model model;
  bool big = false;  // more than FAMSEQ_MAX_MEMBERS members: no enumeration plan, sum-product engine only
  famseq::PlanOptions opt{};
  famseq::Plan plan{};
  famseq::KParams kp{};
  bool plan_dirty = true;
  int device = -1;
  int n_cus = 0;
  int blocks_per_cu = 0;
  int64_t grid_override = 0;
  int64_t chunk_sites = 0;
  int engine = FAMSEQ_ENGINE_ENUM;
  famseq::GenKernel kern[famseq::K_COUNT];
  famseq::GenKernel &lanes(int d) { return kern[famseq::K_LANE + d]; }
  bool plan_only() const { return device < 0; }
  // enumeration engine: the team-per-site kernel is compiled into the library; the lane kernels are generated per
  // pedigree.  enum_impl: -1 auto (lane for large batches), 0 team, 1 lane.  group_digits: -1 auto (by batch size), 0..4 forced.
  int enum_impl = -1;
  int group_digits = -1, last_group_digits = 0;
  // The bulk slot (K_LANE_BULK): a one-lane-per-site launch of a context that is free to choose (enum_impl < 0, group_digits < 0)
  // goes to it from bulk_min_sites sites on.  -2: the default, sixteen chunks per resident wave (16 x 64 x CUs x 4: below that a
  // launch is under 2.5 ms on MI355X, and a second module load and a second set of last bits are not worth it); -1: the slot is off.
  int64_t bulk_min_sites = -2;
  int bulk_any = -1;                // does the pedigree have the form at all, in either block shape (worked out once per context)
  int bulk_differs = -1;            // does variant 8 + b differ from K_LANE's 4 + b (unknown until K_LANE has its variant)
  const char *last_kind = "";       // which enumeration kernel served the last launch: "team", "group", "lane", "bulk"
  int lane_first = -1;  // where the lane kernel's variant contest starts (lane_first_variant(): worked out once per context)
  int lane_reads_rows = -1;  // does the lane call-path kernel re-read fp64 rows from global memory (unknown until it is built)
  int trio_last = 0;         // the trio output form asked for last (famseq_plan_json)
  int trio_prior_last = 0;   // ... and of the site-prior trio kernels
  int64_t lane_min_sites = 256;  // below this the compiled-in team kernel answers at once (no per-pedigree compile for tiny calls) ...
  // ... unless the generated kernel for that batch is loaded or on disk already (a pre-built pedigree, or one this user has run
  // before): then nothing has to be waited for and it serves every batch size (team kernel: 0.0237 ms per 256 ten-member
  // sites, three lanes ... 81 lanes per site: 0.0159).  -1 unknown, 0 would have to be compiled, 1 ready.
  int grp_ready[famseq::kEnumMaxGroupDigits + 1] = {-1, -1, -1, -1, -1};
  // device constants: plan image, factor tables, pow(10, -k/10); column -> member, member -> column or -1, member -> output slot
  famseq::DevBuf d_img, d_tc, d_lut, d_seq, d_col, d_slot;
  std::vector<int32_t> seq_members;
  // the host-buffer entry points: a three-stage pipeline (copy in / compute / copy out, one stream each, so both
  // directions of the host link run at once) over two buffer slots; the posterior and call entries and every side
  // product have their set (their outputs differ in size by an order of magnitude)
  hipStream_t stream[famseq::kStages] = {nullptr, nullptr, nullptr};  // 0 copy in, 1 compute, 2 copy out
  hipEvent_t ev_in[famseq::kSlots] = {}, ev_done[famseq::kSlots] = {}, ev_out[famseq::kSlots] = {};
  famseq::SlotSet slots, side_slots[famseq::SIDE_COUNT];
  famseq::DevBuf d_call[famseq::kSlots];  // the generated kernels' call-path arguments (CallIO), one per slot
  famseq::DevBuf d_phase;                 // FAMSEQ_PHASE_CLOCK: kPhases counters
  // device-resident call path (famseq_bn_call_batch_device): its own argument block, what it holds, and scratch rows for
  // batches the fused kernels do not serve (separate unpack / posterior / Phred stages)
  famseq::DevBuf d_call_dev;
  CallIO call_dev_host{};
  bool call_dev_valid = false;
  famseq::DevBuf dev_tmp[7];  // lk, post, single, gpp, fpp, fgt, status
  int64_t dev_tmp_sites = 0;
  int dev_tmp_seq = 0;
  famseq::DevBuf trio_dev_lk;  // the side products' device entries' likelihood rows for packed input
  // What the device entries share across calls — the column maps, d_call_dev, dev_tmp, trio_dev_lk — is used in the order the
  // calls are issued, whatever streams they are on: state_stream is the stream of the last device-entry call that touches any
  // of it; such a call on another stream records ev_state on state_stream and waits for it, a host entry and a growth of the
  // scratch wait for state_stream on the host.  Every such call is behind its predecessor that way, so the last stream stands
  // for all of them, and calls that stay on one stream record and wait for nothing.  The entries that use none of that state
  // (famseq_bn_batch_device, famseq_bn_prior_batch_device, the side entries on d_lk) take no part.
  hipEvent_t ev_state = nullptr;
  hipStream_t state_stream = nullptr;
  bool state_used = false;
  // The maps and the argument block reach the device on the caller's stream, from pinned memory (an asynchronous copy from
  // pageable memory waits for the stream): a ring of kStageRing slots of stage_bytes each, a slot written again only after the
  // copy out of it has run (ev_stage, recorded behind that copy; stage_used: it has been).
  char *stage_mem = nullptr;
  size_t stage_bytes = 0;
  hipEvent_t ev_stage[famseq::kStageRing] = {};
  bool stage_used[famseq::kStageRing] = {};
  int stage_next = 0;
  // a product's device table (ExtraSpec::via X_CALL: the host entries' masks, assignments, factor tables or weights, allocated
  // once at the largest count and staged per call on the compute stream; X_CONST: the origin kernels' allele rows) and the copy
  // of it the context keeps, which outlives the asynchronous copy out of it
  famseq::DevBuf d_extra[famseq::SIDE_COUNT];
  std::vector<uint8_t> extra_host[famseq::SIDE_COUNT];
  // the mutation rate the origin kernels' allele rows are made for, recovered from the model's tables (origin_state: 0 not
  // looked at, 1 found, -1 the tables are nobody's famseq_transmission_tables: no allele-level model)
  double origin_mrate = 0;
  int origin_state = 0;
  int64_t trio_dev_sites = 0;
  std::string tune_report;  // what famseq_set_option "tune" measured (famseq_plan_json "tune")
  std::string err, json;
};

namespace famseq {

inline int fail(famseq_ctx *c, int code, const std::string &msg) {
  c->err = msg;
  return code;
}

#define HIP_TRY(c, call)                                                                              \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return famseq::fail((c), FAMSEQ_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
  } while (0)

// What a generated kernel takes behind the common eight arguments, in the order of its parameter list: the address of each
// argument's value (hipModuleLaunchKernel's form).  The call-path forms take their CallIO, the site-prior kernels their prior
// rows, a side product's kernels what its ExtraSpec::params names in front of those; the plain forms nothing.
struct MoreArgs {
  static constexpr int kMax = 4;
  void *at[kMax] = {};
  int n = 0;
  MoreArgs() = default;
  MoreArgs(std::initializer_list<const void *> list) {
    for (const void *a : list) add(a);
  }
  void add(const void *a) { at[n++] = const_cast<void *>(a); }
};

// ---- kernels.cpp ----
// The sum-product family (K_ELIM, K_PRIOR and every kind of side_table()): 0, or an error (FAMSEQ_E_ARG: the engine does not serve
// this pedigree; FAMSEQ_E_HIP) that is not remembered, the next call tries again.
int load_or_fail(famseq_ctx *c, int kind);
// The mutation-rate entries' tables (famseq_rate_tables' blocks): the model's factor table rebuilt with the transmission tables
// of each rate.
void rate_tables(const Model &m, const double *rates, int32_t n_rates, double *tables);
// The origin kernels' precondition: the model's three transmission tables are, bit for bit, famseq_transmission_tables(mu) for
// mu = pcp2Xm[18] (c->origin_mrate).  0, or FAMSEQ_E_ARG with its message; asks nothing of a device.
int origin_model(famseq_ctx *c);
// 0, or FAMSEQ_E_ARG with the engine's message where it does not serve the context's pedigree: the characteristic-function
// entries' ExtraSpec::precondition, which says so before the device is asked for
int charfn_served(famseq_ctx *c);
// ... the same question of a model alone: true and the rate in *mu, or false; changes nothing
bool origin_rate(const Model &m, double *mu);
// The lane kinds and both call-path forms: false when the kernel is unavailable, which is remembered and said once on
// stderr; the caller falls back (team kernel, separate stages).
bool load_or_remember(famseq_ctx *c, int kind);
void drop_lane_kernels(famseq_ctx *c);  // what a new pick of the lane variant makes stale
int lane_first_variant(const famseq_ctx *c);  // 4 where the lane kernel has the once-per-site form (variants 4-7), else 0
hipError_t launch_generated(famseq_ctx *c, const GenKernel &g, int64_t n_sites, const double *d_lk, const uint8_t *d_flags, void *d_out_a,
                            void *d_out_b, uint8_t *d_status, hipStream_t stream, int sites_per_chunk = 0, const MoreArgs &more = {});
// call_sites: the size of the host call this launch is a chunk of (0: the launch is the call).  Whether the bulk slot serves is
// decided from it, so that every chunk of a call goes the same way and equal calls give equal bits, resident or staged.
hipError_t launch_engine(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint8_t *d_flags, double *d_post, double *d_single,
                         uint8_t *d_status, hipStream_t stream, int64_t call_sites = 0);
int64_t bulk_min_sites(const famseq_ctx *c);  // the threshold in force (-1: off)
void bulk_prebuild(famseq_ctx *c);            // a plan-only context that holds K_LANE compiles the bulk object too, where the pedigree has one
bool call_fuses(famseq_ctx *c, int64_t n_sites, bool packed_in);
bool launch_engine_fused(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint8_t *d_flags, uint8_t *d_status, bool packed_in,
                         const CallIO *d_io, hipStream_t stream, hipError_t *err);
int tune(famseq_ctx *c);
void report_phase_clock(famseq_ctx *c);

// ---- pipeline.cpp ----
struct HostIO {
  const double *lk = nullptr;      // exactly one of lk / pl16
  const uint16_t *pl16 = nullptr;  // [n_sites][n_seq][3]
  const uint8_t *flags = nullptr;
  const double *prior = nullptr;  // [n_sites][6]: the founders' prior per site (famseq_bn_prior_batch); the sum-product kernel K_PRIOR
  double *post = nullptr, *single = nullptr;  // raw outputs [n_sites][N][3]
  uint8_t *status = nullptr;
  double *gpp = nullptr, *fpp = nullptr;  // called outputs [n_sites][n_seq][3]
  int8_t *fgt = nullptr;                  // [n_sites][n_seq]
  char *text = nullptr;                   // the same three as printed: [n_sites][n_seq][FAMSEQ_TEXT_STRIDE]
};
int upload_lut(famseq_ctx *c);
CallIO make_call_io(const famseq_ctx *c, const uint16_t *d_pl, double *d_gpp, double *d_fpp, int8_t *d_fgt, int32_t n_seq,
                    unsigned long long *d_phase_clk = nullptr);
int run_host(famseq_ctx *c, int64_t n_sites, const HostIO &io, int n_seq);
// Which of a side kernel's trailing arguments differ from chunk to chunk of a host call.
struct PerChunk {
  // a host array with `row` bytes per site, staged chunk by chunk alongside the likelihoods (NULL: none): the site-prior forms'
  // rows, or a product's per-site table (ExtraSpec::via X_SITE).  The chunk's device copy is argument `at` of lead, or, at < 0,
  // one more argument behind lead (where the prior rows stand; NULL for a plain form, which does not read it).
  const void *staged = nullptr;
  size_t row = 0;
  int at = -1;
  // base_at >= 0: argument base_at of lead is site_base + the index of the chunk's first site in the call
  int base_at = -1;
  int64_t site_base = 0;
};
// The side products' host entries: lk or packed PLs through kernel `g`, whose two outputs have a_row / b_row bytes per site.
// lead: what the kernel takes between the common arguments and the prior rows, the same for every chunk but for what `per` says.
int side_batch(famseq_ctx *c, SlotSet &t, const GenKernel &g, int64_t n_sites, const double *lk, const uint16_t *pl16, int32_t n_seq,
               const uint8_t *flags, void *out_a, size_t a_row, void *out_b, size_t b_row, uint8_t *status, const MoreArgs &lead = {},
               const PerChunk &per = {});

}  // namespace famseq
#endif
