// kernels.cpp — the generated (per-pedigree) kernels of a context: how each kind is made, the one loader, the launchers,
// which kernel serves which batch, and the tuner.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "bn_kernel.h"
#include "ctx.h"
#include "elim_codegen.h"

namespace famseq {

void rate_tables(const Model &m, const double *rates, int32_t n_rates, double *tables) {
  Model at = m;
  for (int32_t r = 0; r < n_rates; ++r) {
    famseq_transmission_tables(rates[r], at.pcp2, at.pcp2Xf, at.pcp2Xm);
    build_factor_tables(at, tables + size_t(r) * FAMSEQ_RATE_TABLE_DOUBLES);
  }
}

namespace {

// The side products' ExtraSpec::check: the first value of a host entry's table that is out of range.
int check_masks(famseq_ctx *c, const void *table, int32_t n_patterns, int64_t) {
  const uint8_t *masks = static_cast<const uint8_t *>(table);
  for (size_t i = 0, N = c->model.n_members, n = size_t(n_patterns) * N; i < n; ++i)
    if (masks[i] > 7)
      return fail(c, FAMSEQ_E_ARG, "masks: pattern " + std::to_string(i / N) + ", member " + std::to_string(i % N) + " is " +
                                       std::to_string(masks[i]) + "; a mask is 0..7 (bit g: genotype g allowed)");
  return 0;
}
int check_af0(famseq_ctx *c, const void *table, int32_t, int64_t n_sites) {
  const double *af0 = static_cast<const double *>(table);
  for (int64_t s = 0; s < n_sites; ++s)
    if (!(af0[s] >= 0.0 && af0[s] <= 1.0))
      return fail(c, FAMSEQ_E_ARG, "af0 entries must be finite numbers in [0, 1] (site " + std::to_string(s) + ")");
  return 0;
}
int check_assign(famseq_ctx *c, const void *table, int32_t n_assign, int64_t) {
  const int32_t *assign = static_cast<const int32_t *>(table);
  const int N = c->model.n_members;
  for (size_t i = 0, n = size_t(n_assign) * N; i < n; ++i)
    if (assign[i] < -1 || assign[i] >= N)
      return fail(c, FAMSEQ_E_ARG, "assign: assignment " + std::to_string(i / N) + ", member " + std::to_string(i % N) + " is " +
                                       std::to_string(assign[i]) + "; an entry is -1 (no data) or a member index 0.." + std::to_string(N - 1));
  return 0;
}
int check_rates(famseq_ctx *c, const void *table, int32_t n_rates, int64_t) {
  const double *rates = static_cast<const double *>(table);
  for (int32_t r = 0; r < n_rates; ++r)
    if (!(rates[r] >= 0.0 && rates[r] <= 1.0))
      return fail(c, FAMSEQ_E_ARG, "rates[" + std::to_string(r) + "] must be a finite number in [0, 1]");
  return 0;
}
int check_weights(famseq_ctx *c, const void *table, int32_t n_weights, int64_t) {
  const double *weights = static_cast<const double *>(table);
  const size_t N = c->model.n_members;
  for (size_t i = 0, n = size_t(n_weights) * 3 * N; i < n; ++i)
    if (!(weights[i] >= 0.0 && weights[i] <= 1.79769313486231570815e308)) {
      char v[40];
      std::snprintf(v, sizeof v, "%g", weights[i]);
      return fail(c, FAMSEQ_E_ARG, "a weight is a finite number >= 0: weight table " + std::to_string(i / (3 * N)) + ", member " +
                                       std::to_string(i / 3 % N) + ", genotype " + std::to_string(i % 3) + " is " + v);
    }
  return 0;
}
int check_cweights(famseq_ctx *c, const void *table, int32_t n_tables, int64_t) {
  const double *cw = static_cast<const double *>(table);
  const size_t N = c->model.n_members;
  for (size_t i = 0, n = size_t(n_tables) * 6 * N; i < n; ++i)
    if (!(cw[i] >= -1.79769313486231570815e308 && cw[i] <= 1.79769313486231570815e308)) {
      char v[40];
      std::snprintf(v, sizeof v, "%g", cw[i]);
      return fail(c, FAMSEQ_E_ARG, "a complex weight is a pair of finite numbers: weight table " + std::to_string(i / (6 * N)) + ", member " +
                                       std::to_string(i / 6 % N) + ", genotype " + std::to_string(i / 2 % 3) + ", " +
                                       (i % 2 ? "imaginary" : "real") + " part is " + v);
    }
  return 0;
}

#define FS_STR_(x) #x
#define FS_STR(x) FS_STR_(x)

}  // namespace

// The columns of a row: SideProduct and, the last, its ExtraSpec (ctx.h).
SideTable &side_table() {
  static SideTable table = {
      {"trio", "trio posteriors", "1 (dnm), 2 (joint) or 3 (both)", K_TRIO, K_TRIO_PRIOR, 3, kTrioVariants, trio_source,
       [](const Model &m, int, size_t row[2]) {  // joint[K][27], dnm[K]
         const size_t K = trio_children(m).size();
         row[0] = 27 * K * sizeof(double), row[1] = K * sizeof(double);
       }},
      {"map", "joint MAP call", "1", K_MAP, K_MAP_PRIOR, 1, kMapVariants,
       [](const Model &m, int v, int, bool site_prior) { return map_source(m, v, site_prior); },
       [](const Model &m, int, size_t row[2]) { row[0] = size_t(m.n_members), row[1] = sizeof(double); }},  // map_gt[N], map_post
      {"evidence", "site evidence", "1", K_EVID, K_EVID_PRIOR, 1, kEvidenceVariants,
       [](const Model &m, int v, int, bool site_prior) { return evidence_source(m, v, site_prior); },
       [](const Model &, int, size_t row[2]) { row[0] = row[1] = sizeof(double); }},  // loglik, pref
      {"loo", "leave-one-out posteriors", "1", K_LOO, K_LOO_PRIOR, 1, kLooVariants,
       [](const Model &m, int v, int, bool site_prior) { return loo_source(m, v, site_prior); },
       [](const Model &m, int, size_t row[2]) { row[0] = 3 * size_t(m.n_members) * sizeof(double), row[1] = size_t(m.n_members) * sizeof(double); }},  // loo[N][3], fit[N]
      {"pattern", "genotype-pattern posteriors", "1", K_PATTERN, K_PATTERN_PRIOR, 1, kPatternVariants,
       [](const Model &m, int v, int, bool site_prior) { return pattern_source(m, v, site_prior); },
       [](const Model &, int n_patterns, size_t row[2]) { row[0] = size_t(n_patterns) * sizeof(double), row[1] = sizeof(double); },  // pat_post[M], loglik
       {X_CALL, "tn", "n_patterns", 1, FAMSEQ_MAX_PATTERNS, "masks", "n_patterns rows of one byte per member", check_masks,
        [](const Model &m) { return size_t(m.n_members); }}},
      {"sample", "joint posterior draws", "1", K_SAMPLE, K_SAMPLE_PRIOR, 1, kSampleVariants,
       [](const Model &m, int v, int, bool site_prior) { return sample_source(m, v, site_prior); },
       [](const Model &m, int n_draws, size_t row[2]) { row[0] = size_t(n_draws) * m.n_members, row[1] = size_t(n_draws) * sizeof(double); },  // samp_gt[K][N], samp_post[K]
       {X_NONE, "sbn", "n_draws", 1, FAMSEQ_MAX_DRAWS}},
      {"af", "founder allele frequency", "1", K_AF, -1, 1, kAfVariants,
       [](const Model &m, int v, int, bool) { return af_source(m, v); },
       [](const Model &, int, size_t row[2]) { row[0] = sizeof(double), row[1] = 2 * sizeof(double); },  // af, loglik[2]
       {X_SITE, "tn", "n_iter", 0, FAMSEQ_MAX_AF_ITER, "af0", "one start value per site", check_af0,
        [](const Model &) { return sizeof(double); }}},
      {"relabel", "relabelling evidence", "1", K_RELABEL, K_RELABEL_PRIOR, 1, kRelabelVariants,
       [](const Model &m, int v, int, bool site_prior) { return relabel_source(m, v, site_prior); },
       [](const Model &, int n_assign, size_t row[2]) { row[0] = size_t(n_assign) * sizeof(double), row[1] = sizeof(double); },  // alt_loglik[M], loglik
       {X_CALL, "tn", "n_assign", 1, FAMSEQ_MAX_RELABEL, "assign", "n_assign rows of one int32 per member", check_assign,
        [](const Model &m) { return size_t(m.n_members) * sizeof(int32_t); }}},
      {"mutrate", "mutation-rate likelihood profile", "1", K_MUTRATE, K_MUTRATE_PRIOR, 1, kMutrateVariants,
       [](const Model &m, int v, int, bool site_prior) { return mutrate_source(m, v, site_prior); },
       [](const Model &, int n_rates, size_t row[2]) { row[0] = size_t(n_rates) * sizeof(double), row[1] = sizeof(double); },  // rate_loglik[R], loglik
       // (the host entries take the rates and stage the tables made from them; the device entries take the tables)
       {X_CALL, "tn", "n_rates", 1, FAMSEQ_MAX_RATES, "rates", "n_rates mutation rates", check_rates,
        [](const Model &) { return FAMSEQ_RATE_TABLE_DOUBLES * sizeof(double); },
        [](const famseq_ctx *c, const void *rates, int32_t n_rates, void *staged) {
          rate_tables(c->model, static_cast<const double *>(rates), n_rates, static_cast<double *>(staged));
        },
        "d_tables", "n_rates factor tables of " FS_STR(FAMSEQ_RATE_TABLE_DOUBLES) " doubles"}},
      {"origin", "phase by transmission", "1", K_ORIGIN, K_ORIGIN_PRIOR, 1, kOriginVariants,
       [](const Model &m, int v, int, bool site_prior) { return origin_source(m, v, site_prior); },
       [](const Model &m, int, size_t row[2]) { row[0] = row[1] = 4 * trio_children(m).size() * sizeof(double); },  // origin[K][4], hettx[K][4]
       {X_CONST, "t", nullptr, 1, 1, nullptr, nullptr, nullptr, [](const Model &) { return FAMSEQ_ALLELE_TABLE_DOUBLES * sizeof(double); },
        [](const famseq_ctx *c, const void *, int32_t, void *staged) { build_allele_tables(c->origin_mrate, static_cast<double *>(staged)); },
        nullptr, nullptr, origin_model}},  // (said before the device is asked for)
      {"weight", "per-member genotype weights", "1", K_WEIGHT, K_WEIGHT_PRIOR, 1, kWeightVariants,
       [](const Model &m, int v, int, bool site_prior) { return weight_source(m, v, site_prior); },
       [](const Model &, int n_weights, size_t row[2]) { row[0] = size_t(n_weights) * sizeof(double), row[1] = sizeof(double); },  // wt_loglik[M], loglik
       {X_CALL, "tn", "n_weights", 1, FAMSEQ_MAX_WEIGHTS, "weights", "n_weights tables of three doubles per member", check_weights,
        [](const Model &m) { return 3 * size_t(m.n_members) * sizeof(double); }, nullptr, "d_weights"}},
      {"maxmarg", "max-marginals", "1", K_MAXMARG, K_MAXMARG_PRIOR, 1, kMaxmargVariants,
       [](const Model &m, int v, int, bool site_prior) { return maxmarg_source(m, v, site_prior); },
       [](const Model &m, int, size_t row[2]) { row[0] = 3 * size_t(m.n_members) * sizeof(double), row[1] = 2 * sizeof(double); }},  // maxmarg[N][3], top[2]
      {"charfn", "count characteristic function", "1", K_CHARFN, K_CHARFN_PRIOR, 1, kCharfnVariants,
       [](const Model &m, int v, int, bool site_prior) { return charfn_source(m, v, site_prior); },
       [](const Model &, int n_tables, size_t row[2]) { row[0] = 2 * size_t(n_tables) * sizeof(double), row[1] = sizeof(double); },  // cf[M][2], loglik
       {X_CALL, "tn", "n_tables", 1, FAMSEQ_MAX_CWEIGHTS, "cweights", "n_tables tables of three complex numbers per member", check_cweights,
        [](const Model &m) { return 6 * size_t(m.n_members) * sizeof(double); }, nullptr, "d_cweights", nullptr, charfn_served}},
  };
  return table;
}

namespace {

// How a kind of generated kernel is made.
struct KernelSpec {
  std::function<std::string(int)> source;  // variant -> HIP source
  int n_variants, first;                   // the variant contest (jit_pick_variant) runs first .. n_variants - 1
  bool honours_pick;                       // a note of the tuner's, keyed by the variant-0 source, names the variant instead
  std::string entry;
  int block_threads;
  // where given: the kernel whose variant this one takes — that kernel's note, else that kernel's contest, so that a
  // context runs both in one variant whatever the compiler's register allocation makes of either
  std::function<std::string(int)> variant_of = nullptr;
};

}  // namespace

int64_t bulk_min_sites(const famseq_ctx *c) {
  if (c->bulk_min_sites != -2) return c->bulk_min_sites;
  return int64_t(16) * 64 * 4 * (c->n_cus > 0 ? c->n_cus : 256);  // (a plan-only context has no device: MI355X's 256 CUs)
}

// 4 where the pedigree's lane kernel has the once-per-site form (variants 4-7 differ from 0-3), else 0.  Generating the
// candidates to find out costs milliseconds, so it is done once per context; a generator that throws means "no such form".
int lane_first_variant(const famseq_ctx *c) {
  famseq_ctx *w = const_cast<famseq_ctx *>(c);
  if (w->lane_first < 0) {
    try {
      w->lane_first = enumgen_first_variant(c->model);
    } catch (const std::exception &) {
      w->lane_first = 0;
    }
  }
  return w->lane_first;
}

namespace {

bool is_lane(int kind) { return kind >= K_LANE && kind <= K_LANE + kEnumMaxGroupDigits; }

// Which side product a kind belongs to (p == nullptr: none), in which form.
struct SideKind {
  const SideProduct *p;
  bool site_prior;
  int form;
};
SideKind side_of(int kind) {
  for (const SideProduct &p : side_table())
    for (bool site_prior : {false, true})
      if ((!site_prior || p.has_prior()) && kind >= p.kind_of(1, site_prior) && kind <= p.kind_of(p.n_forms, site_prior)) return {&p, site_prior, kind - p.kind_of(1, site_prior) + 1};
  return {nullptr, false, 0};
}

KernelSpec kernel_spec(const famseq_ctx *c, int kind) {
  const Model &m = c->model;
  if (is_lane(kind)) {
    const int d = kind - K_LANE;  // (the lanes-per-site forms always use the 6-member block: no measured pick to honour)
    // (one lane per site: the contest starts at the once-per-site variants where the pedigree has that form; elsewhere 4-7 are
    // the texts of 0-3 again, reached only when all of those spill, and then cache hits)
    const bool once = d == 0 && lane_first_variant(c) == 4;
    // (a pick may name any of kEnumVariants; the contest ranges over the first kEnumContestVariants)
    return {[&m, d](int v) { return enumgen_source(m, v, d); }, kEnumContestVariants, once ? 4 : 0, d == 0, "famseq_enum_lane",
            enumgen_block_threads(m, d)};
  }
  if (const SideKind k = side_of(kind); k.p) {
    const auto source = [&m, k](bool site_prior) { return [&m, k, site_prior](int v) { return k.p->source(m, v, k.form, site_prior); }; };
    KernelSpec spec{source(k.site_prior), k.p->n_variants, 0, false, std::string("famseq_") + k.p->stem + (k.site_prior ? "_prior" : ""),
                    elim_block_threads(m)};
    // a site-prior form takes the variant its plain sibling takes for the pedigree (its contest): none of its own, as K_PRIOR
    if (k.site_prior) spec.variant_of = source(false);
    return spec;
  }
  switch (kind) {
    case K_LANE_CALL: {
      // the same block size as the plain lane kernel runs with (variants 0-1 / 2-3: kEnumVariants), so that a batch
      // gives the same bits whether it goes through the fused kernel or through the separate stages
      // (variants 4-7 are 0-3 in the once-per-site form: the call path keeps the per-prefix text of the same block shape)
      const int lane = c->kern[K_LANE].variant;
      // v & 1: the single posterior fenced member by member; v & 2: the leaner stage-out (see kElimCallVariants)
      return {[&m, lane](int v) { return enumgen_source(m, enumgen_call_variant(lane, v & 1), 0, true, !(v & 2)); }, 4, 0, false, "famseq_enum_lane",
              enumgen_block_threads(m)};
    }
    case K_ELIM:
      return {[&m](int v) { return elim_source(m, v); }, kElimVariants, elim_first_variant(m), true, "famseq_elim", elim_block_threads(m)};
    case K_ELIM_CALL:
      return {[&m](int v) { return elim_source(m, v, true); }, kElimCallVariants, elim_first_variant(m, true), false, "famseq_elim",
              elim_block_threads(m, true)};
    case K_PRIOR:  // the variant famseq_elim takes for the pedigree (its measured pick, "pick_elim", or its contest): none of its own
      return {[&m](int v) { return prior_source(m, v); }, kElimVariants, elim_first_variant(m), true, "famseq_elim_prior", elim_block_threads(m),
              [&m](int v) { return elim_source(m, v); }};
  }
  throw std::logic_error("kernel_spec: no such kind");
}

bool have(const famseq_ctx *c, const GenKernel &g) { return g.k.fn || (c->plan_only() && !g.k.path.empty()); }

// Generate, compile (or fetch) and load one kernel: 0, or FAMSEQ_E_HIP with *why.  What a failure means is the caller's.
int load_kernel(famseq_ctx *c, int kind, std::string *why) {
  GenKernel &g = c->kern[kind];
  if (have(c, g)) return 0;
  if (kind == K_LANE_BULK) {  // one text, no pick, no contest: K_LANE's block shape and fencing in the outer-leaf plan
    try {
      const int variant = 8 + (c->kern[K_LANE].variant & 3);
      const std::string src = enumgen_source(c->model, variant, 0);
      int scratch = -1;
      const std::string path = jit_compile(src, &scratch);
      if (scratch > 0) throw std::runtime_error("the bulk form spills " + std::to_string(scratch) + " bytes per lane");
      g.variant = variant;
      if (c->plan_only()) {
        g.k.path = path;
        return 0;
      }
      if (hipSetDevice(c->device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
      g.k = jit_load(src, "famseq_enum_lane");
      g.block_threads = enumgen_block_threads(c->model, 0);
    } catch (const std::exception &e) {
      *why = e.what();
      return FAMSEQ_E_HIP;
    }
    int nb = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, g.k.fn, g.block_threads, 0) != hipSuccess) nb = 1;
    g.blocks_per_cu = std::max(nb, 1);
    return 0;
  }
  try {
    const KernelSpec s = kernel_spec(c, kind);
    // a measured pick (the autotuner's note, or the table build() ships) is loaded as it is: the spill contest is
    // the static rule for pedigrees nobody has measured, and must not move off a measurement
    const std::function<std::string(int)> &chooser = s.variant_of ? s.variant_of : s.source;
    const int pick = s.honours_pick ? jit_read_pick(chooser(0)) : -1;
    std::string src;
    if (pick >= 0 && pick < (is_lane(kind) ? kEnumVariants : s.n_variants)) {
      src = s.source(pick);
      g.variant = pick;
    } else if (s.variant_of) {
      (void)jit_pick_variant(chooser, s.n_variants, &g.variant, s.first);
      src = s.source(g.variant);
    } else {
      src = jit_pick_variant(s.source, s.n_variants, &g.variant, s.first);
    }
    if (c->plan_only()) {  // generate and compile into the cache (this is how build() pre-builds)
      g.k.path = jit_compile(src);
      return 0;
    }
    if (hipSetDevice(c->device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
    g.k = jit_load(src, s.entry);
    g.block_threads = s.block_threads;
  } catch (const std::exception &e) {
    *why = e.what();
    return FAMSEQ_E_HIP;
  }
  int nb = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, g.k.fn, g.block_threads, 0) != hipSuccess) nb = 1;
  g.blocks_per_cu = std::max(nb, 1);
  return 0;
}

}  // namespace

bool origin_rate(const Model &m, double *mu_out) {
  const double mu = m.pcp2Xm[18];  // the son's T(2 | 0, 0)
  if (!(mu >= 0.0 && mu <= 1.0)) return false;
  double a[27], xf[27], xm[27];
  famseq_transmission_tables(mu, a, xf, xm);
  if (std::memcmp(a, m.pcp2, sizeof a) != 0 || std::memcmp(xf, m.pcp2Xf, sizeof xf) != 0 || std::memcmp(xm, m.pcp2Xm, sizeof xm) != 0) return false;
  *mu_out = mu;
  return true;
}

int origin_model(famseq_ctx *c) {
  if (c->origin_state == 0) c->origin_state = origin_rate(c->model, &c->origin_mrate) ? 1 : -1;
  if (c->origin_state > 0) return 0;
  return fail(c, FAMSEQ_E_ARG, "phase by transmission: there is no allele-level model for custom transmission tables (the model's pcp2, pcp2Xf and "
                               "pcp2Xm are not famseq_transmission_tables of one mutation rate)");
}

int charfn_served(famseq_ctx *c) {
  if (have(c, c->kern[K_CHARFN]) || have(c, c->kern[K_CHARFN_PRIOR])) return 0;  // (a kernel that exists was generated for it)
  std::string why;
  if (elim_supported(c->model, &why)) return 0;
  return fail(c, FAMSEQ_E_ARG, std::string(side_table()[SIDE_CHARFN].what) + " (sum-product engine): " + why);
}

int load_or_fail(famseq_ctx *c, int kind) {
  const SideKind k = side_of(kind);
  if (k.p && k.p->n_forms > 1) (k.site_prior ? c->trio_prior_last : c->trio_last) = k.form;  // (the trio kernels: famseq_plan_json)
  if (have(c, c->kern[kind])) return 0;
  std::string why;
  if (!elim_supported(c->model, &why)) {
    const std::string what = k.p ? std::string(k.site_prior ? "site priors, " : "") + k.p->what + " (sum-product engine): "
                                 : kind == K_PRIOR ? "site priors (sum-product engine): " : "elimination engine: ";
    return fail(c, FAMSEQ_E_ARG, what + why);
  }
  if (k.p && k.p->kind == K_ORIGIN && origin_model(c) != 0) return FAMSEQ_E_ARG;
  if (load_kernel(c, kind, &why) != 0) return fail(c, FAMSEQ_E_HIP, why);
  return 0;
}

bool load_or_remember(famseq_ctx *c, int kind) {
  GenKernel &g = c->kern[kind];
  if (g.k.fn) return true;
  if (g.failed) return false;
  if (have(c, g)) return true;
  std::string why;
  if ((kind == K_LANE_CALL || kind == K_LANE_BULK) && !load_or_remember(c, K_LANE)) {  // its block shape and fencing are the plain kernel's
    why = "the plain lane kernel is unavailable: " + c->kern[K_LANE].error;
  } else {
    const int rc = load_kernel(c, kind, &why);
    if (kind == K_LANE_CALL && g.variant >= 0)  // (the answer depends on the variant taken)
      c->lane_reads_rows = enumgen_reads_global_rows(c->model, enumgen_call_variant(c->kern[K_LANE].variant, g.variant & 1)) ? 1 : 0;
    if (rc == 0) return true;
  }
  g.failed = true;
  const bool quiet = std::getenv("FAMSEQ_QUIET") != nullptr;  // else said once per ctx and kernel, where a user of the CLI or of the
                                                              // library sees it (also in famseq_plan_json)
  if (kind == K_LANE_BULK) {  // K_LANE serves instead: same results to the project's tolerance, the super-leaf table rebuilt per step
    g.error = why;
    if (!quiet)
      std::fprintf(stderr, "famseq: the large-batch form of the per-pedigree enumeration kernel is unavailable (%s); the plain form serves every batch\n",
                   why.substr(0, 300).c_str());
  } else if (is_lane(kind)) {
    const int d = kind - K_LANE;
    std::string &lane_error = c->kern[K_LANE].error;
    if (d == 0 || lane_error.empty()) lane_error = why;
    if (!quiet)
      std::fprintf(stderr, "famseq: the per-pedigree enumeration kernel%s is unavailable (%s); %s\n", d ? " (lanes-per-site form)" : "",
                   why.substr(0, 300).c_str(),
                   d ? "such batches take the one-lane-per-site or the compiled-in kernel"
                     : "large batches fall back to the compiled-in team-per-site kernel (about 4x slower)");
  } else {
    g.error = why;
    if (!quiet)
      std::fprintf(stderr, "famseq: the fused call-path form of the %s kernel is unavailable (%s); famseq_bn_call_batch runs the "
                           "separate unpack / posterior / Phred stages instead (same results)\n",
                   kind == K_ELIM_CALL ? "sum-product" : "enumeration", why.substr(0, 300).c_str());
  }
  return false;
}

// A pick (the tuner's note, "pick_lane" / "pick_elim") is read by two loaders only — K_LANE and K_ELIM, the kinds whose
// kernel_spec honours it — and the lane call-path form takes its block shape from K_LANE's variant.  Those three are what
// a new pick makes stale; the lanes-per-site and sum-product call-path kernels and the side products (side_table()) run their own
// contests and cannot be moved by one, so they stay loaded.  (The site-prior kernel takes K_ELIM's variant: whoever drops
// K_ELIM for a new pick drops K_PRIOR with it.  A side product's site-prior form takes its plain sibling's contest's variant; no
// pick moves those, and nothing drops a side product's kernel: whoever comes to drop one drops its site-prior form with it.)
void drop_lane_kernels(famseq_ctx *c) {
  c->kern[K_LANE].drop();
  c->kern[K_LANE_CALL].drop();
  c->lane_reads_rows = -1;
  GenKernel &bulk = c->kern[K_LANE_BULK];  // (its text follows K_LANE's variant: a verdict on the old one says nothing of the new)
  bulk.drop();
  bulk.failed = false, bulk.error.clear();
  c->bulk_differs = -1;
}

namespace {

// How many of the outermost looped members' digits go on lanes for a batch of n_sites.  Cost model
// (measured on the 10-member benchmark pedigree, tools/small_batch_rates.py): a lane's work is its
// share of the enumeration, 3^N / 3^d configurations, plus what every lane of a group repeats (single
// posterior, tables of the fixed levels, its columns of the reduction: about 250 N configuration
// times); lanes run at full speed while there is at most one wave per SIMD (n_cus * 256 lanes), beyond
// that the time grows with the lane count.  More lanes per site pay while the batch leaves SIMDs idle.
int pick_group_digits(const famseq_ctx *c, int64_t n_sites) {
  const int dmax = enumgen_max_group_digits(c->model);
  if (c->group_digits >= 0) return std::min(c->group_digits, dmax);
  if (c->enum_impl == 1) return 0;  // an explicit choice of the lane-per-site kernel is exactly that kernel
  const double full_speed_lanes = double(std::max(1, c->n_cus)) * 256.0;
  const double configs = std::pow(3.0, c->model.n_members), per_lane = 250.0 * c->model.n_members;
  int best = 0;
  double best_t = 0;
  for (int d = 0, g = 1; d <= dmax; ++d, g *= 3) {
    const double t = std::max(1.0, double(n_sites) * g / full_speed_lanes) * (configs / g + (d ? per_lane : 0.0));
    if (d == 0 || t < best_t * 0.9) {
      best = d;
      best_t = t;
    }
  }
  return best;
}

// Is a call of n_sites a bulk call: the context free to choose, the call at or above the threshold, the pedigree one that has the
// form?  Such a call runs one lane per site whatever the cost model of small batches says (at the default threshold it says
// so anyway; a lower threshold is its owner's word that the bulk form serves from there on).
bool bulk_wanted(famseq_ctx *c, int64_t n_sites) {
  const int64_t min_sites = bulk_min_sites(c);
  if (c->enum_impl >= 0 || c->group_digits >= 0 || min_sites < 0 || n_sites < min_sites) return false;
  if (c->bulk_any < 0) {
    try {
      c->bulk_any = enumgen_has_outer_leaf(c->model, 4) || enumgen_has_outer_leaf(c->model, 6) ? 1 : 0;
    } catch (const std::exception &) {
      c->bulk_any = 0;
    }
  }
  return c->bulk_any == 1;
}

// Does the bulk slot serve a one-lane-per-site launch that belongs to a call of n_sites?  (K_LANE is loaded: its variant is known.)
bool bulk_serves(famseq_ctx *c, int64_t n_sites) {
  if (!bulk_wanted(c, n_sites)) return false;
  if (c->bulk_differs < 0) {
    try {
      c->bulk_differs = enumgen_has_outer_leaf(c->model, c->kern[K_LANE].variant) ? 1 : 0;
    } catch (const std::exception &) {
      c->bulk_differs = 0;
    }
  }
  return c->bulk_differs == 1 && load_or_remember(c, K_LANE_BULK);
}

// Can the generated kernel with 3^d lanes per site run without a compilation (loaded, or its code object on disk)?
bool generated_ready(famseq_ctx *c, int d) {
  if (c->lanes(d).k.fn) return true;
  if (c->lanes(d).failed) return false;
  if (c->grp_ready[d] < 0) {
    try {
      const int pick = d == 0 ? jit_read_pick(enumgen_source(c->model, 0, 0)) : -1;
      // (the variant the loader would take first; a spilling first variant sends it on to others, which may need the compiler:
      // then this says "not ready" and the tiny batch stays on the compiled-in kernel, which is always right)
      c->grp_ready[d] = jit_cached(enumgen_source(c->model, pick >= 0 && pick < kEnumVariants ? pick : (d == 0 ? lane_first_variant(c) : 0), d)) ? 1 : 0;
    } catch (const std::exception &) {
      c->grp_ready[d] = 0;
    }
  }
  return c->grp_ready[d] == 1;
}

int grid_for(const famseq_ctx *c, int64_t n_sites) {
  const int64_t passes = (n_sites + c->plan.teams_per_block - 1) / c->plan.teams_per_block;
  int64_t resident = c->grid_override > 0 ? c->grid_override : int64_t(c->n_cus) * c->blocks_per_cu;
  return (int)std::max<int64_t>(1, std::min(passes, resident));
}

}  // namespace

void bulk_prebuild(famseq_ctx *c) {
  if (c->plan_only() && !c->kern[K_LANE].k.path.empty() && bulk_min_sites(c) >= 0) {
    const int impl = c->enum_impl, digits = c->group_digits;
    c->enum_impl = c->group_digits = -1;  // (what a context that is free to choose would load)
    (void)bulk_serves(c, bulk_min_sites(c));
    c->enum_impl = impl, c->group_digits = digits;
  }
}

// The generated kernels share one argument list; what the third and fourth are depends on the kind (posterior and single
// posterior rows, joint and de novo posteriors, MAP genotypes and their posterior, log10 likelihood and hom-ref posterior, leave-one-out rows and fit, pattern
// posteriors and log10 likelihood, drawn configurations and their posteriors, allele frequency and its two log10 likelihoods), so they pass through untyped; so does what some kinds take behind the eighth (MoreArgs).
hipError_t launch_generated(famseq_ctx *c, const GenKernel &g, int64_t n_sites, const double *d_lk, const uint8_t *d_flags, void *d_out_a,
                            void *d_out_b, uint8_t *d_status, hipStream_t stream, int sites_per_chunk, const MoreArgs &more) {
  const int spc = sites_per_chunk > 0 ? sites_per_chunk : g.block_threads;
  const int64_t chunks = (n_sites + spc - 1) / spc;
  int64_t resident = c->grid_override > 0 ? c->grid_override : int64_t(c->n_cus) * g.blocks_per_cu;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min(chunks, resident));
  long ns = (long)n_sites;
  double lc = c->model.lc;
  const double *tc = c->d_tc.as<double>();
  void *args[8 + MoreArgs::kMax] = {&d_lk, &d_flags, &d_out_a, &d_out_b, &d_status, &ns, &tc, &lc};  // the plain forms take these eight
  for (int i = 0; i < more.n; ++i) args[8 + i] = more.at[i];
  return hipModuleLaunchKernel(g.k.fn, grid, 1, 1, (unsigned)g.block_threads, 1, 1, 0, stream, args, nullptr);
}

hipError_t launch_engine(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint8_t *d_flags, double *d_post, double *d_single,
                         uint8_t *d_status, hipStream_t stream, int64_t call_sites) {
  if (c->engine == FAMSEQ_ENGINE_ELIM)
    return launch_generated(c, c->kern[K_ELIM], n_sites, d_lk, d_flags, d_post, d_single, d_status, stream);
  const int64_t whole = call_sites > 0 ? call_sites : n_sites;
  const bool bulk = bulk_wanted(c, whole);  // (every chunk of such a call, a short last one too)
  const bool want_lane = c->enum_impl == 1 || bulk || (c->enum_impl < 0 && (n_sites >= c->lane_min_sites ||
                                                                            generated_ready(c, pick_group_digits(c, n_sites))));
  if (want_lane) {
    int d = bulk ? 0 : pick_group_digits(c, n_sites);
    if (d > 0 && !load_or_remember(c, K_LANE + d)) d = 0;  // that group size does not build: one lane per site before the compiled-in kernel
    if (load_or_remember(c, K_LANE + d)) {
      c->last_group_digits = d;
      if (d == 0 && bulk_serves(c, whole)) {
        c->last_kind = "bulk";
        return launch_generated(c, c->kern[K_LANE_BULK], n_sites, d_lk, d_flags, d_post, d_single, d_status, stream);
      }
      c->last_kind = d > 0 ? "group" : "lane";
      return launch_generated(c, c->lanes(d), n_sites, d_lk, d_flags, d_post, d_single, d_status, stream,
                              d > 0 ? enumgen_sites_per_chunk(c->model, d) : 0);
    }
  }
  c->last_kind = "team";
  return launch_bn_enum(c->plan, c->kp, grid_for(c, n_sites), c->d_img.as<uint32_t>(), c->d_tc.as<double>(), n_sites, d_lk, d_flags, d_post,
                        d_single, d_status, stream);
}

// The fused call path: one launch does PL -> likelihood, posterior, Phred scaling and the genotype call
// (famseq_bn_call_batch).  Served by the call-path forms of the generated kernels (one lane per site).
// Does this batch go through one (loading it on first use), or through the separate stages instead (team kernel,
// lanes-per-site mode, or a lane kernel that re-reads fp64 rows from global memory while the input is packed)?
// The one place that decides.
bool call_fuses(famseq_ctx *c, int64_t n_sites, bool packed_in) {
  const bool elim = c->engine == FAMSEQ_ENGINE_ELIM;
  if (c->big) return false;  // no call-path form of the wide-pedigree kernel: separate stages
  if (!elim) {
    const bool want_lane = c->enum_impl == 1 || (c->enum_impl < 0 && n_sites >= c->lane_min_sites);
    if (!want_lane || pick_group_digits(c, n_sites) != 0) return false;
  }
  if (!load_or_remember(c, elim ? K_ELIM_CALL : K_LANE_CALL)) return false;
  if (!elim && packed_in && c->lane_reads_rows != 0) return false;  // (set with the lane call-path kernel, for the variant it took)
  return true;
}

bool launch_engine_fused(famseq_ctx *c, int64_t n_sites, const double *d_lk, const uint8_t *d_flags, uint8_t *d_status, bool packed_in,
                         const CallIO *d_io, hipStream_t stream, hipError_t *err) {
  const bool elim = c->engine == FAMSEQ_ENGINE_ELIM;
  if (!call_fuses(c, n_sites, packed_in)) return false;
  if (!elim) c->last_group_digits = 0;
  *err = launch_generated(c, c->kern[elim ? K_ELIM_CALL : K_LANE_CALL], n_sites, d_lk, d_flags, nullptr, nullptr, d_status, stream, 0, {&d_io});
  return true;
}

// famseq_set_option(ctx, "tune", 1): where static rules pick a generated kernel's variant (the sum-product kernel's
// fence variant by pedigree size, the enumeration kernel's 7- or 6-member block), time the candidates on THIS device
// and pedigree — synthetic rows, a few milliseconds each — and leave the winner's index as a note in the kernel
// cache; every later context for the pedigree starts from it.  Opt-in: it compiles every candidate.
int tune(famseq_ctx *c) {
  if (c->device < 0) return fail(c, FAMSEQ_E_NODEVICE, "tuning times kernels: it needs a device");
  HIP_TRY(c, hipSetDevice(c->device));
  const Model &mdl = c->model;
  const int N = mdl.n_members;
  // about 10 ms of enumeration per launch, 64 K - 2 M sites; the sum-product kernel, whose time does not grow with
  // 3^N, always gets 8 M (at 64 K sites its launch is most of what a timer sees)
  // ... in whole ROUNDS of the chip: a candidate at one wave per SIMD takes 64 K sites at a time, one at two waves 128 K;
  // a batch of 2.3 rounds times the tail, not the kernel (a thirteen-member pedigree's two blocks came out 25 % apart that
  // way).  Up to eight rounds while a launch stays under a quarter of a second.
  const double configs = std::pow(3.0, N), t_round = 65536.0 * configs / 2.4e13;
  int64_t rounds = std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)(0.25 / t_round)));
  if (rounds > 1) rounds &= ~int64_t(1);
  const int64_t by_time = (int64_t)(0.01 * 2.4e13 / configs) / 131072 * 131072;
  const int64_t n_enum = std::min<int64_t>(int64_t(1) << 21, std::max<int64_t>(by_time, 65536 * rounds));
  const int64_t n_elim = int64_t(1) << 23, n_max = std::max(n_enum, n_elim);  // 8 M: it has to stream from HBM (2 M sites half fit the Infinity Cache)
  int64_t n = n_enum;  // sites of the launches being timed
  const size_t w = size_t(n_max) * 3 * N;
  DevBuf lk, post, single, status;
  if (lk.alloc(w * 8) != hipSuccess || post.alloc(w * 8) != hipSuccess || single.alloc(w * 8) != hipSuccess ||
      status.alloc(size_t(n_max)) != hipSuccess)
    return fail(c, FAMSEQ_E_HIP, "tune: device buffers");
  double *d_lk = lk.as<double>();
  {
    // PL-shaped rows — one genotype at 1, the others 10^-(k/10) — for the first 64 K sites, doubled on the device from there
    const size_t w0 = std::min(w, size_t(1 << 16) * 3 * N);
    std::vector<double> h(w0);
    uint64_t z = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < w0; i += 3) {
      z = z * 6364136223846793005ull + 1442695040888963407ull;
      const unsigned a = unsigned(z >> 33) % 3, p1 = 3 + unsigned(z >> 40) % 88, p2 = p1 + unsigned(z >> 50) % 160;
      h[i + a] = 1.0, h[i + (a + 1) % 3] = std::pow(10.0, -0.1 * p1), h[i + (a + 2) % 3] = std::pow(10.0, -0.1 * p2);
    }
    bool up = hipMemcpy(d_lk, h.data(), w0 * 8, hipMemcpyHostToDevice) == hipSuccess;
    for (size_t have = w0; up && have < w; have *= 2)
      up = hipMemcpy(d_lk + have, d_lk, std::min(have, w - have) * 8, hipMemcpyDeviceToDevice) == hipSuccess;
    if (!up) return fail(c, FAMSEQ_E_HIP, "tune: upload");
  }
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  std::string report;
  // best of three launches of one candidate, ms (< 0: it could not be built)
  auto time_one = [&](const std::string &src, const char *entry, int bt) {
    GenKernel g;
    try {
      g.k = jit_load(src, entry);
    } catch (const std::exception &) {
      return -1.0;
    }
    g.block_threads = bt, g.blocks_per_cu = 1;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&g.blocks_per_cu, g.k.fn, bt, 0) != hipSuccess || g.blocks_per_cu < 1)
      g.blocks_per_cu = 1;
    double best = -1;
    for (int rep = 0; rep < 4; ++rep) {
      (void)hipEventRecord(e0, c->stream[1]);
      const hipError_t e = launch_generated(c, g, n, d_lk, nullptr, post.p, single.p, status.as<uint8_t>(), c->stream[1]);
      (void)hipEventRecord(e1, c->stream[1]);
      if (e != hipSuccess || hipEventSynchronize(e1) != hipSuccess) {
        best = -1;
        break;
      }
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (rep > 0 && (best < 0 || ms < best)) best = ms;  // the first launch warms up
    }
    jit_unload(g.k);
    return best;
  };
  auto race = [&](const char *what, const std::vector<int> &cands, const std::function<std::string(int)> &gen, const char *entry, int bt) {
    int win = -1;
    double win_ms = 0;
    report += std::string(report.empty() ? "" : "; ") + what + ":";
    for (int v : cands) {
      const double ms = time_one(gen(v), entry, bt);
      char buf[64];
      std::snprintf(buf, sizeof buf, " v%d %.4f ms", v, ms);
      report += buf;
      if (ms > 0 && (win < 0 || ms < win_ms * 0.97)) win = v, win_ms = ms;  // a later candidate has to win by 3 % (two runs of one
                                                                            // table disagreed on 17 of 78 pedigrees at 1 %: all within 2 %)
    }
    if (win >= 0) {
      jit_write_pick(gen(0), win);
      report += " -> v" + std::to_string(win);
    }
    return win;
  };
  std::string failed;
  try {
    // (the two block shapes, in the form the pedigree's contest starts from: variants 0 / 2, or 4 / 6 where the once-per-site form exists)
    const int f0 = lane_first_variant(c);
    if (enumgen_describe(mdl, f0) != enumgen_describe(mdl, f0 + 2))
      (void)race(f0 ? "enumeration (7- / 6-member block, once-per-site form)" : "enumeration (7- / 6-member block)", {f0, f0 + 2},
                 [&mdl](int v) { return enumgen_source(mdl, v, 0); }, "famseq_enum_lane", enumgen_block_threads(mdl, 0));
    else
      report += "enumeration: one block shape, nothing to choose";
    n = n_elim;
    if (elim_supported(mdl, nullptr))
      (void)race("sum-product (likelihoods re-read from LDS: fence-free, fenced; in registers: fence-free, fenced)", {0, 1, 4, 5},
                 [&mdl](int v) { return elim_source(mdl, v); }, "famseq_elim", elim_block_threads(mdl));
  } catch (const std::exception &e) {
    failed = e.what();
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (!failed.empty()) return fail(c, FAMSEQ_E_HIP, "tune: " + failed);
  c->tune_report = report + " (synthetic sites per launch: " + std::to_string(n_enum) + " enumeration, " + std::to_string(n_elim) + " sum-product)";
  // the kernels this context holds may have lost: drop them (which, and why no others: drop_lane_kernels), the next use loads the picks
  GenKernel &lane = c->kern[K_LANE], &elim = c->kern[K_ELIM];
  const bool had_lane = lane.k.fn != nullptr, had_elim = elim.k.fn != nullptr, had_lc = c->kern[K_LANE_CALL].k.fn != nullptr;
  drop_lane_kernels(c);
  elim.drop();
  c->kern[K_PRIOR].drop();  // follows famseq_elim's pick: loaded again on its next use
  if (had_lane && !load_or_remember(c, K_LANE)) return fail(c, FAMSEQ_E_HIP, "lane kernel unavailable after tuning: " + lane.error);
  if (had_lc && !load_or_remember(c, K_LANE_CALL))
    return fail(c, FAMSEQ_E_HIP, "call-path kernel unavailable after tuning: " + c->kern[K_LANE_CALL].error);
  if (had_elim || c->engine == FAMSEQ_ENGINE_ELIM) {
    const int rc = load_or_fail(c, K_ELIM);
    if (rc != 0) return rc;
  }
  if (lane.variant >= 0 || elim.variant >= 0)  // what this context runs from here on (the notes are honoured as written)
    c->tune_report += "; loaded:" + (lane.variant >= 0 ? " enumeration v" + std::to_string(lane.variant) : std::string()) +
                      (elim.variant >= 0 ? " sum-product v" + std::to_string(elim.variant) : std::string());
  return 0;
}

// FAMSEQ_PHASE_CLOCK on the plain kernels: their counters sit in a module global; print and clear them.
void report_phase_clock(famseq_ctx *c) {
  for (int kind : {K_ELIM, K_LANE}) {
    const JitKernel &k = c->kern[kind].k;
    if (!k.module) continue;
    hipDeviceptr_t p = nullptr;
    size_t bytes = 0;
    if (hipModuleGetGlobal(&p, &bytes, k.module, "fs_phase_clk") != hipSuccess || bytes < 8 * sizeof(unsigned long long)) continue;
    unsigned long long ph[8] = {};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(ph, p, sizeof ph, hipMemcpyDeviceToHost) != hipSuccess) continue;
    unsigned long long tot = 0;
    for (unsigned long long v : ph) tot += v;
    std::fprintf(stderr, "famseq phase clock, %s kernel (wave cycles):", kind == K_ELIM ? "sum-product" : "enumeration");
    for (int i = 0; i < 8; ++i) std::fprintf(stderr, " [%d] %.1f%%", i, tot ? 100.0 * double(ph[i]) / double(tot) : 0.0);
    std::fprintf(stderr, "  total %llu\n", tot);
    (void)hipMemset(p, 0, sizeof ph);
  }
}

}  // namespace famseq
