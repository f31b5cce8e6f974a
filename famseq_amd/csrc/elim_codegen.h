// elim_codegen.h — source generator of the exact sum-product ("elimination") engine.
#ifndef FAMSEQ_ELIM_CODEGEN_H_
#define FAMSEQ_ELIM_CODEGEN_H_

#include <string>
#include <vector>

#include "famseq_hip.h"
#include "model.h"

namespace famseq {

// Loop-free pedigree (member/nuclear-family graph is a forest)?  `why` receives the reason if not.
bool elim_supported(const Model &m, std::string *why);
// members conditioned on to cut the pedigree's loops (0 for a loop-free pedigree), -1 if unsupported
int elim_conditioned_members(const Model &m);
// HIP source of `extern "C" __global__ famseq_elim(lk, flags, post, single, status, n_sites, tc, lc)`
// specialised for the model's topology, sexes and sequenced set.  Throws if unsupported.
// variant = 4 * r + f.  f = 0..3: decreasing instruction-level parallelism / register pressure (0 no compiler fences,
// 1 a fence per family->member message and the transmission tables through scalar loads, 2 fences after every block,
// 3 also between the members of the single posterior).  r: where the likelihoods live during the message passing —
// 0 re-read from the lane's LDS row at each use (the marginals wait in registers until the row is free), 1 read once
// into registers, the row being the output stage from then on (a tenth of the LDS reads, issued together; round 3:
// equal for trios and quads, +2...17 % from five members on with one exception in ten pedigrees, x1.4-2 beyond twenty
// members: profiles/r03a/exp_elim_registers_first*.txt).  jit_pick_variant takes the first that does not spill, from
// elim_first_variant on.  The call-path form has the r = 0 family only.
constexpr int kElimVariants = 12;  // 8..11 (r = 2): no LDS staging at all, rows straight from and to global memory (the widest pedigrees)
// The call-path form: fence level f = v & 3 of the r = 0 family, and (v & 4) how its stage-out walks the rows — 0: the row width a
// constant (no per-step bound to test, every load of the walk in flight together; more registers), 4: read from the arguments.
constexpr int kElimCallVariants = 8;
// call_mode: the fused call path's form (packed PLs or fp64 rows in; GPP / FPP / FGT / status out)
std::string elim_source(const Model &m, int variant, bool call_mode = false);
int elim_block_threads(const Model &m, bool call_mode = false);
int elim_first_variant(const Model &m, bool call_mode = false);  // where jit_pick_variant starts (see elim_block_threads)

// Site priors (famseq_bn_prior_batch).  HIP source of `extern "C" __global__ famseq_elim_prior(lk, flags, post, single, status,
// n_sites, tc, lc, prior)`: famseq_elim with the founders' genotype prior read per site from prior[n_sites][6] (doubles 0-2: female
// founders and every founder at an autosomal site; 3-5: male founders at a chrX site) instead of the model's genoProb rows; the
// flags' Known bit is not read.  Variants and their numbering are elim_source's (the plain form only); fed the model's own rows
// it returns famseq_elim's bits.  Throws if the engine does not serve the pedigree.
std::string prior_source(const Model &m, int variant);

// Trio posteriors (famseq_trio_batch): the children are the members with parents, in PED order.
std::vector<int> trio_children(const Model &m);
// HIP source of `extern "C" __global__ famseq_trio(lk, flags, joint, dnm, status, n_sites, tc, lc)`: per site and child k the
// posterior joint[27 k + 9 gc + 3 gm + gf] of the child's and its parents' genotypes in the full network, and dnm[k], its mass
// where the mutation-free transmission table is 0.  form: 1 dnm only, 2 joint only, 3 both (what is not in the form is never
// written).  variant 0..3: the fence levels of famseq_elim's (kTrioVariants).  Throws if the engine does not serve the pedigree.
constexpr int kTrioVariants = 4;
// site_prior: the entry point is famseq_trio_prior, with a trailing `prior` [n_sites][6] as famseq_elim_prior takes it (see
// prior_source): the founders' prior is the site's row, the Known bit is not read; every other statement is famseq_trio's.
std::string trio_source(const Model &m, int variant, int form, bool site_prior = false);

// The joint MAP configuration (famseq_map_batch).  HIP source of
// `extern "C" __global__ famseq_map(lk, flags, map_gt, map_post, status, n_sites, tc, lc)`: per site the most probable joint
// genotype assignment of the whole pedigree, map_gt[N] (int8, PED order), and its posterior probability map_post = w(g*) / sum_g
// w(g); the same graph as famseq_elim under the (max, x) semiring with back-pointers, Z from the sum pass.  variant 0..3: the
// fence levels of famseq_elim's.  Throws if the engine does not serve the pedigree.
constexpr int kMapVariants = 4;
// site_prior: famseq_map_prior, with a trailing `prior` [n_sites][6] (as trio_source's).
std::string map_source(const Model &m, int variant, bool site_prior = false);

// The evidence (famseq_evidence_batch).  HIP source of
// `extern "C" __global__ famseq_evidence(lk, flags, loglik, pref, status, n_sites, tc, lc)`: per site loglik = log10 sum_g prod_m
// f_m(g_m | g_mother, g_father), the data's likelihood under the pedigree (the sum pass of famseq_map, the reference's 1e7 taken
// out), and pref = w(0, ..., 0) / sum_g w(g), the posterior probability that every member is hom-ref.  variant 0..3: the fence
// levels of famseq_elim's.  Throws if the engine does not serve the pedigree.
constexpr int kEvidenceVariants = 4;
// site_prior: famseq_evidence_prior, with a trailing `prior` [n_sites][6] (as trio_source's).
std::string evidence_source(const Model &m, int variant, bool site_prior = false);

// Leave-one-out posteriors and per-member fit (famseq_loo_batch).  HIP source of
// `extern "C" __global__ famseq_loo(lk, flags, loo, fit, status, n_sites, tc, lc)`: per site and member p (PED order)
// loo[3 p + g] = P(g_p = g | the likelihood rows of every member but p), from the messages famseq_elim forms with p's own row
// left out of the product (never divided out), and fit[p] = sum_g loo[3 p + g] lk[3 p + g] = Z / Z_-p, the predictive likelihood
// of p's row given its relatives.  variant 0..3: the fence levels of famseq_elim's.  Throws if the engine does not serve the pedigree.
constexpr int kLooVariants = 4;
// site_prior: famseq_loo_prior, with a trailing `prior` [n_sites][6] (as trio_source's).
std::string loo_source(const Model &m, int variant, bool site_prior = false);

// Max-marginals and the runner-up of the joint call (famseq_maxmarg_batch).  HIP source of
// `extern "C" __global__ famseq_maxmarg(lk, flags, maxmarg, top, status, n_sites, tc, lc)`: per site and member p (PED order)
// maxmarg[3 p + a] = max_{g: g_p = a} w(g) / Z — famseq_map's max pass in both directions, without back-pointers — and
// top = (w(g*) / Z, the second-largest w / Z): top[0] is famseq_map's map_post bit for bit (the same expressions for W and Z).
// An entry without a supporting configuration of positive weight is exactly 0.0.  variant 0..3: the fence levels of
// famseq_elim's; every variant gives the same bits.  Throws if the engine does not serve the pedigree.
constexpr int kMaxmargVariants = 4;
// site_prior: famseq_maxmarg_prior, with a trailing `prior` [n_sites][6] (as trio_source's).
std::string maxmarg_source(const Model &m, int variant, bool site_prior = false);

// Genotype-pattern posteriors (famseq_pattern_batch).  HIP source of
// `extern "C" __global__ famseq_pattern(lk, flags, ppost, loglik, status, n_sites, tc, lc, mask, n_patterns)`: per site and pattern
// m — mask[m][p] holds in bit g whether member p (PED order) may have genotype g — ppost[m] = Z_m / Z, the posterior probability
// that every member's genotype is one its mask allows, Z_m being the network's total weight with the disallowed entries of every
// likelihood row set to zero; and loglik, famseq_evidence's.  The sum pass of famseq_evidence, n_patterns + 1 times on one read of
// the site's rows.  variant 0..3: the fence levels of famseq_elim's.  Throws if the engine does not serve the pedigree.
constexpr int kPatternVariants = 4;
// site_prior: famseq_pattern_prior, with a trailing `prior` [n_sites][6] behind n_patterns (as trio_source's).
std::string pattern_source(const Model &m, int variant, bool site_prior = false);

// Relabelling evidence (famseq_relabel_batch).  HIP source of
// `extern "C" __global__ famseq_relabel(lk, flags, alt, loglik, status, n_sites, tc, lc, assign, n_assign)`: per site and
// assignment j — assign[j][p] names the member whose likelihood row member p (PED order) is given, -1 (or anything else outside
// 0 .. N-1) the row (1, 1, 1) — alt[j] = log10 Z_a, the network's total weight with the rows so assigned, famseq_evidence's scale
// (-inf where it is exactly 0); and loglik, famseq_evidence's.  The sum pass of famseq_evidence, n_assign + 1 times on one read of
// the site's rows.  variant 0..3: the fence levels of famseq_elim's; every variant gives the same bits.  Throws if the engine does
// not serve the pedigree.
constexpr int kRelabelVariants = 4;
// site_prior: famseq_relabel_prior, with a trailing `prior` [n_sites][6] behind n_assign (as trio_source's).
std::string relabel_source(const Model &m, int variant, bool site_prior = false);

// The mutation-rate likelihood profile (famseq_mutrate_batch).  HIP source of
// `extern "C" __global__ famseq_mutrate(lk, flags, rate_ll, loglik, status, n_sites, tc, lc, rt, n_rates)`: per site and rate r
// rate_ll[r] = log10 Z_r, the network's total weight with the children's transmission entries taken from block r of
// rt[n_rates][432] (build_factor_tables' layout; the founders' priors stay tc's, or the site's own), famseq_evidence's scale
// (-inf where it is exactly 0); and loglik, famseq_evidence's, under tc itself.  The sum pass of famseq_evidence, n_rates + 1
// times on one read of the site's rows.  variant 0..3: the fence levels of famseq_elim's; every variant gives the same bits, and
// in every one a pass's entries arrive by scalar loads (variant 0 takes the chrX loop as well).  Throws if the engine does not serve the pedigree.
constexpr int kMutrateVariants = 4;
// site_prior: famseq_mutrate_prior, with a trailing `prior` [n_sites][6] behind n_rates (as trio_source's).
std::string mutrate_source(const Model &m, int variant, bool site_prior = false);

// Per-member genotype weights (famseq_weight_batch).  HIP source of
// `extern "C" __global__ famseq_weight(lk, flags, wt_ll, loglik, status, n_sites, tc, lc, wt, n_weights)`: per site and table m
// wt_ll[m] = log10 Z_m, the network's total weight with member p's likelihood entry g multiplied (once, rounded) by
// wt[m][p][g] — every member's, sequenced or not — on famseq_evidence's scale (-inf where it is exactly 0, not clamped); and
// loglik, famseq_evidence's, on the rows as they are.  The sum pass of famseq_evidence, n_weights + 1 times on one read of the
// site's rows; a pass's weights are read through a wave-uniform pointer.  variant 0..3: the fence levels of famseq_elim's;
// every variant gives the same bits.  Throws if the engine does not serve the pedigree.
constexpr int kWeightVariants = 4;
// site_prior: famseq_weight_prior, with a trailing `prior` [n_sites][6] behind n_weights (as trio_source's).
std::string weight_source(const Model &m, int variant, bool site_prior = false);

// The posterior characteristic function of an additive statistic (famseq_charfn_batch).  HIP source of
// `extern "C" __global__ famseq_charfn(lk, flags, cf, loglik, status, n_sites, tc, lc, cw, n_tables)`: per site and table m
// cf[m] = (Re Z_m / Z0, Im Z_m / Z0), Z_m the network's total weight with member p's likelihood entry g multiplied by the complex
// number cw[m][p][g] = (re, im) — every member's, sequenced or not — and Z0 the total weight on the rows as they are (true
// divisions, nothing clamped); and loglik, famseq_evidence's.  The real sum pass of famseq_evidence once, then a complex sum pass
// per table on the same read of the site's rows: every message a pair of doubles, the transmission entries, priors and scales
// real; a pass's weights are read through a wave-uniform pointer.  variant 0..3: the fence levels of famseq_elim's; every
// variant gives the same bits.  Throws if the engine does not serve the pedigree.
constexpr int kCharfnVariants = 4;
// site_prior: famseq_charfn_prior, with a trailing `prior` [n_sites][6] behind n_tables (as trio_source's).
std::string charfn_source(const Model &m, int variant, bool site_prior = false);

// Phase by transmission (famseq_origin_batch).  HIP source of
// `extern "C" __global__ famseq_origin(lk, flags, origin, hettx, status, n_sites, tc, lc, al)`: per site and child k
// (trio_children's order) origin[k][2 a + b], the posterior that the child received allele a (0 ref, 1 alt) from its mother and b
// from its father, and hettx[k] = (P(g_m = 1, a = 1), P(g_m = 1, a = 0), P(g_f = 1, b = 1), P(g_f = 1, b = 0)): the network of
// famseq_evidence with the child's transmission factor replaced by tm(a | g_m) tf(b | g_f), whose rows the kernel reads from
// al[48] (build_allele_tables) — the text holds no rate.  variant 0..3: the fence levels of famseq_elim's, every one with the
// chrX loop (the rows arrive by scalar loads).  Throws if the engine does not serve the pedigree.
constexpr int kOriginVariants = 4;
// site_prior: famseq_origin_prior, with a trailing `prior` [n_sites][6] behind al (as trio_source's).
std::string origin_source(const Model &m, int variant, bool site_prior = false);
// al[FAMSEQ_ALLELE_TABLE_DOUBLES] for the mutation rate mu: [chrX][child sex: 0 son, 1 daughter][parent: 0 mother, 1 father]
// [allele][parent's genotype]
void build_allele_tables(double mu, double *tables);

// The founders' allele frequency by maximum likelihood (famseq_af_batch).  HIP source of
// `extern "C" __global__ famseq_af(lk, flags, af, loglik, status, n_sites, tc, lc, af0, n_iter)`: per site n_iter EM steps on the
// allele frequency q of the founders' Hardy-Weinberg prior from af0 — a step is one sum pass of famseq_evidence and the founders'
// marginals under the rows of its q — all on one read of the site's rows: af = q after the steps, loglik[0] = log10 Z(q) and
// loglik[1] = log10 Z(0), famseq_evidence's scale.  The prior is the unknown, so there is no site-prior form.  variant 0..3: the
// fence levels of famseq_elim's; every variant gives the same bits.  Throws if the engine does not serve the pedigree.
constexpr int kAfVariants = 4;
std::string af_source(const Model &m, int variant);

// Exact joint posterior draws (famseq_sample_batch).  HIP source of
// `extern "C" __global__ famseq_sample(lk, flags, samp_gt, samp_post, status, n_sites, tc, lc, seed, site_base, n_draws)`: per site
// and draw k a joint configuration samp_gt[k][N] (int8, PED order) drawn with probability w(g) / Z and samp_post[k], that
// probability: the sum pass of famseq_map, then per draw the walk of its back-track with a weighted random choice (Philox4x32-10,
// counter (site_base + site, draw, block)) where that takes an arg-max.  variant 0..3: the fence levels of famseq_elim's; every
// variant draws the same bits.  Throws if the engine does not serve the pedigree, or if its messages do not fit the lanes' LDS rows.
constexpr int kSampleVariants = 4;
// site_prior: famseq_sample_prior, with a trailing `prior` [n_sites][6] behind n_draws (as trio_source's).
std::string sample_source(const Model &m, int variant, bool site_prior = false);

}  // namespace famseq
#endif
