// tests/asan_host_check.cpp — the host side of libfamseq_hip.so under AddressSanitizer + UBSan
// (`make asan`; CPU only, never on the GPU box).  Links the library's own host translation units
// (model, plan, both kernel generators, jit, the C ABI), compiled by g++ with
// -fsanitize=address,undefined, and drives them the way the ABI's callers do on plan-only
// contexts: model setup and its rejections, plan options (valid and invalid), every variant and form of
// both generators (the sum-product family's site-prior, trio and MAP kernels among them), the JSON description, the error paths of the compute entry points without a
// device (the side products' table of extra arguments and its value checks among them), and the JIT's failure path (no compiler) of every kind of generated kernel.  Any sanitizer
// report aborts with a non-zero exit status; the program prints one line per pedigree.
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "elim_codegen.h"
#include "enum_codegen.h"
#include "famseq_hip.h"

namespace {

struct Ped {
  const char *name;
  std::vector<int32_t> id, mo, fa, sex;
  std::vector<uint8_t> seq;
};

Ped chain(int n) {  // founder couple, then each generation marries in a founder: n members, depth ~n/2
  Ped p;
  p.name = "chain";
  for (int i = 1; i <= n; ++i) {
    p.id.push_back(i);
    const bool child = i >= 3 && i % 2 == 1;
    p.mo.push_back(child ? (i - 1) : 0);
    p.fa.push_back(child ? (i - 2) : 0);
    p.sex.push_back(i % 2 == 1 ? 1 : 2);
    p.seq.push_back(i % 5 != 0);
  }
  return p;
}

int fails = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); \
      ++fails;                                                           \
    }                                                                    \
  } while (0)

// Every failed compilation leaves its source and the compiler's log in the cache: the number of files there tells whether
// a call went as far as the compiler.
const char *cache_dir = nullptr;
int cache_files() {
  int n = 0;
  if (DIR *d = opendir(cache_dir)) {
    while (readdir(d)) ++n;
    closedir(d);
  }
  return n;
}

// No compiler: the option fails with a message, twice in a row.  A kind that remembers its failure (sticky) answers the
// second time without generating or compiling again; the others try again.  The plan is read in between.
size_t fails_twice(famseq_ctx *c, const char *key, int64_t value, bool sticky) {
  size_t bytes = 0;
  for (int rep = 0; rep < 2; ++rep) {
    const int before = cache_files();
    CHECK(famseq_set_option(c, key, value) != 0);
    CHECK(std::strlen(famseq_last_error(c)) > 0);
    if (rep == 1) CHECK(sticky ? cache_files() == before : cache_files() > before);
    bytes += std::strlen(famseq_plan_json(c));
  }
  return bytes;
}

void drive(const Ped &p) {
  famseq_model m;
  const int n = (int)p.id.size();
  const int rc = famseq_model_init(&m, n, p.id.data(), p.mo.data(), p.fa.data(), p.sex.data(), p.seq.empty() ? nullptr : p.seq.data(),
                                   1e-7, 1.0);
  CHECK(rc == 0);
  if (rc != 0) return;
  char err[256] = "";
  famseq_ctx *c = famseq_create(&m, -1, err, sizeof err);
  CHECK(c != nullptr);
  if (!c) {
    std::fprintf(stderr, "%s: %s\n", p.name, err);
    return;
  }
  size_t bytes = std::strlen(famseq_plan_json(c));
  for (int a = 0; a <= 7; ++a) (void)famseq_set_option(c, "fixed_digits", a);  // 7 is out of range: must be refused cleanly
  for (int l = 0; l <= 6; ++l) (void)famseq_set_option(c, "low_members", l);
  for (int bt : {64, 256, 768, 100, 4096}) (void)famseq_set_option(c, "block_threads", bt);
  CHECK(famseq_set_option(c, "no_such_option", 1) == FAMSEQ_E_ARG);
  CHECK(famseq_set_option(c, "engine", 7) == FAMSEQ_E_ARG);
  bytes += std::strlen(famseq_plan_json(c));
  for (int v = 0; v < famseq::kEnumVariants; ++v) bytes += famseq::enumgen_source(m, v).size();
  bytes += famseq::enumgen_describe(m).size();
  std::string why;
  const bool elim = famseq::elim_supported(m, &why);
  if (elim) {  // every form of the sum-product family: plain, call path, site priors, trio and MAP (with and without site priors)
    for (int v = 0; v < famseq::kElimVariants; ++v) bytes += famseq::elim_source(m, v).size() + famseq::prior_source(m, v).size();
    for (int v = 0; v < famseq::kElimCallVariants; ++v) bytes += famseq::elim_source(m, v, true).size();
    for (int prior = 0; prior <= 1; ++prior) {
      for (int v = 0; v < famseq::kTrioVariants; ++v)
        for (int form = 1; form <= 3; ++form) bytes += famseq::trio_source(m, v, form, prior != 0).size();
      for (int v = 0; v < famseq::kMapVariants; ++v) bytes += famseq::map_source(m, v, prior != 0).size();
    }
  }
  // no compiler: the JIT's failure path (message, no leak, the ctx stays usable)
  CHECK(famseq_set_option(c, "enum_impl", 1) != 0);
  if (elim) CHECK(famseq_set_option(c, "engine", FAMSEQ_ENGINE_ELIM) != 0);
  CHECK(std::strlen(famseq_last_error(c)) > 0);
  // ... and of the other kinds: lanes-per-site and the call-path forms remember (the first enum_impl above already made
  // the plain lane kernel's verdict), the sum-product family (plain, trio, MAP) tries again on every call
  CHECK(famseq_set_option(c, "enum_impl", 1) != 0);
  if (famseq::enumgen_max_group_digits(m) >= 1) bytes += fails_twice(c, "group_digits", 1, true);
  bytes += fails_twice(c, "call_kernels", 1, true);
  bytes += fails_twice(c, "call_kernels", 2, true);
  if (elim) {
    bytes += fails_twice(c, "engine", FAMSEQ_ENGINE_ELIM, false);
    for (int form = 1; form <= 3; ++form) bytes += fails_twice(c, "trio_kernels", form, false);
    bytes += fails_twice(c, "map_kernels", 1, false);
  } else {  // refused for the pedigree, before anything is generated
    CHECK(famseq_set_option(c, "trio_kernels", 1) == FAMSEQ_E_ARG && std::strstr(famseq_last_error(c), "trio posteriors (sum-product engine): "));
    CHECK(famseq_set_option(c, "map_kernels", 1) == FAMSEQ_E_ARG && std::strstr(famseq_last_error(c), "joint MAP call (sum-product engine): "));
  }
  // compute entry points on a ctx without a device
  std::vector<double> lk(3 * n * 4, 0.25), post(3 * n * 4);
  std::vector<uint8_t> st(4);
  CHECK(famseq_bn_batch(c, 4, lk.data(), nullptr, post.data(), nullptr, st.data()) == FAMSEQ_E_NODEVICE);
  CHECK(famseq_bn_batch_device(c, 4, lk.data(), nullptr, post.data(), nullptr, nullptr, nullptr) == FAMSEQ_E_NODEVICE);
  CHECK(famseq_bn_batch(c, -1, lk.data(), nullptr, post.data(), nullptr, nullptr) == FAMSEQ_E_ARG);
  famseq_ctx *cs[1] = {c};
  const int64_t ns[1] = {4};
  const double *dl[1] = {lk.data()};
  double *dp[1] = {post.data()};
  CHECK(famseq_bn_batch_device_sharded(cs, 1, ns, dl, nullptr, dp, nullptr, nullptr) == FAMSEQ_E_NODEVICE);
  CHECK(famseq_bn_batch_sharded(cs, 1, 4, lk.data(), nullptr, post.data(), nullptr, nullptr) == FAMSEQ_E_NODEVICE);
  {  // the entries that take lk or packed PLs: exactly one of the two (checked first), then the device
    std::vector<uint16_t> pl(3 * n * 4, 0);
    std::vector<int32_t> seq(n);
    for (int i = 0; i < n; ++i) seq[i] = i;
    std::vector<double> gpp(3 * n * 4), fpp(3 * n * 4), dnm(4 * n), joint(27 * 4 * n);
    std::vector<int8_t> fgt(n * 4);
    std::vector<char> text(size_t(n) * 4 * FAMSEQ_TEXT_STRIDE);
    for (int both = 0; both <= 1; ++both) {
      const double *l = both ? lk.data() : nullptr;
      const uint16_t *q = both ? pl.data() : nullptr;
      CHECK(famseq_bn_call_batch(c, 4, l, q, nullptr, seq.data(), n, gpp.data(), fpp.data(), fgt.data(), st.data()) == FAMSEQ_E_ARG);
      CHECK(famseq_bn_call_text_batch(c, 4, l, q, nullptr, seq.data(), n, text.data(), st.data()) == FAMSEQ_E_ARG);
      CHECK(famseq_trio_batch(c, 4, l, q, seq.data(), n, nullptr, joint.data(), dnm.data(), st.data()) == FAMSEQ_E_ARG);
      CHECK(famseq_map_batch(c, 4, l, q, seq.data(), n, nullptr, fgt.data(), post.data(), st.data()) == FAMSEQ_E_ARG);
      CHECK(std::strstr(famseq_last_error(c), "exactly one of") != nullptr);
    }
    CHECK(famseq_bn_call_batch(c, 4, lk.data(), nullptr, nullptr, seq.data(), n, gpp.data(), fpp.data(), fgt.data(), st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_bn_call_batch(c, 4, nullptr, pl.data(), nullptr, seq.data(), n, gpp.data(), fpp.data(), fgt.data(), st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_bn_call_text_batch(c, 4, lk.data(), nullptr, nullptr, seq.data(), n, text.data(), st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_bn_call_text_batch(c, 4, lk.data(), nullptr, nullptr, seq.data(), n, nullptr, st.data()) == FAMSEQ_E_ARG);
    CHECK(famseq_trio_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, joint.data(), dnm.data(), st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_map_batch(c, 4, nullptr, pl.data(), seq.data(), n, nullptr, fgt.data(), post.data(), st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(std::strstr(famseq_last_error(c), "no CPU path") != nullptr);
    // the side products whose entries take a table, a count or sampling's scalars: the table's row is walked and its check reads
    // every value of the caller's array (then the device is what is missing); the last value bad, no count, no table
    std::vector<uint8_t> masks(2 * n, 7);
    std::vector<int32_t> assign(2 * n, -1);
    std::vector<double> rates(2, 1e-7), weights(2 * 3 * n, 1.0), af0(4, 0.1), out(FAMSEQ_RATE_TABLE_DOUBLES + 64 * n);
    double *o = out.data();
    CHECK(famseq_pattern_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, masks.data(), 2, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_relabel_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, assign.data(), 2, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_mutrate_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, rates.data(), 2, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_weight_prior_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, lk.data(), weights.data(), 2, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_af_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, af0.data(), 8, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_sample_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, 7, 1000, 3, fgt.data(), o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_origin_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    CHECK(famseq_loo_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, o, o, st.data()) == FAMSEQ_E_NODEVICE);
    masks.back() = 8, assign.back() = n, rates.back() = 1.5, weights.back() = -1.0, af0.back() = 1.5;
    CHECK(famseq_pattern_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, masks.data(), 2, o, o, st.data()) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "masks: pattern 1, member") != nullptr);
    CHECK(famseq_relabel_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, assign.data(), 2, o, o, st.data()) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "assign: assignment 1, member") != nullptr);
    CHECK(famseq_mutrate_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, rates.data(), 2, o, o, st.data()) == FAMSEQ_E_ARG);
    CHECK(famseq_rate_tables(c, rates.data(), 2, o) == FAMSEQ_E_ARG && std::strstr(famseq_last_error(c), "rates[1] must be") != nullptr);
    CHECK(famseq_rate_tables(c, rates.data(), 1, o) == 0);
    CHECK(famseq_weight_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, weights.data(), 2, o, o, st.data()) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "weight table 1, member") != nullptr);
    CHECK(famseq_af_batch(c, 4, lk.data(), nullptr, seq.data(), n, nullptr, af0.data(), 8, o, o, st.data()) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "(site 3)") != nullptr);
    CHECK(famseq_weight_batch_device(c, 4, nullptr, nullptr, seq.data(), n, nullptr, weights.data(), 33, o, o, st.data(), nullptr) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "n_weights must be 1..32, got 33") != nullptr);
    CHECK(famseq_mutrate_batch_device(c, 4, nullptr, nullptr, seq.data(), n, nullptr, nullptr, 2, o, o, st.data(), nullptr) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "d_tables must be given (n_rates factor tables of 432 doubles)") != nullptr);
    CHECK(famseq_sample_batch(c, 4, nullptr, nullptr, seq.data(), n, nullptr, 7, -1, 3, fgt.data(), o, st.data()) == FAMSEQ_E_ARG);
    CHECK(std::strstr(famseq_last_error(c), "site_base must be >= 0, got -1") != nullptr);
  }
  std::vector<int8_t> g(n * 4);
  famseq_call_genotypes(lk.data(), n * 4, g.data());
  famseq_destroy(c);
  std::printf("%-8s N=%2d elim=%d  %zu bytes of plan JSON + generated source\n", p.name, n, (int)elim, bytes);
}

}  // namespace

int main() {
  setenv("FAMSEQ_HIPCC", "/bin/false", 1);  // the generators run; nothing is compiled
  setenv("FAMSEQ_NO_HIPRTC", "1", 1);       // (neither in-process nor by hipcc)
  setenv("FAMSEQ_QUIET", "1", 1);
  char tmpl[] = "/tmp/famseq_asan_XXXXXX";
  const char *dir = mkdtemp(tmpl);
  if (!dir) return 2;
  setenv("FAMSEQ_KERNEL_CACHE", dir, 1);
  cache_dir = dir;

  std::vector<Ped> peds;
  peds.push_back({"single", {1}, {0}, {0}, {1}, {}});
  peds.push_back({"pair", {1, 2}, {0, 0}, {0, 0}, {1, 2}, {}});
  peds.push_back({"trio", {1, 2, 3}, {0, 0, 2}, {0, 0, 1}, {1, 2, 1}, {0, 0, 1}});
  peds.push_back({"ped5", {1, 2, 3, 4, 5}, {0, 0, 2, 2, 2}, {0, 0, 1, 1, 1}, {1, 2, 1, 2, 1}, {}});
  peds.push_back({"ped10", {1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, {0, 0, 2, 2, 0, 0, 5, 5, 4, 4}, {0, 0, 1, 1, 0, 0, 3, 3, 6, 6},
                  {1, 2, 1, 2, 2, 1, 1, 2, 1, 2}, {}});
  peds.push_back({"ped15", {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {0, 0, 2, 2, 2, 0, 0, 0, 6, 6, 4, 4, 8, 8, 8},
                  {0, 0, 1, 1, 1, 0, 0, 0, 3, 3, 7, 7, 5, 5, 5}, {1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1}, {}});
  // first-cousin marriage: a loop, cut by conditioning
  peds.push_back({"cousins", {1, 2, 3, 4, 5, 6, 7, 8, 9}, {0, 0, 2, 2, 0, 0, 5, 4, 8}, {0, 0, 1, 1, 0, 0, 3, 6, 7},
                  {1, 2, 1, 2, 2, 1, 1, 2, 1}, {}});
  Ped c20 = chain(20);
  c20.name = "chain20";
  peds.push_back(c20);
  for (const Ped &p : peds) drive(p);

  // rejections
  famseq_model m;
  const int32_t id3[] = {1, 2, 3}, half_mo[] = {0, 0, 2}, half_fa[] = {0, 0, 0}, sex3[] = {1, 2, 1};
  CHECK(famseq_model_init(&m, 3, id3, half_mo, half_fa, sex3, nullptr, 1e-7, 1.0) == FAMSEQ_E_PED_HALF);
  const int32_t mo3[] = {0, 0, 1}, fa3[] = {0, 0, 2};
  CHECK(famseq_model_init(&m, 3, id3, mo3, fa3, sex3, nullptr, 1e-7, 1.0) == FAMSEQ_E_PED_SEX);
  CHECK(famseq_model_init(&m, 0, id3, mo3, fa3, sex3, nullptr, 1e-7, 1.0) != 0);
  CHECK(famseq_model_init(&m, 21, id3, mo3, fa3, sex3, nullptr, 1e-7, 1.0) != 0);
  {  // a member who is their own ancestor: refused at famseq_create
    const int32_t good_mo[] = {0, 0, 2}, good_fa[] = {0, 0, 1};
    CHECK(famseq_model_init(&m, 3, id3, good_mo, good_fa, sex3, nullptr, 1e-7, 1.0) == 0);
    m.mother[1] = 2;  // 2's mother is her own child 3 ...
    m.father[1] = 0;
    char err[128] = "";
    CHECK(famseq_create(&m, -1, err, sizeof err) == nullptr && std::strlen(err) > 0);
    CHECK(famseq_create(nullptr, -1, err, sizeof err) == nullptr);
  }
  {  // the size-independent model: a 40-member chain through famseq_pedigree (the generators run, nothing compiles);
     // creation fails for want of a compiler — cleanly, with the reason — and the argument checks hold
    const Ped w = chain(40);
    const int n = (int)w.id.size();
    std::vector<int32_t> mo(n), fa(n);
    famseq_pedigree p;
    CHECK(famseq_pedigree_init(&p, n, w.id.data(), w.mo.data(), w.fa.data(), w.sex.data(), nullptr, 1e-7, 1.0, mo.data(), fa.data()) == 0);
    CHECK(p.n_members == n && p.mother == mo.data() && p.sequenced == nullptr);
    famseq::Model model(p);
    size_t bytes = 0;
    for (int v = 0; v < famseq::kElimVariants; ++v) bytes += famseq::elim_source(model, v).size();
    CHECK(bytes > 100000);
    char err[256] = "";
    CHECK(famseq_create_pedigree(&p, -1, err, sizeof err) == nullptr && std::strstr(err, "sum-product engine only") != nullptr);
    CHECK(famseq_create_pedigree(nullptr, -1, err, sizeof err) == nullptr);
    CHECK(famseq_pedigree_init(&p, n, w.id.data(), w.mo.data(), w.fa.data(), w.sex.data(), nullptr, 1e-7, 1.0, nullptr, fa.data()) == FAMSEQ_E_ARG);
    p.mother = nullptr;  // a struct without its arrays is refused, not dereferenced
    CHECK(famseq_create_pedigree(&p, -1, err, sizeof err) == nullptr);
    std::printf("chain40  N=40 through famseq_pedigree: %zu bytes of generated source\n", bytes);
  }
  double t0[27], t1[27], t2[27];
  for (double mu : {0.0, 1e-7, 1e-3, 0.5}) famseq_transmission_tables(mu, t0, t1, t2);
  CHECK(famseq_last_error(nullptr) != nullptr);
  famseq_destroy(nullptr);
  std::string cmd = std::string("rm -rf '") + dir + "'";
  if (std::system(cmd.c_str()) != 0) ++fails;
  std::printf("asan_host_check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
