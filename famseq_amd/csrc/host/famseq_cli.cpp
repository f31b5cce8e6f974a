// famseq_cli.cpp — FamSeq-compatible command line over libfamseq_hip's C ABI.
//
// Keeps the reference's CLI and file surface for the `-method 1` path:
//   FamSeq vcf -vcfFile f -pedFile p -output o [-v] [-a] [-d] [-o] [-l loc] [-method 1]
//              [-mRate r] [-genoProbN a b c] [-genoProbK a b c] [-genoProbXN a c]
//              [-genoProbXK a c] [-LRC x] [-dnm] [-map] [-siteQ] [-loo] [-afTag KEY | -afTagAll KEY]
//              [-seg dominant|recessive|both -affected ID[,ID...] [-unaffected ID[,ID...]]] [-sample K [-seed S]]
//              [-afEM T [-afStart X]] [-swapCheck FILE] [-mRateScan FILE [-mRateGrid r1,r2,...]] [-phase] [-mapQ]
//              [-segPen F0,F1,F2[/F0,F1,F2...] -affected ID[,ID...] [-unaffected ID[,ID...]]]
//              [-countDist carriers|alleles|homalt [-countOf ID[,ID...]]]
//   FamSeq LK -lkFile f -pedFile p -output o [-lkType n|log10|ln|PS] [...]
// Reference behaviour being reproduced (all cites /root/reference/src):
//   flag parsing + defaults + messages   checkInput.cpp:149-578, 671-1067; FamSeq.cpp:28-156
//   readPed / setFam                     file.cpp:24-62, 1888-1968
//   VCF driver                           file.cpp:108-1004  (header rewrite :143-196, column
//                                        mapping :200-232, location filter :235-360, site rules
//                                        :362-473, Known/chrType :476-486, missing samples
//                                        :488-518, PL/GL -> likelihood :584-592/:821-828,
//                                        failure output :607-620, Phred text :684-765/:922-1001)
//   LK driver                            file.cpp:1640-1886
// Differences by design: ONE pass over the input (the reference reads the file twice), sites are
// queued and evaluated in batches on the GPU (famseq_bn_batch) with the output order preserved,
// -method 2 is the exact sum-product engine (the marginals of the reference's Elston-Stewart peeling), -method 3 (MCMC) is
// not part of this build, -dnm (vcf mode) adds each child's de novo mutation posterior (DNP) from the trio kernel, and -map (vcf
// mode) each member's genotype in the most probable joint configuration of the family and that configuration's posterior (JGT, JP),
// -siteQ (vcf mode) the family's variant quality and the site's log10 likelihood under the pedigree to the INFO column (FQ, FLL),
// -loo (vcf mode) each sample's leave-one-out genotype probabilities and fit (LOP, LOF), and -seg (vcf mode) the posterior probability
// that the variant segregates with the phenotype of the members named by -affected / -unaffected, under a dominant and / or a
// recessive model, to the INFO column (PSD, PSR), and -sample K (vcf mode) each sample's alt-allele counts in K joint configurations
// of the family drawn from their posterior (SGT), and -afEM T (vcf mode) the maximum-likelihood allele frequency among the founders after
// T EM steps and its log10 likelihood ratio against an allele frequency of 0, to the INFO column (FAF, FAL), and -swapCheck FILE (vcf
// mode) writes, behind the last site, the log10 Bayes factor of every two sequenced samples' exchange over the whole file, and
// -mRateScan FILE (vcf mode) the file's log10 likelihood at every mutation rate of a grid, and -phase (vcf mode) each child's genotype
// phased by transmission, maternal|paternal, with its posterior (PGT, PGP), and -segPen (vcf mode) the log10 Bayes factor of the
// phenotypes of -affected / -unaffected under one or more penetrance models, to the INFO column (PSL).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <iostream>
#include <limits>
#include <charconv>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <sstream>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "famseq_hip.h"
#include "fmt_g6.h"

namespace {

using std::string;
using std::vector;

// ---- small text helpers ------------------------------------------------------------------

// normal.cpp:15-53 with trim=false: empty tokens are kept, including a trailing one.
vector<string> split_keep(const string &s, char sep) {
  vector<string> out;
  if (s.empty()) return out;
  size_t head = 0, tail;
  while ((tail = s.find(sep, head)) != string::npos) {
    out.emplace_back(s, head, tail - head);
    head = tail + 1;
  }
  out.emplace_back(s, head);
  return out;
}

// the same split without copies: views into `s` (valid while `s` lives)
void split_views(std::string_view s, char sep, vector<std::string_view> &out) {
  out.clear();
  if (s.empty()) return;
  size_t head = 0, tail;
  while ((tail = s.find(sep, head)) != std::string_view::npos) {
    out.push_back(s.substr(head, tail - head));
    head = tail + 1;
  }
  out.push_back(s.substr(head));
}

// Output text of one formatting thread: appended through a raw pointer (no per-piece capacity checks beyond room()),
// kept from batch to batch.  Numbers go through famseq_fmt::g6 — printf's %g exactly, a third of to_chars' cost.
struct TextBuf {
  vector<char> v;
  size_t n = 0;
  char *room(size_t need) {
    if (v.size() < n + need) v.resize(std::max(v.size() * 2, n + need + (size_t(1) << 16)));
    return v.data() + n;
  }
  void put(const char *s, size_t len) {
    std::memcpy(room(len), s, len);
    n += len;
  }
  void put(std::string_view s) { put(s.data(), s.size()); }
  void ch(char c) { *room(1) = c, ++n; }
  void num(double x) {
    char *p = room(32);
    n += size_t(famseq_fmt::g6(p, x) - p);
  }
  // "a,b,c:d,e,f:" — the GPP and FPP triples of one sample
  void triples(const double *g, const double *f) {
    char *p = room(6 * 32 + 8), *q = p;
    q = famseq_fmt::g6(q, g[0]), *q++ = ',';
    q = famseq_fmt::g6(q, g[1]), *q++ = ',';
    q = famseq_fmt::g6(q, g[2]), *q++ = ':';
    q = famseq_fmt::g6(q, f[0]), *q++ = ',';
    q = famseq_fmt::g6(q, f[1]), *q++ = ',';
    q = famseq_fmt::g6(q, f[2]), *q++ = ':';
    n += size_t(q - p);
  }
  // the same as the device wrote it (famseq_bn_call_text_batch): "a,b,c:d,e,f:0/1\t", FAMSEQ_TEXT_STRIDE bytes, the count in the last
  void record(const char *r) {
    char *p = room(FAMSEQ_TEXT_STRIDE);
    std::memcpy(p, r, FAMSEQ_TEXT_STRIDE);
    n += size_t((unsigned char)r[FAMSEQ_TEXT_STRIDE - 1]);
  }
  // Called sample `at` (site * samples + column) of a batch, from the device's records or, where text is null, from its numbers.
  // tab = false leaves the closing tab to the caller, who has more fields to put in front of it.
  void called(const char *text, const double *gpp, const double *fpp, const int8_t *fgt, size_t at, bool tab = true) {
    if (text) {
      record(text + at * FAMSEQ_TEXT_STRIDE);
      n -= !tab;
    } else {
      triples(gpp + 3 * at, fpp + 3 * at);
      put(fgt[at] == 0 ? "0/0\t" : (fgt[at] == 1 ? "0/1\t" : "1/1\t"), tab ? 4 : 3);
    }
  }
};

// Where the numbers become text: on the device (default — one more streaming kernel behind the call kernel, a record per
// sample comes back: famseq_bn_call_text_batch) or on the host's cores (FAMSEQ_HOST_FORMAT=1: famseq_fmt::g6, sixty calls per
// ten-member site, 0.74 of the 0.88 s loop per 3 M sites on 16 threads).  Both print the same bytes (csrc/g6_core.h).
bool device_text() {
  const char *e = std::getenv("FAMSEQ_HOST_FORMAT");
  return !(e && std::atoi(e) != 0);
}

// pow(10, -|x|/10) for a PL/GL field (file.cpp:588-590).  Integer fields (the usual PL) go
// through a table filled with the same libm pow call, so the value is identical.
struct PlTable {
  vector<double> lut;
  PlTable() : lut(4096) {
    for (size_t k = 0; k < lut.size(); ++k) lut[k] = std::pow(10.0, -std::fabs(double(k)) / 10.0);
  }
  // the likelihood of a packed integer PL: what operator() returned when it packed it
  double value(uint16_t v) const { return v < lut.size() ? lut[v] : std::pow(10.0, -std::fabs(double(v)) / 10.0); }
  // *packed receives the integer PL (clamped to 65534: anything >= 3240 is exactly 0 anyway) or
  // is left untouched and *integral cleared when the field is not a plain non-negative integer.
  double operator()(const char *b, const char *e, uint16_t *packed, bool *integral) const {
    unsigned long v = 0;
    const char *p = b;
    while (p < e && *p >= '0' && *p <= '9' && v < 100000000ul) v = v * 10 + unsigned(*p++ - '0');
    if (p == e && p > b) {
      *packed = uint16_t(v < 65534 ? v : 65534);
      return v < lut.size() ? lut[v] : std::pow(10.0, -std::fabs(double(v)) / 10.0);
    }
    *integral = false;
    const double x = std::atof(string(b, e).c_str());
    return std::pow(10.0, -std::fabs(x) / 10.0);
  }
};

// ---- options -----------------------------------------------------------------------------

struct Options {
  bool lk_mode = false;
  bool pack_mode = false;  // `FamSeq pack`: vcf -> packed binary PL file (no GPU)
  bool tune_mode = false;  // `FamSeq tune`: time this pedigree's kernel variants on this GPU, keep the winners' indices in the kernel cache
  bool pl_mode = false;    // `FamSeq PL`: packed binary PL file -> calls
  bool unpack_mode = false;  // `FamSeq unpack`: packed PL file + packed result file -> the text `FamSeq PL` writes
  bool bin_output = false;   // `FamSeq PL -binOutput`: results as a packed result file, not as text
  string pl_file, po_file;
  vector<string> vcf_files;
  string lk_file, ped_file, out_file, loc_file;
  bool var_only = false, all_line = false, diff_only = false, pos_order = false;
  int method = 1, lk_type = 1;
  double mrate = 1e-7, lrc = 1;
  vector<double> gN, gK, gXN, gXK;
  int num_burn = -999, num_rep = -999;
  bool dnm = false;  // -dnm: a DNP field per sample (vcf mode)
  bool map = false;  // -map: JGT and JP fields per sample (vcf mode)
  bool siteq = false;  // -siteQ: FQ and FLL keys in the INFO column (vcf mode)
  bool phase = false;  // -phase: PGT and PGP fields per sample, the phased genotype by transmission and its probability (vcf mode)
  bool loo = false;    // -loo: LOP and LOF fields per sample, the leave-one-out posteriors and the member's fit (vcf mode)
  bool mapq = false;   // -mapQ: a JGQ field per sample, the quality of its joint call, and the runner-up's JP2 in the INFO column (vcf mode)
  int sample = 0;      // -sample K: an SGT field per sample, its alt-allele counts in K joint posterior draws of the family (vcf mode)
  uint64_t seed = 0;   // -seed S: the draws' seed
  // -seg dominant|recessive|both: PSD and / or PSR keys in the INFO column (vcf mode), the posterior probability of the genotype
  // pattern that model gives the members of -affected and -unaffected (PED IDs, comma-separated)
  string seg, affected, unaffected;
  // -segPen F0,F1,F2[/F0,F1,F2...]: for each penetrance model (the probability of being affected given 0, 1, 2 alt alleles) the
  // log10 Bayes factor of the phenotypes of -affected / -unaffected (vcf mode).  pen: three numbers per model; pen_bad: the first
  // model that is not three numbers in [0, 1], as it was given
  bool pen_given = false, pen_is_bad = false;
  vector<double> pen;
  string pen_bad;
  // -afEM T [-afStart X]: FAF and FAL keys in the INFO column (vcf mode), the founders' allele frequency after T EM steps from X and
  // the log10 likelihood ratio against "no founder carries the allele" (kAfUnset: not given; kAfBad: given, not a number)
  static constexpr int kAfUnset = -1, kAfBad = -2;
  int af_em = kAfUnset;
  double af_start = 0.5;
  bool af_start_given = false;
  // -swapCheck FILE: after the last site, the report of every two sequenced samples' exchange (vcf mode): the log10 Bayes factor
  // of the file's fit to the pedigree with the two relabelled against the labelling as given
  string swap_file;
  bool swap_given = false;
  // -mRateScan FILE [-mRateGrid r1,r2,...]: after the last site, the file's log10 likelihood at every mutation rate of the grid
  // (vcf mode).  rate_grid_bad: the first entry of -mRateGrid that is no number in [0, 1], as it was given
  string rate_file;
  bool rate_scan_given = false, rate_grid_given = false, rate_grid_is_bad = false;
  vector<double> rate_grid = {0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3};
  string rate_grid_bad;
  // -countDist carriers|alleles|homalt [-countOf ID[,ID...]]: a PCD key in the INFO column (vcf mode), the exact posterior
  // distribution of the number of carriers / alt alleles / hom-alt members among the members of -countOf (PED IDs; default all)
  bool count_given = false, count_of_given = false;
  string count_kind, count_of;
  string af_tag;     // -afTag KEY: the founders' prior of a line from the allele frequency KEY= of its INFO column (vcf mode)
  bool af_conflict = false;  // both -afTag and -afTagAll were given
  bool af_all = false;  // -afTagAll KEY: -afTag KEY, applied to every field a line prints (DNP, JGT and JP too: may go with -dnm / -map)
};

// returns 0 good, 1 warnings, -1 stop (checkInput.h:345-349)
int parse_options(int argc, char **argv, Options &o) {
  int rv = 0;
  auto missing = [&](int i) { return i == argc || argv[i][0] == '-'; };
  for (int i = 2; i < argc; i++) {
    if (argv[i][0] != '-') {
      std::cout << "Cannot recognize parameter: \"" << argv[i] << "\" in the command." << std::endl;
      rv = 1;
      continue;
    }
    const string opt(argv[i] + 1);
    auto need_file = [&](string &dst, const char *what) {
      i++;
      if (missing(i)) {
        std::cout << "The " << what << " hasn't been set. Please check input." << std::endl;
        return false;
      }
      dst = argv[i];
      return true;
    };
    auto probs = [&](vector<double> &dst, int n, const char *msg) {
      vector<double> tmp(3, 0);
      for (int j = 0; j < n; j++) {
        i++;
        if (missing(i)) {
          std::cout << msg << std::endl;
          i--;
          rv = 1;
          return;
        }
        tmp[n == 3 ? j : 2 * j] = std::atof(argv[i]);  // X priors: {a, 0, c} (checkInput.cpp:340-372)
      }
      dst = tmp;
    };
    if (!o.lk_mode && opt == "vcfFile") {
      bool first = true;
      while (true) {
        i++;
        if (first && missing(i)) {
          std::cout << "The vcf file hasn't been set. Please check input." << std::endl;
          return -1;
        }
        first = false;
        if (missing(i)) {
          i--;
          break;
        }
        o.vcf_files.push_back(argv[i]);
      }
    } else if (o.pl_mode && opt == "plFile") {
      if (!need_file(o.pl_file, "packed PL file")) return -1;
    } else if (o.unpack_mode && opt == "poFile") {
      if (!need_file(o.po_file, "packed result file")) return -1;
    } else if (o.pl_mode && !o.unpack_mode && opt == "binOutput") {
      o.bin_output = true;
    } else if (o.lk_mode && opt == "lkFile") {
      if (!need_file(o.lk_file, "likelihood file")) return -1;
    } else if (opt == "pedFile") {
      if (!need_file(o.ped_file, "ped file")) return -1;
    } else if (!o.lk_mode && opt == "l") {
      if (!need_file(o.loc_file, "location file")) return -1;
    } else if (opt == "output") {
      if (!need_file(o.out_file, "output file")) return -1;
    } else if (!o.lk_mode && opt == "v") {
      o.var_only = true;
    } else if (!o.lk_mode && opt == "a") {
      o.all_line = true;
    } else if (!o.lk_mode && opt == "d") {
      o.diff_only = true;
    } else if (!o.lk_mode && opt == "o") {
      o.pos_order = true;
    } else if (opt == "method") {
      i++;
      if (missing(i)) {
        std::cout << "Method hasn't been set. The default method (BN) will be used." << std::endl;
        i--;
        rv = 1;
      } else {
        o.method = std::atoi(argv[i]);
      }
    } else if (opt == "mRate") {
      i++;
      if (missing(i)) {
        std::cout << "Mutation rate hasn't been set. The default (1e-7) will be used." << std::endl;
        i--;
        rv = 1;
      } else {
        o.mrate = std::atof(argv[i]);
      }
    } else if (o.lk_mode && opt == "lkType") {
      i++;
      if (missing(i)) {
        std::cout << "Likelihood type hasn't been set. The default normal (n) will be used." << std::endl;
        i--;
        rv = 1;
      } else {
        const string t(argv[i]);
        if (t == "n") o.lk_type = 1;
        else if (t == "log10") o.lk_type = 2;
        else if (t == "ln") o.lk_type = 3;
        else if (t == "PS") o.lk_type = 4;
        else {
          std::cout << "Cannot recognize the likelihood type: " << t << ". The default normal (n) will be used." << std::endl;
          o.lk_type = 1;
          rv = 1;
        }
      }
    } else if (opt == "genoProbN") {
      probs(o.gN, 3, "genoProbN hasn't been set. The default (0.9985,0.001,0.0005) will be used.");
    } else if (opt == "genoProbK") {
      probs(o.gK, 3, "genoProbK hasn't been set. The default (0.45,0.1,0.45) will be used.");
    } else if (opt == "genoProbXN") {
      probs(o.gXN, 2, "genoProbN hasn't been set. The default (0.999,0.001) will be used.");
    } else if (opt == "genoProbXK") {
      probs(o.gXK, 2, "genoProbN hasn't been set. The default (0.5,0.5) will be used.");
    } else if (opt == "numBurnIn" || opt == "numRep") {
      i++;
      if (missing(i)) {
        std::cout << "Number of " << (opt == "numRep" ? "MCMC repeat" : "burn in")
                  << " times hasn't been set. The default will be used." << std::endl;
        i--;
        rv = 1;
      } else {
        (opt == "numRep" ? o.num_rep : o.num_burn) = std::atoi(argv[i]);
      }
    } else if (opt == "dnm") {
      o.dnm = true;
    } else if (opt == "map") {
      o.map = true;
    } else if (opt == "siteQ") {
      o.siteq = true;
    } else if (opt == "loo") {
      o.loo = true;
    } else if (opt == "phase") {
      o.phase = true;
    } else if (opt == "mapQ") {
      o.mapq = true;
    } else if (opt == "sample" || opt == "seed") {
      i++;
      if (missing(i)) {
        std::cout << "The value of -" << opt << " hasn't been set. The option is ignored." << std::endl;
        i--;
        rv = 1;
      } else if (opt == "seed") {
        o.seed = std::strtoull(argv[i], nullptr, 10);
      } else {
        o.sample = std::atoi(argv[i]);
        if (o.sample < 1 || o.sample > FAMSEQ_MAX_DRAWS) {
          std::cout << "-sample takes the number of draws per site, 1.." << FAMSEQ_MAX_DRAWS << ", not \"" << argv[i] << "\". The option is ignored."
                    << std::endl;
          o.sample = 0;
          rv = 1;
        }
      }
    } else if (opt == "afEM" || opt == "afStart") {
      i++;
      if (missing(i)) {
        std::cout << "The value of -" << opt << " hasn't been set. The option is ignored." << std::endl;
        i--;
        rv = 1;
      } else {  // (what the value may be: check_af_em, with the other side options' checks)
        char *end = nullptr;
        if (opt == "afEM") {
          const long t = std::strtol(argv[i], &end, 10);
          o.af_em = end == argv[i] || *end || t < 0 || t > 1000000 ? Options::kAfBad : (int)t;
        } else {
          o.af_start = std::strtod(argv[i], &end);
          if (end == argv[i] || *end) o.af_start = -1;
          o.af_start_given = true;
        }
      }
    } else if (opt == "swapCheck") {
      i++;
      if (missing(i)) {
        std::cout << "The report file of -swapCheck hasn't been set. The option is ignored." << std::endl;
        i--;
        rv = 1;
      } else {
        o.swap_file = argv[i];
        o.swap_given = true;
      }
    } else if (opt == "mRateScan") {  // (what may be wrong with either: check_rate_scan, with the other side options' checks)
      o.rate_scan_given = true;
      if (!missing(i + 1)) o.rate_file = argv[++i];
    } else if (opt == "mRateGrid") {
      o.rate_grid_given = true;
      o.rate_grid.clear();
      // (no value, or one that starts like an option: the grid stays empty, which check_rate_scan refuses)
      const string text = missing(i + 1) ? "" : argv[++i];
      for (size_t at = 0; !text.empty() && at <= text.size();) {
        const size_t end = std::min(text.find(',', at), text.size());
        const string entry = text.substr(at, end - at);
        char *stop = nullptr;
        const double v = std::strtod(entry.c_str(), &stop);
        if ((entry.empty() || *stop || !(v >= 0.0 && v <= 1.0)) && !o.rate_grid_is_bad) o.rate_grid_is_bad = true, o.rate_grid_bad = entry;
        o.rate_grid.push_back(v);
        at = end + 1;
      }
    } else if (opt == "segPen") {  // (what may be wrong with it: check_seg_pen, with the other side options' checks)
      o.pen_given = true;
      o.pen.clear();
      // (no value, or one that starts like an option: one empty model, which check_seg_pen refuses)
      const string text = missing(i + 1) ? "" : argv[++i];
      for (size_t at = 0; at <= text.size();) {
        const size_t end = std::min(text.find('/', at), text.size());
        const string model = text.substr(at, end - at);
        int got = 0;
        bool bad = false;
        for (size_t f = 0; f <= model.size();) {
          const size_t fe = std::min(model.find(',', f), model.size());
          const string entry = model.substr(f, fe - f);
          char *stop = nullptr;
          const double v = std::strtod(entry.c_str(), &stop);
          bad = bad || entry.empty() || *stop || !(v >= 0.0 && v <= 1.0);
          if (got < 3) o.pen.push_back(v);
          ++got, f = fe + 1;
        }
        if ((bad || got != 3) && !o.pen_is_bad) o.pen_is_bad = true, o.pen_bad = model;
        for (; got < 3; ++got) o.pen.push_back(0.0);
        at = end + 1;
      }
    } else if (opt == "countDist" || opt == "countOf") {  // (what may be wrong with either: check_count_dist, with the other side options' checks)
      // (no value, or one that starts like an option: an empty one, which check_count_dist refuses)
      (opt == "countDist" ? o.count_given : o.count_of_given) = true;
      (opt == "countDist" ? o.count_kind : o.count_of) = missing(i + 1) ? "" : argv[++i];
    } else if (opt == "seg" || opt == "affected" || opt == "unaffected") {
      i++;
      if (missing(i)) {
        std::cout << "The value of -" << opt << " hasn't been set. The option is ignored." << std::endl;
        i--;
        rv = 1;
      } else {
        (opt == "seg" ? o.seg : (opt == "affected" ? o.affected : o.unaffected)) = argv[i];
      }
    } else if (opt == "afTag" || opt == "afTagAll") {
      i++;
      if (missing(i)) {
        std::cout << "The INFO key of -" << opt << " hasn't been set. The option is ignored." << std::endl;
        i--;
        rv = 1;
      } else if (!o.af_tag.empty() && o.af_all != (opt == "afTagAll")) {
        o.af_conflict = true;
      } else {
        o.af_tag = argv[i];
        o.af_all = opt == "afTagAll";
      }
    } else if (opt == "LRC") {
      i++;
      if (missing(i)) {
        std::cerr << "Likelihood ratio criteria is not set. The default will be used." << std::endl;
        i--;
        rv = 1;
      } else {
        o.lrc = std::atof(argv[i]);
      }
    } else {
      std::cout << "Cannot recognize option: \"" << opt << "\" in the command." << std::endl;
      rv = 1;
    }
  }
  if (!o.lk_mode && o.vcf_files.empty()) {
    std::cout << "The name of vcf file must be set. Please input the vcf file name." << std::endl;
    return -1;
  }
  if (o.pl_mode && o.pl_file.empty()) {
    std::cout << "The name of packed PL file must be set. Please input the file name (-plFile)." << std::endl;
    return -1;
  }
  if (o.unpack_mode && o.po_file.empty()) {
    std::cout << "The name of packed result file must be set. Please input the file name (-poFile)." << std::endl;
    return -1;
  }
  if (o.lk_mode && !o.pl_mode && o.lk_file.empty()) {
    std::cout << "The name of likelihood file must be set. Please input the likelihood file name." << std::endl;
    return -1;
  }
  if (o.ped_file.empty()) {
    std::cout << "The name of ped file must be set. Please input the ped file name." << std::endl;
    return -1;
  }
  if (o.out_file.empty() && !o.tune_mode) {
    std::cout << "The name of output file must be set. Please input the output file name." << std::endl;
    return -1;
  }
  if (o.method < 1 || o.method > 3) {
    std::cout << "Method could only be 1 or 3. The default method (BN) will be used." << std::endl;
    o.method = 1;
    rv = 1;
  }
  if (o.mrate < 0 || o.mrate > 0.5) {
    std::cout << "Mutation rate is set out of range. The default (1e-7) will be used." << std::endl;
    o.mrate = 1e-7;
    rv = 1;
  }
  if (o.var_only && o.all_line) {
    std::cout << "varOnly is setted, allLine is blocked." << std::endl;
    o.all_line = false;
    rv = 1;
  }
  if (o.lrc < 0) {
    std::cerr << "Likelihood ration criteria is not set correctly. The default will be used." << std::endl;
    o.lrc = 1;
    rv = 1;
  }
  if (o.diff_only) {  // file.cpp:124-128
    o.all_line = false;
    o.var_only = true;
  }
  return rv;
}

// ---- pedigree ------------------------------------------------------------------------------

struct Ped {
  vector<int32_t> id, mid, fid, gender;
  vector<string> name;
  int n() const { return (int)id.size(); }
};

bool read_ped(const string &path, Ped &p) {  // file.cpp:24-62
  std::ifstream fin(path.c_str());
  if (!fin.is_open()) {
    std::cout << "Cannot open " << path << std::endl;
    return false;
  }
  string line;
  std::getline(fin, line);
  while (std::getline(fin, line)) {
    if (line.size() < 2) break;
    std::istringstream in(line);
    int a = 0, b = 0, c = 0, d = 0;
    string nm;
    in >> a >> b >> c >> d >> nm;
    p.id.push_back(a);
    p.mid.push_back(b);
    p.fid.push_back(c);
    p.gender.push_back(d);
    p.name.push_back(nm);
  }
  return true;
}

// The sample columns of an input matched to PED members by name (file.cpp:200-232, :1671-1689: a column takes the first member
// of its name); columns that are not in the PED are ignored.
struct ColumnMap {
  vector<int> member;         // [column] its PED index, -1: not in the PED
  vector<uint8_t> sequenced;  // [PED index] some column is this member's
  vector<int> cols;           // the matched columns in input order ...
  vector<int32_t> members;    // ... and their PED indices
};

ColumnMap map_columns(const string *names, size_t n, const Ped &ped) {
  ColumnMap cm;
  cm.member.assign(n, -1);
  cm.sequenced.assign(ped.n(), 0);
  for (size_t i = 0; i < n; i++)
    for (int j = 0; j < ped.n(); j++)
      if (names[i] == ped.name[j]) {
        cm.member[i] = j;
        cm.sequenced[j] = 1;
        cm.cols.push_back((int)i);
        cm.members.push_back(j);
        break;
      }
  return cm;
}

// The header lines of the three fields every driver adds; GPP's description names the method in the spelling of its driver.
void put_format_header(std::ostream &out, const char *gpp_by) {
  out << "##FORMAT=<ID=GPP,Number=G,Type=Integer,Description=\"Normalized, Phred-scaled for posterior probability " << gpp_by << "\">"
      << std::endl;
  out << "##FORMAT=<ID=FPP,Number=G,Type=Integer,Description=\"Normalized, Phred-scaled for posterior probability "
         "calculated by FamSeqPro\">" << std::endl;
  out << "##FORMAT=<ID=FGT,Number=1,Type=String,Description=\"Genotype called by FamSeqPro\">" << std::endl;
}

// ---- batched caller: queue of output records, flushed through the GPU in order -------------

struct Record {
  string text;     // literal line (site < 0); unused for computed lines
  long site = -1;  // index into the pending batch, -1 for literal records
  string raw;      // the input line: computed lines print pieces of it (and the failure warning all of it)
  uint32_t prefix_len = 0;  // columns 1-9 of raw, without the tab after FORMAT (vcf mode)
  const char *head = nullptr;  // LK mode: a fixed first column instead
  uint32_t n_fmt = 0;       // FORMAT keys: a missing sample prints that many "NA:"
  struct Sample {
    uint32_t off, len;  // the sample's field in raw
    bool missing;       // shorter than 5 characters (file.cpp:565): printed as NA per FORMAT key
  };
  vector<Sample> samples;  // sequenced samples, in output column order
};

double now_s();

// n items in at most `parts` contiguous ranges, one thread each: f(lo, hi, part).  Returns the number of parts.
template <class F>
int parallel_ranges(size_t n, F f) {
  unsigned t = std::thread::hardware_concurrency();
  if (const char *e = std::getenv("FAMSEQ_THREADS")) t = (unsigned)std::atoi(e);
  t = std::max(1u, std::min(t, 32u));
  if (n < 2048) t = 1;
  vector<std::thread> pool;
  for (unsigned k = 1; k < t; ++k) pool.emplace_back([=] { f(n * k / t, n * (k + 1) / t, (int)k); });
  f(0, n / t, 0);
  for (std::thread &th : pool) th.join();
  return (int)t;
}
template <class F>
void parallel_for(size_t n, F f) {
  parallel_ranges(n, [&](size_t lo, size_t hi, int) {
    for (size_t i = lo; i < hi; ++i) f(i);
  });
}

// Queue of output records between the LK driver's line loop and the GPU (the vcf driver has its own block
// pipeline, run_vcf).  Records are kept in input order; a full batch is handed to a flusher thread — GPU call
// (famseq_bn_call_batch: posterior, Phred scaling and genotype call all on the device), formatting on all
// cores, one write per formatting thread — while the driver's thread goes on filling the next batch.
class BatchCaller {
 public:
  double t_gpu = 0, t_format = 0, t_write = 0, t_stall = 0;  // FAMSEQ_TIMING: where the flusher spends its time; driver waiting for it
  BatchCaller(famseq_ctx *ctx, int n_members, const vector<int32_t> &seq_members, std::ostream &out, size_t cap)
      : ctx_(ctx), n_(n_members), seq_(seq_members.begin(), seq_members.end()), out_(out), cap_(cap) {}
  ~BatchCaller() { wait(); }

  void literal(string line) {
    Record r;
    r.text = std::move(line);
    cur_.q.push_back(std::move(r));
  }
  // lk: N x 3 in PED order; pl: n_seq x 3 packed integer PLs in column order, or NULL when some
  // field of the site is not a plain integer (the batch then goes through the fp64 input)
  bool site(Record &&r, const vector<double> &lk, const uint16_t *pl, uint8_t flags) {
    r.site = (long)cur_.flags.size();
    cur_.lk.insert(cur_.lk.end(), lk.begin(), lk.end());
    if (pl && cur_.packed_ok) cur_.pl.insert(cur_.pl.end(), pl, pl + 3 * seq_.size());
    else cur_.packed_ok = false;
    cur_.flags.push_back(flags);
    cur_.q.push_back(std::move(r));
    return cur_.flags.size() < cap_ || submit();
  }
  // Everything queued so far is computed and written when this returns.
  bool flush() {
    const bool ok = submit();
    wait();
    return ok && ok_;
  }

 private:
  struct Batch {
    vector<Record> q;
    vector<double> lk;
    vector<uint16_t> pl;
    vector<uint8_t> flags;
    bool packed_ok = true;
    void clear() {
      q.clear();
      lk.clear();
      pl.clear();
      flags.clear();
      packed_ok = true;
    }
  };

  void wait() {
    if (worker_.joinable()) {
      const double t0 = now_s();
      worker_.join();
      t_stall += now_s() - t0;
    }
  }
  // hand the current batch to the flusher (after the previous one is through) and start a fresh one
  bool submit() {
    wait();
    if (!ok_) return false;
    std::swap(cur_, fly_);
    cur_.clear();
    worker_ = std::thread([this] { ok_ = write_out(fly_); });
    return true;
  }

  bool write_out(Batch &b) {
    const int64_t s = (int64_t)b.flags.size();
    const size_t k = seq_.size();
    gpp_.resize(size_t(s) * k * 3);
    fpp_.resize(size_t(s) * k * 3);
    fgt_.resize(size_t(s) * k);
    status_.resize(b.flags.size());
    const double t0 = now_s();
    if (s > 0) {
      const bool packed = b.packed_ok && !b.pl.empty();
      const int rc = famseq_bn_call_batch(ctx_, s, packed ? nullptr : b.lk.data(), packed ? b.pl.data() : nullptr,
                                          b.flags.data(), seq_.data(), (int32_t)k, gpp_.data(), fpp_.data(), fgt_.data(),
                                          status_.data());
      if (rc != 0) {
        std::cerr << "famseq_bn_call_batch failed (" << rc << "): " << famseq_last_error(ctx_) << std::endl;
        return false;
      }
    }
    const double t1 = now_s();
    t_gpu += t1 - t0;
    // every formatting thread appends its contiguous range of records to one buffer: T writes per batch
    if (text_.size() < 64) text_.resize(64);
    const int parts = parallel_ranges(b.q.size(), [&](size_t lo, size_t hi, int part) {
      TextBuf &line = text_[part];
      line.n = 0;
      for (size_t i = lo; i < hi; ++i) {
        const Record &r = b.q[i];
        if (r.site < 0) {
          line.put(r.text);
        } else {
          if (r.head) {
            line.put(r.head, std::strlen(r.head));
          } else {
            line.put(r.raw.data(), r.prefix_len);  // columns 1-8 + FORMAT
            line.put(":GPP:FPP:FGT\t", 13);
          }
          if (status_[r.site] & 3) {  // file.cpp:607-620
            for (const Record::Sample &sm : r.samples) {
              line.put(r.raw.data() + sm.off, sm.len);
              line.put(":NA:NA:NA\t", 10);
            }
          } else {
            for (size_t j = 0; j < k; ++j) {
              const Record::Sample &sm = r.samples[j];
              if (sm.missing) {
                for (uint32_t q = 0; q < r.n_fmt; ++q) line.put("NA:", 3);
              } else {
                line.put(r.raw.data() + sm.off, sm.len);
                line.ch(':');
              }
              line.called(nullptr, gpp_.data(), fpp_.data(), fgt_.data(), size_t(r.site) * k + j);
            }
          }
        }
        line.ch('\n');
      }
    });
    const double t2 = now_s();
    t_format += t2 - t1;
    for (const Record &r : b.q)  // the reference's warning on stdout, in input order (file.cpp:607-612)
      if (r.site >= 0 && (status_[r.site] & 3))
        std::cout << "Warning: this variant hasn't been calculated: " << std::endl << r.raw << std::endl;
    for (int part = 0; part < parts; ++part) out_.write(text_[part].v.data(), (std::streamsize)text_[part].n);
    t_write += now_s() - t2;
    return true;
  }

  famseq_ctx *ctx_;
  int n_;
  vector<int32_t> seq_;  // PED index of each sequenced output column, in input column order
  std::ostream &out_;
  size_t cap_;
  Batch cur_, fly_;  // being filled by the driver / being written out by the flusher
  std::thread worker_;
  bool ok_ = true;
  vector<double> gpp_, fpp_;
  vector<int8_t> fgt_;
  vector<uint8_t> status_;
  vector<TextBuf> text_;
};

size_t batch_capacity() {
  const char *e = std::getenv("FAMSEQ_BATCH");
  const long v = e ? std::atol(e) : 0;
  return v > 0 ? size_t(v) : size_t(1) << 16;
}

// ---- model + ctx ---------------------------------------------------------------------------

// The size-independent model of the ABI (famseq_pedigree) with the arrays it points into: the reference's drivers
// take a PED file of any length (readPed, file.cpp:24-62), and so does its -method 2.
struct CliModel {
  famseq_pedigree p;
  vector<int32_t> mo, fa;
  vector<uint8_t> seq;
  int init(const Ped &ped, const vector<uint8_t> &sequenced, double mrate, double lrc) {
    mo.assign(ped.n(), -1);
    fa.assign(ped.n(), -1);
    seq = sequenced;
    return famseq_pedigree_init(&p, ped.n(), ped.id.data(), ped.mid.data(), ped.fid.data(), ped.gender.data(), seq.data(), mrate,
                                lrc, mo.data(), fa.data());
  }
  void set_priors(const Options &o) {  // -genoProbN ...: the ones that were given
    const vector<double> *src[4] = {&o.gN, &o.gK, &o.gXN, &o.gXK};
    double *dst[4] = {p.genoProbN, p.genoProbK, p.genoProbXN, p.genoProbXK};
    for (int k = 0; k < 4; ++k)
      if (src[k]->size() == 3) std::copy(src[k]->begin(), src[k]->end(), dst[k]);
  }
};

famseq_ctx *make_ctx(const Options &o, const Ped &ped, const vector<uint8_t> &sequenced, CliModel &m) {
  const int rc = m.init(ped, sequenced, o.mrate, o.lrc);
  if (rc == FAMSEQ_E_PED_HALF) std::cout << "This is not a fulfill family. Please check the ped file." << std::endl;
  if (rc == FAMSEQ_E_PED_SEX) std::cerr << "A mother is not a female or a father is not a male in the ped file." << std::endl;
  if (rc != 0) {
    std::cout << "Cannot initiate family. Please check ped file." << std::endl;
    return nullptr;
  }
  m.set_priors(o);
  const char *dev = std::getenv("FAMSEQ_DEVICE");
  char err[512] = {0};
  if (ped.n() > FAMSEQ_MAX_MEMBERS && o.method != 2) {  // the reference's own advice for -method 1 is "family size less than seven"
    std::cout << "The pedigree has " << ped.n() << " members: -method 1 enumerates 3^N joint genotypes and serves up to "
              << FAMSEQ_MAX_MEMBERS << ". Use -method 2 for this pedigree." << std::endl;
    return nullptr;
  }
  famseq_ctx *ctx = famseq_create_pedigree(&m.p, dev ? std::atoi(dev) : 0, err, sizeof err);
  if (!ctx) {
    std::cerr << "Cannot create the GPU context: " << err << std::endl;
    return nullptr;
  }
  // -method 2 (the reference's Elston-Stewart peeling, family.cpp:1126-1403) computes the same
  // marginals exactly: here that is the sum-product engine (loops are handled by conditioning on up
  // to three members).
  if (o.method == 2 && famseq_set_option(ctx, "engine", FAMSEQ_ENGINE_ELIM) != 0) {
    std::cout << "-method 2 cannot serve this pedigree: " << famseq_last_error(ctx) << std::endl
              << "Use -method 1 for this pedigree." << std::endl;
    famseq_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

// -dnm, -map, -siteQ, -loo, -afTag / -afTagAll (flag_text: the one to name): does the sum-product engine, which their kernels are forms
// of, serve this pedigree?  Asked on a plan-only context before any input is read.
bool sum_product_serves(const Options &o, const Ped &ped, const char *flag_text) {
  CliModel m;
  vector<uint8_t> all(ped.n(), 1);
  if (m.init(ped, all, o.mrate, o.lrc) != 0) return true;  // (the driver reports a bad pedigree itself)
  char err[512] = {0};
  famseq_ctx *probe = famseq_create_pedigree(&m.p, -1, err, sizeof err);
  const int k = probe ? famseq_trio_children(probe, nullptr) : FAMSEQ_E_ARG;  // (elim_supported: what every loader asks first)
  if (k < 0) std::cout << flag_text << " cannot serve this pedigree: " << (probe ? famseq_last_error(probe) : err) << std::endl;
  famseq_destroy(probe);
  return k >= 0;
}

bool phenotype_roles(const Options &o, const Ped &ped, vector<int> &role);

// -seg: the mask rows of its patterns in the order they are printed (PSD, PSR), [n_patterns][N] in PED order, from the PED IDs of
// -affected and -unaffected.  false with a message: an unknown model, no -affected, an ID the PED file does not hold, an ID in both.
bool segregation_masks(const Options &o, const Ped &ped, vector<uint8_t> &masks, vector<const char *> &keys) {
  if (o.seg != "dominant" && o.seg != "recessive" && o.seg != "both") {
    std::cout << "-seg takes dominant, recessive or both, not \"" << o.seg << "\"." << std::endl;
    return false;
  }
  if (o.affected.empty()) {
    std::cout << "-seg needs the affected members: -affected ID[,ID...] (PED IDs)." << std::endl;
    return false;
  }
  vector<int> role;
  if (!phenotype_roles(o, ped, role)) return false;
  masks.clear(), keys.clear();
  for (int model = 0; model < 2; ++model) {  // dominant: affected 6, unaffected 1; recessive: 4, 3; anyone else 7
    if (o.seg != "both" && o.seg != (model ? "recessive" : "dominant")) continue;
    keys.push_back(model ? "PSR=" : "PSD=");
    for (int i = 0; i < ped.n(); ++i) masks.push_back(role[i] == 1 ? (model ? 4 : 6) : (role[i] == 2 ? (model ? 3 : 1) : 7));
  }
  return true;
}

// The members of -affected and -unaffected (-seg, -segPen): role[i] of member i (PED order) 1 affected, 2 unaffected, 0 neither.
// false with a message: an ID the PED file does not hold, an ID in both.
bool phenotype_roles(const Options &o, const Ped &ped, vector<int> &role) {
  role.assign(ped.n(), 0);
  for (int r = 1; r <= 2; ++r) {
    std::istringstream in(r == 1 ? o.affected : o.unaffected);
    string tok;
    while (std::getline(in, tok, ',')) {
      char *end = nullptr;
      const long id = std::strtol(tok.c_str(), &end, 10);
      int at = -1;
      for (int i = 0; i < ped.n() && !tok.empty() && *end == 0; ++i)
        if (ped.id[i] == id) at = i;
      if (at < 0) {
        std::cout << (r == 1 ? "-affected" : "-unaffected") << ": \"" << tok << "\" is not an individual ID of the PED file." << std::endl;
        return false;
      }
      if (role[at] != 0 && role[at] != r) {
        std::cout << "Individual " << tok << " is listed both as affected and as unaffected." << std::endl;
        return false;
      }
      role[at] = r;
    }
  }
  return true;
}

// -segPen: the weight tables of its models, [n_models][N][3] in PED order: an affected member's row is the model's (f0, f1, f2),
// an unaffected member's 1 - f, anyone else's ones.  false with a message, as phenotype_roles.
bool penetrance_tables(const Options &o, const Ped &ped, vector<double> &tables) {
  vector<int> role;
  if (!phenotype_roles(o, ped, role)) return false;
  tables.clear();
  for (size_t m = 0; m < o.pen.size() / 3; ++m)
    for (int i = 0; i < ped.n(); ++i)
      for (int g = 0; g < 3; ++g) tables.push_back(role[i] == 1 ? o.pen[3 * m + g] : (role[i] == 2 ? 1.0 - o.pen[3 * m + g] : 1.0));
  return true;
}

// -countDist: the score of each genotype of a counted member, by kind; null for a kind it does not know
const int *count_kind_scores(const string &kind) {
  static const int carriers[3] = {0, 1, 1}, alleles[3] = {0, 1, 2}, homalt[3] = {0, 0, 1};
  return kind == "carriers" ? carriers : (kind == "alleles" ? alleles : (kind == "homalt" ? homalt : nullptr));
}

// -countDist: which members are counted (-countOf's PED IDs; without it everyone), counted[i] of member i (PED order).  false with
// a message: an ID the PED file does not hold, an ID named twice.
bool counted_members(const Options &o, const Ped &ped, vector<uint8_t> &counted) {
  counted.assign(ped.n(), o.count_of_given ? 0 : 1);
  if (!o.count_of_given) return true;
  if (o.count_of.empty()) {
    std::cout << "-countOf takes the members to count, ID[,ID...] (PED IDs): the list is empty." << std::endl;
    return false;
  }
  std::istringstream in(o.count_of);
  string tok;
  while (std::getline(in, tok, ',')) {
    char *end = nullptr;
    const long id = std::strtol(tok.c_str(), &end, 10);
    int at = -1;
    for (int i = 0; i < ped.n() && !tok.empty() && *end == 0; ++i)
      if (ped.id[i] == id) at = i;
    if (at < 0) {
      std::cout << "-countOf: \"" << tok << "\" is not an individual ID of the PED file." << std::endl;
      return false;
    }
    if (counted[at]) {
      std::cout << "-countOf: individual " << tok << " is named twice." << std::endl;
      return false;
    }
    counted[at] = 1;
  }
  return true;
}

// -countDist: D, the largest value the count reaches, and the tables of its characteristic function at the frequencies
// j = 0 .. (D + 1) / 2, [n_tables][N][3][2] in PED order: omega^(j * score), omega = exp(2 pi i / (D + 1)), the exponent reduced
// mod D + 1 in integers.  (main has checked the options: kind and members are good here.)
int count_tables(const Options &o, const Ped &ped, vector<double> &tables) {
  vector<uint8_t> counted;
  const int *score = count_kind_scores(o.count_kind);
  if (!score || !counted_members(o, ped, counted)) return -1;
  int D = 0;
  for (int i = 0; i < ped.n(); ++i) D += counted[i] ? score[2] : 0;
  const int M = D + 1;
  tables.clear();
  for (int j = 0; j <= M / 2; ++j)
    for (int i = 0; i < ped.n(); ++i)
      for (int g = 0; g < 3; ++g) {
        const double x = 2.0 * M_PI * double((long(j) * (counted[i] ? score[g] : 0)) % M) / M;
        tables.push_back(std::cos(x)), tables.push_back(std::sin(x));
      }
  return D;
}

// -afTag: the allele frequency of a line, the first value of KEY= in its INFO column; < 0 where there is none to use (no such
// key, not a number, outside (0, 1)).
double info_af(std::string_view info, const string &key) {
  size_t at = 0;
  while (at < info.size()) {
    size_t end = info.find(';', at);
    if (end == std::string_view::npos) end = info.size();
    const std::string_view f = info.substr(at, end - at);
    if (f.size() > key.size() + 1 && f[key.size()] == '=' && f.compare(0, key.size(), key) == 0) {
      std::string_view v = f.substr(key.size() + 1);
      v = v.substr(0, v.find(','));
      const string text(v);
      char *stop = nullptr;
      const double q = std::strtod(text.c_str(), &stop);
      if (stop == text.c_str() || *stop != 0 || !(q > 0 && q < 1)) return -1;
      return q;
    }
    at = end + 1;
  }
  return -1;
}

void put_triple(std::ostream &o, const double *p) { o << p[0] << ":" << p[1] << ":" << p[2]; }

// the header of the LK and PL drivers' text: the columns `cols` of `names` are the samples'
void put_lk_header(std::ostream &out, const Options &o, const CliModel &m, const vector<string> &names, const vector<int> &cols) {
  put_format_header(out, "calculated by individual-base Method");
  out << "##FS mutation rate=" << o.mrate << " " << std::endl;
  out << "##FS genotype frequency in pupulation: "; put_triple(out, m.p.genoProbN); out << std::endl;
  out << "#FORMAT\t";
  for (int c : cols) out << names[c] << '\t';
  out << std::endl;
}

// ---- packed PL file (row N4 of SURVEY.md 8(f)): the text-free feed for the GPU ---------------
//   bytes 0-7   "FSPL0001"
//   8-11        uint32 n_seq            sequenced samples (columns)
//   12-15       uint32 record_bytes     = 1 + 6*n_seq
//   16-23       uint64 n_sites          (0 while being written; patched on close)
//   24-...      n_seq x char[32]        sample names, NUL padded
//   then n_sites records: uint8 flags (bit0 Known, bit1 chrX); uint16 pl[n_seq][3] little endian,
//   integer PL clamped to 65534, 0xFFFF x3 = sample missing at the site.
// Only sites the vcf driver would compute are written (same site rules, file.cpp:362-555).
const char kPlMagic[9] = "FSPL0001";

struct PackWriter {
  std::ofstream out;
  uint32_t n_seq = 0;
  uint64_t n_sites = 0, skipped = 0;
  bool open(const string &path, const vector<string> &names) {
    out.open(path.c_str(), std::ios::binary);
    if (!out.is_open()) return false;
    n_seq = (uint32_t)names.size();
    const uint32_t rec = 1 + 6 * n_seq;
    const uint64_t zero = 0;
    out.write(kPlMagic, 8);
    out.write(reinterpret_cast<const char *>(&n_seq), 4);
    out.write(reinterpret_cast<const char *>(&rec), 4);
    out.write(reinterpret_cast<const char *>(&zero), 8);
    for (const string &n : names) {
      char buf[32] = {0};
      std::strncpy(buf, n.c_str(), 31);
      out.write(buf, 32);
    }
    return bool(out);
  }
  void add(uint8_t flags, const uint16_t *pl) {
    out.write(reinterpret_cast<const char *>(&flags), 1);
    out.write(reinterpret_cast<const char *>(pl), 6 * n_seq);
    ++n_sites;
  }
  bool close() {
    out.seekp(16);
    out.write(reinterpret_cast<const char *>(&n_sites), 8);
    out.close();
    return !out.fail();
  }
};

// Packed result file (`FamSeq PL -binOutput`), little-endian: "FSPO0001", n_seq u32, reserved u32,
// n_sites u64, n_seq x 32-byte names; then blocks of  n u64 | status[n] u8 | gpp[n][n_seq][3] f64 |
// fpp[n][n_seq][3] f64 | fgt[n][n_seq] i8  — exactly what famseq_bn_call_batch hands back, so that a
// run is bounded by the host link and the disk, not by printing 6 n_seq numbers per site.
const char kPoMagic[8] = {'F', 'S', 'P', 'O', '0', '0', '0', '1'};

// One batch of the packed-PL driver.  The arrays the GPU call reads and writes live in pinned host
// memory (famseq_alloc_pinned: both directions of the host link at their full rate).
struct PlBatch {
  size_t cap = 0, k = 0, n = 0;
  uint8_t *flags = nullptr, *status = nullptr;
  uint16_t *pl = nullptr;
  double *gpp = nullptr, *fpp = nullptr;
  int8_t *fgt = nullptr;
  char *text = nullptr;  // as_text: the device's records instead of gpp / fpp / fgt
  bool alloc(size_t cap_, size_t k_, bool as_text) {
    cap = cap_;
    k = k_;
    flags = static_cast<uint8_t *>(famseq_alloc_pinned(cap));
    status = static_cast<uint8_t *>(famseq_alloc_pinned(cap));
    pl = static_cast<uint16_t *>(famseq_alloc_pinned(cap * k * 6));
    if (as_text) {
      text = static_cast<char *>(famseq_alloc_pinned(cap * k * FAMSEQ_TEXT_STRIDE));
      return flags && status && pl && text;
    }
    gpp = static_cast<double *>(famseq_alloc_pinned(cap * k * 24));
    fpp = static_cast<double *>(famseq_alloc_pinned(cap * k * 24));
    fgt = static_cast<int8_t *>(famseq_alloc_pinned(cap * k));
    return flags && status && pl && gpp && fpp && fgt;
  }
  void release() {
    for (void *q : {(void *)flags, (void *)status, (void *)pl, (void *)gpp, (void *)fpp, (void *)fgt, (void *)text}) famseq_free_pinned(q);
  }
  // the GPU call of this batch's first n sites
  int call(famseq_ctx *ctx, size_t n_sites, const double *lk, const int32_t *seq_members) {
    if (text)
      return famseq_bn_call_text_batch(ctx, (int64_t)n_sites, lk, lk ? nullptr : pl, flags, seq_members, (int32_t)k, text, status);
    return famseq_bn_call_batch(ctx, (int64_t)n_sites, lk, lk ? nullptr : pl, flags, seq_members, (int32_t)k, gpp, fpp, fgt, status);
  }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Write `bytes` at `off` of fd from `parts` threads (the copy into the page cache is the slow part of
// storing 490 bytes per site; it parallelises, a single stream writer does not).
bool pwrite_parallel(int fd, const void *data, size_t bytes, off_t off, int parts) {
  if (bytes < (size_t(1) << 20)) parts = 1;
  std::vector<std::thread> pool;
  std::vector<char> good(parts, 1);
  for (int t = 0; t < parts; ++t)
    pool.emplace_back([&, t] {
      size_t lo = bytes * t / parts, hi = bytes * (t + 1) / parts;
      const char *p = static_cast<const char *>(data);
      while (lo < hi) {
        const ssize_t w = ::pwrite(fd, p + lo, hi - lo, off + (off_t)lo);
        if (w <= 0) {
          good[t] = 0;
          return;
        }
        lo += (size_t)w;
      }
    });
  for (std::thread &th : pool) th.join();
  for (char g : good)
    if (!g) return false;
  return true;
}

// FIFO hand-off between the stages of the packed-PL pipeline (reader -> GPU -> writer -> reader).
// -1 = the producer is done.
class Channel {
 public:
  void put(int v) {
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_back(v);
    }
    cv_.notify_one();
  }
  int take() {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return !q_.empty(); });
    const int v = q_.front();
    q_.pop_front();
    return v;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<int> q_;
};

bool run_pl(const Options &o, const Ped &ped) {
  std::ifstream fin(o.pl_file.c_str(), std::ios::binary);
  if (!fin.is_open()) {
    std::cout << "Cannot open " << o.pl_file << std::endl;
    return false;
  }
  char magic[8];
  uint32_t n_seq = 0, rec = 0;
  uint64_t n_sites = 0;
  fin.read(magic, 8);
  fin.read(reinterpret_cast<char *>(&n_seq), 4);
  fin.read(reinterpret_cast<char *>(&rec), 4);
  fin.read(reinterpret_cast<char *>(&n_sites), 8);
  if (!fin || std::memcmp(magic, kPlMagic, 8) != 0 || n_seq == 0 || n_seq > 4096 || rec != 1 + 6 * n_seq) {
    std::cout << o.pl_file << " is not a packed PL file." << std::endl;
    return false;
  }
  vector<string> names(n_seq);
  for (uint32_t i = 0; i < n_seq; i++) {
    char buf[33] = {0};
    fin.read(buf, 32);
    names[i] = buf;
  }
  const ColumnMap cm = map_columns(names.data(), n_seq, ped);
  if (cm.members.empty()) {
    std::cout << "No sample of " << o.pl_file << " is in the ped file." << std::endl;
    return false;
  }
  const size_t k = cm.members.size();

  // unpack mode: the results come from a packed result file instead of the GPU
  std::ifstream fpo;
  if (o.unpack_mode) {
    fpo.open(o.po_file.c_str(), std::ios::binary);
    char pm[8];
    uint32_t pk = 0, reserved = 0;
    uint64_t pn = 0;
    fpo.read(pm, 8);
    fpo.read(reinterpret_cast<char *>(&pk), 4);
    fpo.read(reinterpret_cast<char *>(&reserved), 4);
    fpo.read(reinterpret_cast<char *>(&pn), 8);
    if (!fpo || std::memcmp(pm, kPoMagic, 8) != 0 || pk != k) {
      std::cout << o.po_file << " is not a packed result file for these samples." << std::endl;
      return false;
    }
    for (size_t j = 0; j < k; j++) {
      char buf[33] = {0};
      fpo.read(buf, 32);
      if (names[cm.cols[j]] != buf) {
        std::cout << o.po_file << " was written for other samples than " << o.pl_file << " holds." << std::endl;
        return false;
      }
    }
  }

  CliModel m;
  famseq_ctx *ctx = nullptr;
  if (o.unpack_mode) {  // only the header needs the model's priors
    if (m.init(ped, cm.sequenced, o.mrate, o.lrc) != 0) {
      std::cout << "Cannot initiate family. Please check ped file." << std::endl;
      return false;
    }
    if (o.gN.size() == 3) std::copy(o.gN.begin(), o.gN.end(), m.p.genoProbN);
  } else {
    const double t0 = now_s();
    ctx = make_ctx(o, ped, cm.sequenced, m);
    if (!ctx) return false;
    if (std::getenv("FAMSEQ_TIMING")) std::cerr << "FamSeq PL: context (HIP start-up, plan, kernels) " << now_s() - t0 << " s" << std::endl;
  }
  std::ofstream fout(o.out_file.c_str(), o.bin_output ? std::ios::binary : std::ios::out);
  uint64_t written = 0;
  if (o.bin_output) {
    const uint32_t k32 = (uint32_t)k, reserved = 0;
    fout.write(kPoMagic, 8);
    fout.write(reinterpret_cast<const char *>(&k32), 4);
    fout.write(reinterpret_cast<const char *>(&reserved), 4);
    fout.write(reinterpret_cast<const char *>(&written), 8);
    for (int c : cm.cols) {
      char buf[32] = {0};
      std::strncpy(buf, names[c].c_str(), 31);
      fout.write(buf, 32);
    }
  } else {
    put_lk_header(fout, o, m, names, cm.cols);
  }

  // Text of one batch (what `FamSeq PL` prints per site), formatted on all cores: one buffer per thread, written in order.
  vector<TextBuf> text(64);
  auto put_uint = [](TextBuf &t, unsigned v) {
    char *p = t.room(8);
    t.n += size_t(std::to_chars(p, p + 8, v).ptr - p);
  };
  auto format_and_write = [&](size_t n, const uint16_t *pl, const uint8_t *status, const double *gpp, const double *fpp, const int8_t *fgt,
                              const char *rec) {
    const int parts = parallel_ranges(n, [&](size_t lo, size_t hi, int part) {
      TextBuf &line = text[part];
      line.n = 0;
      for (size_t s = lo; s < hi; ++s) {
        line.put("PL:GPP:FPP:FGT\t", 15);
        for (size_t j = 0; j < k; j++) {
          const uint16_t *p = &pl[(s * k + j) * 3];
          if (p[0] == 0xFFFF && p[1] == 0xFFFF && p[2] == 0xFFFF) {
            line.put("NA", 2);
          } else {
            put_uint(line, p[0]), line.ch(',');
            put_uint(line, p[1]), line.ch(',');
            put_uint(line, p[2]);
          }
          if (status[s] & 3) {
            line.put(":NA:NA:NA\t", 10);
            continue;
          }
          line.ch(':');
          line.called(rec, gpp, fpp, fgt, s * k + j);
        }
        line.ch('\n');
      }
    });
    for (int part = 0; part < parts; ++part) fout.write(text[part].v.data(), (std::streamsize)text[part].n);
  };

  if (!o.unpack_mode) {
    // `FamSeq PL`: read, GPU and write run concurrently — a reader thread de-interleaves batch b + 1 out
    // of the memory-mapped file while the GPU call of batch b runs on this thread and a writer thread
    // stores (or prints) batch b - 1.  Three batches of pinned buffers go round; order is kept by the
    // FIFOs.  (The serial loop this replaces spent two thirds of its time with the GPU idle.)
    const long header = (long)fin.tellg();
    fin.close();
    const int fd = ::open(o.pl_file.c_str(), O_RDONLY);
    struct stat st;
    if (fd < 0 || ::fstat(fd, &st) != 0) {
      std::cout << "Cannot open " << o.pl_file << std::endl;
      return false;
    }
    const size_t body = (size_t)st.st_size > (size_t)header ? (size_t)st.st_size - (size_t)header : 0;
    const size_t total = body / rec;  // whole records only, like the stream reader
    const char *map = nullptr;
    if (total) {
      void *mp = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (mp == MAP_FAILED) {
        std::cout << "Cannot map " << o.pl_file << std::endl;
        ::close(fd);
        return false;
      }
      ::madvise(mp, (size_t)st.st_size, MADV_SEQUENTIAL);
      map = static_cast<const char *>(mp);
    }
    const size_t cap = std::min(batch_capacity(), std::max<size_t>(total, 1));
    constexpr int kBatches = 3;
    PlBatch bt[kBatches];
    bool ok = true;
    const double t_alloc0 = now_s();
    for (PlBatch &b : bt) ok = b.alloc(cap, k, !o.bin_output && device_text()) && ok;
    const double t_alloc = now_s() - t_alloc0;
    if (!ok) std::cerr << "cannot allocate pinned host buffers" << std::endl;
    double t_read = 0, t_gpu = 0, t_write = 0;
    const double t_start = now_s();
    Channel to_reader, to_gpu, to_writer;
    for (int i = 0; i < kBatches; i++) to_reader.put(i);
    std::thread reader([&] {
      for (size_t at = 0; at < total && ok;) {
        const int i = to_reader.take();
        const double t0 = now_s();
        PlBatch &b = bt[i];
        b.n = std::min(cap, total - at);
        const char *raw = map + header + at * rec;
        parallel_for(b.n, [&](size_t s) {  // de-interleave: flags[] and the PED-matched columns of pl[]
          const char *r = raw + s * rec;
          b.flags[s] = uint8_t(r[0]);
          for (size_t j = 0; j < k; j++) std::memcpy(&b.pl[(s * k + j) * 3], r + 1 + 6 * cm.cols[j], 6);
        });
        at += b.n;
        t_read += now_s() - t0;
        to_gpu.put(i);
      }
      to_gpu.put(-1);
    });
    bool write_ok = true;
    // packed results go out through pwrite on a descriptor of their own (positions are known: the
    // header, then fixed-layout blocks), several threads per block
    int ofd = -1;
    off_t opos = 0;
    if (o.bin_output) {
      fout.flush();
      opos = (off_t)fout.tellp();
      ofd = ::open(o.out_file.c_str(), O_WRONLY);
      if (ofd < 0) write_ok = false;
    }
    std::thread writer([&] {
      for (;;) {
        const int i = to_writer.take();
        if (i < 0) break;
        const double t0 = now_s();
        PlBatch &b = bt[i];
        if (o.bin_output) {
          const uint64_t bn = b.n;
          const size_t wide = b.n * k * 24;
          bool g = write_ok && ::pwrite(ofd, &bn, 8, opos) == 8 && pwrite_parallel(ofd, b.status, b.n, opos + 8, 1);
          g = g && pwrite_parallel(ofd, b.gpp, wide, opos + 8 + (off_t)b.n, 4);
          g = g && pwrite_parallel(ofd, b.fpp, wide, opos + 8 + (off_t)(b.n + wide), 4);
          g = g && pwrite_parallel(ofd, b.fgt, b.n * k, opos + 8 + (off_t)(b.n + 2 * wide), 1);
          opos += 8 + (off_t)(b.n + 2 * wide + b.n * k);
          write_ok = g;
          written += b.n;
        } else {
          format_and_write(b.n, b.pl, b.status, b.gpp, b.fpp, b.fgt, b.text);
          write_ok = write_ok && !fout.fail();
        }
        t_write += now_s() - t0;
        to_reader.put(i);
      }
    });
    for (;;) {  // the GPU stage, on the thread that owns the context
      const int i = to_gpu.take();
      if (i < 0) break;
      PlBatch &b = bt[i];
      if (ok) {
        const double t0 = now_s();
        const int rc = b.call(ctx, b.n, nullptr, cm.members.data());
        t_gpu += now_s() - t0;
        if (rc != 0) {
          std::cerr << "famseq_bn_call_batch failed (" << rc << "): " << famseq_last_error(ctx) << std::endl;
          ok = false;
        }
      }
      if (ok) to_writer.put(i);
      else to_reader.put(i);  // keep the reader from waiting on a batch that will never be written
    }
    to_writer.put(-1);
    reader.join();
    writer.join();
    for (PlBatch &b : bt) b.release();
    if (map) ::munmap(const_cast<char *>(map), (size_t)st.st_size);
    ::close(fd);
    if (o.bin_output) {
      if (ofd >= 0) {
        write_ok = write_ok && ::pwrite(ofd, &written, 8, 16) == 8;
        ::close(ofd);
      }
    }
    fout.close();
    if (std::getenv("FAMSEQ_TIMING"))
      std::cerr << "FamSeq PL: " << total << " sites, pipeline " << now_s() - t_start << " s (busy: reader " << t_read << ", GPU calls "
                << t_gpu << ", writer " << t_write << "); pinned buffers " << t_alloc << " s" << std::endl;
    famseq_destroy(ctx);
    return ok && write_ok && !fout.fail();
  }

  // `FamSeq unpack`: the result file's blocks set the pace; no GPU, a plain loop
  size_t cap = batch_capacity();
  vector<char> raw(cap * rec);
  vector<uint8_t> status(cap);
  vector<uint16_t> pl(cap * k * 3);
  vector<double> gpp(cap * k * 3), fpp(cap * k * 3);
  vector<int8_t> fgt(cap * k);
  bool ok = true;
  while (ok) {
    uint64_t bn = 0;
    fpo.read(reinterpret_cast<char *>(&bn), 8);
    if (!fpo || bn == 0) break;
    if (bn > cap) {
      cap = (size_t)bn;
      raw.resize(cap * rec); status.resize(cap); pl.resize(cap * k * 3);
      gpp.resize(cap * k * 3); fpp.resize(cap * k * 3); fgt.resize(cap * k);
    }
    const size_t n = (size_t)bn;
    fin.read(raw.data(), (std::streamsize)(n * rec));
    fpo.read(reinterpret_cast<char *>(status.data()), (std::streamsize)n);
    fpo.read(reinterpret_cast<char *>(gpp.data()), (std::streamsize)(n * k * 24));
    fpo.read(reinterpret_cast<char *>(fpp.data()), (std::streamsize)(n * k * 24));
    fpo.read(reinterpret_cast<char *>(fgt.data()), (std::streamsize)(n * k));
    if (!fpo || size_t(fin.gcount()) != n * rec) {
      std::cout << "The packed files end early or do not belong together." << std::endl;
      ok = false;
      break;
    }
    parallel_for(n, [&](size_t s) {  // the PED-matched columns of pl[]
      const char *r = raw.data() + s * rec;
      for (size_t j = 0; j < k; j++) std::memcpy(&pl[(s * k + j) * 3], r + 1 + 6 * cm.cols[j], 6);
    });
    format_and_write(n, pl.data(), status.data(), gpp.data(), fpp.data(), fgt.data(), nullptr);
  }
  fout.close();
  return ok && !fout.fail();
}

// ---- VCF driver ----------------------------------------------------------------------------

int chrom_number(const string &c) {  // file.cpp:321-343
  if (c == "X" || c == "chrX") return 23;
  if (c == "Y" || c == "chrY") return 24;
  if (c == "MT") return 25;
  return std::atoi(c.compare(0, 3, "chr") == 0 ? c.c_str() + 3 : c.c_str());
}

// The input as std::getline would cut it — lines up to the next '\n', a last line without one counts — over the
// memory-mapped file: no copy per line, and what the output echoes of a line (columns 1-9, the sample fields) is
// pointed at in place until the batch is written.  What cannot be mapped (a pipe) is read whole.
struct LineSource {
  const char *cur = nullptr, *end = nullptr;
  void *map = nullptr;
  size_t map_len = 0;
  string owned;
  bool open(const string &path) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
      void *mp = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (mp != MAP_FAILED) {
        ::madvise(mp, (size_t)st.st_size, MADV_SEQUENTIAL);
        map = mp, map_len = (size_t)st.st_size;
        cur = static_cast<const char *>(mp), end = cur + map_len;
        ::close(fd);
        return true;
      }
    }
    // Not a regular file (a pipe, /dev/stdin) or one that cannot be mapped: read whole into memory — the parsed items
    // point into the input text until their block is written, which a bounded read-ahead buffer would have to guarantee
    // block by block.  A piped VCF therefore needs memory of its size; give large inputs as files (the usage text says so).
    char buf[1 << 16];
    ssize_t r;
    while ((r = ::read(fd, buf, sizeof buf)) > 0) owned.append(buf, size_t(r));
    ::close(fd);
    cur = owned.data(), end = cur + owned.size();
    return true;
  }
  bool next(std::string_view &line) {
    if (cur >= end) return false;
    const char *nl = static_cast<const char *>(std::memchr(cur, '\n', size_t(end - cur)));
    line = std::string_view(cur, size_t((nl ? nl : end) - cur));
    cur = nl ? nl + 1 : end;
    return true;
  }
  ~LineSource() {
    if (map) ::munmap(map, map_len);
  }
};

// run `f(t)` on threads 0..n-1 (the caller's thread takes 0)
template <class F>
void on_threads(int n, F f) {
  vector<std::thread> pool;
  for (int t = 1; t < n; ++t) pool.emplace_back([=] { f(t); });
  f(0);
  for (std::thread &th : pool) th.join();
}

// parts 0..n_parts-1 on at most `threads` threads, dealt round-robin
template <class F>
void on_parts(int n_parts, unsigned threads, F f) {
  const int nt = (int)std::min<unsigned>(threads, (unsigned)n_parts);
  on_threads(nt, [&](int j) {
    for (int t = j; t < n_parts; t += nt) f(t);
  });
}

// What one parsing thread makes of its contiguous range of a block's lines, in input order.  The same thread
// formats the same range once the block's sites are back from the GPU.
struct Item {
  const char *raw;       // site: the input line (mapped; columns 1-9 and the sample fields are printed from it)
  uint32_t raw_len;
  uint32_t prefix_len;   // site: columns 1-9 without the tab after FORMAT
  uint32_t n_fmt;        // site: FORMAT keys (a missing sample prints that many "NA:")
  int32_t site;          // the line's index in the block = its site in the batch; -1: an echoed line, text = echo[echo_off, +echo_len)
  uint32_t echo_off, echo_len;
  uint32_t smp;          // site: its samples are samples[smp, +n_seq)
};
struct Part {
  vector<Item> items;
  vector<char> echo;
  vector<Record::Sample> samples;      // n_seq per site
  vector<uint32_t> explicit_sites;     // sites with a PL/GL field that is not a plain integer ...
  vector<double> explicit_lk;          // ... and their N x 3 likelihoods (the batch then goes in as fp64)
  bool any_failed = false;
  void clear() {
    items.clear(), echo.clear(), samples.clear(), explicit_sites.clear(), explicit_lk.clear();
    any_failed = false;
  }
};

// ---- side outputs: what -dnm, -map, -siteQ, -loo, -sample, -seg and -afEM add to a line, one row of kSide each; -swapCheck and
// ---- -mRateScan, which add nothing to any line and write a report of their own behind the last site (SideRow::report), are rows too
// The order is the one main checks them and prints its notices in; it is also the order of the fields in a sample column (DNP,
// JGT:JP, LOP:LOF, SGT, PGT:PGP, JGQ) and of the keys joined to the INFO column (FQ;FLL, then PSD;PSR, then FAF;FAL, then PSL, then JP2, then PCD).  Header
// lines have their own order.
enum SideId { kDnm, kMap, kSiteQ, kLoo, kSample, kSeg, kAfEm, kSwap, kRateScan, kPhase, kSegPen, kMapQ, kCountDist };
constexpr int kSides = kCountDist + 1;
const SideId kHeaderOrder[kSides] = {kDnm, kMap, kLoo, kSample, kSeg, kSiteQ, kAfEm, kSwap, kRateScan, kPhase, kSegPen, kMapQ, kCountDist};

// One side output of a block: the two arrays its C entry fills ([site][...], read as the entry's own types) and its status per site.
struct SideOut {
  vector<double> a, b;
  vector<uint8_t> status;
  const uint8_t *flags = nullptr;  // the block's flags per site (-phase: a son's field at a chrX site is haploid)
  const int8_t *a8() const { return reinterpret_cast<const int8_t *>(a.data()); }
};

struct VcfRun;
struct SideBytes { size_t a, b; };
struct SideRow {
  SideId id;
  const char *flag;   // as the notices name it
  const char *entry;  // its C entries are <entry>_batch and <entry>_prior_batch (VcfRun::call_side; -afEM: the first alone)
  bool method2;       // a form of the sum-product engine only: implies -method 2
  bool (*on)(const Options &);
  void (*off)(Options &);
  bool (*check)(const Options &, const Ped &);  // its own arguments, said with a message (exit -1); null: nothing to check
  void (*header)(std::ostream &, const Options &);
  const char *keys, *na;  // its FORMAT keys and what a failed site prints for them; null: it writes INFO keys
  SideBytes (*bytes)(const VcfRun &);  // per site, of the two arrays
  // its per-line text is empty (no header line, no FORMAT or INFO key: the output file is the one without it); what its kernel
  // says of a block is summed up site by site (VcfRun::add_report / add_rate_report) and written behind the last site
  // (VcfRun::write_report / write_rate_report)
  bool report = false;
  bool info_too = false;  // beside its FORMAT keys it joins a key to the INFO column (-mapQ: JGQ per sample, JP2 per site)
};
extern const SideRow kSide[kSides];
constexpr size_t kInfoColumn = ~size_t(0);  // put_side's j where a row with FORMAT keys is asked for its INFO key
// Row id's fields behind column j of site s, from the ':' on, or its INFO keys for site s: a switch, which the formatter's loop inlines
[[gnu::always_inline]] inline void put_side(SideId id, TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j);

bool any_side(const Options &o) { return std::any_of(kSide, kSide + kSides, [&](const SideRow &r) { return r.on(o); }); }

struct Slot {
  vector<std::string_view> lines;
  vector<Part> parts;
  int n_parts = 0;
  size_t n_sites = 0;  // sites of the batch: the block's lines, or (large pedigrees) its sites moved together
  bool packed = true;
  bool staged = false;        // parsed into pk_pl / pk_flags because the HIP runtime was not up yet: the flusher copies them over
  vector<uint16_t> pk_pl;     // pack mode (and staged blocks): the block's arrays live here, nothing is pinned
  vector<uint8_t> pk_flags;
  PlBatch io;          // pinned: pl + flags in, gpp / fpp / fgt / status out
  uint16_t *pl_arr = nullptr;  // where this block is parsed to: io's arrays or the pk_ ones
  uint8_t *flags_arr = nullptr;
  vector<double> lk;   // fp64 input, only for a block with a non-integer PL/GL field
  vector<double> prior;  // -afTag: [line][6], the founders' prior rows (a line that is no site keeps the model's)
  vector<TextBuf> text;
  SideOut side[kSides];
  int64_t site_base = 0;  // -sample: the block's first site among the sites of the file
};

// One `FamSeq vcf` (or `pack`) run: what is set up once — never changed by the stages — what the stages do change, and the stages.
struct VcfRun {
  const Options &o;
  const Ped &ped;
  LineSource fin;
  std::ofstream fout;
  CliModel m;
  bool use_af = false;
  vector<uint8_t> seg_masks;  // -seg: the patterns' mask rows and INFO keys
  vector<const char *> seg_keys;
  // -segPen: the models' weight tables [n_models][N][3], and the all-ones likelihood rows of the null call (grown to the largest
  // block: the phenotypes' probability under the pedigree and the founders' prior alone, by the block's flags and priors)
  vector<double> pen_tables, ones_lk;
  // -countDist: the count's largest value D, the complex weight tables of its characteristic function at the frequencies
  // 0 .. (D + 1) / 2 (count_tables) and the inverse transform's cos / sin of 2 pi r / (D + 1), r = 0 .. D
  int count_D = 0;
  vector<double> count_cw, count_cos, count_sin;
  // -swapCheck: the exchange of every two sequenced samples, in VCF column order, as assignment rows [pair][N] (PED order), and
  // what the sites so far add up to, in file order: per pair the sum of alt_loglik - loglik over the used sites where alt_loglik
  // is finite and the number of used sites where it is -inf; the used and the skipped (status != 0) sites, the used sites' loglik
  vector<int32_t> swap_assign;
  vector<std::pair<int, int>> swap_cols;  // the two columns of a pair, as indices into cm.cols
  vector<double> swap_bf;
  vector<uint64_t> swap_impossible;
  uint64_t swap_used = 0, swap_skipped = 0;
  double swap_loglik = 0;
  vector<string> sample_names;  // -swapCheck: the VCF's name of column j of cm.cols
  // -mRateScan: what the sites so far add up to, in file order: per rate of the grid the sum of rate_loglik over the used sites
  // (one -inf makes it -inf) and the number of used sites where it is -inf; the used and the skipped (status != 0) sites, the
  // used sites' loglik under the run's own -mRate
  vector<double> rate_sum;
  vector<uint64_t> rate_impossible;
  uint64_t rate_used = 0, rate_skipped = 0;
  double rate_own = 0;
  double model_rows[2][6];  // -afTag: the rows of a line without a usable frequency, by its Known flag: what the model itself would have used
  ColumnMap cm;
  size_t ncol = 0, n_seq = 0, N3 = 0;
  vector<int> kid_of_col;  // -dnm: column j -> its member's index among the children (famseq_trio_children: the members with parents, PED order), -1 for a founder
  int n_kids = 0;
  vector<vector<int>> loc = vector<vector<int>>(25);
  const PlTable pl;
  PackWriter packer;
  const bool as_text = device_text();
  vector<const SideRow *> sides, fields, infos;  // the rows that are on, in kSide's order: all of them, those with FORMAT keys, those with INFO keys
  string format_keys = ":GPP:FPP:FGT";           // what a site's FORMAT column gains, with the tab behind it
  size_t block = 0;
  unsigned n_threads = 1, parse_threads = 1, format_threads = 1;
  int compact_from = 12;  // members from which a block's sites are moved together before the GPU call
  // ... and what the stages change
  Slot slots[4];  // one being cut and parsed, one at the GPU, one being formatted, one being written
  Channel to_flusher, to_formatter, to_writer, to_driver;
  std::atomic<bool> hip_up{false}, flush_ok{true};
  std::future<famseq_ctx *> ctx_future;
  famseq_ctx *ctx = nullptr;
  uint64_t sites_before = 0;  // sites of the blocks cut so far
  double t_lines = 0, t_parse = 0, t_gather = 0, t_stall = 0, t_gpu = 0, t_format = 0, t_write = 0, t_ctx_wait = 0;

  // the model (its priors are needed for the header before the ctx exists), -seg's masks, -afTag's rows, the active side rows
  bool set_up() {
    vector<uint8_t> all(ped.n(), 1);
    if (m.init(ped, all, o.mrate, o.lrc) != 0) {
      std::cout << "Cannot initiate family. Please check ped file." << std::endl << "Cannot set family." << std::endl;
      return false;
    }
    m.set_priors(o);
    use_af = !o.af_tag.empty() && !o.pack_mode;
    // (main has checked -seg's options: this cannot fail here)
    if (!o.seg.empty() && !o.pack_mode && !segregation_masks(o, ped, seg_masks, seg_keys)) return false;
    if (o.pen_given && !o.pack_mode && !penetrance_tables(o, ped, pen_tables)) return false;
    if (o.count_given && !o.pack_mode) {
      if ((count_D = count_tables(o, ped, count_cw)) < 0) return false;
      for (int r = 0; r <= count_D; ++r) {
        const double x = 2.0 * M_PI * r / (count_D + 1);
        count_cos.push_back(std::cos(x)), count_sin.push_back(std::sin(x));
      }
    }
    for (int k = 0; k < 3; ++k) {
      model_rows[0][k] = m.p.genoProbN[k], model_rows[0][3 + k] = m.p.genoProbXN[k];
      model_rows[1][k] = m.p.genoProbK[k], model_rows[1][3 + k] = m.p.genoProbXK[k];
    }
    for (const SideRow &row : kSide) {
      if (!row.on(o)) continue;
      sides.push_back(&row);
      if (row.report) continue;
      if (row.keys) fields.push_back(&row), format_keys += row.keys;
      if (!row.keys || row.info_too) infos.push_back(&row);
    }
    format_keys += '\t';
    N3 = size_t(3) * ped.n();
    block = std::min<size_t>(batch_capacity(), size_t(1) << 16);
    n_threads = std::thread::hardware_concurrency();
    if (const char *e = std::getenv("FAMSEQ_THREADS")) n_threads = (unsigned)std::atoi(e);
    n_threads = std::max(1u, std::min(n_threads, 32u));
    // A block is cut into n_threads parts; how many threads walk them while parsing and while formatting can be set apart
    // (formatting is the loop's critical path and runs beside the next block's parsing: tools/cli_throughput.py)
    parse_threads = format_threads = n_threads;
    if (const char *e = std::getenv("FAMSEQ_PARSE_THREADS")) parse_threads = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("FAMSEQ_FORMAT_THREADS")) format_threads = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("FAMSEQ_COMPACT_FROM")) compact_from = std::atoi(e);  // test aid
    for (Slot &sl : slots) sl.parts.resize(n_threads), sl.text.resize(n_threads);
    return true;
  }

  // -swapCheck: every two sequenced samples, in VCF column order (head: the #CHROM line's columns)
  void set_up_swaps(const vector<string> &head) {
    const size_t N = size_t(ped.n()), k = cm.cols.size();
    for (int c : cm.cols) sample_names.push_back(head[9 + c]);
    for (size_t a = 0; a < k; ++a)
      for (size_t b = a + 1; b < k; ++b) {
        swap_cols.push_back({int(a), int(b)});
        const size_t at = swap_assign.size();
        for (size_t p = 0; p < N; ++p) swap_assign.push_back(int32_t(p));
        swap_assign[at + cm.members[a]] = cm.members[b], swap_assign[at + cm.members[b]] = cm.members[a];
      }
  }

  void format_tags(bool fallback) {
    put_format_header(fout, fallback ? "calbulated by Single Method" : "calculated by individual-based Method");
    for (SideId id : kHeaderOrder)
      if (kSide[id].on(o)) kSide[id].header(fout, o);
  }
  void fs_info() {
    fout << "##FS mutation rate=" << o.mrate << " " << std::endl;
    fout << "##FS genotype frequency in pupulation (Rare): "; put_triple(fout, m.p.genoProbN); fout << std::endl;
    fout << "##FS genotype frequency in population (Common): "; put_triple(fout, m.p.genoProbK); fout << std::endl;
    fout << "##FS genotype frequency for chromosome X of male in population (Rare): "; put_triple(fout, m.p.genoProbXN); fout << std::endl;
    fout << "##FS genotype frequency for chromosome X of male in population (Common): "; put_triple(fout, m.p.genoProbXK); fout << std::endl;
    if (use_af)
      fout << "##FS genotype frequency of a site with 0 < " << o.af_tag << " < 1 in INFO: Hardy-Weinberg at that allele frequency"
           << (o.af_all ? " (-afTagAll: for every field of the line)" : "") << std::endl;
  }
  // The header (file.cpp:143-196): lines are echoed with a one-line lag, the run's own lines go behind the input's FORMAT lines
  // and in front of its contig lines, or behind all of them where it has neither.  Returns the last header line, the #CHROM one;
  // `line` is the first data line where have_line.
  string echo_header(std::string_view &line, bool &have_line) {
    string title;
    bool need_tags = true, need_info = true;
    auto after_hashes = [](std::string_view l, size_t n) { return l.size() > 2 ? l.substr(2, n) : std::string_view(); };
    while (fin.next(line)) {
      if (!line.empty() && line[0] == '#') {
        if (title.size() > 2) {
          fout << title << std::endl;
          if (title.compare(2, 6, "FORMAT") == 0 && after_hashes(line, 4) == "INFO" && need_tags) {
            format_tags(false);
            need_tags = false;
          }
          if (after_hashes(line, 6) == "contig" && need_info) {
            fs_info();
            need_info = false;
          }
        }
        title.assign(line);
        continue;
      }
      have_line = true;
      break;
    }
    if (need_tags) format_tags(true);
    if (need_info) fs_info();
    return title;
  }
  // column mapping (file.cpp:200-232) and the output's #CHROM line
  bool map_header(const vector<string> &head) {
    if (head.size() < 9) {
      std::cerr << "The vcf file has no #CHROM header line." << std::endl;
      return false;
    }
    ncol = head.size() - 9;
    cm = map_columns(head.data() + 9, ncol, ped);
    n_seq = cm.cols.size();
    for (int i = 0; i < 9; i++) fout << head[i] << '\t';
    for (int c : cm.cols) fout << head[9 + c] << '\t';
    fout << std::endl;
    vector<int> kid(ped.n(), -1);
    for (int p = 0; p < ped.n(); ++p)
      if (m.mo[p] >= 0) kid[p] = n_kids++;
    for (int32_t p : cm.members) kid_of_col.push_back(kid[p]);
    return true;
  }
  // location filter (file.cpp:235-298)
  bool read_locations() {
    std::ifstream fl(o.loc_file.c_str());
    if (!fl.is_open()) {
      std::cout << "Cannot open " << o.loc_file << std::endl;
      return false;
    }
    string l;
    while (std::getline(fl, l)) {
      if (l.size() < 2) break;
      const vector<string> t = split_keep(l, '\t');
      if (t.size() < 2) continue;
      int c = t[0] == "X" ? 23 : t[0] == "Y" ? 24 : t[0] == "MT" ? 25 : std::atoi(t[0].c_str());
      const int p = std::atoi(t[1].c_str());
      if (c < 1 || c > 25 || p == 0) continue;
      loc[c - 1].push_back(p);
    }
    for (auto &v : loc) std::sort(v.begin(), v.end());
    return true;
  }

  // One input line -> an Item (or nothing).  Pure function of the line (no shared state).  Line q of a block is site q of
  // the batch: a site's flag byte and packed PLs are written where the GPU call will read them (flags_q, pl16: the
  // caller has set them to "all samples missing", which is what a line that is no site stays — computed and ignored;
  // compacting the sites first cost a pass over the batch, and the GPU idles nine tenths of the loop).
  void parse_line(std::string_view line, size_t q, Part &out, uint8_t *flags_q, uint16_t *pl16, double *prior_q) const {
    if (line[0] == '#') return;
    thread_local vector<std::string_view> t, fmt, sub;
    thread_local vector<double> lkrow;
    split_views(line, '\t', t);
    if (t.size() < 9 + ncol) return;  // malformed line (the reference would read out of bounds)
    auto echo = [&] {
      if (o.pack_mode) return;
      const size_t at = out.echo.size();
      for (int i = 0; i < 9; i++) {
        out.echo.insert(out.echo.end(), t[i].begin(), t[i].end());
        out.echo.push_back('\t');
      }
      for (int c : cm.cols) {
        out.echo.insert(out.echo.end(), t[9 + c].begin(), t[9 + c].end());
        out.echo.push_back('\t');
      }
      out.items.push_back(Item{nullptr, 0, 0, 0, -1, uint32_t(at), uint32_t(out.echo.size() - at), 0});
    };
    if (!o.loc_file.empty()) {
      const int c = chrom_number(string(t[0]));
      const int p = std::atoi(string(t[1]).c_str());
      if (c < 1 || c > 25 || p == 0) return;
      if (!std::binary_search(loc[c - 1].begin(), loc[c - 1].end(), p)) return;
    }
    // site rules, in the reference's order (file.cpp:362-473)
    if (t[3] == "." || t[3] == "-" || t[3].size() != 1 || t[4].size() != 1) {
      if (o.all_line) echo();
      return;
    }
    if (o.var_only && (t[4] == "." || t[4] == "-")) return;
    if (t[0] == "Y" || t[0] == "chrY" || t[0] == "MT") {
      if (o.all_line) echo();
      return;
    }
    const bool is_x = t[0] == "X" || t[0] == "chrX" || t[0] == "CHRX";
    const string chrom(t[0]);
    const int cn = std::atoi(chrom.compare(0, 3, "chr") == 0 ? chrom.c_str() + 3 : chrom.c_str());
    if (!((0 < cn && cn < 23) || is_x)) {
      if (o.all_line) echo();
      return;
    }
    const uint8_t flags = uint8_t((t[2] != "." ? FAMSEQ_FLAG_KNOWN : 0) | (is_x ? FAMSEQ_FLAG_CHRX : 0));
    split_views(t[8], ':', fmt);
    size_t n_miss = 0;
    for (int c : cm.cols) n_miss += t[9 + c].size() < 5;
    if (n_miss == n_seq) {
      if (o.all_line) echo();
      return;
    }
    int i_pl = -1;
    for (size_t k = 0; k < fmt.size(); k++)
      if (fmt[k] == "PL" || fmt[k] == "GL") i_pl = (int)k;
    if (i_pl < 0) {  // echoed unchanged even without -a (file.cpp:541-555, :770-784)
      echo();
      return;
    }
    const char *base = line.data();
    out.items.push_back(Item{base, uint32_t(line.size()), uint32_t(t[8].data() + t[8].size() - base), uint32_t(fmt.size()),
                             int32_t(q), 0, 0, uint32_t(out.samples.size())});
    *flags_q = flags;
    if (prior_q) {
      const double af = info_af(t[7], o.af_tag);
      if (af > 0) famseq_hwe_priors(1, &af, prior_q);
      else std::copy(model_rows[flags & FAMSEQ_FLAG_KNOWN ? 1 : 0], model_rows[flags & FAMSEQ_FLAG_KNOWN ? 1 : 0] + 6, prior_q);
    }
    lkrow.assign(N3, 1.0);
    bool integral = true;
    size_t col = 0;
    for (int c : cm.cols) {
      const size_t this_col = col++;
      const std::string_view f = t[9 + c];
      out.samples.push_back({uint32_t(f.data() - base), uint32_t(f.size()), f.size() < 5});
      if (f.size() < 5) continue;  // missing sample: flat likelihood (file.cpp:927-933)
      split_views(f, ':', sub);
      if (sub.size() != fmt.size()) continue;  // row stays {1,1,1} (file.cpp:573-578)
      const std::string_view pls = sub[i_pl];
      const char *b = pls.data(), *end = b + pls.size();
      for (int g = 0; g < 3; g++) {
        const char *e = static_cast<const char *>(std::memchr(b, ',', size_t(end - b)));
        if (!e) e = end;
        lkrow[size_t(3) * cm.member[c] + g] = pl(b, e, &pl16[3 * this_col + g], &integral);
        b = e < end ? e + 1 : end;
      }
    }
    if (!integral) {
      out.explicit_sites.push_back(uint32_t(q));
      out.explicit_lk.insert(out.explicit_lk.end(), lkrow.begin(), lkrow.end());
    }
  }

  // ---- the pipeline.  A block of input lines is ONE batch: the driver's thread cuts it into lines, has it parsed on all
  // cores (each thread its contiguous range, into its own Part and into its range of the batch's pinned arrays)
  // and hands the block to the flusher thread — GPU call (famseq_bn_call_batch: posterior, Phred scaling and
  // genotype call on the device), formatting (each thread the range it parsed), one write per thread — while it goes on
  // with the next block in the other slot.  (Before: lines copied one by one out of an ifstream, parsed results moved
  // one by one into the batch by this thread, 0.94 of the loop's 1.0 s per 1 M ten-member sites.)

  bool pin(Slot &sl, size_t n) {
    if (sl.io.cap >= n) return true;
    sl.io.release();
    sl.io = PlBatch();
    if (sl.io.alloc(n, std::max<size_t>(n_seq, 1), as_text)) return true;
    std::cerr << "cannot allocate pinned host buffers" << std::endl;
    return false;
  }
  // Cut the next block off the input (`line` holds the next unread line) and parse it.  False: nothing was cut, or its pinned
  // arrays could not be had (*ok cleared).
  bool cut_and_parse(Slot &sl, std::string_view &line, bool &more, bool *ok) {
    const double t1 = now_s();
    sl.lines.clear();
    while (more && sl.lines.size() < block) {
      if (line.size() < 2) {  // the reference stops at the first empty line
        more = false;
        break;
      }
      sl.lines.push_back(line);
      more = fin.next(line);
    }
    const size_t nl = sl.lines.size();
    if (nl == 0) return false;
    sl.n_parts = nl < 2048 ? 1 : (int)n_threads;
    const double t2 = now_s();
    t_lines += t2 - t1;
    sl.staged = !o.pack_mode && !hip_up;
    if (o.pack_mode || sl.staged) {
      sl.pk_pl.resize(nl * 3 * n_seq), sl.pk_flags.resize(nl);
    } else if (!pin(sl, nl)) {  // pinned, sized by the first block (a short file does not pay for 65,536 sites)
      *ok = false;
      return false;
    }
    uint16_t *const pl_arr = sl.pl_arr = o.pack_mode || sl.staged ? sl.pk_pl.data() : sl.io.pl;
    uint8_t *const flags_arr = sl.flags_arr = o.pack_mode || sl.staged ? sl.pk_flags.data() : sl.io.flags;
    if (use_af) sl.prior.resize(nl * 6);
    double *const prior_arr = use_af ? sl.prior.data() : nullptr;
    on_parts(sl.n_parts, parse_threads, [&](int t) {
      Part &pt = sl.parts[t];
      pt.clear();
      const size_t lo = nl * t / sl.n_parts, hi = nl * (t + 1) / sl.n_parts;
      std::memset(flags_arr + lo, 0, hi - lo);
      for (size_t q = lo; prior_arr && q < hi; ++q) std::copy(model_rows[0], model_rows[0] + 6, prior_arr + 6 * q);
      std::memset(pl_arr + lo * 3 * n_seq, 0xFF, (hi - lo) * 6 * n_seq);  // 0xFFFF x3 = missing sample
      for (size_t q = lo; q < hi; ++q) parse_line(sl.lines[q], q, pt, flags_arr + q, pl_arr + q * 3 * n_seq, prior_arr ? prior_arr + 6 * q : nullptr);
    });
    t_parse += now_s() - t2;
    bool packed = true;
    size_t real = 0;
    for (int t = 0; t < sl.n_parts; ++t) {
      packed = packed && sl.parts[t].explicit_sites.empty();
      real += sl.parts[t].samples.size();
    }
    sl.n_sites = real ? nl : 0, sl.packed = packed;  // a block without a single site (or without a sequenced sample) calls nothing
    return true;
  }
  // pack mode: records of the integer sites, in input order; nothing goes to the GPU
  void pack_records(const Slot &sl) {
    for (int t = 0; t < sl.n_parts; ++t) {
      const Part &pt = sl.parts[t];
      size_t x = 0;
      for (const Item &it : pt.items) {
        if (it.site < 0) continue;
        if (x < pt.explicit_sites.size() && pt.explicit_sites[x] == uint32_t(it.site)) {
          ++x, packer.skipped++;
          continue;
        }
        packer.add(sl.flags_arr[it.site], sl.pl_arr + size_t(it.site) * 3 * n_seq);
      }
    }
  }
  // A line that is no site costs the GPU a site's work: nothing next to the text work for the usual pedigree, but
  // 3^N configurations each.  From twelve members on (0.5 M configurations) the sites are moved together first —
  // in place and in order, one thread: 60 bytes per site.  (-sample: always, so that a site's position in the batch
  // is its position among the block's sites, and site_base counts the sites of the blocks before.)
  void move_sites_together(Slot &sl) {
    const size_t nl = sl.lines.size();
    double *const prior_arr = use_af ? sl.prior.data() : nullptr;
    size_t n_real = 0;
    for (int t = 0; t < sl.n_parts; ++t)
      for (const Item &it : sl.parts[t].items) n_real += it.site >= 0;
    if (n_real > 0 && n_real < nl && (ped.n() >= compact_from || o.sample)) {
      size_t d = 0;
      for (int t = 0; t < sl.n_parts; ++t) {
        Part &pt = sl.parts[t];
        size_t x = 0;
        for (Item &it : pt.items) {
          if (it.site < 0) continue;
          const size_t q = size_t(it.site);
          if (d != q) {
            sl.flags_arr[d] = sl.flags_arr[q];
            std::memmove(sl.pl_arr + d * 3 * n_seq, sl.pl_arr + q * 3 * n_seq, 6 * n_seq);
            if (prior_arr) std::memmove(prior_arr + 6 * d, prior_arr + 6 * q, 48);
          }
          if (x < pt.explicit_sites.size() && pt.explicit_sites[x] == q) pt.explicit_sites[x++] = uint32_t(d);
          it.site = int32_t(d++);
        }
      }
      sl.n_sites = d;
    }
    sl.site_base = (int64_t)sites_before;  // -sample: a site's index is its ordinal among the file's sites, whatever the blocks
    sites_before += n_real;
  }
  // fp64 rows: the table's value for every integer field (what the parser computed for it), the parsed rows of the others
  void build_lk_rows(Slot &sl) {
    const size_t n = sl.n_sites;
    sl.lk.resize(n * N3);
    on_threads(sl.n_parts, [&](int t) {
      const size_t lo = n * t / sl.n_parts, hi = n * (t + 1) / sl.n_parts;
      double *rows = sl.lk.data();
      std::fill(rows + lo * N3, rows + hi * N3, 1.0);
      for (size_t q = lo; q < hi; ++q)
        for (size_t j = 0; j < n_seq; ++j) {
          const uint16_t *p = &sl.pl_arr[(q * n_seq + j) * 3];
          if (p[0] == 0xFFFF && p[1] == 0xFFFF && p[2] == 0xFFFF) continue;
          for (int g = 0; g < 3; ++g) rows[q * N3 + size_t(3) * cm.members[j] + g] = pl.value(p[g]);
        }
    });
    for (int t = 0; t < sl.n_parts; ++t) {
      const Part &pt = sl.parts[t];
      for (size_t x = 0; x < pt.explicit_sites.size(); ++x)
        std::copy(&pt.explicit_lk[x * N3], &pt.explicit_lk[(x + 1) * N3], sl.lk.data() + size_t(pt.explicit_sites[x]) * N3);
    }
  }

  // The block's batch through a side output's kernel (full network, whatever -LRC and -method say; -afTagAll: under the rows FPP
  // and FGT were computed with): its plain or its site-prior entry, whose own arguments ride between the input and the outputs.
  void call_side(const SideRow &row, Slot &sl) {
    SideOut &so = sl.side[row.id];
    const SideBytes by = row.bytes(*this);
    so.a.resize((sl.n_sites * by.a + 7) / 8), so.b.resize((sl.n_sites * by.b + 7) / 8), so.status.resize(sl.n_sites);
    const double *lk = sl.packed ? nullptr : sl.lk.data();
    const uint16_t *pl16 = sl.packed ? sl.io.pl : nullptr;
    auto entry = [&](auto plain, auto with_prior, auto... tail) {
      return use_af ? with_prior(ctx, (int64_t)sl.n_sites, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags, sl.prior.data(), tail...)
                    : plain(ctx, (int64_t)sl.n_sites, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags, tail...);
    };
    double *const a = so.a.data(), *const b = so.b.data(), *const none = nullptr;
    int8_t *const a8 = reinterpret_cast<int8_t *>(a);
    uint8_t *const st = so.status.data();
    int rc = 0;
    switch (row.id) {
      case kDnm: rc = entry(famseq_trio_batch, famseq_trio_prior_batch, none, n_kids ? b : none, st); break;
      case kMap: rc = entry(famseq_map_batch, famseq_map_prior_batch, a8, b, st); break;
      case kSiteQ: rc = entry(famseq_evidence_batch, famseq_evidence_prior_batch, a, b, st); break;
      case kLoo: rc = entry(famseq_loo_batch, famseq_loo_prior_batch, a, b, st); break;
      case kMapQ: rc = entry(famseq_maxmarg_batch, famseq_maxmarg_prior_batch, a, b, st); break;
      case kSample: rc = entry(famseq_sample_batch, famseq_sample_prior_batch, o.seed, sl.site_base, (int32_t)o.sample, a8, none, st); break;
      case kSeg: rc = entry(famseq_pattern_batch, famseq_pattern_prior_batch, seg_masks.data(), (int32_t)seg_keys.size(), a, none, st); break;
      case kSwap: return call_swap(sl, so, lk, pl16);
      case kSegPen: rc = call_seg_pen(sl, so, lk, pl16); break;
      case kCountDist: {
        const int32_t T = (count_D + 1) / 2 + 1;
        vector<double> cf(sl.n_sites * size_t(T) * 2);
        rc = entry(famseq_charfn_batch, famseq_charfn_prior_batch, count_cw.data(), T, cf.data(), none, st);
        if (rc == 0) count_distributions(sl, so, cf);
        break;
      }
      case kPhase:
        so.flags = sl.io.flags;
        rc = entry(famseq_origin_batch, famseq_origin_prior_batch, n_kids ? a : none, none, st);
        break;
      case kRateScan:
        rc = entry(famseq_mutrate_batch, famseq_mutrate_prior_batch, o.rate_grid.data(), (int32_t)o.rate_grid.size(), a, b, st);
        if (rc == 0) add_rate_report(sl, so);
        break;
      case kAfEm: {  // the prior is its unknown: one entry, whatever -afTagAll says of the line
        const vector<double> af0(sl.n_sites, o.af_start);
        rc = famseq_af_batch(ctx, (int64_t)sl.n_sites, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags, af0.data(), (int32_t)o.af_em, a, b, st);
        break;
      }
    }
    if (rc != 0) {
      std::cerr << row.entry << (use_af && row.id != kAfEm ? "_prior_batch" : "_batch") << " failed (" << rc << "): " << famseq_last_error(ctx) << std::endl;
      flush_ok = false;
    }
  }
  // -segPen: two launches per block.  The first on the block's rows, the second — the null — on all-ones rows with the block's
  // flags and priors: the phenotypes' probability under the pedigree and the founders' prior alone.  Leaves in so.a[s * M + m]
  // what PSL prints, (wt_ll - loglik) - (wt_ll0 - loglik0): NaN where the site failed or the null is -inf, and no status but 0
  // (a failed site prints "." like a value that does not exist).
  int call_seg_pen(Slot &sl, SideOut &so, const double *lk, const uint16_t *pl16) {
    const size_t n = sl.n_sites, M = o.pen.size() / 3;
    if (ones_lk.size() < n * N3) ones_lk.assign(n * N3, 1.0);
    double *const a = so.a.data(), *const a0 = a + n * M, *const b = so.b.data(), *const b0 = b + n;
    uint8_t *const st = so.status.data();
    vector<uint8_t> st0(n);
    const double *w = pen_tables.data();
    int rc;
    if (use_af) {
      rc = famseq_weight_prior_batch(ctx, (int64_t)n, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags, sl.prior.data(), w, (int32_t)M, a, b, st);
      if (rc == 0) rc = famseq_weight_prior_batch(ctx, (int64_t)n, ones_lk.data(), nullptr, nullptr, 0, sl.io.flags, sl.prior.data(), w, (int32_t)M, a0, b0, st0.data());
    } else {
      rc = famseq_weight_batch(ctx, (int64_t)n, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags, w, (int32_t)M, a, b, st);
      if (rc == 0) rc = famseq_weight_batch(ctx, (int64_t)n, ones_lk.data(), nullptr, nullptr, 0, sl.io.flags, w, (int32_t)M, a0, b0, st0.data());
    }
    if (rc != 0) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t s = 0; s < n; ++s) {
      for (size_t m = 0; m < M; ++m) {
        const double null = a0[s * M + m] - b0[s];
        a[s * M + m] = (st[s] != 0 || st0[s] != 0 || !std::isfinite(null)) ? nan : (a[s * M + m] - b[s]) - null;
      }
      st[s] = 0;
    }
    return 0;
  }
  // -countDist: the inverse DFT of a block's characteristic functions cf[site][j][2], j = 0 .. M / 2 with M = D + 1, the missing
  // frequencies the conjugates of those given: so.a[s * M + k] = p_k = (1 / M) sum_j Re(phi_j omega^(-j k)), (D + 1)^2 operations
  // per site.  A value in [-1e-12, 0) — rounding below an exact 0, within the entry's absolute bar — becomes 0.0; nothing is
  // renormalised.  A failed site's row is NaN and, like -segPen's, leaves no status but 0: it prints "PCD=.".
  void count_distributions(Slot &sl, SideOut &so, const vector<double> &cf) {
    const size_t M = size_t(count_D) + 1, T = M / 2 + 1;
    on_threads(sl.n_parts, [&](int t) {
      for (size_t s = sl.n_sites * t / sl.n_parts; s < sl.n_sites * (t + 1) / sl.n_parts; ++s) {
        double *p = so.a.data() + s * M;
        if (so.status[s] != 0) {
          std::fill(p, p + M, std::numeric_limits<double>::quiet_NaN());
          so.status[s] = 0;
          continue;
        }
        const double *phi = cf.data() + s * T * 2;
        for (size_t k = 0; k < M; ++k) {
          double sum = 0;
          for (size_t j = 0; j < M; ++j) {
            const size_t jj = j < T ? j : M - j, r = j * k % M;
            const double re = phi[2 * jj], im = j < T ? phi[2 * jj + 1] : -phi[2 * jj + 1];
            sum += re * count_cos[r] + im * count_sin[r];
          }
          const double v = sum / double(M);
          p[k] = v < 0 && v >= -1e-12 ? 0.0 : v;
        }
      }
    });
  }
  // -swapCheck: the pairs in groups of at most FAMSEQ_MAX_RELABEL per call, each group's columns summed up over the block's
  // sites in file order behind its call (a pair's sum is its own: the order of the pairs does not enter).  The first group also
  // counts the sites and sums their loglik, which is every group's.
  void call_swap(Slot &sl, SideOut &so, const double *lk, const uint16_t *pl16) {
    const size_t n_pairs = swap_cols.size(), N = size_t(ped.n());
    if (swap_bf.empty()) swap_bf.assign(n_pairs, 0.0), swap_impossible.assign(n_pairs, 0);
    for (size_t first = 0; first == 0 || first < n_pairs; first += FAMSEQ_MAX_RELABEL) {
      const size_t n = std::min<size_t>(FAMSEQ_MAX_RELABEL, n_pairs - first);
      // (a file with one sequenced sample has no pair: the identity alone, for the sites' count and their loglik)
      vector<int32_t> ident(N);
      for (size_t p = 0; p < N; ++p) ident[p] = int32_t(p);
      const int32_t *assign = n_pairs ? swap_assign.data() + first * N : ident.data();
      const int32_t n_assign = n_pairs ? int32_t(n) : 1;
      double *const alt = n_pairs ? so.a.data() : nullptr;
      const int rc = use_af ? famseq_relabel_prior_batch(ctx, (int64_t)sl.n_sites, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags,
                                                         sl.prior.data(), assign, n_assign, alt, so.b.data(), so.status.data())
                            : famseq_relabel_batch(ctx, (int64_t)sl.n_sites, lk, pl16, cm.members.data(), (int32_t)n_seq, sl.io.flags, assign,
                                                   n_assign, alt, so.b.data(), so.status.data());
      if (rc != 0) {
        std::cerr << (use_af ? "famseq_relabel_prior_batch" : "famseq_relabel_batch") << " failed (" << rc << "): " << famseq_last_error(ctx) << std::endl;
        flush_ok = false;
        return;
      }
      add_report(sl, so, first, n_pairs ? n : 0);
    }
  }
  // the block's sites (not its other lines), in file order
  void add_report(const Slot &sl, const SideOut &so, size_t first, size_t n) {
    for (int t = 0; t < sl.n_parts; ++t)
      for (const Item &it : sl.parts[t].items) {
        if (it.site < 0) continue;
        const size_t s = size_t(it.site);
        if (so.status[s] != 0) {
          swap_skipped += first == 0;
          continue;
        }
        if (first == 0) ++swap_used, swap_loglik += so.b[s];
        for (size_t k = 0; k < n; ++k) {
          const double alt = so.a[s * n + k];
          if (std::isfinite(alt)) swap_bf[first + k] += alt - so.b[s];
          else ++swap_impossible[first + k];
        }
      }
  }
  bool write_report() const {
    std::FILE *f = std::fopen(o.swap_file.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "#sites_used=%llu\tsites_skipped=%llu\tlog10_lik=%.6f\n", (unsigned long long)swap_used, (unsigned long long)swap_skipped, swap_loglik);
    std::fprintf(f, "#sample_a\tsample_b\tlog10_BF\tsites_impossible\n");
    for (size_t k = 0; k < swap_cols.size(); ++k)
      std::fprintf(f, "%s\t%s\t%.6f\t%llu\n", sample_names[swap_cols[k].first].c_str(), sample_names[swap_cols[k].second].c_str(),
                   swap_bf.empty() ? 0.0 : swap_bf[k], (unsigned long long)(swap_impossible.empty() ? 0 : swap_impossible[k]));
    return std::fclose(f) == 0;
  }
  // -mRateScan: the block's sites (not its other lines), in file order
  void add_rate_report(const Slot &sl, const SideOut &so) {
    const size_t n = o.rate_grid.size();
    if (rate_sum.empty()) rate_sum.assign(n, 0.0), rate_impossible.assign(n, 0);
    for (int t = 0; t < sl.n_parts; ++t)
      for (const Item &it : sl.parts[t].items) {
        if (it.site < 0) continue;
        const size_t s = size_t(it.site);
        if (so.status[s] != 0) {
          ++rate_skipped;
          continue;
        }
        ++rate_used, rate_own += so.b[s];
        for (size_t k = 0; k < n; ++k) {
          rate_sum[k] += so.a[s * n + k];
          rate_impossible[k] += std::isinf(so.a[s * n + k]);
        }
      }
  }
  bool write_rate_report() const {
    std::FILE *f = std::fopen(o.rate_file.c_str(), "w");
    if (!f) return false;
    const size_t n = o.rate_grid.size();
    const vector<double> sum = rate_sum.empty() ? vector<double>(n, 0.0) : rate_sum;  // (a file without a site)
    auto put = [&](double v) { std::isinf(v) ? std::fprintf(f, "\t-inf") : std::fprintf(f, "\t%.6f", v); };
    std::fprintf(f, "# -mRateScan: %llu sites used, %llu skipped; -mRate %g log10_lik %.6f\n", (unsigned long long)rate_used,
                 (unsigned long long)rate_skipped, o.mrate, rate_own);
    std::fprintf(f, "rate\tlog10_lik\tdelta\tn_impossible\n");
    size_t best = 0;
    for (size_t k = 0; k < n; ++k) {
      std::fprintf(f, "%g", o.rate_grid[k]);
      put(sum[k]);
      put(sum[k] - rate_own);
      std::fprintf(f, "\t%llu\n", (unsigned long long)(rate_impossible.empty() ? 0 : rate_impossible[k]));
      if (sum[k] > sum[best]) best = k;  // (the first of the largest)
    }
    std::fprintf(f, "best\t%g\n", o.rate_grid[best]);
    return std::fclose(f) == 0;
  }
  void gpu_loop() {
    for (;;) {
      const int i = to_flusher.take();
      if (i < 0) break;
      Slot &sl = slots[i];
      if (!ctx && ctx_future.valid()) {  // the first block: the context has been coming up meanwhile
        const double tw = now_s();
        ctx = ctx_future.get();
        t_ctx_wait = now_s() - tw;
        if (!ctx) flush_ok = false;
      }
      const size_t n_staged = sl.pk_flags.size();
      if (sl.staged && flush_ok && !pin(sl, n_staged)) flush_ok = false;
      if (sl.staged && flush_ok) {  // parsed before the runtime was up: into the pinned arrays now
        std::memcpy(sl.io.pl, sl.pk_pl.data(), n_staged * 6 * n_seq);
        std::memcpy(sl.io.flags, sl.pk_flags.data(), n_staged);
      }
      const double t0 = now_s();
      if (sl.n_sites > 0 && flush_ok) {
        const double *lk_in = sl.packed ? nullptr : sl.lk.data();
        const int rc = use_af ? famseq_bn_prior_call_batch(ctx, (int64_t)sl.n_sites, lk_in, lk_in ? nullptr : sl.io.pl, sl.io.flags, sl.prior.data(),
                                                           cm.members.data(), (int32_t)n_seq, sl.io.gpp, sl.io.fpp, sl.io.fgt, sl.io.text, sl.io.status)
                              : sl.io.call(ctx, sl.n_sites, lk_in, cm.members.data());
        if (rc != 0) {
          std::cerr << (use_af ? "famseq_bn_prior_call_batch" : "famseq_bn_call_batch") << " failed (" << rc << "): " << famseq_last_error(ctx) << std::endl;
          flush_ok = false;
        }
        for (const SideRow *row : sides)
          if (flush_ok) call_side(*row, sl);
      }
      t_gpu += now_s() - t0;
      to_formatter.put(i);
    }
    to_formatter.put(-1);
  }

  // -siteQ, -seg, -afEM: columns 1-8 + FORMAT of a site with "FQ=<x>;FLL=<y>", "PSD=<p>;PSR=<q>" and / or "FAF=<q>;FAL=<r>" joined to
  // its INFO column (an INFO of "." is replaced); a site whose evidence (pattern, allele-frequency kernel) failed does without those
  // keys, and keeps its INFO where none is left to add.
  void put_prefix_info(TextBuf &out, const Slot &sl, size_t s, const char *raw, size_t len) const {
    size_t info = 0, end = 0;  // the INFO column is raw[info, end): between the seventh and the eighth tab
    int tabs = 0;
    for (size_t q = 0; q < len && tabs < 8; ++q)
      if (raw[q] == '\t') {
        if (++tabs == 7) info = q + 1;
        if (tabs == 8) end = q;
      }
    bool any = false;
    for (const SideRow *row : infos) any = any || sl.side[row->id].status[s] == 0;
    if (tabs < 8 || !any) {
      out.put(raw, len);
      return;
    }
    out.put(raw, info);
    if (!(end - info == 1 && raw[info] == '.')) {
      out.put(raw + info, end - info);
      if (end > info) out.ch(';');
    }
    bool first = true;
    for (const SideRow *row : infos) {
      if (sl.side[row->id].status[s] != 0) continue;
      if (!first) out.ch(';');
      first = false;
      put_side(row->id, out, *this, sl.side[row->id], s, kInfoColumn);
    }
    out.put(raw + end, len - end);
  }
  // the text of part t of a block, the lines that thread t parsed.  bare: no side field, the sample's text closes its column itself
  template <bool bare>
  void format_part(Slot &sl, int t) const {
    Part &pt = sl.parts[t];
    TextBuf &out = sl.text[t];
    out.n = 0;
    const size_t k = n_seq;
    for (const Item &it : pt.items) {
      if (it.site < 0) {
        out.put(pt.echo.data() + it.echo_off, it.echo_len);
      } else {
        const size_t s = size_t(it.site);
        const Record::Sample *sm = &pt.samples[it.smp];
        if (infos.empty()) out.put(it.raw, it.prefix_len);  // columns 1-8 + FORMAT
        else put_prefix_info(out, sl, s, it.raw, it.prefix_len);
        out.put(format_keys);
        if (sl.io.status[s] & 3) {  // file.cpp:607-620
          pt.any_failed = true;
          for (size_t j = 0; j < k; ++j) {
            out.put(it.raw + sm[j].off, sm[j].len);
            out.put(":NA:NA:NA\t", bare ? 10 : 9);
            if (bare) continue;
            for (const SideRow *row : fields) out.put(row->na);
            out.ch('\t');
          }
        } else {
          for (size_t j = 0; j < k; ++j) {
            if (sm[j].missing) {
              for (uint32_t q = 0; q < it.n_fmt; ++q) out.put("NA:", 3);
            } else {
              out.put(it.raw + sm[j].off, sm[j].len);
              out.ch(':');
            }
            out.called(sl.io.text, sl.io.gpp, sl.io.fpp, sl.io.fgt, s * k + j, bare);
            if (bare) continue;
            for (const SideRow *row : fields) put_side(row->id, out, *this, sl.side[row->id], s, j);
            out.ch('\t');
          }
        }
      }
      out.ch('\n');
    }
  }
  // ... the results are turned into text on their own thread (and its helpers) while the next block is at the GPU ...
  void format_loop() {
    for (;;) {
      const int i = to_formatter.take();
      if (i < 0) break;
      Slot &sl = slots[i];
      const double t1 = now_s();
      if (flush_ok) {
        on_parts(sl.n_parts, format_threads, [&](int t) { fields.empty() ? format_part<true>(sl, t) : format_part<false>(sl, t); });
        t_format += now_s() - t1;
      }
      to_writer.put(i);
    }
    to_writer.put(-1);
  }
  // ... and the text goes out on a third thread, so that block k + 1 is at the GPU and being formatted while block k is
  // written (formatting 0.50 s + writing 0.25 s per 3 M ten-member sites were one thread's work in round 2)
  void write_loop() {
    for (;;) {
      const int i = to_writer.take();
      if (i < 0) break;
      Slot &sl = slots[i];
      if (flush_ok) {
        const double t2 = now_s();
        for (int t = 0; t < sl.n_parts; ++t) {
          const Part &pt = sl.parts[t];
          if (pt.any_failed)  // the reference's warning on stdout, in input order (file.cpp:607-612)
            for (const Item &it : pt.items)
              if (it.site >= 0 && (sl.io.status[it.site] & 3))
                std::cout << "Warning: this variant hasn't been calculated: " << std::endl << std::string_view(it.raw, it.raw_len) << std::endl;
        }
        // (one pwrite per thread at its own offset was tried: 0.33 s per 1.47 GB as well — the page cache, not the stream)
        for (int t = 0; t < sl.n_parts; ++t) fout.write(sl.text[t].v.data(), (std::streamsize)sl.text[t].n);
        if (fout.fail()) {
          std::cerr << "cannot write " << o.out_file << std::endl;
          flush_ok = false;
        }
        t_write += now_s() - t2;
      }
      to_driver.put(i);
    }
  }
};

// ---- the rows.  A field's text by the drivers' rule for FPP where it is Phred-scaled: fabs(-10 log10 p), 99999 for 0
// (file.cpp:696-745); a field whose own kernel failed at the site prints what a failed site prints.
double phred(double p) { return p == 0 ? 99999.0 : std::fabs(-10.0 * std::log10(p)); }

inline void put_dnp(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {  // "." for a founder
  const int kid = r.kid_of_col[j];
  if (kid < 0) return out.put(":.", 2);
  if (so.status[s] != 0) return out.put(":NA", 3);
  out.ch(':');
  out.num(so.b[s * size_t(r.n_kids) + size_t(kid)]);
}
inline void put_map(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {
  if (so.status[s] != 0) return out.put(":NA:NA", 6);
  const int gt = so.a8()[s * size_t(r.ped.n()) + size_t(r.cm.members[j])];
  out.put(gt == 0 ? ":0/0:" : (gt == 1 ? ":0/1:" : ":1/1:"), 5);
  out.num(so.b[s]);
}
inline void put_loo(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {
  if (so.status[s] != 0) return out.put(":NA:NA", 6);
  const size_t mem = s * size_t(r.ped.n()) + size_t(r.cm.members[j]);
  for (int g = 0; g < 3; ++g) {
    out.ch(g ? ',' : ':');
    out.num(phred(so.a[3 * mem + size_t(g)]));
  }
  out.ch(':');
  out.num(phred(so.b[mem]));
}
inline void put_sgt(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {  // the draws' alt-allele counts, draw 0 first
  if (so.status[s] != 0) return out.put(":NA", 3);
  const size_t n = size_t(r.ped.n());
  const int8_t *g = so.a8() + s * size_t(r.o.sample) * n + size_t(r.cm.members[j]);
  for (int k = 0; k < r.o.sample; ++k) {
    out.ch(k ? ',' : ':');
    out.ch(char('0' + g[size_t(k) * n]));
  }
}
inline void put_fq(TextBuf &out, const VcfRun &, const SideOut &so, size_t s, size_t) {
  out.put("FQ=", 3);
  out.num(phred(so.b[s]));
  out.put(";FLL=", 5);
  out.num(so.a[s]);
}
// (plain probabilities: the value of interest is near 1, where Phred has no resolution)
inline void put_seg(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t) {
  const size_t n_seg = r.seg_keys.size();
  for (size_t m = 0; m < n_seg; ++m) {
    if (m) out.ch(';');
    out.put(r.seg_keys[m], 4);
    out.num(so.a[s * n_seg + m]);
  }
}

// (FAL: inf where the data exclude an allele frequency of 0)
inline void put_faf(TextBuf &out, const VcfRun &, const SideOut &so, size_t s, size_t) {
  out.put("FAF=", 4);
  out.num(so.a[s]);
  out.put(";FAL=", 5);
  out.num(so.b[2 * s] - so.b[2 * s + 1]);
}

// -phase: "a|b" (the maternal allele first) of the largest of the child's four origin posteriors, the lowest index 2 a + b among
// equals, and that posterior; a son at a chrX site has the maternal allele alone; "." for a founder and at a failed site
inline void put_phase(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {
  const int kid = r.kid_of_col[j];
  if (kid < 0 || so.status[s] != 0) return out.put(":.:.", 4);
  const double *p = so.a.data() + 4 * (s * size_t(r.n_kids) + size_t(kid));
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (p[i] > p[best]) best = i;
  out.ch(':');
  out.ch(char('0' + (best >> 1)));
  if (!((so.flags[s] & FAMSEQ_FLAG_CHRX) && r.ped.gender[size_t(r.cm.members[j])] == 1)) {
    out.ch('|');
    out.ch(char('0' + (best & 1)));
  }
  out.ch(':');
  out.num(p[best]);
}

// -segPen: one value per model, printed as FLL's are; "-inf" where the data rule the phenotypes out under the model, "." where
// there is no value (VcfRun::call_seg_pen)
inline void put_psl(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t) {
  const size_t M = r.o.pen.size() / 3;
  out.put("PSL=", 4);
  for (size_t m = 0; m < M; ++m) {
    if (m) out.ch(',');
    const double v = so.a[s * M + m];
    if (std::isnan(v)) out.ch('.');
    else if (std::isinf(v)) v < 0 ? out.put("-inf", 4) : out.put("inf", 3);
    else out.num(v);
  }
}

// -mapQ: JGQ, the Phred-scaled ratio of the largest entry of the member's max-marginal row to its second largest (99999 where
// the second largest is 0: no configuration of positive weight calls the member differently), printed as FPP is; in the INFO
// column JP2, the runner-up configuration's posterior
inline void put_mapq(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {
  if (j == kInfoColumn) {
    out.put("JP2=", 4);
    return out.num(so.b[2 * s + 1]);
  }
  if (so.status[s] != 0) return out.put(":NA", 3);
  const double *m = so.a.data() + 3 * (s * size_t(r.ped.n()) + size_t(r.cm.members[j]));
  int best = 0;
  for (int g = 1; g < 3; ++g)
    if (m[g] > m[best]) best = g;
  const double second = std::max(m[(best + 1) % 3], m[(best + 2) % 3]);
  out.ch(':');
  out.num(second == 0 ? 99999.0 : std::fabs(-10.0 * std::log10(second / m[best])));
}

// -countDist: the D + 1 probabilities of the count, printed as FLL's value is; "." where the site failed
// (VcfRun::count_distributions)
inline void put_pcd(TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t) {
  const size_t M = size_t(r.count_D) + 1;
  out.put("PCD=", 4);
  if (std::isnan(so.a[s * M])) return out.ch('.');
  for (size_t k = 0; k < M; ++k) {
    if (k) out.ch(',');
    out.num(so.a[s * M + k]);
  }
}

[[gnu::always_inline]] inline void put_side(SideId id, TextBuf &out, const VcfRun &r, const SideOut &so, size_t s, size_t j) {
  switch (id) {
    case kCountDist: return put_pcd(out, r, so, s, j);
    case kMapQ: return put_mapq(out, r, so, s, j);
    case kSegPen: return put_psl(out, r, so, s, j);
    case kPhase: return put_phase(out, r, so, s, j);
    case kDnm: return put_dnp(out, r, so, s, j);
    case kMap: return put_map(out, r, so, s, j);
    case kSiteQ: return put_fq(out, r, so, s, j);
    case kLoo: return put_loo(out, r, so, s, j);
    case kSample: return put_sgt(out, r, so, s, j);
    case kSeg: return put_seg(out, r, so, s, j);
    case kAfEm: return put_faf(out, r, so, s, j);
    case kSwap: return;  // (a report row: nothing on a line)
    case kRateScan: return;
  }
}

// -seg's own options: -affected / -unaffected without it, an unknown model or ID
bool check_seg(const Options &o, const Ped &ped) {
  if (o.seg.empty()) {  // (with -segPen the two lists are its own and this row is off)
    std::cout << "-affected and -unaffected belong to -seg dominant|recessive|both, which was not given." << std::endl;
    return false;
  }
  vector<uint8_t> masks;
  vector<const char *> keys;
  return segregation_masks(o, ped, masks, keys);
}

// -segPen's own: 1 .. FAMSEQ_MAX_WEIGHTS models of three numbers in [0, 1], -affected, and the IDs of both lists
bool check_seg_pen(const Options &o, const Ped &ped) {
  if (o.pen_is_bad) {
    std::cout << "-segPen takes penetrance models F0,F1,F2[/F0,F1,F2...], three numbers in [0, 1] each, not \"" << o.pen_bad << "\"." << std::endl;
    return false;
  }
  if (o.pen.size() / 3 > FAMSEQ_MAX_WEIGHTS) {
    std::cout << "-segPen takes at most " << FAMSEQ_MAX_WEIGHTS << " models, not " << o.pen.size() / 3 << "." << std::endl;
    return false;
  }
  if (o.affected.empty()) {
    std::cout << "-segPen needs the affected members: -affected ID[,ID...] (PED IDs)." << std::endl;
    return false;
  }
  vector<double> tables;
  return penetrance_tables(o, ped, tables);
}

// -countDist's own: -countOf without it, an unknown kind, an ID the PED file does not hold or names twice, a count whose
// distribution needs more frequencies than one call takes
bool check_count_dist(const Options &o, const Ped &ped) {
  if (!o.count_given) {
    std::cout << "-countOf belongs to -countDist carriers|alleles|homalt, which was not given." << std::endl;
    return false;
  }
  const int *score = count_kind_scores(o.count_kind);
  if (!score) {
    std::cout << "-countDist takes carriers, alleles or homalt, not \"" << o.count_kind << "\"." << std::endl;
    return false;
  }
  vector<uint8_t> counted;
  if (!counted_members(o, ped, counted)) return false;
  const int D = score[2] * int(std::count(counted.begin(), counted.end(), 1)), tables = (D + 1) / 2 + 1;
  if (tables > FAMSEQ_MAX_CWEIGHTS) {
    std::cout << "-countDist " << o.count_kind << ": the count reaches D = " << D << ", whose distribution needs " << tables
              << " frequencies; one call takes at most " << FAMSEQ_MAX_CWEIGHTS << ". Count fewer members (-countOf)." << std::endl;
    return false;
  }
  return true;
}

// -afEM's own options: -afStart without it, a step count or a start value out of range
bool check_af_em(const Options &o, const Ped &) {
  if (o.af_em == Options::kAfUnset) {
    std::cout << "-afStart belongs to -afEM T, which was not given." << std::endl;
    return false;
  }
  if (o.af_em < 0 || o.af_em > FAMSEQ_MAX_AF_ITER) {
    std::cout << "-afEM takes the number of EM steps, 0.." << FAMSEQ_MAX_AF_ITER << "." << std::endl;
    return false;
  }
  if (!(o.af_start > 0.0 && o.af_start < 1.0)) {
    std::cout << "-afStart takes the allele frequency the steps start from, a number in (0, 1); default 0.5." << std::endl;
    return false;
  }
  return true;
}

// -swapCheck's own: the report file must be writable before any input is read (opened for appending: an existing file is kept
// as it is until the run's own report replaces it)
bool check_swap(const Options &o, const Ped &) {
  std::FILE *f = o.swap_file.empty() ? nullptr : std::fopen(o.swap_file.c_str(), "a");
  if (!f) {
    std::cout << "Cannot write " << o.swap_file << " (the report file of -swapCheck)." << std::endl;
    return false;
  }
  std::fclose(f);
  return true;
}

// -mRateScan's own: its two options go together, the grid holds 1 .. FAMSEQ_MAX_RATES numbers in [0, 1], and the report file must
// be writable before any input is read (as check_swap)
bool check_rate_scan(const Options &o, const Ped &) {
  if (!o.rate_scan_given) {
    std::cout << "-mRateGrid gives the rates of -mRateScan FILE, which hasn't been set." << std::endl;
    return false;
  }
  if (o.rate_grid.empty()) {
    std::cout << "-mRateGrid takes the mutation rates to scan, r1,r2,...: the grid is empty." << std::endl;
    return false;
  }
  if (o.rate_grid.size() > FAMSEQ_MAX_RATES) {
    std::cout << "-mRateGrid takes at most " << FAMSEQ_MAX_RATES << " rates, not " << o.rate_grid.size() << "." << std::endl;
    return false;
  }
  if (o.rate_grid_is_bad) {
    std::cout << "-mRateGrid takes mutation rates, numbers in [0, 1], not \"" << o.rate_grid_bad << "\"." << std::endl;
    return false;
  }
  std::FILE *f = o.rate_file.empty() ? nullptr : std::fopen(o.rate_file.c_str(), "a");
  if (!f) {
    std::cout << "Cannot write " << (o.rate_file.empty() ? "the report file of -mRateScan: it hasn't been set." : o.rate_file + " (the report file of -mRateScan).")
              << std::endl;
    return false;
  }
  std::fclose(f);
  return true;
}

const SideRow kSide[kSides] = {
    {kDnm, "-dnm", "famseq_trio", false, [](const Options &o) { return o.dnm; }, [](Options &o) { o.dnm = false; }, nullptr,
     [](std::ostream &out, const Options &) {
       out << "##FORMAT=<ID=DNP,Number=1,Type=Float,Description=\"Posterior probability of a de novo mutation (genotype "
              "Mendelian-inconsistent with the parents')\">" << std::endl;
     },
     ":DNP", ":NA", [](const VcfRun &r) { return SideBytes{0, 8 * size_t(r.n_kids)}; }},
    {kMap, "-map", "famseq_map", false, [](const Options &o) { return o.map; }, [](Options &o) { o.map = false; }, nullptr,
     [](std::ostream &out, const Options &) {
       out << "##FORMAT=<ID=JGT,Number=1,Type=String,Description=\"Genotype in the most probable joint genotype configuration of "
              "the whole family\">" << std::endl;
       out << "##FORMAT=<ID=JP,Number=1,Type=Float,Description=\"Posterior probability of that joint configuration\">" << std::endl;
     },
     ":JGT:JP", ":NA:NA", [](const VcfRun &r) { return SideBytes{size_t(r.ped.n()), 8}; }},
    {kSiteQ, "-siteQ", "famseq_evidence", true, [](const Options &o) { return o.siteq; }, [](Options &o) { o.siteq = false; }, nullptr,
     [](std::ostream &out, const Options &) {
       out << "##INFO=<ID=FQ,Number=1,Type=Float,Description=\"Family variant quality: Phred-scaled posterior probability that every "
              "member of the family is homozygous reference\">" << std::endl;
       out << "##INFO=<ID=FLL,Number=1,Type=Float,Description=\"log10 likelihood of the site's data under the pedigree\">" << std::endl;
     },
     nullptr, nullptr, [](const VcfRun &) { return SideBytes{8, 8}; }},
    {kLoo, "-loo", "famseq_loo", true, [](const Options &o) { return o.loo; }, [](Options &o) { o.loo = false; }, nullptr,
     [](std::ostream &out, const Options &) {
       out << "##FORMAT=<ID=LOP,Number=G,Type=Float,Description=\"Phred-scaled genotype probabilities given the data of every other "
              "member of the family, the sample's own left out\">" << std::endl;
       out << "##FORMAT=<ID=LOF,Number=1,Type=Float,Description=\"Phred-scaled predictive likelihood of the sample's data given the "
              "other members' (99999: impossible given the relatives)\">" << std::endl;
     },
     ":LOP:LOF", ":NA:NA", [](const VcfRun &r) { return SideBytes{24 * size_t(r.ped.n()), 8 * size_t(r.ped.n())}; }},
    {kSample, "-sample", "famseq_sample", false, [](const Options &o) { return o.sample != 0; }, [](Options &o) { o.sample = 0; }, nullptr,
     [](std::ostream &out, const Options &o) {
       out << "##FORMAT=<ID=SGT,Number=.,Type=Integer,Description=\"Alternate allele counts of the sample in " << o.sample
           << " joint genotype configurations of the whole family drawn from their posterior (seed " << o.seed << ")\">" << std::endl;
     },
     ":SGT", ":NA", [](const VcfRun &r) { return SideBytes{size_t(r.o.sample) * size_t(r.ped.n()), 0}; }},
    // (on: any of its three options, so that main can say which one is missing)
    // (with -segPen and without -seg the two lists are -segPen's)
    {kSeg, "-seg", "famseq_pattern", true,
     [](const Options &o) { return !o.seg.empty() || (!o.pen_given && !(o.affected.empty() && o.unaffected.empty())); },
     [](Options &o) { o.seg.clear(), o.affected.clear(), o.unaffected.clear(); }, check_seg,
     [](std::ostream &out, const Options &o) {
       if (o.seg != "recessive")
         out << "##INFO=<ID=PSD,Number=1,Type=Float,Description=\"Posterior probability that the affected members, and no unaffected one, "
                "carry the variant (dominant segregation pattern)\">" << std::endl;
       if (o.seg != "dominant")
         out << "##INFO=<ID=PSR,Number=1,Type=Float,Description=\"Posterior probability that the affected members, and no unaffected one, "
                "are homozygous for the variant (recessive segregation pattern)\">" << std::endl;
     },
     nullptr, nullptr, [](const VcfRun &r) { return SideBytes{8 * r.seg_keys.size(), 0}; }},
    // (on: either of its options, so that main can say which one is missing)
    {kAfEm, "-afEM", "famseq_af", true, [](const Options &o) { return o.af_em != Options::kAfUnset || o.af_start_given; },
     [](Options &o) { o.af_em = Options::kAfUnset, o.af_start_given = false; }, check_af_em,
     [](std::ostream &out, const Options &o) {
       out << "##INFO=<ID=FAF,Number=1,Type=Float,Description=\"Maximum-likelihood allele frequency among the family's founders after "
           << o.af_em << " EM steps from " << o.af_start << "\">" << std::endl;
       out << "##INFO=<ID=FAL,Number=1,Type=Float,Description=\"log10 likelihood ratio of the site's data at that allele frequency against "
              "no founder carrying the allele\">" << std::endl;
     },
     nullptr, nullptr, [](const VcfRun &) { return SideBytes{8, 16}; }},
    {kSwap, "-swapCheck", "famseq_relabel", true, [](const Options &o) { return o.swap_given; },
     [](Options &o) { o.swap_given = false, o.swap_file.clear(); }, check_swap, [](std::ostream &, const Options &) {}, nullptr, nullptr,
     [](const VcfRun &r) { return SideBytes{8 * std::min<size_t>(FAMSEQ_MAX_RELABEL, r.swap_cols.size()), 8}; }, /*report=*/true},
    // (on: either of its options, so that main can say which one is missing)
    {kRateScan, "-mRateScan", "famseq_mutrate", true, [](const Options &o) { return o.rate_scan_given || o.rate_grid_given; },
     [](Options &o) { o.rate_scan_given = o.rate_grid_given = false, o.rate_file.clear(); }, check_rate_scan, [](std::ostream &, const Options &) {},
     nullptr, nullptr, [](const VcfRun &r) { return SideBytes{8 * r.o.rate_grid.size(), 8}; }, /*report=*/true},
    {kPhase, "-phase", "famseq_origin", true, [](const Options &o) { return o.phase; }, [](Options &o) { o.phase = false; }, nullptr,
     [](std::ostream &out, const Options &) {
       out << "##FORMAT=<ID=PGT,Number=1,Type=String,Description=\"Phased genotype by transmission, maternal|paternal allele (0 ref, 1 alt): "
              "the most probable pair of alleles received from mother and father given the whole family's data; the maternal allele "
              "alone for a son on chromosome X; . for a founder\">" << std::endl;
       out << "##FORMAT=<ID=PGP,Number=1,Type=Float,Description=\"Posterior probability of that maternal|paternal pair\">" << std::endl;
     },
     ":PGT:PGP", ":.:.", [](const VcfRun &r) { return SideBytes{32 * size_t(r.n_kids), 0}; }},
    // (its bytes: wt_loglik and loglik of the block's rows and of the null call's, VcfRun::call_seg_pen)
    {kSegPen, "-segPen", "famseq_weight", true, [](const Options &o) { return o.pen_given; },
     [](Options &o) { o.pen_given = false, o.pen.clear(); }, check_seg_pen,
     [](std::ostream &out, const Options &) {
       out << "##INFO=<ID=PSL,Number=.,Type=Float,Description=\"log10 Bayes factor of the phenotypes of the affected and unaffected members "
              "under each penetrance model of -segPen: their probability given the whole family's data over their probability under the "
              "pedigree and the founders' prior alone (-inf: the data rule them out; .: no value)\">" << std::endl;
     },
     nullptr, nullptr, [](const VcfRun &r) { return SideBytes{16 * (r.o.pen.size() / 3), 16}; }},
    // (not tied to -map: with both, JGT stays the MAP kernel's, whose tie rule differs from a row's arg-max only under exact ties)
    {kMapQ, "-mapQ", "famseq_maxmarg", true, [](const Options &o) { return o.mapq; }, [](Options &o) { o.mapq = false; }, nullptr,
     [](std::ostream &out, const Options &) {
       out << "##FORMAT=<ID=JGQ,Number=1,Type=Float,Description=\"Quality of the sample's genotype in the most probable joint configuration of "
              "the whole family: Phred-scaled ratio of the posterior of the best configuration in which the sample has another genotype to "
              "that of the best configuration (99999: no such configuration has any probability)\">" << std::endl;
       out << "##INFO=<ID=JP2,Number=1,Type=Float,Description=\"Posterior probability of the second most probable joint genotype "
              "configuration of the whole family\">" << std::endl;
     },
     ":JGQ", ":NA", [](const VcfRun &r) { return SideBytes{24 * size_t(r.ped.n()), 16}; }, /*report=*/false, /*info_too=*/true},
    // (on: either of its options, so that main can say which one is missing; its first array: the distribution, D + 1 doubles)
    {kCountDist, "-countDist", "famseq_charfn", true, [](const Options &o) { return o.count_given || o.count_of_given; },
     [](Options &o) { o.count_given = o.count_of_given = false; }, check_count_dist,
     [](std::ostream &out, const Options &o) {
       out << "##INFO=<ID=PCD,Number=.,Type=Float,Description=\"Posterior distribution of the number of "
           << (o.count_kind == "carriers" ? "carriers of the variant" : (o.count_kind == "alleles" ? "alternate alleles" : "homozygous-alternate members"))
           << " among " << (o.count_of_given ? "the members " + o.count_of : string("all members")) << " of the family: the probabilities of 0, 1, ... "
              "given the whole family's data, each to 1e-12 absolute (.: the site failed)\">" << std::endl;
     },
     nullptr, nullptr, [](const VcfRun &r) { return SideBytes{8 * (size_t(r.count_D) + 1), 0}; }},
};

// `FamSeq vcf` and `FamSeq pack`: the wiring of a VcfRun's stages
bool run_vcf(const Options &o, const Ped &ped) {
  VcfRun r{o, ped};
  if (!r.fin.open(o.vcf_files[0])) {
    std::cout << "Cannot open " << o.vcf_files[0] << std::endl;
    return false;
  }
  if (!r.set_up()) return false;
  if (!o.pack_mode) r.fout.open(o.out_file.c_str());  // pack mode writes a binary file: the text header goes nowhere
  std::string_view line;
  bool more = false;  // `line` holds a data line that has not been cut into a block yet
  const vector<string> head = split_keep(r.echo_header(line, more), '\t');
  if (!r.map_header(head)) return false;
  if (!o.loc_file.empty() && !r.read_locations()) return false;
  if (o.swap_given && !o.pack_mode) r.set_up_swaps(head);
  if (o.pack_mode) {
    vector<string> names;
    for (int c : r.cm.cols) names.push_back(head[9 + c]);
    if (names.empty() || !r.packer.open(o.out_file, names)) {
      std::cout << "Cannot write " << o.out_file << " (or no sample of the vcf file is in the ped file)." << std::endl;
      return false;
    }
  } else if (r.cm.cols.empty()) {  // nothing to compute and nothing to print per sample: say so instead of walking the file
    std::cout << "No sample of the vcf file is in the ped file (the names in the ped file's fifth column must match the vcf header)." << std::endl;
    return false;
  }
  // HIP start-up (runtime initialisation, context, streams, code objects: about a quarter of a second) runs on its own
  // thread while this one cuts and parses the first block(s); the flusher thread, the first to need the context, waits for it.
  // Until it is there the blocks are parsed into ordinary memory (pinned buffers need the runtime) and copied over — 6 bytes
  // per sample and site — once it is.
  if (!o.pack_mode)
    r.ctx_future = std::async(std::launch::async, [&] {
      famseq_ctx *c = make_ctx(o, ped, r.cm.sequenced, r.m);
      r.hip_up = true;
      return c;
    });
  std::thread flusher([&] { r.gpu_loop(); }), formatter([&] { r.format_loop(); }), writer([&] { r.write_loop(); });
  const double t_begin = now_s();
  for (int i = 0; i < 4; ++i) r.to_driver.put(i);
  bool ok = true;
  while (more && ok && r.flush_ok) {
    const double t0 = now_s();
    const int i = r.to_driver.take();  // a slot whose previous block is written
    Slot &sl = r.slots[i];
    r.t_stall += now_s() - t0;
    if (!r.cut_and_parse(sl, line, more, &ok)) {
      r.to_driver.put(i);
      break;
    }
    const double t3 = now_s();
    if (o.pack_mode) {
      r.pack_records(sl);
    } else {
      r.move_sites_together(sl);
      if (!sl.packed) r.build_lk_rows(sl);
    }
    r.t_gather += now_s() - t3;
    (o.pack_mode ? r.to_driver : r.to_flusher).put(i);
  }
  r.to_flusher.put(-1);
  flusher.join();
  formatter.join();
  writer.join();
  if (!r.ctx && r.ctx_future.valid()) r.ctx = r.ctx_future.get();  // a file without a single data line: nobody asked for it yet
  ok = ok && r.flush_ok && (o.pack_mode || r.ctx);
  if (std::getenv("FAMSEQ_TIMING") && !o.pack_mode)
    std::cerr << "FamSeq vcf: loop " << now_s() - t_begin << " s; this thread: cutting lines " << r.t_lines << ", parsing " << r.t_parse
              << ", fp64 rows / pack records " << r.t_gather << ", waiting for the flusher " << r.t_stall << "; flusher thread: GPU calls " << r.t_gpu
              << ", formatting " << r.t_format << ", writing " << r.t_write << ", waiting for the context " << r.t_ctx_wait << std::endl;
  if (o.pack_mode) {
    std::cout << r.packer.n_sites << " sites packed";
    if (r.packer.skipped) std::cout << ", " << r.packer.skipped << " skipped (PL/GL field is not a plain integer)";
    std::cout << std::endl;
    return r.packer.close();
  }
  for (Slot &sl : r.slots) sl.io.release();
  r.fout.close();
  famseq_destroy(r.ctx);
  if (ok && o.swap_given && !r.write_report()) {
    std::cout << "Cannot write " << o.swap_file << " (the report file of -swapCheck)." << std::endl;
    return false;
  }
  if (ok && o.rate_scan_given && !r.write_rate_report()) {
    std::cout << "Cannot write " << o.rate_file << " (the report file of -mRateScan)." << std::endl;
    return false;
  }
  return ok && !r.fout.fail();
}

// ---- LK driver (file.cpp:1640-1886) ----------------------------------------------------------

bool run_lk(const Options &o, const Ped &ped) {
  std::ifstream fin(o.lk_file.c_str());
  if (!fin.is_open()) {
    std::cout << "Cannot open " << o.lk_file << std::endl;
    return false;
  }
  string title, line;
  std::getline(fin, title);
  const vector<string> head = split_keep(title, '\t');
  const ColumnMap cm = map_columns(head.data(), head.size(), ped);
  CliModel m;
  famseq_ctx *ctx = make_ctx(o, ped, cm.sequenced, m);
  if (!ctx) return false;
  std::ofstream fout(o.out_file.c_str());
  put_lk_header(fout, o, m, head, cm.cols);
  BatchCaller caller(ctx, ped.n(), cm.members, fout, batch_capacity());
  vector<double> lk(size_t(3) * ped.n());
  bool ok = true;
  while (ok && std::getline(fin, line)) {
    if (line.size() < 2) break;
    vector<std::string_view> t;
    split_views(line, '\t', t);
    if (!cm.cols.empty() && t.size() <= size_t(cm.cols.back())) continue;  // short row
    std::fill(lk.begin(), lk.end(), 1.0);
    Record r;
    r.head = "LK:GPP:FPP:FGT\t";
    for (int c : cm.cols) {
      r.samples.push_back({uint32_t(t[c].data() - line.data()), uint32_t(t[c].size()), false});
      const vector<string> v = split_keep(string(t[c]), ',');
      for (int g = 0; g < 3 && g < (int)v.size(); g++) {
        double x = std::atof(v[g].c_str());
        if (o.lk_type == 2) x = std::pow(10.0, x);
        else if (o.lk_type == 3) x = std::exp(x);
        else if (o.lk_type == 4) x = std::pow(10.0, -x / 10.0);
        lk[size_t(3) * cm.member[c] + g] = x;
      }
    }
    r.raw = line;
    ok = caller.site(std::move(r), lk, nullptr, 0);  // calPostProbBN() defaults: Known=false, chrType=0 (file.cpp:1751)
  }
  ok = ok && caller.flush();
  famseq_destroy(ctx);
  return ok;
}

// ---- `FamSeq tune -vcfFile f -pedFile p`: the generated kernels depend on the pedigree and on which of its members the
// vcf file has columns for; time their variants on this GPU (famseq_set_option "tune") and leave the picks in the cache.
bool run_tune(const Options &o, const Ped &ped) {
  LineSource fin;
  if (!fin.open(o.vcf_files[0])) {
    std::cout << "Cannot open " << o.vcf_files[0] << std::endl;
    return false;
  }
  std::string_view line;
  string title;
  while (fin.next(line) && !line.empty() && line[0] == '#') title.assign(line);
  const vector<string> head = split_keep(title, '\t');
  const size_t first = std::min<size_t>(9, head.size());
  CliModel m;
  famseq_ctx *ctx = make_ctx(o, ped, map_columns(head.data() + first, head.size() - first, ped).sequenced, m);
  if (!ctx) return false;
  const int rc = famseq_set_option(ctx, "tune", 1);
  if (rc != 0) std::cout << "Tuning failed: " << famseq_last_error(ctx) << std::endl;
  else {
    const string plan = famseq_plan_json(ctx);
    const size_t k = plan.find("\"tune\":\"");
    std::cout << (k == string::npos ? plan : plan.substr(k + 8, plan.size() - k - 10)) << std::endl;
  }
  famseq_destroy(ctx);
  return rc == 0;
}

void usage_top() {
  std::cout << std::endl
            << "Program: FamSeq (Sequence calling using pedigree information), MI355X build of the -method 1 path"
            << std::endl << "Usage:\tFamSeq <input type> [options]" << std::endl << std::endl
            << "Input type: \tvcf\t\tinput vcf file" << std::endl << "\t\tLK\t\tinput likelihood file" << std::endl
            << std::endl << "Type FamSeq -h for help." << std::endl << std::endl;
}

void help() {
  std::cout << "Usage:\tFamSeq <input type> [options]" << std::endl << std::endl
            << "FamSeq vcf [options] for vcf input, FamSeq LK [options] for likelihood-only input." << std::endl
            << std::endl << "Options:" << std::endl << std::endl
            << "-vcfFile\tThe name of input vcf file." << std::endl
            << "-lkFile\t\tThe name of input likelihood only format file." << std::endl
            << "-lkType\t\tn:normal(default); log10: log10 scaled; ln: ln scaled; PS: phred scaled." << std::endl
            << "-pedFile\tThe name of the file storing the pedigree information." << std::endl
            << "-output\t\tThe name of output file" << std::endl
            << "-method\t\t1(default): Bayesian network enumeration; 2: exact sum-product." << std::endl
            << "-mRate\t\tMutation rate. The default value is 1e-7" << std::endl
            << "-v\t\tOnly record the position at which the genotype is not RR in the output file." << std::endl
            << "-a\t\tRecord all the position in the output file." << std::endl
            << "-l\t\tLocation file (chromosome<TAB>position): only these positions are processed." << std::endl
            << "-genoProbN\tPr(G) for autosome, variant not in dbSNP. Default 0.9985 0.001 0.0005." << std::endl
            << "-genoProbK\tPr(G) for autosome, variant in dbSNP. Default 0.45 0.1 0.45." << std::endl
            << "-genoProbXN\tPr(G) for chromosome X of males, not in dbSNP. Default 0.999 0.001." << std::endl
            << "-genoProbXK\tPr(G) for chromosome X of males, in dbSNP. Default 0.5 0.5." << std::endl
            << "-LRC\t\tLikelihood ratio criterion for the single-sample shortcut. Default 1." << std::endl
            << "-afTag KEY\t(vcf) Founders' genotype prior per line: Hardy-Weinberg at the allele frequency KEY= of the INFO column (the first" << std::endl
            << "\t\tvalue of a list), where it lies in (0, 1); the model's priors elsewhere. Implies -method 2; not with -dnm / -map." << std::endl
            << "-afTagAll KEY\t(vcf) -afTag KEY for every field the line prints: DNP, JGT and JP are computed under the line's prior too." << std::endl
            << "\t\tMay be combined with -dnm and -map; not with -afTag. Implies -method 2." << std::endl
            << "-dnm\t\t(vcf) Add DNP, each child's posterior probability of a de novo mutation, to every sample column." << std::endl
            << "-map\t\t(vcf) Add JGT and JP, each member's genotype in the most probable joint configuration of the family and" << std::endl
            << "\t\tthat configuration's posterior probability, to every sample column." << std::endl
            << "-siteQ\t\t(vcf) Add FQ, the Phred-scaled posterior probability that no member of the family carries a variant, and FLL," << std::endl
            << "\t\tthe log10 likelihood of the site under the pedigree, to the INFO column. Implies -method 2; may be combined with" << std::endl
            << "\t\t-dnm, -map and -afTagAll; not with -afTag." << std::endl
            << "-loo\t\t(vcf) Add LOP, the sample's Phred-scaled genotype probabilities given every other member's data with its own" << std::endl
            << "\t\tleft out, and LOF, the Phred-scaled likelihood of its own data given theirs (99999: impossible given the relatives)," << std::endl
            << "\t\tto every sample column. Implies -method 2; may be combined with -dnm, -map, -siteQ and -afTagAll; not with -afTag." << std::endl
            << "-sample K\t(vcf) Add SGT, the sample's alt-allele counts in K (1.." << FAMSEQ_MAX_DRAWS << ") joint genotype configurations of the whole" << std::endl
            << "\t\tfamily drawn from their posterior, draw 0 first; -seed S (default 0) seeds them. A line's draws depend on the seed" << std::endl
            << "\t\tand on its ordinal among the file's sites, not on FAMSEQ_BATCH. May be combined with -dnm, -map, -siteQ, -loo, -seg" << std::endl
            << "\t\tand -afTagAll; not with -afTag." << std::endl
            << "-seg MODEL\t(vcf) MODEL dominant, recessive or both, with -affected ID[,ID...] and optionally -unaffected ID[,ID...] (PED IDs):" << std::endl
            << "\t\tadd PSD (dominant: the affected carry the variant, the unaffected do not) and / or PSR (recessive: the affected are" << std::endl
            << "\t\thomozygous for it, the unaffected are not), the posterior probability of that pattern given the whole family's data," << std::endl
            << "\t\tto the INFO column. Implies -method 2; may be combined with -dnm, -map, -siteQ, -loo and -afTagAll; not with -afTag." << std::endl
            << "-afEM T\t\t(vcf) Add FAF, the maximum-likelihood allele frequency among the family's founders after T (0.." << FAMSEQ_MAX_AF_ITER << ") EM steps" << std::endl
            << "\t\tfrom -afStart X (in (0, 1), default 0.5), and FAL, the log10 likelihood ratio of the site's data at that frequency against" << std::endl
            << "\t\t\"no founder carries the allele\" (inf where the data exclude that), to the INFO column. No prior enters either; no other" << std::endl
            << "\t\tfield changes. Implies -method 2; may be combined with -dnm, -map, -siteQ, -loo, -sample, -seg and -afTagAll; not with -afTag." << std::endl
            << "-phase\t\t(vcf) Add PGT, the sample's genotype phased by transmission as maternal|paternal allele (the most probable pair of" << std::endl
            << "\t\talleles received from mother and father given the whole family's data; the maternal allele alone for a son on" << std::endl
            << "\t\tchromosome X; . for a founder), and PGP, that pair's posterior probability, to every sample column. Implies -method 2;" << std::endl
            << "\t\tmay be combined with every other option above, under -afTagAll with the line's prior; not with -afTag." << std::endl
            << "-swapCheck FILE\t(vcf) After the last site write FILE: for every two sequenced samples, in VCF column order, log10_BF, the sum over" << std::endl
            << "\t\tthe file's sites of the log10 likelihood of the site under the pedigree with the two samples exchanged minus that with the" << std::endl
            << "\t\tlabels as given (positive favours the exchange), and sites_impossible, the sites the exchange makes impossible, which the" << std::endl
            << "\t\tsum leaves out; line 1 counts the sites used and skipped (failed) and gives the file's log10 likelihood. Adds nothing to" << std::endl
            << "\t\tany output line. Implies -method 2; may be combined with every other option above, under -afTagAll with the line's prior;" << std::endl
            << "\t\tnot with -afTag." << std::endl
            << "-mRateScan FILE\t(vcf) After the last site write FILE: for every mutation rate of -mRateGrid r1,r2,... (1.." << FAMSEQ_MAX_RATES << " numbers in [0, 1];" << std::endl
            << "\t\tdefault 0,1e-9,1e-8,1e-7,1e-6,1e-5,1e-4,1e-3) log10_lik, the sum over the file's sites of the log10 likelihood of the" << std::endl
            << "\t\tsite under the pedigree at that rate (-inf once one site is impossible at it), delta, that sum minus the one at the run's" << std::endl
            << "\t\town -mRate, and n_impossible, the sites impossible at the rate; the last line names the best rate of the grid, line 1 counts" << std::endl
            << "\t\tthe sites used and skipped (failed). Adds nothing to any output line. Implies -method 2; may be combined with every other" << std::endl
            << "\t\toption above, under -afTagAll with the line's prior; not with -afTag." << std::endl
            << "-segPen MODELS\t(vcf) MODELS F0,F1,F2[/F0,F1,F2...], 1.." << FAMSEQ_MAX_WEIGHTS << " penetrance models (the probability of being affected given 0, 1," << std::endl
            << "\t\t2 alt alleles, numbers in [0, 1]), with -affected ID[,ID...] and optionally -unaffected ID[,ID...] (PED IDs): add PSL, one" << std::endl
            << "\t\tvalue per model, the log10 Bayes factor of the phenotypes: their probability given the whole family's data (phenocopies" << std::endl
            << "\t\tand incomplete penetrance allowed: -seg dominant is the corner 0,1,1) over their probability under the pedigree and the" << std::endl
            << "\t\tfounders' prior alone; -inf where the data rule them out, . where the site failed. With or without -seg. Implies" << std::endl
            << "\t\t-method 2; may be combined with every other option above, under -afTagAll with the line's prior; not with -afTag." << std::endl
            << "-mapQ\t\t(vcf) Add JGQ, the quality of the sample's genotype in the most probable joint configuration of the family (what -map" << std::endl
            << "\t\tprints as JGT): the Phred-scaled ratio between that configuration's posterior and the best configuration's in which the" << std::endl
            << "\t\tsample has another genotype (99999: none has any probability), to every sample column, and JP2, the posterior of the" << std::endl
            << "\t\tsecond most probable configuration, to the INFO column. With or without -map. Implies -method 2; may be combined with" << std::endl
            << "\t\tevery other option above, under -afTagAll with the line's prior; not with -afTag." << std::endl
            << "-countDist KIND\t(vcf) KIND carriers, alleles or homalt, optionally with -countOf ID[,ID...] (PED IDs; default every member): add PCD," << std::endl
            << "\t\tthe exact posterior distribution of the number of members who carry the variant / of alt alleles they hold between" << std::endl
            << "\t\tthem / of hom-alt members, p0,p1,...,pD given the whole family's data, each to 1e-12 absolute (. where the site failed);" << std::endl
            << "\t\tat most " << 2 * FAMSEQ_MAX_CWEIGHTS - 1 << " values. alleles sums the genotype indices as coded: a male's genotype 2 at a chrX site counts 2." << std::endl
            << "\t\tImplies -method 2; may be combined with every other option above, under -afTagAll with the line's prior; not with -afTag." << std::endl
            << "pack\t\tFamSeq pack -vcfFile f -pedFile p -output f.fspl: write the computable sites as packed integer PLs." << std::endl
            << "PL\t\tFamSeq PL -plFile f.fspl -pedFile p -output o [-binOutput]: call variants from a packed PL file" << std::endl
            << "\t\t(-binOutput: write a packed result file instead of text)." << std::endl
            << "unpack\t\tFamSeq unpack -plFile f.fspl -poFile r.fspo -pedFile p -output o: the text of a packed result file." << std::endl
            << "tune\t\tFamSeq tune -vcfFile f -pedFile p: time this pedigree's kernel variants on this GPU once and keep the" << std::endl
            << "\t\tfaster ones' indices in the kernel cache (later runs start from them)." << std::endl
            << "Environment: FAMSEQ_DEVICE (GPU index, default 0), FAMSEQ_BATCH (sites per GPU batch)." << std::endl;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 1) {
    usage_top();
    return -1;
  }
  const string mode(argv[1]);
  if (mode == "-h") {
    help();
    return 0;
  }
  if (mode != "vcf" && mode != "LK" && mode != "pack" && mode != "PL" && mode != "unpack" && mode != "tune") {
    std::cout << "Cannot recognize the input type: \"" << argv[1] << "\"." << std::endl
              << "The input type can only be vcf or LK (or pack / PL / unpack for the packed binary formats, or tune)" << std::endl << std::endl
              << "Type FamSeq -h for help." << std::endl;
    return -1;
  }
  if (argc == 2) {
    std::cout << std::endl << "Usage:\tFamSeq " << mode << " [options]" << std::endl << std::endl
              << "Type FamSeq -h for help." << std::endl;
    return -1;
  }
  Options o;
  o.lk_mode = mode == "LK" || mode == "PL" || mode == "unpack";
  o.pl_mode = mode == "PL" || mode == "unpack";
  o.unpack_mode = mode == "unpack";
  o.pack_mode = mode == "pack";
  o.tune_mode = mode == "tune";
  const int rc = parse_options(argc, argv, o);
  if (rc < 0) return -1;
  if (rc > 0)
    std::cout << "There are some improper parameters in the command line. Some parameters are set to default."
              << std::endl;
  if (o.method == 3) {
    std::cout << "This build implements -method 1 (Bayesian network) and -method 2 (exact sum-product, "
                 "the result of Elston-Stewart peeling); -method 3 (MCMC) is not part of it." << std::endl;
    return -1;
  }
  Ped ped;
  if (!read_ped(o.ped_file, ped)) {
    std::cout << "Cannot read Ped file: " << o.ped_file << "." << std::endl << "Cannot set family." << std::endl;
    return -1;
  }
  for (const SideRow &row : kSide) {  // (outside vcf mode nothing reads the options this switches off)
    if (!row.on(o)) continue;
    if (mode != "vcf") {
      std::cout << row.flag << " applies to vcf mode only; ignored here." << std::endl;
      row.off(o);
      continue;
    }
    if (row.check && !row.check(o, ped)) return -1;
    if (!sum_product_serves(o, ped, row.flag)) return 255;
    if (row.method2) o.method = 2;  // the evidence, leave-one-out and pattern kernels are the sum-product engine's
  }
  if (o.af_conflict) {
    std::cout << "-afTag and -afTagAll cannot be combined: give the INFO key once." << std::endl;
    return -1;
  }
  if (!o.af_tag.empty()) {
    if (mode != "vcf") {
      std::cout << (o.af_all ? "-afTagAll" : "-afTag") << " applies to vcf mode only; ignored here." << std::endl;
      o.af_tag.clear();
    } else if (!o.af_all && any_side(o)) {
      std::cout << "-afTag cannot be combined with -dnm or -map: their kernels use the model's priors, and one output line must not mix two models."
                << std::endl;
      return -1;
    } else if (!sum_product_serves(o, ped, o.af_all ? "-afTagAll" : "-afTag")) {
      return 255;
    } else {
      o.method = 2;  // site priors are served by the sum-product engine
    }
  }
  const double t0 = now_s();
  if (o.tune_mode) return run_tune(o, ped) ? 0 : -1;
  const bool ok = o.pl_mode ? run_pl(o, ped) : (o.lk_mode ? run_lk(o, ped) : run_vcf(o, ped));
  if (std::getenv("FAMSEQ_TIMING")) std::cerr << "FamSeq " << mode << ": " << now_s() - t0 << " s in the driver" << std::endl;
  // Every output file has been closed by its driver.  Leave without the static destructors: unloading the HIP runtime takes
  // about a tenth of a second, which is a tenth of what a three-million-site file takes altogether.
#if defined(__SANITIZE_ADDRESS__)
  return ok ? 0 : -1;  // (the sanitizer build checks for leaks at exit)
#else
  std::cout.flush();
  std::cerr.flush();
  std::fflush(nullptr);
  std::_Exit(ok ? 0 : 255);
#endif
}
