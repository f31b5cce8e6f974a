// elim_codegen.cpp — generates the exact sum-product ("elimination") kernel for one pedigree.
//
// Same marginals as the 3^N enumeration of family::calPostProbBN
// (/root/reference/src/family.cpp:882-954, :990-1120), computed by message passing on the
// pedigree's factor graph instead of visiting every joint genotype:
//   variable nodes = members, factor nodes = nuclear families (mother, father, children) with
//   Phi_F = prod_children T_c[g_c | g_m, g_f]; member-local factors are prior*lk for founders
//   and lk for the others (exactly the indProb terms of family.cpp:899-909).
// On a loop-free pedigree (the domain of the reference's own Elston-Stewart -method 2,
// family.cpp:1126-1403) the factor graph is a forest and two messages per edge give every
// marginal exactly: O(27 N) flops per site instead of 2*3^N, which makes the path HBM-bound.
// A pedigree with loops (consanguinity, marriage loops) is made a forest by conditioning on the
// smallest set of members that cuts every cycle (up to three): their genotypes are enumerated in a
// loop around the message passing, 3^|cut| passes per site (Emitter::conditioned_body).
//
// The kernel is emitted as straight-line HIP for this one topology: every index is a literal,
// so a lane keeps a whole site (likelihoods, messages) in registers; one lane = one site.
// Arithmetic: fp64; sums of products written as explicit FMA chains; the single posterior, the
// shortcut vote and the failure rules are the same statements as in bn_kernel.hip (bit-identical
// to the CPU reference).  One member per connected component carries the reference's 1e7 scale.
#include "elim_codegen.h"

#include <algorithm>
#include <cstdlib>
#include <functional>
#include <map>
#include <numeric>
#include <set>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "kernel_shell.h"

namespace famseq {

namespace {

struct Family {
  int mo, fa;
  std::vector<int> kids;
};

struct Graph {
  int N = 0;
  std::vector<Family> fam;
  std::vector<std::vector<int>> nb;  // member -> adjacent families
  std::vector<int> scaled;           // loop-free pedigrees: one member per connected component carries 1e7
  // Pedigrees with loops: the members of `cut` are conditioned on (their genotypes are enumerated
  // around the message passing), which leaves a forest.  comp[p] = component of the non-cut member p
  // in that forest, rep[c] = one member of component c.
  std::vector<int> cut, comp, rep;
  bool is_cut(int p) const {
    for (int c : cut)
      if (c == p) return true;
    return false;
  }
};

// Union-find pass over the bipartite member/family graph without the members in `cut`.
// Returns false on a cycle.  comp (optional) receives a component id per member (-1 for cut ones).
bool forest_without(const Graph &g, const std::vector<int> &cut, std::vector<int> *comp, std::vector<int> *rep) {
  const int nf = (int)g.fam.size();
  std::vector<int> parent(g.N + nf);
  std::iota(parent.begin(), parent.end(), 0);
  std::function<int(int)> find = [&](int x) { return parent[x] == x ? x : parent[x] = find(parent[x]); };
  auto cutm = [&](int p) {
    for (int c : cut)
      if (c == p) return true;
    return false;
  };
  for (int f = 0; f < nf; ++f) {
    std::vector<int> mem = {g.fam[f].mo, g.fam[f].fa};
    mem.insert(mem.end(), g.fam[f].kids.begin(), g.fam[f].kids.end());
    int live = 0;
    for (int p : mem) {
      if (cutm(p)) continue;
      ++live;
      const int a = find(p), b = find(g.N + f);
      if (a == b) return false;
      parent[a] = b;
    }
    if (!cut.empty() && live == 0) return false;  // a family of conditioned members only: not handled
  }
  if (comp) {
    comp->assign(g.N, -1);
    rep->clear();
    std::map<int, int> id;
    for (int p = 0; p < g.N; ++p) {
      if (cutm(p)) continue;
      const int r = find(p);
      if (!id.count(r)) {
        id[r] = (int)rep->size();
        rep->push_back(p);
      }
      (*comp)[p] = id[r];
    }
  }
  return true;
}

bool build_graph(const Model &m, Graph &g, std::string *why) {
  g.N = m.n_members;
  std::map<std::pair<int, int>, int> idx;
  g.nb.assign(g.N, {});
  for (int i = 0; i < g.N; ++i) {
    if (m.mother[i] < 0) continue;
    const auto key = std::make_pair(m.mother[i], m.father[i]);
    auto it = idx.find(key);
    if (it == idx.end()) {
      it = idx.emplace(key, (int)g.fam.size()).first;
      g.fam.push_back({key.first, key.second, {}});
      if (key.first == key.second) {
        if (why) *why = "a member's mother and father are the same individual";
        return false;
      }
      g.nb[key.first].push_back(it->second);
      g.nb[key.second].push_back(it->second);
    }
    g.fam[it->second].kids.push_back(i);
    g.nb[i].push_back(it->second);
  }
  if (forest_without(g, {}, &g.comp, &g.rep)) {
    g.scaled = g.rep;  // one member per connected component
    return true;
  }
  // A loop (consanguinity, marriage loop): the smallest set of members whose conditioning breaks
  // every cycle, up to three of them (3^|cut| passes of message passing per site).
  for (int size = 1; size <= 3; ++size) {
    std::vector<int> pick(size);
    std::function<bool(int, int)> search = [&](int k, int from) {
      if (k == size) return forest_without(g, pick, &g.comp, &g.rep);
      for (int p = from; p < g.N; ++p) {
        pick[k] = p;
        if (search(k + 1, p + 1)) return true;
      }
      return false;
    };
    if (search(0, 0)) {
      g.cut = pick;
      return true;
    }
  }
  if (why) *why = "the pedigree's loops need more than three conditioning members; use the enumeration engine";
  return false;
}

struct EmitOptions {
  int fences = 0;          // 0 none, 1 after every family->member message, 2 also after local factors and child sums
  bool scalar_t = false;   // transmission entries from tcx[] (uniform pointer: scalar loads) instead of the lane's LDS table
  // where the normalised marginals go — "q" (registers: the shell's compute-first flow), "row" (the lane's LDS row, free
  // once the likelihoods sit in registers: the shell's registers-first flow) or "pg" (global memory: lane_shell)
  const char *out = "q";
  bool lean = false;       // local factors re-formed at each use (see Emitter::loc)
  int lean_from = 1 << 30; // ... for members lean_from and above only (their likelihoods sit in the lane's LDS row: lane_shell)
  // the founders' prior is the site's own — the lane's variables pa_<g> (female founders; every founder off chrX) / pm_<g>
  // (male), see prior_source — instead of the model's rows in tcf[]
  bool site_prior = false;
  // where given: every transmission entry is read from this pointer's block instead (tcx's layout: kind * 27 + 9 gc + 3 gm + gf),
  // whatever scalar_t says — famseq_mutrate's pass-local table
  const char *t_from = nullptr;
};

// fence level f of a kernel's variant (0..3; 3 fences the single posterior too, which is the shell's): what the emitter does
EmitOptions emit_options(int f, const char *out, bool site_prior) {
  EmitOptions o;
  o.fences = std::min(f, 2);
  o.scalar_t = f >= 1;
  o.out = out;
  o.site_prior = site_prior;
  return o;
}

class Emitter {
 public:
  Emitter(const Model &m, const Graph &g, const EmitOptions &o)
      : m_(m), g_(g), fences_(o.fences), out_(o.out), lean_(o.lean), lean_from_(o.lean_from), site_prior_(o.site_prior),
        t_from_(o.t_from ? o.t_from : (o.scalar_t ? "tcx" : "tcf")) {}

  std::string body() {
    if (g_.cut.empty()) {
      for (int p = 0; p < g_.N; ++p) {
        marginal(p);
        normalise(p, "m" + num(p));
      }
      return o_.str();
    }
    return conditioned_body();
  }

  // Pedigree with loops: enumerate the genotypes of the cut members around the message passing.
  // For one assignment a of the cut members every family sees an indicator in their place, the rest
  // is a forest, and with  Z_c = total weight of component c,  L = 1e7 * prod_cut local(a):
  //   member p of component c :  acc[p][g] += m_p[g] * L * prod_{c' != c} Z_c'
  //   cut member k            :  acc[k][a_k] += L * prod_c Z_c
  // (unnormalised marginals: the normalisation happens once, after the last assignment).
  std::string conditioned_body() {
    std::ostringstream decls;
    for (int p = 0; p < g_.N; ++p) decls << "      double acc" << p << "_0 = 0, acc" << p << "_1 = 0, acc" << p << "_2 = 0;\n";
    const std::string loop = cut_loop(decls.str(), /*wc=*/true, /*wall=*/true, [&] {
      for (int p = 0; p < g_.N; ++p) {
        if (g_.is_cut(p)) {
          for (int g = 0; g < 3; ++g) o_ << "      acc" << p << "_" << g << " += a" << p << " == " << g << " ? Wall : 0.0;\n";
          continue;
        }
        marginal(p);
        for (int g = 0; g < 3; ++g)
          o_ << "      acc" << p << "_" << g << " = __builtin_fma(m" << p << "_" << g << ", Wc" << g_.comp[p] << ", acc" << p << "_" << g
             << ");\n";
        fence(1);
      }
    });
    for (int p = 0; p < g_.N; ++p) normalise(p, "acc" + num(p));
    return loop + o_.str();
  }

  // Trio posteriors (famseq_trio): for every child c (a member with parents, PED order) the clique belief of its nuclear
  // family F restricted to (c, mother, father),
  //   b_c(gc, gm, gf) = T_c(gc | gm, gf) * v_c->F(gc) * C(gm, gf),  C = v_mo->F(gm) * v_fa->F(gf) * prod_{other kids k} a_k(gm, gf)
  // (C is fac2var's product for the message F -> c), normalised by its own sum, the total weight of c's component.  `mask`
  // [2][K][27]: the entries where the mutation-free transmission table of the child is 0 (autosomes, chrX); their mass is the
  // de novo posterior.  joint: store the 27 values too.  Loops: accumulated over the cut assignments with the weight of the
  // rest of the network (as conditioned_body does for marginals), normalised once after the last assignment.
  std::string trio_body(const std::vector<int> &kids, const std::vector<std::vector<double>> &mask, bool joint) {
    const int K = (int)kids.size();
    if (g_.cut.empty()) {
      for (int c = 0; c < (int)g_.rep.size(); ++c)  // a component without a family (a lone founder): its weight is its local factor
        if (g_.nb[g_.rep[c]].empty()) {
          const std::string l = loc(g_.rep[c]);
          o_ << "      if (((" << l << "_0 + " << l << "_1) + " << l << "_2) <= 0) bn_fail = true;\n";
        }
      for (int k = 0; k < K; ++k) {
        const std::string b = trio(family_of(kids[k]), kids[k], mask, k);
        trio_out(k, b + "s", b + "A", b + "X", joint ? b + "_" : "");
      }
      return o_.str();
    }
    std::ostringstream decls;
    for (int k = 0; k < K; ++k) {
      decls << "      double tt" << k << " = 0, tA" << k << " = 0, tX" << k << " = 0;\n";
      if (joint) {
        decls << "      double";
        for (int i = 0; i < 27; ++i) decls << (i ? ", " : " ") << "tj" << k << "_" << i << " = 0";
        decls << ";\n";
      }
    }
    const std::string loop = cut_loop(decls.str(), /*wc=*/true, /*wall=*/false, [&] {
      for (int k = 0; k < K; ++k) {
        const int F = family_of(kids[k]);
        const std::string b = trio(F, kids[k], mask, k), W = "Wc" + num(family_comp(F));
        o_ << "      tt" << k << " = __builtin_fma(" << b << "s, " << W << ", tt" << k << ");\n"
           << "      tA" << k << " = __builtin_fma(" << b << "A, " << W << ", tA" << k << ");\n"
           << "      tX" << k << " = __builtin_fma(" << b << "X, " << W << ", tX" << k << ");\n";
        if (joint)
          for (int i = 0; i < 27; ++i)
            o_ << "      tj" << k << "_" << i << " = __builtin_fma(" << b << "_" << i << ", " << W << ", tj" << k << "_" << i << ");\n";
        fence(1);
      }
    });
    for (int k = 0; k < K; ++k) trio_out(k, "tt" + num(k), "tA" + num(k), "tX" + num(k), joint ? "tj" + num(k) + "_" : "");
    return loop + o_.str();
  }

  // Phase by transmission (famseq_origin): for every child c (PED order, as trio_body) the network with c's transmission factor
  // replaced by its allele-level form tm(a | gm) * tf(b | gf), a and b the alleles (0 ref, 1 alt) c received from mother and
  // father and c's genotype gamma(a, b): a + b, at a chrX site 2 a for a son.  With C and x what trio() multiplies (fac2var's
  // product for the message F -> c, and c's own message), per child, every sum in the order written:
  //   p(a, gm, gf) = tm(a | gm) * C(gm, gf)                          M(a, gf) = (p(a, 0, gf) + p(a, 1, gf)) + p(a, 2, gf)
  //   q(a, b, gf)  = tf(b | gf) * M(a, gf)                           O(a, b)  = ((q(a, b, 0) + q(a, b, 1)) + q(a, b, 2)) * x(gamma(a, b))
  //   r(a, b)      = (tf(b | 0) * p(a, 1, 0) + tf(b | 1) * p(a, 1, 1)) + tf(b | 2) * p(a, 1, 2)      [the mother het: M's middle terms]
  //   Hm(a)        = r(a, 0) * x(gamma(a, 0)) + r(a, 1) * x(gamma(a, 1))
  //   Hf(b)        = q(0, b, 1) * x(gamma(0, b)) + q(1, b, 1) * x(gamma(1, b))                        [the father het: O's middle terms]
  // Outputs: origin[2 a + b] = O(a, b) / s, s = ((O(0,0) + O(0,1)) + O(1,0)) + O(1,1), the total weight of c's component, and
  // hettx = (Hm(1), Hm(0), Hf(1), Hf(0)) / s.  Products and sums of non-negative numbers only: a term with a factor of exactly 0
  // is exactly 0.0.  The allele rows are not in the text (a kernel is cached per pedigree, not per rate): alx[], the block of
  // the chrX pass under way of build_allele_tables' table, a wave-uniform pointer, so that an entry arrives by a scalar load.
  // Loops: the eight sums accumulated over the cut assignments with the weight of the rest of the network, normalised once
  // behind the last assignment, as trio_body does.
  std::string origin_body(const std::vector<int> &kids) {
    const int K = (int)kids.size();
    const std::string head = "      const double *alx = al_g + x_ * 24;\n";
    if (g_.cut.empty()) {
      for (int c = 0; c < (int)g_.rep.size(); ++c)  // (a lone founder's component: as trio_body)
        if (g_.nb[g_.rep[c]].empty()) {
          const std::string l = loc(g_.rep[c]);
          o_ << "      if (((" << l << "_0 + " << l << "_1) + " << l << "_2) <= 0) bn_fail = true;\n";
        }
      for (int k = 0; k < K; ++k) {
        const std::string n = origin(family_of(kids[k]), kids[k]);
        origin_out(k, n + "O", n + "H");
      }
      return head + o_.str();
    }
    std::ostringstream decls;
    for (int k = 0; k < K; ++k)
      decls << "      double to" << k << "_0 = 0, to" << k << "_1 = 0, to" << k << "_2 = 0, to" << k << "_3 = 0, th" << k << "_0 = 0, th" << k
            << "_1 = 0, th" << k << "_2 = 0, th" << k << "_3 = 0;\n";
    const std::string loop = cut_loop(decls.str(), /*wc=*/true, /*wall=*/false, [&] {
      for (int k = 0; k < K; ++k) {
        const int F = family_of(kids[k]);
        const std::string n = origin(F, kids[k]), W = "Wc" + num(family_comp(F));
        for (const char *t : {"o", "h"})
          for (int i = 0; i < 4; ++i)
            o_ << "      t" << t << k << "_" << i << " = __builtin_fma(" << n << (t[0] == 'o' ? "O" : "H") << "_" << i << ", " << W << ", t" << t << k
               << "_" << i << ");\n";
        fence(1);
      }
    });
    for (int k = 0; k < K; ++k) origin_out(k, "to" + num(k), "th" + num(k));
    return head + loop + o_.str();
  }

  // The joint MAP configuration (famseq_map): g* = argmax_g w(g) and its posterior w(g*) / Z, by message passing under two
  // semirings on the same graph.  One root per component (g_.rep); only the messages that point towards a root are formed.
  //   sum pass  Z = prod_c sum_g m_root(g): marginal(root), the code every other form uses.
  //   max pass  (mx_: the same three message kinds, their names prefixed "x", + / fma replaced by max) keeps an arg-max beside
  //             every maximum, packed into 32-bit words: a child summary nine 2-bit entries (the child's genotype for each
  //             (gm, gf)), a family -> parent message three 2-bit entries (the other parent's), a family -> child message three
  //             4-bit entries (3 gm + gf).
  //   back-track from each root outwards through the families in reverse message order (steps_): shifts of the packed words
  //             by run-time genotypes, never an indexed array.
  // Tie rule: every arg-max scans 0, 1, 2 (parent pairs in the order 3 gm + gf) and replaces on strictly greater only, so
  // among values this arithmetic holds equal the lowest wins.  Loops: per assignment of the cut members (first in loop order
  // wins ties) W = Lam * prod_c max_c against the best so far, the back-track under that branch (a few dozen integer
  // instructions; a second run of the body for the best assignment would cost a whole pass); Z accumulates Lam * prod_c Z_c.
  // Leaves: Z_, W_ (doubles) and the genotypes packed four members to a word in gw<k> (set only where the shell keeps them).
  std::string map_body() {
    if (g_.cut.empty()) {
      component_sums();
      map_assignment(false);
      return o_.str();
    }
    return cut_loop("      double Zt_ = 0, Wb_ = 0;\n", /*wc=*/false, /*wall=*/false, [&] { map_assignment(true); }) +
           "      const double Z_ = Zt_, W_ = Wb_;\n";
  }

  // The evidence (famseq_evidence): Z = sum_g w(g), the sum pass of map_body alone, and W0 = w(0, ..., 0), the weight of the
  // configuration in which every member is hom-ref: one product of the members' factors in PED order, formed once per site,
  // outside the cut loop.  Where the likelihoods sit in registers it stands in front of the message passing, where every one
  // of them has just been read (two registers from there on); where they are read from the lane's row at each use (lean) it
  // stands behind it, where nothing else is alive while its N loads are in flight (in front, the 64-member kernel spilled
  // 200 B per lane).  Both carry the scale Z carries: 1e7 per connected component of a loop-free pedigree (the members of
  // g_.scaled), one 1e7 under conditioning (Lam); evidence_scale_digits() says how many decimal digits that is.
  // Leaves: Z_, W0_.
  std::string evidence_body() {
    std::string w0;
    for (int c = 0; c < evidence_scale_digits() / 7; ++c) w0 = w0.empty() ? "10000000.0" : "(" + w0 + " * 10000000.0)";
    for (int p = 0; p < g_.N; ++p)
      w0 = "(" + w0 + " * " + (m_.mother[p] < 0 ? unscaled_loc(p, 0) : "(" + T(p, 0, 0, 0) + " * " + unscaled_loc(p, 0) + ")") + ")";
    w0 = "      const double W0_ = " + w0 + ";\n";
    const std::string front = lean_ ? "" : w0, back = lean_ ? w0 : "";
    if (g_.cut.empty()) {
      o_ << front;
      fence(1);
      component_sums();
      o_ << "      const double Z_ = " << times_sums("") << ";\n";
      fence(1);
      return o_.str() + back;
    }
    return front + cut_loop("      double Zt_ = 0;\n", /*wc=*/false, /*wall=*/true, [&] { o_ << "      Zt_ = Zt_ + Wall;\n"; fence(1); }) +
           "      const double Z_ = Zt_;\n" + back;
  }
  // the decimal digits of scale in evidence_body's Z_ and W0_
  int evidence_scale_digits() const { return 7 * (g_.cut.empty() ? (int)g_.scaled.size() : 1); }

  // ---- The per-pass products (famseq_pattern, famseq_relabel, famseq_mutrate, famseq_weight): the sum pass of evidence_body run
  // count + 1 times on one read of the site's rows — pass 0 on the network as it is, pass k >= 1 on what row k - 1 of the
  // product's table makes of it.  What they share is written here once:
  //   - the loop is `#pragma unroll 1`: the pass's text stands once whatever the count is;
  //   - per pass: Zp_, the pass's total weight (scaled as evidence_body's Z_: evidence_scale_digits()), then `per_pass`
  //     (pass_product(): pass 0 keeps the evidence, a later pass stores its result);
  //   - only pass 0's Z that is not a positive finite number fails the site: per_pass breaks out of the loop there.
  // `before` stands in front of the loop and `inside` in front of the pass: what the product does to the network, which is all
  // that pattern_body, relabel_body, mutrate_body and weight_body write.  `counter` is the loop's variable (part of the text).
  std::string pass_loop(const std::string &before, const std::string &inside, const std::string &counter, const std::string &per_pass) {
    return before + "#pragma unroll 1\n      for (int " + counter + " = 0; " + counter + " <= last_; ++" + counter + ") {\n" + inside + sum_pass() +
           per_pass + "      }\n";
  }
  // A pass that takes the members' rows changed, entry by entry (pattern_body, weight_body), the change made where the names
  // l<p>_<g> are resolved, before loc() sees them, so the founders' priors, the site's own prior rows, the male chrX row and a
  // cut member's lam all follow unchanged.  Where the likelihoods sit in registers they are copied in front of the loop
  // (r<p>_<g>: the shell's l<p>_<g> under another name) and a pass's changed values shadow the shell's names; in the lean form
  // the names are macros and are defined again, the row read afresh at each use (v_) and changed there.  value(p, g, row) gives
  // the statements in front of entry g of member p, if any, and the entry as an expression of `row` (r<p>_<g> or v_).
  using RowValue = std::function<std::pair<std::string, std::string>(int p, int g, const std::string &row)>;
  void changed_rows(std::ostream &before, std::ostream &inside, const RowValue &value) {
    for (int p = 0; p < g_.N; ++p) {
      if (!lean_) before << "      const double r" << p << "_0 = l" << p << "_0, r" << p << "_1 = l" << p << "_1, r" << p << "_2 = l" << p << "_2;\n";
      for (int g = 0; g < 3; ++g) {
        const std::string l = "l" + num(p) + "_" + num(g);
        const auto [pre, v] = value(p, g, lean_ ? "v_" : "r" + num(p) + "_" + num(g));
        if (lean_)
          before << "#undef " << l << "\n#define " << l << " __extension__ ({ const double v_ = lgv[" << 3 * p + g << "]; " << pre << v << "; })\n";
        else
          inside << pre << "      const double " << l << " = " << v << ";\n";
      }
    }
  }

  // Genotype-pattern posteriors (famseq_pattern): pass m = 1 .. n_patterns takes member p's entry g as
  // (mask[m - 1][p] >> g) & 1 ? l_g : 0.0 — a select, no multiplication, no rounding (changed_rows).  The masks are
  // wave-uniform: the shell packs them into LDS words once per workgroup (s_mw: four bits per member, eight members per word,
  // row 0 all ones), and a pass reads its NMW words into scalar registers.
  std::string pattern_body(const std::string &counter, const std::string &per_pass) {
    const int nmw = (g_.N + 7) / 8;
    std::ostringstream before, inside;
    for (int k = 0; k < nmw; ++k)
      inside << "      const unsigned mw" << k << " = __builtin_amdgcn_readfirstlane(s_mw[" << counter << " * " << nmw << " + " << k << "]);\n";
    changed_rows(before, inside, [&](int p, int g, const std::string &row) {
      return std::make_pair(std::string(), "(mw" + num(p / 8) + " >> " + num(4 * (p % 8) + g) + ") & 1u ? " + row + " : 0.0");
    });
    return pass_loop(before.str(), inside.str(), counter, per_pass);
  }

  // Relabelling evidence (famseq_relabel): pass j gives member p the likelihood row that row j of the assignment table names
  // (pass 0: the identity).  The substitution is made where the names l<p>_<g> are resolved, before loc() sees them, so the
  // founders' priors, the site's own prior rows, the male chrX row and a cut member's lam all follow unchanged.  The table is
  // wave-uniform: the shell packs it into LDS words once per workgroup (s_aw: `bits` bits per member, row 0 the identity, "no
  // data" and every entry outside 0 .. N-1 stored as N), and a pass reads its words into scalar registers; e<p> = 3 * entry is
  // scalar arithmetic.  The names are macros in both forms and are defined again here:
  //   rows in LDS (lds_rows)  the lane's row holds N + 1 triples, the last (1, 1, 1): member p's entry g is lrow[e<p> + g], and
  //                           "no data" is an index like any other;
  //   lean                    read from the site's row in global memory at each use, at the entry clamped into the row (N reads
  //                           member 0's), a select putting 1.0 in the place of what was read.
  std::string relabel_body(const std::string &counter, const std::string &per_pass, bool lds_rows, int bits) {
    const int per = 32 / bits, naw = (g_.N + per - 1) / per;
    std::ostringstream before, inside;
    for (int p = 0; p < g_.N; ++p)
      for (int g = 0; g < 3; ++g) {
        before << "#undef l" << p << "_" << g << "\n#define l" << p << "_" << g;
        if (lds_rows) before << " lrow[e" << p << " + " << g << "]\n";
        else before << " __extension__ ({ const double v_ = lgv[e" << p << " + " << g << "]; o" << p << " ? 1.0 : v_; })\n";
      }
    for (int k = 0; k < naw; ++k)
      inside << "      const unsigned aw" << k << " = __builtin_amdgcn_readfirstlane(s_aw[" << counter << " * " << naw << " + " << k << "]);\n";
    for (int p = 0; p < g_.N; ++p) {
      const std::string entry = "(int)((aw" + num(p / per) + " >> " + num(bits * (p % per)) + ") & " + num((1 << bits) - 1) + "u)";
      if (lds_rows) inside << "      const int e" << p << " = 3 * " << entry << ";\n";
      else
        inside << "      const int n" << p << " = " << entry << ";\n      const bool o" << p << " = n" << p << " >= " << g_.N << ";\n"
               << "      const int e" << p << " = o" << p << " ? 0 : 3 * n" << p << ";\n";
    }
    return pass_loop(before.str(), inside.str(), counter, per_pass);
  }

  // The mutation-rate likelihood profile (famseq_mutrate): pass 0 with the transmission entries of the context's own table
  // (tc_g), pass r + 1 with those of block r of rt_g (build_factor_tables' layout, 432 doubles a block).  Every T() of the pass
  // reads trt[] (EmitOptions::t_from), which the pass sets in front; the founders' priors (tcf[], or the site's own rows), the
  // rows and a cut member's lam are the operands they are in evidence_body, so a pass is that body's statements on another table.
  // trt is wave-uniform in every variant (the pass number through readfirstlane, x_ the chrX loop's, which the fence-free
  // variant takes as well here): the entries arrive by scalar loads, as tcx's do, and cost neither a VGPR nor a vector-memory
  // instruction per use, which a table addressed by the lane's flags would.
  std::string mutrate_body(const std::string &counter, const std::string &per_pass) {
    return pass_loop("",
                     "      const int pu_ = __builtin_amdgcn_readfirstlane(" + counter + ");\n"
                     "      const double *trt = (pu_ == 0 ? tc_g : rt_g + (long)(pu_ - 1) * RTD) + x_ * 216;\n",
                     counter, per_pass);
  }

  // Per-member genotype weights (famseq_weight): pass m = 1 .. n_weights takes member p's entry g as
  // r<p>_<g> * wt[(m - 1) * 3 N + 3 p + g] — one rounded multiplication (changed_rows; lean: row and weight read afresh at each
  // use and multiplied there) — and the pass is evidence_body's statements on the rows lk * w formed in double.  Every member has
  // a weight, sequenced or not (a phenotype needs no reads): an unsequenced member's row is the one the shell supplies.
  // The weights are read where they lie, through wtp, a wave-uniform pointer (the pass number through readfirstlane, member
  // and genotype constants of the text), as mutrate_body reads trt: they arrive by scalar loads and cost neither a VGPR nor a
  // vector-memory instruction per use; (32 + 1) * 3 N doubles would not fit the LDS beside the tables of the wide pedigrees.
  // Pass 0 multiplies by 1.0, which changes no bit of a row (x * 1.0 is x for every double), so the text is the same in every
  // pass; its wtp points at the batch's first likelihood row — 3 N readable doubles whatever the call gave as its table, whose
  // values the select drops — so that wt_g is not read by a call that wants no weighted pass.
  std::string weight_body(const std::string &counter, const std::string &per_pass) {
    std::ostringstream before, inside;
    inside << "      const int pu_ = __builtin_amdgcn_readfirstlane(" << counter << ");\n"
           << "      const double *wtp = pu_ == 0 ? lk_g : wt_g + (long)(pu_ - 1) * W3;\n";
    changed_rows(before, inside, [&](int p, int g, const std::string &row) {
      const std::string at = "wtp[" + num(3 * p + g) + "]", w = lean_ ? "w_" : "wg" + num(p) + "_" + num(g);
      return std::make_pair(lean_ ? "const double w_ = " + at + "; " : "      const double " + w + " = " + at + ";\n",
                            row + " * (pu_ == 0 ? 1.0 : " + w + ")");
    });
    return pass_loop(before.str(), inside.str(), counter, per_pass);
  }

  // Exact count distributions (famseq_charfn): the sum pass over complex per-member weights.  Pass 0 is the real sum pass on the
  // rows as they are (sum_pass(): Zp_, then `pass0`), in a scope of its own in front of the loop; passes 1 .. last_ are one
  // `#pragma unroll 1` loop around the complex pass (complex_pass(): Zp_r / Zp_i, then `per_pass`), entered only where pass 0
  // did not fail the site.  Pass m takes member p's entry g as the pair (l * w_re, l * w_im), w = cw[m - 1][p][g] — two rounded
  // multiplications, formed where the member's local factor is (in registers under the lean threshold, at each use from it on).
  // The table is read where it lies, through cwp, a wave-uniform pointer (the pass number through readfirstlane, member,
  // genotype and part constants of the text), as weight_body reads wtp: the entries arrive by scalar loads.
  std::string charfn_body(const std::string &counter, const std::string &pass0, const std::string &per_pass) {
    const std::string first = "      {\n" + sum_pass() + pass0 + "      }\n";
    return first + "      if (!bn_fail) {\n#pragma unroll 1\n      for (int " + counter + " = 1; " + counter + " <= last_; ++" + counter + ") {\n" +
           "      const int pu_ = __builtin_amdgcn_readfirstlane(" + counter + ");\n"
           "      const double *cwp = cw_g + (long)(pu_ - 1) * CW6;\n" +
           complex_pass() + per_pass + "      }\n      }\n";
  }

  // The founders' allele frequency by maximum likelihood (famseq_af): EM on q, every step one sum pass and the founders' marginals
  // under the Hardy-Weinberg rows of the step's q, all steps on one read of the site's rows.  The loop is `#pragma unroll 1`
  // over it_ = -1 .. n_it_ and its text stands once whatever n_it_ is: pass -1 runs at q = 0 (the rows (1, 0, 0) exactly) and keeps
  // only its total weight, pass t = 0 .. n_it_ runs at q_t, and every pass but the first and the last takes the update
  //   q' = min(sum_founders count_f / C, 1),  count_f = (m_f1 + 2 m_f2) / (m_f0 + m_f1 + m_f2)  [a male founder at a chrX site:
  //   m_f2 / (m_f0 + m_f1 + m_f2)],  C = 2 founders  [chrX: 2 female founders + male founders],  founders in PED order.
  // A pass forms its rows pa_<g> / pm_<g> from its q with famseq_hwe_priors' expressions, shadowing the shell's (which hold
  // the start value's rows, for the single posterior's failure rule); founder_prior(), loc() and a cut member's lam follow.  Its
  // total weight is evidence_body's: the same statements, so that a call without steps has famseq_evidence_prior's bits.  The
  // founders' marginals are marginal(p)'s; under conditioning they are accumulated over the cut assignments with the weight of
  // the rest of the network, as conditioned_body does (a cut founder adds Wall at its assigned genotype).  They stand behind a
  // wave-uniform branch (upd_), so the two passes that need the total weight alone form the messages towards the roots only.
  // Reads qs_ (the start value), n_it_, xs_ (the site is on chrX); sets bn_fail where a pass's total weight or a founder's row
  // sum is not a positive finite number.  Leaves q_ (after n_it_ steps), Zq_ = Z(q_) and Z0_ = Z(0), scaled as evidence_body's Z_.
  std::string af_body() {
    std::vector<int> founders;
    int n_female = 0, n_male = 0;
    for (int p = 0; p < g_.N; ++p)
      if (m_.mother[p] < 0) {
        founders.push_back(p);
        ++(kind(p) == 0 ? n_male : n_female);
      }
    const char *finite = " <= 1.79769313486231570815e308";
    std::ostringstream head;
    head << "      double q_ = qs_, Z0_ = 0, Zq_ = 0;\n"
         << "#pragma unroll 1\n      for (int it_ = -1; it_ <= n_it_; ++it_) {\n"
         << "      const bool upd_ = it_ >= 0 && it_ < n_it_;\n"
         << "      const double qp_ = it_ < 0 ? 0.0 : q_, pp_ = 1 - qp_;\n"
         << "      const double pa_0 = pp_ * pp_, pa_1 = 2 * qp_ * pp_, pa_2 = qp_ * qp_;\n"
         << "      const double pm_0 = xs_ ? pp_ : pa_0, pm_1 = xs_ ? 0.0 : pa_1, pm_2 = xs_ ? qp_ : pa_2;\n";
    // the step: from the founders' rows `row`<p>_<g>, in PED order
    auto update = [&](const std::string &row) {
      std::ostringstream u;
      u << "      double A_ = 0;\n";
      for (int p : founders) {
        const std::string r = row + num(p);
        const std::string both = "(" + r + "_1 + 2 * " + r + "_2)";
        u << "      { const double s = (" << r << "_0 + " << r << "_1) + " << r << "_2; if (!(s > 0 && s" << finite << ")) bn_fail = true;\n"
          << "        A_ = A_ + " << (kind(p) == 0 ? "(xs_ ? " + r + "_2 : " + both + ")" : both) << " / s; }\n";
      }
      u << "      const double qn_ = A_ / (xs_ ? " << 2 * n_female + n_male << ".0 : " << 2 * (n_female + n_male) << ".0);\n"
        << "      q_ = qn_ < 1.0 ? qn_ : 1.0;\n";
      return u.str();
    };
    const std::string keep =
        "      if (it_ < 0) Z0_ = Zp_;\n"
        "      else {\n"
        "        if (!(Zp_ > 0 && Zp_" + std::string(finite) + ")) { bn_fail = true; break; }\n"
        "        Zq_ = Zp_;\n"
        "      }\n";
    std::string pass;
    if (g_.cut.empty()) {
      fence(1);
      component_sums();
      o_ << "      const double Zp_ = " << times_sums("") << ";\n";
      fence(1);
      o_ << keep << "      if (upd_) {\n";
      for (int p : founders) marginal(p);
      o_ << update("m") << "      }\n";
      pass = o_.str();
    } else {
      std::ostringstream decls;
      decls << "      double Zt_ = 0;\n";
      for (int p : founders) decls << "      double acc" << p << "_0 = 0, acc" << p << "_1 = 0, acc" << p << "_2 = 0;\n";
      pass = cut_loop(decls.str(), /*wc=*/true, /*wall=*/true, [&] {
               o_ << "      Zt_ = Zt_ + Wall;\n";
               fence(1);
               o_ << "      if (upd_) {\n";
               for (int p : founders) {
                 if (g_.is_cut(p)) {
                   for (int g = 0; g < 3; ++g) o_ << "      acc" << p << "_" << g << " += a" << p << " == " << g << " ? Wall : 0.0;\n";
                   continue;
                 }
                 marginal(p);
                 for (int g = 0; g < 3; ++g)
                   o_ << "      acc" << p << "_" << g << " = __builtin_fma(m" << p << "_" << g << ", Wc" << g_.comp[p] << ", acc" << p << "_" << g
                      << ");\n";
                 fence(1);
               }
               o_ << "      }\n";
             }) +
             "      const double Zp_ = Zt_;\n" + keep + "      if (upd_) {\n" + update("acc") + "      }\n";
    }
    return head.str() + pass + "      }\n";
  }

  // Leave-one-out (famseq_loo): for every member p its cavity row k<p>_g, the product of everything the network says of g_p but
  // p's own likelihood: the founder's prior (a child has none) times the message of every adjacent family.  Member p's
  // marginal is c<p>_g * prod of the same messages; here the likelihood is left out of the product, never divided out of it
  // (rows hold exact zeros, where the cavity is finite and positive).  Outputs: loo = k / sum_g k and fit = sum_g k_g l_g /
  // sum_g k_g = Z / Z_-p.  The reference's 1e7: the prior of a g_.scaled member is taken without it, the messages that reach
  // the component's other members carry it (through c<scaled>), under conditioning Lam carries it: it stays where the
  // messages have it and cancels in both outputs, each being a ratio of two sums of one row.
  // Loops: accumulated over the assignments of the cut members, with the weight of the rest of the network, as
  // conditioned_body does for marginals.  A cut member k adds, at its assigned genotype, the weight of the assignment
  // without its own likelihood: Wall's product formed with lam<k> replaced by its prior part (1 for a child).
  std::string loo_body() {
    if (g_.cut.empty()) {
      for (int p = 0; p < g_.N; ++p) loo_out(p, cavity(p));
      return o_.str();
    }
    std::ostringstream decls;
    for (int p = 0; p < g_.N; ++p) decls << "      double acc" << p << "_0 = 0, acc" << p << "_1 = 0, acc" << p << "_2 = 0;\n";
    const std::string loop = cut_loop(decls.str(), /*wc=*/true, /*wall=*/false, [&] {
      for (int p = 0; p < g_.N; ++p) {
        if (g_.is_cut(p)) {
          std::string w = "10000000.0";
          for (int k : g_.cut) {
            if (k != p) {
              w = "(" + w + " * lam" + num(k) + ")";
            } else if (m_.mother[p] < 0) {
              o_ << "      const double pri" << p << " = a" << p << " == 0 ? " << founder_prior(p, 0) << " : (a" << p << " == 1 ? "
                 << founder_prior(p, 1) << " : " << founder_prior(p, 2) << ");\n";
              w = "(" + w + " * pri" + num(p) + ")";
            }
          }
          o_ << "      const double wx" << p << " = " << times_sums(w) << ";\n";
          for (int g = 0; g < 3; ++g) o_ << "      acc" << p << "_" << g << " += a" << p << " == " << g << " ? wx" << p << " : 0.0;\n";
          continue;
        }
        const std::string k = cavity(p);
        for (int g = 0; g < 3; ++g)
          o_ << "      acc" << p << "_" << g << " = __builtin_fma(" << k << "_" << g << ", Wc" << g_.comp[p] << ", acc" << p << "_" << g
             << ");\n";
        fence(1);
      }
    });
    for (int p = 0; p < g_.N; ++p) loo_out(p, "acc" + num(p));
    return loop + o_.str();
  }

  // Max-marginals (famseq_maxmarg): for every member p and genotype a, M[p][a] = max over the configurations g with g_p = a of
  // w(g) — marginal(p) in the (max, x) semiring: every family -> member message of the max pass, both directions, and no
  // back-pointer (bp_ off: a message is a plain maximum, v_max_f64; on non-negative finite numbers that is the value arg_max's
  // strict-greater compare-select keeps).  With xm<p>_g = loc(p) * prod_F xf<F>v<p>_g and Xc<c> the maximum of component c (the
  // row maximum of its root, as map_assignment forms it), member p of component c has the row xm<p>_g * prod_{c' != c} Xc<c'>.
  // Z_ and W_ are map_body's own expressions — the sum pass towards the roots (its sums pinned where they are formed: pin_sums),
  // the roots' maxima multiplied left to right — so that W_ / Z_ has famseq_map's bits; a row's maximum equals W_ to rounding only (another order of multiplication).
  // The runner-up: every configuration but the best differs from it at some member, so the second-largest weight is the largest
  // row entry beside the rows' arg-maxes (scanned 0, 1, 2, replaced on strictly greater); under exact ties it equals W_.
  // Loops: inside the cut loop.  Accumulators start at 0; per assignment a member p that is not cut takes acc<p>_g =
  // max(acc<p>_g, xm<p>_g * (Lam * prod_{c' != c} Xc<c'>)), a cut member k acc<k>_{a_k} = max(acc<k>_{a_k}, Lam * prod_c Xc<c>);
  // Zt_ and Wb_ accumulate as in map_body.  An entry without a supporting configuration of positive weight is a product with a
  // factor of exactly 0 in every assignment: exactly 0.0.
  // Each row is stored as it is formed, divided by Z_ (a true division, map_post's arithmetic): 3 doubles per message alive in
  // both directions, the live set of loo_body.  Sets mm_w / mm_n (W_ / Z_, the runner-up / Z_) and bn_fail.
  std::string maxmarg_body() {
    const char *ok = "      if (!(Z_ > 0 && Z_ <= 1.79769313486231570815e308) || !(W_ > 0)) bn_fail = true;\n";
    bp_ = false;
    if (g_.cut.empty()) {
      component_sums();
      pin_sums();
      max_roots();
      o_ << "      const double Z_ = " << times_sums("", -1, "Zs") << ", W_ = " << times_sums("", -1, "Xc") << ";\n" << ok << "      double nx_ = 0;\n";
      fence(1);
      for (int p = 0; p < g_.N; ++p) {
        const std::string rest = times_sums("", g_.comp[p], "Xc");
        std::string row = max_marginal(p);
        if (!rest.empty()) {
          o_ << "      const double xo" << p << " = " << rest << ";\n";
          for (int g = 0; g < 3; ++g) o_ << "      const double xr" << p << "_" << g << " = " << row << "_" << g << " * xo" << p << ";\n";
          row = "xr" + num(p);
        }
        maxmarg_out(p, row);
      }
      o_ << "      mm_w = W_ / Z_; mm_n = nx_ / Z_;\n";
      return o_.str();
    }
    std::ostringstream decls;
    decls << "      double Zt_ = 0, Wb_ = 0;\n";
    for (int p = 0; p < g_.N; ++p) decls << "      double acc" << p << "_0 = 0, acc" << p << "_1 = 0, acc" << p << "_2 = 0;\n";
    const std::string loop = cut_loop(decls.str(), /*wc=*/false, /*wall=*/false, [&] {
      pin_sums();
      max_roots();
      o_ << "      Zt_ = Zt_ + " << times_sums("Lam", -1, "Zs") << ";\n      const double Wa_ = " << times_sums("Lam", -1, "Xc") << ";\n"
         << "      if (Wa_ > Wb_) Wb_ = Wa_;\n";
      fence(1);
      for (int p = 0; p < g_.N; ++p) {
        if (g_.is_cut(p)) {
          for (int g = 0; g < 3; ++g)
            o_ << "      acc" << p << "_" << g << " = a" << p << " == " << g << " ? __builtin_fmax(acc" << p << "_" << g << ", Wa_) : acc" << p << "_" << g
               << ";\n";
          continue;
        }
        const std::string row = max_marginal(p);
        o_ << "      const double xo" << p << " = " << times_sums("Lam", g_.comp[p], "Xc") << ";\n";
        for (int g = 0; g < 3; ++g)
          o_ << "      acc" << p << "_" << g << " = __builtin_fmax(acc" << p << "_" << g << ", " << row << "_" << g << " * xo" << p << ");\n";
        fence(1);
      }
    });
    o_ << "      const double Z_ = Zt_, W_ = Wb_;\n" << ok << "      double nx_ = 0;\n";
    for (int p = 0; p < g_.N; ++p) maxmarg_out(p, "acc" + num(p));
    o_ << "      mm_w = W_ / Z_; mm_n = nx_ / Z_;\n";
    return loop + o_.str();
  }

  // Exact joint posterior draws (famseq_sample): nd_ configurations per site, each drawn with probability w(g) / Z, by the walk
  // map_body's back-track takes with a weighted random choice in the place of every arg-max (forward filtering, backward sampling).
  //   collect   map_body's sum pass: component_sums(), one root per component, only the messages that point towards a root.
  //   rows      the member -> family messages of that pass (three doubles per member that is not a root) go to the lane's LDS row
  //             sv[], where a run-time genotype indexes them (what the compiler makes of the row: sample_source).
  //   walk      per draw: each root from its marginal, then the families in reverse message order (sum_steps_).  Given a parent the
  //             other parent from v_other(g') prod_k a_k(g, g'); given a child the parent pair from the nine terms
  //             T(g | gm, gf) v_mo(gm) v_fa(gf) prod_k a_k(gm, gf) in the order 3 gm + gf; each remaining child from
  //             T(gc | gm, gf) v_c(gc).  The child summaries a_k at the genotypes at hand are formed again (three FMAs, the operands
  //             read from LDS), never kept.
  //   decision  fs_pick3 / fs_pick9: s the terms' sum left to right, t = u s, the first i with t < e_0 + ... + e_i, else the last
  //             i with e_i > 0: products, sums and compares only.  A term of exactly 0 is never taken.
  //   words     decision d of a draw, in emitted order, takes word d of the draw's Philox stream: element d % 4 of block d / 4
  //             (counter (site, site >> 32, draw, block), key the seed's halves); u = (word + 0.5) 2^-32.
  //   weight    the drawn configuration's w(g): the product of the members' factors at the drawn genotypes, scaled as Z is.
  // Loops: inside the cut loop.  Assignment as_ of weight Wall: Zt_ += Wall, then draw k takes it where u(k, as_) Zt_ < Wall (the
  // first of positive weight always, one of weight 0 never: streaming weighted selection; u(k, as_) is word D + as_ of the draw's
  // stream, D the decisions of a draw) and runs the walk under that branch with the cut members at their assigned genotypes,
  // overwriting its row and its weight in the outputs; the weights are divided by the final Zt_ behind the loop.
  // Reads nd_, sp_ (the site's samp_post row or null), gg (its samp_gt rows or null), ilo_ / ihi_ / key0_ / key1_; sets bn_fail.
  std::string sample_body() {
    const bool loops = !g_.cut.empty();
    if (!loops) {
      component_sums();
      o_ << "      const double Z_ = " << times_sums("") << ";\n";
      fence(1);
      o_ << "      if (!(Z_ > 0 && Z_ <= 1.79769313486231570815e308)) bn_fail = true;\n      else {\n";
      sample_draws(false);
      o_ << "      }\n";
      return o_.str();
    }
    return cut_loop("      double Zt_ = 0;\n", /*wc=*/false, /*wall=*/true, [&] {
             o_ << "      Zt_ = Zt_ + Wall;\n";
             fence(1);
             o_ << "      if (Wall > 0 && Wall <= 1.79769313486231570815e308) {\n";
             sample_draws(true);
             o_ << "      }\n";
           }) +
           "      if (!(Zt_ > 0 && Zt_ <= 1.79769313486231570815e308)) bn_fail = true;\n"
           "      else if (sp_) {\n#pragma unroll 1\n        for (int k_ = 0; k_ < nd_; ++k_) sp_[k_] = sp_[k_] / Zt_;\n      }\n";
  }
  int sample_row_doubles() const { return 3 * (int)sv_at_.size(); }  // of the lane's LDS row (sample_body)
  int sample_decisions() const { return n_dec_; }                    // D: the decision words of a draw

 private:
  // member p's message to family F at the run-time genotype `g`: from the lane's row, or a cut member's indicator
  std::string sv(int p, int F, const std::string &g) {
    if (g_.is_cut(p)) return "(a" + num(p) + " == (int)(" + g + ") ? 1.0 : 0.0)";
    const std::string key = "v" + num(p) + "f" + num(F);
    if (!sv_at_.count(key)) {
      const int at = 3 * (int)sv_at_.size();
      sv_at_[key] = at;
    }
    return "sv[" + num(sv_at_[key]) + " + " + g + "]";
  }
  // transmission entry of child c at run-time genotypes (the lane's table in LDS)
  std::string Tr(int c, const std::string &gc, const std::string &gm, const std::string &gf) const {
    return "tcf[" + num(kind(c) * 27) + " + 9 * " + gc + " + 3 * " + gm + " + " + gf + "]";
  }
  // member p's likelihood and founder p's prior at the run-time genotype G<p>
  std::string lk_at(int p) const {
    const std::string G = "G" + num(p);
    if (lean_ || p >= lean_from_) return "lgv[" + num(3 * p) + " + " + G + "]";
    return "(" + G + " == 0 ? l" + num(p) + "_0 : (" + G + " == 1 ? l" + num(p) + "_1 : l" + num(p) + "_2))";
  }
  std::string prior_at(int p) const {
    const std::string G = "G" + num(p);
    if (!site_prior_) return "tcf[" + num(kind(p) * 27) + " + 9 * " + G + "]";
    const std::string r = kind(p) == 0 ? "pm_" : "pa_";
    return "(" + G + " == 0 ? " + r + "0 : (" + G + " == 1 ? " + r + "1 : " + r + "2))";
  }

  // sample_body's draw loop for the pedigree as it is, or (loops) for one assignment of the cut members
  void sample_draws(bool loops) {
    std::ostringstream w;  // one draw's walk
    int D = 0;
    auto next_u = [&]() {
      const int d = D++;
      if (d % 4 == 0) w << "          fs_philox4x32_10(ilo_, ihi_, (unsigned)k_, " << d / 4 << "u, key0_, key1_, rw_);\n";
      return "FS_U01(rw_[" + num(d % 4) + "])";
    };
    w << "          unsigned rw_[4];\n          unsigned";
    for (int p = 0; p < g_.N; ++p) w << (p ? ", " : " ") << "G" << p << " = " << (g_.is_cut(p) ? "(unsigned)a" + num(p) : std::string("0"));
    w << ";\n";
    for (size_t c = 0; c < g_.rep.size(); ++c) {
      const int r = g_.rep[c];
      const std::string u = next_u();
      w << "          G" << r << " = fs_pick3(" << u << ", m" << r << "_0, m" << r << "_1, m" << r << "_2);\n";
    }
    for (size_t i = sum_steps_.size(); i-- > 0;) {
      const int F = sum_steps_[i].F, t = sum_steps_[i].t;
      const Family &fam = g_.fam[F];
      const std::string gm = "G" + num(fam.mo), gf = "G" + num(fam.fa);
      std::vector<int> kids;
      for (int c : fam.kids)
        if (c != t) kids.push_back(c);
      w << "          {\n";
      for (int c : kids)
        w << "            const double x" << c << "_0 = " << sv(c, F, "0") << ", x" << c << "_1 = " << sv(c, F, "1") << ", x" << c
          << "_2 = " << sv(c, F, "2") << ";\n";
      // the other children's summaries at (a, b), multiplied on to `e` left to right
      auto with_sums = [&](std::string e, const std::string &a, const std::string &b) {
        for (int c : kids)
          e = "(" + e + " * __builtin_fma(" + Tr(c, "2", a, b) + ", x" + num(c) + "_2, __builtin_fma(" + Tr(c, "1", a, b) + ", x" + num(c) +
              "_1, " + Tr(c, "0", a, b) + " * x" + num(c) + "_0)))";
        return e;
      };
      if (t == fam.mo || t == fam.fa) {
        const int other = t == fam.mo ? fam.fa : fam.mo;
        if (!g_.is_cut(other)) {
          const std::string u = next_u();
          for (int g = 0; g < 3; ++g)
            w << "            const double e" << g << "_ = " << with_sums(sv(other, F, num(g)), t == fam.mo ? gm : num(g), t == fam.mo ? num(g) : gf)
              << ";\n";
          w << "            G" << other << " = fs_pick3(" << u << ", e0_, e1_, e2_);\n";
        }
      } else if (!(g_.is_cut(fam.mo) && g_.is_cut(fam.fa))) {
        const std::string u = next_u();
        w << "            double e_[9];\n";
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b)
            w << "            e_[" << 3 * a + b << "] = "
              << with_sums("((" + Tr(t, "G" + num(t), num(a), num(b)) + " * " + sv(fam.mo, F, num(a)) + ") * " + sv(fam.fa, F, num(b)) + ")", num(a), num(b))
              << ";\n";
        w << "            const unsigned pr_ = fs_pick9(" << u << ", e_);\n";
        if (!g_.is_cut(fam.mo)) w << "            " << gm << " = (pr_ * 11u) >> 5;\n";  // pr_ / 3 for pr_ < 9
        if (!g_.is_cut(fam.fa)) w << "            " << gf << " = pr_ - 3u * ((pr_ * 11u) >> 5);\n";
      }
      for (int c : kids)
        if (!g_.is_cut(c)) {
          const std::string u = next_u();
          w << "            G" << c << " = fs_pick3(" << u << ", " << Tr(c, "0", gm, gf) << " * x" << c << "_0, " << Tr(c, "1", gm, gf) << " * x" << c
            << "_1, " << Tr(c, "2", gm, gf) << " * x" << c << "_2);\n";
        }
      w << "          }\n";
    }
    n_dec_ = D;
    // the configuration's weight, scaled as Z is (evidence_body's W0_ at run-time genotypes)
    w << "          double w_ = 1.0;\n";
    for (int c = 0; c < evidence_scale_digits() / 7; ++c) w << "          w_ = w_ * 10000000.0;\n";
    for (int p = 0; p < g_.N; ++p)
      w << "          w_ = w_ * (" << (m_.mother[p] < 0 ? prior_at(p) : Tr(p, "G" + num(p), "G" + num(m_.mother[p]), "G" + num(m_.father[p]))) << " * "
        << lk_at(p) << ");\n";
    w << "          if (sp_) sp_[k_] = " << (loops ? "w_" : "w_ / Z_") << ";\n";
    // the row: from the lane, in 32-bit words where the row's first byte is 4-aligned, in bytes otherwise
    const int nw = g_.N / 4;
    w << "          if (gg) {\n            signed char *const d_ = gg + (long)k_ * " << g_.N << ";\n            int b_ = 0;\n";
    if (nw > 0) {
      w << "            if (((unsigned long)d_ & 3) == 0) {\n";
      for (int k = 0; k < nw; ++k) {
        w << "              ((unsigned *)d_)[" << k << "] = ";
        for (int j = 0; j < 4; ++j) w << (j ? " | " : "") << "(G" << 4 * k + j << " << " << 8 * j << ")";
        w << ";\n";
      }
      w << "              b_ = " << 4 * nw << ";\n            }\n";
    }
    for (int p = 0; p < g_.N; ++p) w << "            if (b_ <= " << p << ") d_[" << p << "] = (signed char)G" << p << ";\n";
    w << "          }\n";
    // the messages the walk reads, into the lane's row
    for (const auto &kv : sv_at_)
      for (int g = 0; g < 3; ++g) o_ << "        sw[" << kv.second + g << "] = " << kv.first << "_" << g << ";\n";
    o_ << "#pragma unroll 1\n        for (int k_ = 0; k_ < nd_; ++k_) {\n";
    if (loops) {
      // (word D + as_ of the draw's stream)
      o_ << "          unsigned rs_[4];\n"
         << "          fs_philox4x32_10(ilo_, ihi_, (unsigned)k_, (unsigned)(" << D << " + as_) >> 2, key0_, key1_, rs_);\n"
         << "          const unsigned el_ = (unsigned)(" << D << " + as_) & 3u;\n"
         << "          const double us_ = FS_U01(el_ == 0 ? rs_[0] : (el_ == 1 ? rs_[1] : (el_ == 2 ? rs_[2] : rs_[3])));\n"
         << "          if (!(Zt_ == Wall || us_ * Zt_ < Wall)) continue;\n";
    }
    o_ << w.str() << "        }\n";
  }
  std::map<std::string, int> sv_at_;  // sample_body: message name -> its first double in the lane's row
  int n_dec_ = 0;

  // The cut-assignment loop of a pedigree with loops: `decls` (the accumulators) in front, then per assignment as_ of the cut
  // members their genotypes a<k>, their local factors lam<k> and Lam = 1e7 * prod lam<k>, every component's total weight Zc<c>
  // (component_sums), and where the caller uses them Wc<c> = Lam * prod_{c' != c} Zc<c'> (the weight of everything outside
  // component c) and Wall = Lam * prod_c Zc<c>; `tail` emits the rest of the assignment's statements.  Leaves o_ empty.
  std::string cut_loop(const std::string &decls, bool wc, bool wall, const std::function<void()> &tail) {
    const int ncomp = (int)g_.rep.size();
    int total = 1;
    for (size_t k = 0; k < g_.cut.size(); ++k) total *= 3;
    std::ostringstream head;
    head << decls << "#pragma unroll 1\n      for (int as_ = 0; as_ < " << total << "; ++as_) {\n";
    int div = 1;
    for (int k : g_.cut) {
      head << "      const int a" << k << " = (as_ / " << div << ") % 3;\n";
      div *= 3;
    }
    // local factors of the cut members at their assigned genotype, and the reference's 1e7
    std::string lam = "10000000.0";
    for (int k : g_.cut) {
      const std::string c = loc(k);
      o_ << "      const double lam" << k << " = a" << k << " == 0 ? " << c << "_0 : (a" << k << " == 1 ? " << c << "_1 : " << c
         << "_2);\n";
      lam = "(" + lam + " * lam" + num(k) + ")";
    }
    o_ << "      const double Lam = " << lam << ";\n";
    component_sums();
    if (wc)
      for (int c = 0; c < ncomp; ++c) o_ << "      const double Wc" << c << " = " << times_sums("Lam", c) << ";\n";
    if (wall) o_ << "      const double Wall = " << times_sums("Lam") << ";\n";
    tail();
    const std::string out = head.str() + o_.str() + "      }\n";
    o_.str("");
    return out;
  }
  // One sum pass inside a per-pass loop (pass_loop): evidence_body's statements for the total weight, which it leaves in Zp_.
  // Leaves o_ empty.
  std::string sum_pass() {
    if (!g_.cut.empty())
      return cut_loop("      double Zt_ = 0;\n", /*wc=*/false, /*wall=*/true, [&] { o_ << "      Zt_ = Zt_ + Wall;\n"; fence(1); }) +
             "      const double Zp_ = Zt_;\n";
    fence(1);
    component_sums();
    o_ << "      const double Zp_ = " << times_sums("") << ";\n";
    fence(1);
    const std::string pass = o_.str();
    o_.str("");
    return pass;
  }
  // Zc<c>: the total weight of component c, from the marginal of its representative
  void component_sums() {
    for (size_t c = 0; c < g_.rep.size(); ++c) {
      marginal(g_.rep[c]);
      o_ << "      const double Zc" << c << " = (m" << g_.rep[c] << "_0 + m" << g_.rep[c] << "_1) + m" << g_.rep[c] << "_2;\n";
    }
  }
  // `e` times the components' sums, left to right, but for component `skip`
  std::string times_sums(std::string e, int skip = -1, const char *sum = "Zc") const {
    for (int c = 0; c < (int)g_.rep.size(); ++c)
      if (c != skip) e = e.empty() ? sum + num(c) : "(" + e + " * " + sum + num(c) + ")";
    return e;
  }

  // ---- The complex sum pass (charfn_body): the sum pass's messages with member p's likelihood entry the complex number
  // l * w.  The third arithmetic beside the sum pass's and the max pass's: the same three message kinds on the same graph, their
  // names prefixed "z", every value a pair of doubles <name>r / <name>i — or one double <name>, where it is real whatever the
  // weights are: a cut member's indicator and what is made of real values alone (zreal_).  The transmission entries, the founders'
  // priors and the 1e7 scales are real.  A product of two pairs is (a c - b d, a d + b c), of a real and a pair componentwise; a
  // sum, and an fma chain with a real T, componentwise — each component the statement the real pass has, in its order.  So every
  // operation is even (real parts) or odd (imaginary parts) in the imaginary parts: a conjugate table gives the conjugate, and
  // with imaginary parts of +0.0 and real parts >= 0 the imaginary parts stay +0.0 and the real parts are the real pass's bits on
  // the rows l * w_re (b d is +0.0 and x - 0.0 is x).  A product of more than two factors goes left to right through
  // temporaries (zt<id>), so that no operand's text stands more than twice.
  struct Cx {
    std::string re, im;  // im empty: a real value
    bool bind = false;   // an expression that costs a read at each mention (lean local factors): named before it is used twice
    bool real() const { return im.empty(); }
  };
  Cx zval(const std::string &n, const std::string &idx) const {
    const std::string s = n + "_" + idx;
    return zreal_.count(n) ? Cx{s, ""} : Cx{s + "r", s + "i", zbind_.count(n) != 0};
  }
  void zdef(const std::string &s, const Cx &v) {
    if (v.real()) o_ << "      const double " << s << " = " << v.re << ";\n";
    else o_ << "      const double " << s << "r = " << v.re << ", " << s << "i = " << v.im << ";\n";
  }
  Cx ztemp(const Cx &v) {
    const std::string t = "zt" + num(uid_++);
    zdef(t, v);
    return v.real() ? Cx{t, ""} : Cx{t + "r", t + "i"};
  }
  Cx zmul(Cx a, Cx b) {
    if (a.real() && b.real()) return {a.re + " * " + b.re, ""};
    if (a.bind && !b.real()) a = ztemp(a);
    if (b.bind) b = ztemp(b);
    if (a.real()) return {a.re + " * " + b.re, a.re + " * " + b.im};
    if (b.real()) return {a.re + " * " + b.re, a.im + " * " + b.re};
    return {"(" + a.re + " * " + b.re + " - " + a.im + " * " + b.im + ")", "(" + a.re + " * " + b.im + " + " + a.im + " * " + b.re + ")"};
  }
  // the factors' product, left to right
  Cx zprod(const std::vector<Cx> &f) {
    if (f.empty()) return {"1.0", ""};
    Cx acc = f[0];
    for (size_t k = 1; k < f.size(); ++k) {
      if (k > 1) acc = ztemp(acc);
      acc = zmul(acc, f[k]);
    }
    return acc;
  }
  // (a + b) + c
  static Cx zsum3(const Cx &a, const Cx &b, const Cx &c) {
    Cx s{"(" + a.re + " + " + b.re + ") + " + c.re, ""};
    if (!a.real()) s.im = "(" + a.im + " + " + b.im + ") + " + c.im;
    return s;
  }
  // whether every one of the names is real
  bool zall_real(const std::vector<std::string> &names) const {
    for (const std::string &n : names)
      if (!zreal_.count(n)) return false;
    return true;
  }

  // member p's local factor zc<p>_g: loc()'s, on the weighted pair
  std::string zloc(int p) {
    const std::string n = "zc" + num(p);
    if (once(n)) {
      bool scale = false;
      for (int s : g_.scaled) scale |= s == p;
      const bool lean = lean_ || p >= lean_from_;
      if (lean) zbind_.insert(n);
      for (int g = 0; g < 3; ++g)
        for (int part = 0; part < 2; ++part) {
          std::string e = "(l" + num(p) + "_" + num(g) + " * cwp[" + num(6 * p + 2 * g + part) + "])";
          if (m_.mother[p] < 0) e = "(" + founder_prior(p, g) + " * " + e + ")";
          if (scale) e = "(10000000.0 * " + e + ")";
          const std::string v = n + "_" + num(g) + (part ? "i" : "r");
          if (lean) o_ << "#define " << v << " " << e << "\n";
          else o_ << "      const double " << v << " = " << e << ";\n";
        }
      if (!lean) fence(2);
    }
    return n;
  }
  // `name`_g = the product of the messages `in`, per genotype
  void zproducts(const std::string &name, const std::vector<std::string> &in) {
    if (zall_real(in)) zreal_.insert(name);
    for (int g = 0; g < 3; ++g) {
      std::vector<Cx> f;
      for (const std::string &i : in) f.push_back(zval(i, num(g)));
      zdef(name + "_" + num(g), zprod(f));
    }
  }
  std::string zvar2fac(int p, int F) {
    const std::string n = "zv" + num(p) + "f" + num(F);
    if (!once(n)) return n;
    if (g_.is_cut(p)) {
      zreal_.insert(n);
      for (int g = 0; g < 3; ++g) o_ << "      const double " << n << "_" << g << " = a" << p << " == " << g << " ? 1.0 : 0.0;\n";
      return n;
    }
    std::vector<std::string> in = {zloc(p)};
    for (int F2 : g_.nb[p])
      if (F2 != F) in.push_back(zfac2var(F2, p));
    zproducts(n, in);
    return n;
  }
  // T * x + acc, componentwise (acc empty: T * x)
  static Cx zfma(const std::string &T, const Cx &x, const Cx &acc) {
    auto part = [&](const std::string &xv, const std::string &a) { return a.empty() ? T + " * " + xv : "__builtin_fma(" + T + ", " + xv + ", " + a + ")"; };
    return {part(x.re, acc.re), x.real() ? "" : part(x.im, acc.im)};
  }
  std::string zchild_sum(int F, int c) {
    const std::string x = zvar2fac(c, F);
    const std::string n = "za" + num(uid_++);
    if (zreal_.count(x)) zreal_.insert(n);
    for (int gm = 0; gm < 3; ++gm)
      for (int gf = 0; gf < 3; ++gf)
        zdef(n + "_" + num(gm) + num(gf),
             zfma(T(c, 2, gm, gf), zval(x, "2"), zfma(T(c, 1, gm, gf), zval(x, "1"), zfma(T(c, 0, gm, gf), zval(x, "0"), {}))));
    fence(2);
    return n;
  }
  std::string zfac2var(int F, int t) {
    const std::string n = "zf" + num(F) + "v" + num(t);
    if (!once(n)) return n;
    const Family &fam = g_.fam[F];
    std::vector<std::string> in;  // pair_product's factors: the parents' messages present, the other children's summaries
    if (t != fam.mo) in.push_back(zvar2fac(fam.mo, F));
    if (t != fam.fa) in.push_back(zvar2fac(fam.fa, F));
    const size_t n_parents = in.size();
    for (int c : fam.kids)
      if (c != t) in.push_back(zchild_sum(F, c));
    const std::string C = n + "w";
    if (zall_real(in)) zreal_.insert(C), zreal_.insert(n);
    for (int gm = 0; gm < 3; ++gm)
      for (int gf = 0; gf < 3; ++gf) {
        std::vector<Cx> f;
        size_t k = 0;
        if (t != fam.mo) f.push_back(zval(in[k++], num(gm)));
        if (t != fam.fa) f.push_back(zval(in[k++], num(gf)));
        for (k = n_parents; k < in.size(); ++k) f.push_back(zval(in[k], num(gm) + num(gf)));
        zdef(C + "_" + num(gm) + num(gf), zprod(f));
      }
    for (int g = 0; g < 3; ++g) {
      auto c = [&](int gm, int gf) { return zval(C, num(gm) + num(gf)); };
      Cx v;
      if (t == fam.mo) v = zsum3(c(g, 0), c(g, 1), c(g, 2));
      else if (t == fam.fa) v = zsum3(c(0, g), c(1, g), c(2, g));
      else
        for (int gm = 0; gm < 3; ++gm)
          for (int gf = 0; gf < 3; ++gf) {
            const bool first = gm == 0 && gf == 0;
            v = zfma(T(t, g, gm, gf), c(gm, gf), first ? Cx{} : v);
            if (first) v.re = "(" + v.re + ")", v.im = v.im.empty() ? "" : "(" + v.im + ")";
          }
      zdef(n + "_" + num(g), v);
    }
    fence(1);
    return n;
  }
  void zmarginal(int p) {
    if (!once("zm" + num(p))) return;
    std::vector<std::string> in = {zloc(p)};
    for (int F : g_.nb[p]) in.push_back(zfac2var(F, p));
    zproducts("zm" + num(p), in);
  }
  // zZ<c>_0: the total weight of component c
  std::vector<Cx> zcomponent_sums() {
    std::vector<Cx> sums;
    for (size_t c = 0; c < g_.rep.size(); ++c) {
      const std::string m = "zm" + num(g_.rep[c]), n = "zZ" + num((int)c);
      zmarginal(g_.rep[c]);
      if (zreal_.count(m)) zreal_.insert(n);
      zdef(n + "_0", zsum3(zval(m, "0"), zval(m, "1"), zval(m, "2")));
      sums.push_back(zval(n, "0"));
    }
    return sums;
  }
  // One complex pass inside charfn_body's loop: sum_pass()'s statements, which leave the pass's total weight in Zp_r / Zp_i.
  // Leaves o_ empty.
  std::string complex_pass() {
    auto named = [&](const std::string &n, Cx v) {  // the total as a pair whatever it is made of
      if (v.real()) v.im = "0.0";
      zdef(n, v);
    };
    std::string pass;
    if (g_.cut.empty()) {
      fence(1);
      named("Zp_", zprod(zcomponent_sums()));
      fence(1);
      pass = o_.str();
    } else {
      int total = 1;
      for (size_t k = 0; k < g_.cut.size(); ++k) total *= 3;
      std::ostringstream head;
      head << "      double Zt_r = 0, Zt_i = 0;\n#pragma unroll 1\n      for (int as_ = 0; as_ < " << total << "; ++as_) {\n";
      int div = 1;
      for (int k : g_.cut) {
        head << "      const int a" << k << " = (as_ / " << div << ") % 3;\n";
        div *= 3;
      }
      std::vector<Cx> f = {{"10000000.0", ""}};
      for (int k : g_.cut) {
        const std::string c = zloc(k), lam = "zlam" + num(k);
        auto pick = [&](const char *part) {
          return "a" + num(k) + " == 0 ? " + c + "_0" + part + " : (a" + num(k) + " == 1 ? " + c + "_1" + part + " : " + c + "_2" + part + ")";
        };
        zdef(lam, {pick("r"), pick("i")});
        f.push_back({lam + "r", lam + "i"});
      }
      named("zLam", zprod(f));
      f = {{"zLamr", "zLami"}};
      for (const Cx &z : zcomponent_sums()) f.push_back(z);
      named("zWall", zprod(f));
      o_ << "      Zt_r = Zt_r + zWallr; Zt_i = Zt_i + zWalli;\n";
      fence(1);
      pass = head.str() + o_.str() + "      }\n      const double Zp_r = Zt_r, Zp_i = Zt_i;\n";
    }
    o_.str("");
    return pass;
  }
  std::set<std::string> zreal_;  // the complex pass's names that hold one double
  std::set<std::string> zbind_;  // ... and those that are macros over volatile reads

  // member p's unnormalised max-marginal row xm<p>_g (maxmarg_body): local * the max-pass messages of the adjacent families
  std::string max_marginal(int p) {
    const std::string n = "xm" + num(p);
    if (once(n)) {
      mx_ = true;
      std::vector<std::string> in = {loc(p)};
      for (int F : g_.nb[p]) in.push_back(max_fac2var(F, p));
      products(n, in);
      mx_ = false;
    }
    return n;
  }
  // Zs<c>: component c's total weight Zc<c> (component_sums' value, bit for bit), pinned: an empty volatile asm takes it as an
  // operand, and volatile asms keep their order, the fences among them, so the sum pass's arithmetic is over before the max
  // pass's starts.  Left to itself the compiler spreads it over the max pass, whose messages are alive in both directions: the
  // 40-member kernel (eight components) then keeps 1.1 KB of scratch per lane where the pinned one keeps none and the
  // leave-one-out kernel keeps none (profiles/maxmarg/resources.txt).
  void pin_sums() {
    for (size_t c = 0; c < g_.rep.size(); ++c)
      o_ << "      double Zs" << c << " = Zc" << c << "; asm volatile(\"\" : \"+v\"(Zs" << c << ") :: \"memory\");\n";
  }
  // Xc<c>: the maximum of component c, the row maximum of its root's max-marginal (maxmarg_body; map_assignment's values).
  // A row of component c is scaled by the maxima of every other component, so all of them stand in front of the first row.  With
  // several components in the lean form (forty members and more) the messages towards a root are formed in a scope of their own
  // here, the maximum pinned behind it (as pin_sums), and formed again where the component's rows are (the same statements, the
  // same values: done_ is put back).  Kept, the upward messages of every component would be alive at once: the 64-member
  // kernel (thirteen components) 624 B of scratch per lane against 300, the 40-member one 196 AGPRs against 158; the lean form's
  // operands are volatile reads, which the compiler does not merge, and the vector ALU has the time.  Under forty members the
  // operands are registers and the compiler would merge the two copies anyway.
  void max_roots() {
    fence(1);
    const bool again = lean_ && g_.rep.size() > 1;
    for (size_t c = 0; c < g_.rep.size(); ++c) {
      const std::map<std::string, bool> before = done_;
      if (again) o_ << "      double Xc" << c << ";\n      {\n";
      const std::string r = max_marginal(g_.rep[c]);
      o_ << "      " << (again ? "" : "const double ") << "Xc" << c << " = __builtin_fmax(__builtin_fmax(" << r << "_0, " << r << "_1), " << r << "_2);\n";
      if (again) {
        o_ << "      }\n      asm volatile(\"\" : \"+v\"(Xc" << c << ") :: \"memory\");\n";
        done_ = before;
      }
    }
  }
  // member p's max-marginal outputs from its unnormalised row `from`: mg[3 p + g] = from_g / Z_, and the row's largest entry
  // beside its arg-max (first of equals) into the runner-up nx_
  void maxmarg_out(int p, const std::string &from) {
    const std::string a = from + "_0", b = from + "_1", c = from + "_2";
    o_ << "      { const double t_ = " << b << " > " << a << " ? " << b << " : " << a << ";\n"
       << "        const double s_ = " << c << " > t_ ? t_ : (" << b << " > " << a << " ? __builtin_fmax(" << a << ", " << c << ") : __builtin_fmax(" << b << ", " << c
       << "));\n"
       << "        nx_ = __builtin_fmax(nx_, s_);\n"
       << "        if (mg) { mg[" << 3 * p << "] = " << a << " / Z_; mg[" << 3 * p + 1 << "] = " << b << " / Z_; mg[" << 3 * p + 2 << "] = " << c << " / Z_; } }\n";
    fence(1);
  }

  // map_body for one assignment of the cut members (loops) or for the pedigree as it is: the max pass, the back-track, and Z_ / W_
  // (Zt_ / Wb_ over the assignments)
  void map_assignment(bool loops) {
    const int nw = (g_.N + 3) / 4;
    fence(1);
    mx_ = true;
    for (size_t c = 0; c < g_.rep.size(); ++c) {
      const int r = g_.rep[c];
      std::vector<std::string> in = {loc(r)};
      for (int F : g_.nb[r]) in.push_back(max_fac2var(F, r));
      products("xm" + num(r), in);
      o_ << "      double Xc" << c << " = xm" << r << "_0; unsigned G" << r << " = 0;\n"
         << "      if (xm" << r << "_1 > Xc" << c << ") { Xc" << c << " = xm" << r << "_1; G" << r << " = 1; }\n"
         << "      if (xm" << r << "_2 > Xc" << c << ") { Xc" << c << " = xm" << r << "_2; G" << r << " = 2; }\n";
    }
    mx_ = false;
    const std::string z = times_sums(loops ? "Lam" : ""), w = times_sums(loops ? "Lam" : "", -1, "Xc");
    std::ostringstream bt;  // the back-track
    for (int k : g_.cut) bt << "        const unsigned G" << k << " = (unsigned)a" << k << ";\n";
    for (size_t i = steps_.size(); i-- > 0;) {
      const Step &st = steps_[i];
      const Family &fam = g_.fam[st.F];
      const std::string gm = "G" + num(fam.mo), gf = "G" + num(fam.fa);
      if (st.t == fam.mo) {
        if (!g_.is_cut(fam.fa)) bt << "        const unsigned " << gf << " = (" << st.bp << " >> (2 * " << gm << ")) & 3u;\n";
      } else if (st.t == fam.fa) {
        if (!g_.is_cut(fam.mo)) bt << "        const unsigned " << gm << " = (" << st.bp << " >> (2 * " << gf << ")) & 3u;\n";
      } else {
        const std::string pr = "pr" + num(st.F);
        bt << "        const unsigned " << pr << " = (" << st.bp << " >> (4 * G" << st.t << ")) & 15u;\n";
        if (!g_.is_cut(fam.mo)) bt << "        const unsigned " << gm << " = (" << pr << " * 11u) >> 5;\n";  // pr / 3 for pr < 9
        if (!g_.is_cut(fam.fa)) bt << "        const unsigned " << gf << " = " << pr << " - 3u * ((" << pr << " * 11u) >> 5);\n";
      }
      for (size_t k = 0; k < st.kids.size(); ++k)
        if (!g_.is_cut(st.kids[k]))
          bt << "        const unsigned G" << st.kids[k] << " = (" << st.kid_bp[k] << " >> (2 * (3 * " << gm << " + " << gf << "))) & 3u;\n";
    }
    for (int k = 0; k < nw; ++k) {
      bt << "        gw" << k << " = ";
      for (int j = 0; j < 4 && 4 * k + j < g_.N; ++j) bt << (j ? " | " : "") << "(G" << 4 * k + j << " << " << 8 * j << ")";
      for (int j = g_.N - 4 * k; j < 4; ++j) bt << " | (255u << " << 8 * j << ")";  // (beyond the last member: never stored)
      bt << ";\n";
    }
    if (!loops) {
      o_ << "      const double Z_ = " << z << ", W_ = " << w << ";\n      {\n" << bt.str() << "      }\n";
      return;
    }
    o_ << "      Zt_ = Zt_ + " << z << ";\n      const double Wa_ = " << w << ";\n"
       << "      if (Wa_ > Wb_) {\n        Wb_ = Wa_;\n" << bt.str() << "      }\n";
    fence(1);
  }

  int family_of(int c) const {
    for (int F : g_.nb[c])
      for (int k : g_.fam[F].kids)
        if (k == c) return F;
    throw std::logic_error("trio: member " + std::to_string(c) + " has no family");
  }
  // the forest component of family F (every family has a member that is not conditioned on: forest_without)
  int family_comp(int F) const {
    const Family &f = g_.fam[F];
    std::vector<int> mem = {f.mo, f.fa};
    mem.insert(mem.end(), f.kids.begin(), f.kids.end());
    for (int p : mem)
      if (!g_.is_cut(p)) return g_.comp[p];
    throw std::logic_error("trio: a family of conditioned members only");
  }

  // child c's 27 clique terms b<c>_<i> (i = 9 gc + 3 gm + gf), their sum b<c>s and their masked sums b<c>A / b<c>X
  std::string trio(int F, int c, const std::vector<std::vector<double>> &mask, int k) {
    (void)fac2var(F, c);  // its product C of the parents' messages and the other children's summaries
    const std::string C = "f" + num(F) + "v" + num(c) + "w", xc = var2fac(c, F), n = "b" + num(c);
    for (int gc = 0; gc < 3; ++gc)
      for (int gm = 0; gm < 3; ++gm)
        for (int gf = 0; gf < 3; ++gf)
          o_ << "      const double " << n << "_" << 9 * gc + 3 * gm + gf << " = (" << T(c, gc, gm, gf) << " * " << C << "_" << gm << gf
             << ") * " << xc << "_" << gc << ";\n";
    auto sum = [&](const std::string &name, const std::vector<double> *m) {
      std::string e;
      for (int i = 0; i < 27; ++i)
        if (!m || (*m)[27 * k + i] == 0.0) e = e.empty() ? n + "_" + num(i) : "(" + e + " + " + n + "_" + num(i) + ")";
      o_ << "      const double " << name << " = " << (e.empty() ? "0.0" : e) << ";\n";
    };
    sum(n + "s", nullptr);
    sum(n + "A", &mask[0]);
    sum(n + "X", &mask[1]);
    fence(1);
    return n;
  }

  // child k's outputs from its total s, its masked sums (the site's chromosome picks one) and, joint, the 27 terms j<i>
  void trio_out(int k, const std::string &s, const std::string &mA, const std::string &mX, const std::string &j) {
    auto stores = [&](const char *op, const char *by) {
      std::string t = "if (dg) dg[" + num(k) + "] = dm_ " + op + " " + by + ";";
      if (!j.empty()) {
        t += " if (jg) {";
        for (int i = 0; i < 27; ++i) t += " jg[" + num(27 * k + i) + "] = " + j + num(i) + " " + op + " " + by + ";";
        t += " }";
      }
      return t;
    };
    o_ << "      { const double s = " << s << "; if (s <= 0) bn_fail = true;\n"
       << "        const double dm_ = xchr_ ? " << mX << " : " << mA << ";\n"
       << "        if (s < 1e-290) { asm volatile(\"\" ::: \"memory\"); " << stores("/", "s") << " }\n"
       << "        else { const double r = 1.0 / s; " << stores("*", "r") << " } }\n";
  }

  // child c's four unnormalised origin terms o<c>O_<2 a + b> and four het-transmission terms o<c>H_<i> (origin_body's sums)
  std::string origin(int F, int c) {
    (void)fac2var(F, c);  // its product C of the parents' messages and the other children's summaries
    const std::string C = "f" + num(F) + "v" + num(c) + "w", xc = var2fac(c, F), n = "o" + num(c);
    const bool son = m_.gender[c] == 1;
    // build_allele_tables' row of the pass's block: [child sex][parent][allele][genotype]
    auto A = [&](int parent, int a, int g) { return "alx[" + num((son ? 0 : 12) + 6 * parent + 3 * a + g) + "]"; };
    auto p = [&](int a, int gm, int gf) { return n + "p_" + num(a) + num(gm) + num(gf); };
    auto M = [&](int a, int gf) { return n + "M_" + num(a) + num(gf); };
    auto q = [&](int a, int b, int gf) { return n + "q_" + num(a) + num(b) + num(gf); };
    auto x = [&](int a, int b) { return n + "x_" + num(a) + num(b); };
    for (int a = 0; a < 2; ++a)
      for (int gm = 0; gm < 3; ++gm)
        for (int gf = 0; gf < 3; ++gf)
          o_ << "      const double " << p(a, gm, gf) << " = " << A(0, a, gm) << " * " << C << "_" << gm << gf << ";\n";
    for (int a = 0; a < 2; ++a)
      for (int gf = 0; gf < 3; ++gf)
        o_ << "      const double " << M(a, gf) << " = (" << p(a, 0, gf) << " + " << p(a, 1, gf) << ") + " << p(a, 2, gf) << ";\n";
    fence(2);
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        for (int gf = 0; gf < 3; ++gf) o_ << "      const double " << q(a, b, gf) << " = " << A(1, b, gf) << " * " << M(a, gf) << ";\n";
        // the child's message at gamma(a, b): a son's genotype at a chrX site is 2 a
        o_ << "      const double " << x(a, b) << " = ";
        if (son && a + b != 2 * a) o_ << "x_ ? " << xc << "_" << 2 * a << " : " << xc << "_" << a + b;
        else o_ << xc << "_" << a + b;
        o_ << ";\n"
           << "      const double " << n << "O_" << 2 * a + b << " = ((" << q(a, b, 0) << " + " << q(a, b, 1) << ") + " << q(a, b, 2) << ") * "
           << x(a, b) << ";\n";
      }
    for (int a = 1; a >= 0; --a) {  // (hettx's order: the alternative allele first)
      for (int b = 0; b < 2; ++b)
        o_ << "      const double " << n << "r_" << a << b << " = (" << A(1, b, 0) << " * " << p(a, 1, 0) << " + " << A(1, b, 1) << " * " << p(a, 1, 1)
           << ") + " << A(1, b, 2) << " * " << p(a, 1, 2) << ";\n";
      o_ << "      const double " << n << "H_" << 1 - a << " = " << n << "r_" << a << "0 * " << x(a, 0) << " + " << n << "r_" << a << "1 * " << x(a, 1)
         << ";\n";
    }
    for (int b = 1; b >= 0; --b)
      o_ << "      const double " << n << "H_" << 3 - b << " = " << q(0, b, 1) << " * " << x(0, b) << " + " << q(1, b, 1) << " * " << x(1, b) << ";\n";
    fence(1);
    return n;
  }

  // child k's outputs from its four origin terms O_<i> and four het-transmission terms H_<i>: og[4 k + i] = O_i / s and
  // hg[4 k + i] = H_i / s, s the origin terms' sum left to right, in trio_out's arithmetic (one reciprocal; the divisions behind a
  // real branch for a sum in the subnormal range).  A sum that is not a positive finite number fails the site.
  // Plain stores, as trio_out's: a lane's rows lie 32 K bytes from its neighbour's, an instruction writes 8 bytes into each of 64
  // lines, and it is the L2 that makes whole lines of them: 1.7 ms per 10 M ten-member sites, 0.46 of 8 TB/s
  // (profiles/origin/rate.txt).  Non-temporal stores, which serve the outputs that a wave writes as whole lines, do not serve
  // these: each piece would be handed on by itself.
  void origin_out(int k, const std::string &O, const std::string &H) {
    auto stores = [&](const char *op, const char *by) {
      std::string t;
      for (const char *out : {"og", "hg"}) {
        t += std::string(" if (") + out + ") {";
        for (int i = 0; i < 4; ++i)
          t += std::string(" ") + out + "[" + num(4 * k + i) + "] = " + (out[0] == 'o' ? O : H) + "_" + num(i) + " " + op + " " + by + ";";
        t += " }";
      }
      return t;
    };
    o_ << "      { const double s = ((" << O << "_0 + " << O << "_1) + " << O << "_2) + " << O << "_3;\n"
       << "        if (!(s > 0 && s <= 1.79769313486231570815e308)) bn_fail = true;\n"
       << "        if (s < 1e-290) { asm volatile(\"\" ::: \"memory\");" << stores("/", "s") << " }\n"
       << "        else { const double r = 1.0 / s;" << stores("*", "r") << " } }\n";
  }

  const Model &m_;
  const Graph &g_;
  const int fences_;  // (EmitOptions)
  const std::string out_;
  const bool lean_;
  const int lean_from_;
  const bool site_prior_;
  const std::string t_from_;  // the array T() reads
  std::ostringstream o_;
  std::map<std::string, bool> done_;
  int uid_ = 0;
  // the max pass of map_body: messages named x..., and what the back-track needs of each family -> member message
  bool mx_ = false;
  bool bp_ = true;  // the max pass keeps its arg-maxes (map_body); off: plain maxima (maxmarg_body)
  struct Step {
    int F, t;
    std::string bp;                    // the message's packed arg-maxes
    std::vector<int> kids;             // the family's other children ...
    std::vector<std::string> kid_bp;   // ... and their summaries' packed arg-maxes
  };
  std::vector<Step> steps_;
  // the sum pass's family -> member messages in the order they were formed (sample_body walks them backwards)
  struct SumStep {
    int F, t;
  };
  std::vector<SumStep> sum_steps_;

  static std::string num(int x) { return std::to_string(x); }
  // Compiler fence: LDS reads (table entries, likelihoods) may not be hoisted above it.  Without
  // it hipcc front-loads the reads of the whole straight-line program and spills to scratch,
  // which costs real HBM traffic in a kernel that is otherwise memory-bound.  Small pedigrees fit
  // without (and run faster: the blocks overlap), so the fences are a variant (elim_source).
  void fence(int level) { if (fences_ >= level) o_ << "      asm volatile(\"\" ::: \"memory\");\n"; }
  bool once(const std::string &key) {
    if (done_.count(key)) return false;
    done_[key] = true;
    return true;
  }
  int kind(int p) const {
    const bool male = m_.gender[p] == 1;
    return m_.mother[p] < 0 ? (male ? 0 : 1) : (male ? 2 : 3);
  }
  std::string T(int child, int gc, int gm, int gf) const {
    return t_from_ + "[" + num(kind(child) * 27 + 9 * gc + 3 * gm + gf) + "]";
  }

  // member p's local factor at genotype g without the component's scale: lk for a child, prior * lk for a founder (the prior
  // the model's row, or with site priors the lane's own)
  std::string unscaled_loc(int p, int g) const {
    std::string e = "l" + num(p) + "_" + num(g);
    if (m_.mother[p] < 0) e = "(" + founder_prior(p, g) + " * " + e + ")";
    return e;
  }
  // founder p's prior at genotype g: the model's row (by the flags, a male's chrX row among them) or the site's own
  std::string founder_prior(int p, int g) const {
    return site_prior_ ? std::string(kind(p) == 0 ? "pm_" : "pa_") + num(g) : "tcf[" + num(kind(p) * 27 + 9 * g) + "]";
  }

  // member-local factor c{p}_g
  std::string loc(int p) {
    const std::string n = "c" + num(p);
    if (once(n)) {
      bool scale = false;
      for (int s : g_.scaled) scale |= s == p;
      for (int g = 0; g < 3; ++g) {
        std::string e = unscaled_loc(p, g);
        if (scale) e = "(10000000.0 * " + e + ")";
        // lean: not a variable but a macro — the factor is formed again at each of its two or three uses, from a fresh read of
        // the likelihood, instead of living in a register from the first use to the last (3N doubles: the widest pedigrees'
        // register wall)
        if (lean_ || p >= lean_from_) o_ << "#define " << n << "_" << g << " " << e << "\n";
        else o_ << "      const double " << n << "_" << g << " = " << e << ";\n";
      }
      if (!(lean_ || p >= lean_from_)) fence(2);
    }
    return n;
  }

  // member -> family message v{p}f{F}_g = local * prod of the other families' messages
  std::string var2fac(int p, int F) {
    const std::string n = (mx_ ? "xv" : "v") + num(p) + "f" + num(F);
    if (g_.is_cut(p)) {  // a conditioned member: every family sees its assigned genotype, nothing flows through
      if (once(n))
        for (int g = 0; g < 3; ++g)
          o_ << "      const double " << n << "_" << g << " = a" << p << " == " << g << " ? 1.0 : 0.0;\n";
      return n;
    }
    if (once(n)) {
      std::vector<std::string> in = {loc(p)};
      for (int F2 : g_.nb[p])
        if (F2 != F) in.push_back(mx_ ? max_fac2var(F2, p) : fac2var(F2, p));
      products(n, in);
    }
    return n;
  }

  // child summary a<id>_{gm}{gf} = sum_gc T_c[gc|gm,gf] * v{c}f{F}_gc.  Deliberately NOT memoised:
  // a summary is needed by several messages of its family, and keeping 9 doubles per child alive
  // across the whole program costs more (registers -> scratch -> HBM traffic) than recomputing
  // 27 multiply-adds in a kernel whose vector ALU is mostly idle.
  std::string child_sum(int F, int c) {
    const std::string x = var2fac(c, F);
    const std::string n = "a" + num(uid_++);
    for (int gm = 0; gm < 3; ++gm)
      for (int gf = 0; gf < 3; ++gf)
        o_ << "      const double " << n << "_" << gm << gf << " = __builtin_fma(" << T(c, 2, gm, gf) << ", " << x
           << "_2, __builtin_fma(" << T(c, 1, gm, gf) << ", " << x << "_1, " << T(c, 0, gm, gf) << " * " << x << "_0));\n";
    fence(2);
    return n;
  }

  // `name`_g = the product of the messages `in`, per genotype
  void products(const std::string &name, const std::vector<std::string> &in) {
    for (int g = 0; g < 3; ++g) {
      o_ << "      const double " << name << "_" << g << " = ";
      for (size_t k = 0; k < in.size(); ++k) o_ << (k ? " * " : "") << in[k] << "_" << g;
      o_ << ";\n";
    }
  }

  // What family F sends member t, before the reduction over the parents' genotypes: C_{gm}{gf} (named <n>w_{gm}{gf}), the
  // product of the parents' messages present (in the pass under way: var2fac) and of the other children's summaries `sums`
  std::string pair_product(int F, int t, const std::string &n, const std::vector<std::string> &sums) {
    const Family &fam = g_.fam[F];
    const std::string xm = t == fam.mo ? "" : var2fac(fam.mo, F);
    const std::string xf = t == fam.fa ? "" : var2fac(fam.fa, F);
    const std::string C = n + "w";
    for (int gm = 0; gm < 3; ++gm)
      for (int gf = 0; gf < 3; ++gf) {
        std::vector<std::string> terms;
        if (!xm.empty()) terms.push_back(xm + "_" + num(gm));
        if (!xf.empty()) terms.push_back(xf + "_" + num(gf));
        for (const std::string &s : sums) terms.push_back(s + "_" + num(gm) + num(gf));
        o_ << "      const double " << C << "_" << gm << gf << " = ";
        if (terms.empty()) o_ << "1.0";
        for (size_t k = 0; k < terms.size(); ++k) o_ << (k ? " * " : "") << terms[k];
        o_ << ";\n";
      }
    return C;
  }

  // family -> member message f{F}v{t}_g
  std::string fac2var(int F, int t) {
    const std::string n = "f" + num(F) + "v" + num(t);
    if (!once(n)) return n;
    const Family &fam = g_.fam[F];
    std::vector<std::string> sums;
    for (int c : fam.kids)
      if (c != t) sums.push_back(child_sum(F, c));
    const std::string C = pair_product(F, t, n, sums);
    for (int g = 0; g < 3; ++g) {
      o_ << "      const double " << n << "_" << g << " = ";
      if (t == fam.mo) {
        o_ << "(" << C << "_" << g << "0 + " << C << "_" << g << "1) + " << C << "_" << g << "2";
      } else if (t == fam.fa) {
        o_ << "(" << C << "_0" << g << " + " << C << "_1" << g << ") + " << C << "_2" << g;
      } else {
        std::string e;
        for (int gm = 0; gm < 3; ++gm)
          for (int gf = 0; gf < 3; ++gf) {
            const std::string term = T(t, g, gm, gf) + ", " + C + "_" + num(gm) + num(gf);
            e = e.empty() ? "(" + T(t, g, gm, gf) + " * " + C + "_" + num(gm) + num(gf) + ")"
                          : "__builtin_fma(" + term + ", " + e + ")";
          }
        o_ << e;
      }
      o_ << ";\n";
    }
    fence(1);
    sum_steps_.push_back({F, t});
    return n;
  }

  // max pass: one maximum over e[0..n) with its arg-max (first of equals) -> `v` (declared here), `b` |= arg << shift
  void arg_max(const std::string &v, const std::vector<std::string> &e, const std::string &b, int shift) {
    o_ << "      double " << v << " = " << e[0] << ";\n      { unsigned k_ = 0;";
    for (size_t i = 1; i < e.size(); ++i)
      o_ << " { const double e_ = " << e[i] << "; if (e_ > " << v << ") { " << v << " = e_; k_ = " << i << "; } }\n       ";
    o_ << " " << b << " |= k_ << " << shift << "; }\n";
  }

  // max pass child summary xa<id>_{gm}{gf} = max_gc T_c[gc|gm,gf] * xv{c}f{F}_gc, the nine arg-maxes in xa<id>b
  std::string max_child_sum(int F, int c) {
    const std::string x = var2fac(c, F);
    const std::string n = "xa" + num(uid_++);
    if (!bp_) {
      for (int gm = 0; gm < 3; ++gm)
        for (int gf = 0; gf < 3; ++gf)
          o_ << "      const double " << n << "_" << gm << gf << " = __builtin_fmax(__builtin_fmax(" << T(c, 0, gm, gf) << " * " << x << "_0, " << T(c, 1, gm, gf)
             << " * " << x << "_1), " << T(c, 2, gm, gf) << " * " << x << "_2);\n";
      fence(2);
      return n;
    }
    o_ << "      unsigned " << n << "b = 0;\n";
    for (int gm = 0; gm < 3; ++gm)
      for (int gf = 0; gf < 3; ++gf) {
        std::vector<std::string> e;
        for (int gc = 0; gc < 3; ++gc) e.push_back(T(c, gc, gm, gf) + " * " + x + "_" + num(gc));
        arg_max(n + "_" + num(gm) + num(gf), e, n + "b", 2 * (3 * gm + gf));
      }
    fence(2);
    return n;
  }

  // max pass family -> member message xf{F}v{t}_g with its arg-maxes in xf{F}v{t}b; notes the back-track's step
  std::string max_fac2var(int F, int t) {
    const std::string n = "xf" + num(F) + "v" + num(t);
    if (!once(n)) return n;
    const Family &fam = g_.fam[F];
    Step st{F, t, n + "b", {}, {}};
    std::vector<std::string> sums;
    for (int c : fam.kids)
      if (c != t) {
        sums.push_back(max_child_sum(F, c));
        st.kids.push_back(c);
        st.kid_bp.push_back(sums.back() + "b");
      }
    const std::string C = pair_product(F, t, n, sums);
    if (bp_) o_ << "      unsigned " << n << "b = 0;\n";
    for (int g = 0; g < 3; ++g) {
      std::vector<std::string> e;
      if (t == fam.mo) {
        for (int gf = 0; gf < 3; ++gf) e.push_back(C + "_" + num(g) + num(gf));
      } else if (t == fam.fa) {
        for (int gm = 0; gm < 3; ++gm) e.push_back(C + "_" + num(gm) + num(g));
      } else {
        for (int gm = 0; gm < 3; ++gm)
          for (int gf = 0; gf < 3; ++gf) e.push_back(T(t, g, gm, gf) + " * " + C + "_" + num(gm) + num(gf));
      }
      if (bp_) {
        arg_max(n + "_" + num(g), e, n + "b", (e.size() == 9 ? 4 : 2) * g);
        continue;
      }
      std::string mx = e[0];
      for (size_t i = 1; i < e.size(); ++i) mx = "__builtin_fmax(" + mx + ", " + e[i] + ")";
      o_ << "      const double " << n << "_" << g << " = " << mx << ";\n";
    }
    fence(1);
    if (bp_) steps_.push_back(st);
    return n;
  }

  // unnormalised marginal m{p}_g = local * prod of the messages of the adjacent families
  void marginal(int p) {
    if (!once("m" + num(p))) return;
    std::vector<std::string> in = {loc(p)};
    for (int F : g_.nb[p]) in.push_back(fac2var(F, p));
    products("m" + num(p), in);
  }

  // member p's cavity row (loo_body): k{p}_g = the founder's prior * prod of the messages of the adjacent families.  A child of
  // one family and no other: that family's message itself; a founder without a family: its prior.  -> the row's name
  std::string cavity(int p) {
    std::vector<std::string> in;
    for (int F : g_.nb[p]) in.push_back(fac2var(F, p));
    if (m_.mother[p] >= 0 && in.size() == 1) return in[0];
    const std::string n = "k" + num(p);
    for (int g = 0; g < 3; ++g) {
      o_ << "      const double " << n << "_" << g << " = ";
      if (m_.mother[p] < 0) o_ << founder_prior(p, g);
      for (size_t k = 0; k < in.size(); ++k) o_ << (k || m_.mother[p] < 0 ? " * " : "") << in[k] << "_" << g;
      o_ << ";\n";
    }
    return n;
  }

  // member p's leave-one-out outputs from its unnormalised cavity row `from`: og[3 p + g] = from_g / s and fg[p] = the row's
  // product with p's likelihood (read again from the row in the lean form) / s, in normalise()'s arithmetic: one reciprocal,
  // the three (four) divisions behind a real branch for a sum in the subnormal range.  A sum that is not a positive finite
  // number fails the site.
  void loo_out(int p, const std::string &from) {
    auto o3 = [&](int g) { return "og[" + num(3 * p + g) + "]"; };
    const std::string l = "l" + num(p);
    o_ << "      { const double s = (" << from << "_0 + " << from << "_1) + " << from << "_2; if (!(s > 0 && s <= 1.79769313486231570815e308)) bn_fail = true;\n"
       << "        const double t = ((" << from << "_0 * " << l << "_0 + " << from << "_1 * " << l << "_1) + " << from << "_2 * " << l << "_2);\n"
       << "        if (s < 1e-290) { asm volatile(\"\" ::: \"memory\"); if (og) { " << o3(0) << " = " << from << "_0 / s; " << o3(1) << " = " << from
       << "_1 / s; " << o3(2) << " = " << from << "_2 / s; } if (fg) fg[" << p << "] = t / s; }\n"
       << "        else { const double r = 1.0 / s; if (og) { " << o3(0) << " = " << from << "_0 * r; " << o3(1) << " = " << from << "_1 * r; " << o3(2)
       << " = " << from << "_2 * r; } if (fg) fg[" << p << "] = t * r; } }\n";
    fence(1);
  }

  // row p of the output: `from`_g / sum, with the reference's failure rule (family.cpp:943-954)
  void normalise(int p, const std::string &from) {
    // one division per row and three products (this engine is not bit-ordered anyway); a row sum in the subnormal range,
    // whose reciprocal overflows, keeps the three divisions behind a real branch (as the enumeration kernel does)
    auto o3 = [&](int g) { return out_ + "[" + num(3 * p + g) + "]"; };
    o_ << "      { const double s = (" << from << "_0 + " << from << "_1) + " << from << "_2; if (s <= 0) bn_fail = true;\n"
       << "        if (s < 1e-290) { asm volatile(\"\" ::: \"memory\"); " << o3(0) << " = " << from << "_0 / s; " << o3(1) << " = " << from << "_1 / s; "
       << o3(2) << " = " << from << "_2 / s; }\n"
       << "        else { const double r = 1.0 / s; " << o3(0) << " = " << from << "_0 * r; " << o3(1) << " = " << from << "_1 * r; " << o3(2) << " = "
       << from << "_2 * r; } }\n";
  }
};

}  // namespace

bool elim_supported(const Model &m, std::string *why) {
  Graph g;
  return build_graph(m, g, why);
}

int elim_conditioned_members(const Model &m) {
  Graph g;
  return build_graph(m, g, nullptr) ? (int)g.cut.size() : -1;
}

// One-wave workgroups and no register cap, as for the enumeration kernel (enumgen_block_threads): 8 M five-member
// sites 0.662 -> 0.617 ms, quads 0.507 -> 0.481; six members 0.459 -> 0.403 ms per 4 M sites, seven 0.570 -> 0.512,
// eight 0.718 -> 0.607 (the fence-free variant at ONE wave per SIMD with its overflow in AGPRs), ten 0.664 -> 0.640 and
// fifteen 1.118 -> 1.047 (the fence-per-message variant, which fits two waves): profiles/r02c/exp_elim_waves*.txt.
// Which variant runs best is a property of the pedigree more than of its size: on 90 randomly grown pedigrees of 8-14
// members (PL-shaped rows; 2 M sites and, streaming from HBM, 8 M: profiles/r02c/tune_survey_*_sites.txt) the fence-free
// variant wins two times in three, and starting from it loses 3.1 % on average to the better of the two where "the
// fenced one from nine members on" (fitted to the two benchmark pedigrees, which both prefer the fenced one) loses
// 5.6 %.  The one size that goes the other way in both surveys is eleven members (15 of 17 pedigrees, by 10 % on
// average): with that exception 1.3 %.  So the picker starts from the fence-free variant, at eleven members from the
// fenced one, and a pedigree that has been measured — famseq_set_option "tune", or the table of measured picks that
// build() ships for the pedigrees it pre-builds (the benchmark pedigrees among them) — starts from its note.
// The fused call-path form is another kernel — paced by the sixty logarithms per site between its barriers, not by
// memory — and keeps 256-lane workgroups at two waves per SIMD: 0.317 ms per 1 M ten-member sites against 0.487 in
// one-wave workgroups (tools/call_ab.sh).
int elim_block_threads(const Model &m, bool call_mode) {
  return env_int("FAMSEQ_ELIM_BT", call_mode ? (m.n_members <= 10 ? 256 : 128) : 64);  // (the variable: a tuning aid)
}

// Registers-first from five members on (see kElimVariants); within a family the fence-free variant, with which
// jit_pick_variant starts unless it spills.  (Round 2's "the fenced variant at eleven members" was fitted to the r = 0
// family's survey and is not carried over; a pedigree that has been MEASURED starts from its note either way.)
// From forty members on the form without LDS staging (variants 8..): at 48 members the staged form's 74 KB of LDS rows per wave
// leave two waves per CU and it runs at 0.28 of HBM peak (the unstaged one, four waves per CU: 0.35); from about a hundred the
// rows no longer fit the CU's 160 KB at all (profiles/r03a/exp_elim_unstaged.txt: 24 members 0.52 staged / 0.37 unstaged, 32:
// 0.52 / 0.38, 48: 0.28 / 0.35, 64: - / 0.24, 96: - / 0.15 — past sixty members the registers spill and scratch traffic sets the pace).
int elim_first_variant(const Model &m, bool call_mode) {
  if (call_mode) return 0;
  return m.n_members >= 40 ? 8 : (m.n_members >= 5 ? 4 : 0);
}

namespace {

// The one-lane-per-site shell without LDS staging: a lane reads its site's row straight from global memory into registers
// and stores its results straight back — 8 bytes per lane and instruction, a cache line per lane.  What the staged shell
// (kernel_shell) buys with its LDS rows (coalesced 16-byte accesses) costs it the CU's LDS: 3N doubles per lane leave two
// waves per CU at 48 members and nothing beyond about a hundred; this form needs 3.4 KB of LDS (the factor tables) whatever
// N is, runs four waves per CU, and has no barrier after the first.  famseq_elim's variants 8..11 (direct_source) and every side
// product have this form: they start from begin_side() and fill in what differs.
// site_prior: the lane's row of prior_g in three 16-byte loads issued beside the likelihood loads, the Known bit not read.
struct LaneShell {
  std::string entry;       // ("_prior" is appended with site priors)
  std::string comment;
  std::string outputs;     // the declarations of the third and fourth parameters
  std::string defines;     // behind W3 and BT
  std::string shared;      // __shared__ declarations behind the factor tables'
  std::string more_args;   // parameters behind the common eight (in front of prior_g)
  std::string prologue;    // per workgroup: behind the factor tables' staging, in front of the first barrier
  std::string site_decls;  // per site: in front of the flags
  std::string site_vars;   // ... and behind the failure flags
  std::string after_single;  // behind the single posterior's statements
  std::string body;        // what the lanes that pass the guard run (an Emitter's body and what the kernel adds to it)
  std::string epilogue;    // per site: behind the body's block
  int bt = 64, min_waves = 1;
  // famseq_elim's rules: the single posterior is stored (row[]), the shortcut vote taken, the body runs where `full && !single_fail`.
  // Otherwise only the single posterior's failure rule applies (a lk * prior row sum <= 0), nothing of it is stored and every site
  // that passes it runs the body.
  bool shortcut = false;
  bool fence_single = false, chrx_loop = false, site_prior = false;
  // the founders' prior is the kernel's own: it defines pa_<g> / pm_<g> itself (site_vars), the single posterior and the flags
  // follow as with site_prior, and there is no prior_g to read (famseq_af)
  bool own_prior = false;
  // Where the likelihoods live.  lean: read from the lane's row in global memory at each use (volatile: never kept in a
  // register).  Otherwise members lds_from .. N-1 keep theirs in a per-lane LDS row (3 doubles each, odd stride) and are read
  // from there at each use; the others live in registers.  The last members' local factors have the longest live ranges (the
  // upward pass of the first marginal touches every member, and member p's factor is needed again at its own marginal).
  bool lean = false;
  int lds_from = 1 << 30;
  int lds_extra = 0;  // doubles of the lane's LDS row behind the members' (the kernel's own: famseq_relabel's triple of ones)
};

std::string lane_shell(const Model &m, const LaneShell &d) {
  const int N = m.n_members, W3 = 3 * N, first_lds = std::min(N, d.lds_from), n_lds = d.lean ? 0 : N - first_lds, LP = (3 * n_lds + d.lds_extra) | 1;
  // the lane's prior row is asked for before its likelihoods; FAMSEQ_PRIOR_LATE=1 (tuning aid; not famseq_elim_prior's): after them
  const bool prior_late = !d.shortcut && env_int("FAMSEQ_PRIOR_LATE", 0) != 0;
  std::ostringstream s;
  s << source_head(m, d.comment, d.bt, 0, d.defines);
  if (d.site_prior) s << "typedef double v2d __attribute__((ext_vector_type(2)));\n" << kPriorLoad;
  for (int p = d.lean ? 0 : first_lds; p < N; ++p)
    for (int gt = 0; gt < 3; ++gt)
      s << "#define l" << p << "_" << gt << (d.lean ? " lgv[" : " lrow[") << 3 * (d.lean ? p : p - first_lds) + gt << "]\n";
  s << kernel_signature(d.entry + (d.site_prior ? "_prior" : ""), d.min_waves, d.outputs, d.more_args + (d.site_prior ? ", const double *__restrict__ prior_g" : ""))
    << "  __shared__ double s_tc[432];\n"
    << d.shared
    << "  const int tid = threadIdx.x;\n"
    << "  for (int i = tid; i < 432; i += BT) s_tc[i] = tc_g[i];\n"
    << d.prologue
    << (d.site_prior ? "  const bool p16 = ((unsigned long)prior_g & 15) == 0;\n  v2d pu0, pu1, pu2;\n" : "");
  if (n_lds > 0)
    s << "  __shared__ double s_l[BT * " << LP << "];  // the last " << n_lds << " members' likelihoods, one padded row per lane\n"
      << "  typedef const volatile __attribute__((address_space(3))) double lds_cvd;\n"
      << "  double *lw = s_l + tid * " << LP << ";\n  lds_cvd *lrow = (lds_cvd *)lw;\n";
  s << "  LDS_BARRIER();\n"
    << "  const long chunks = (n_sites + BT - 1) / BT;\n"
    << chunk_range()
    << "  const double kNaN = __builtin_nan(\"\");\n"
    << (d.shortcut ? "" : "  (void)lc;\n")
    << "  for (long ch = c_lo; ch < c_hi; ++ch) {\n"
    // a lane beyond the batch's end works on the last site: the same values to the same addresses as that site's own lane
    << "    const long site = ch * BT + tid < n_sites ? ch * BT + tid : n_sites - 1;\n"
    << "    const double *lg = lk_g + site * W3;\n"
    << d.site_decls
    // (site priors: the Known bit chooses between two rows of the model that this kernel does not read)
    << "    const int fl = flags_g ? (flags_g[site] & " << (d.site_prior || d.own_prior ? 2 : 3) << ") : 0;\n"
    << (d.shortcut ? "" : "    const bool xchr_ = (fl & 2) != 0;\n")
    << "    const double *tcf = s_tc + fl * 108;\n"
    << "    bool single_fail = false, full = false, bn_fail = false;\n"
    << (d.shortcut ? "" : "    (void)full;\n")
    << d.site_vars;
  if (d.site_prior && !prior_late) s << "    PRIOR_LOAD(site);\n";
  if (d.site_prior && d.shortcut) s << kPriorNames;
  if (d.lean)
    s << "    typedef const volatile __attribute__((address_space(1))) double glb_cvd;\n    glb_cvd *lgv = (glb_cvd *)lg;\n";
  else {
    for (int p = 0; p < first_lds; ++p)
      for (int gt = 0; gt < 3; ++gt) s << "    const double l" << p << "_" << gt << " = lg[" << 3 * p + gt << "];\n";
    for (int k = 3 * first_lds; k < W3; ++k) s << "    lw[" << k - 3 * first_lds << "] = lg[" << k << "];\n";
  }
  if (d.site_prior && !d.shortcut) s << (prior_late ? "    PRIOR_LOAD(site);\n" : "") << kPriorNames;
  SingleOptions so;
  so.store = d.shortcut, so.fence = d.fence_single, so.site_prior = d.site_prior || d.own_prior;
  s << single_posterior_statements(m, so) << d.after_single
    << (d.shortcut ? open_body(d.chrx_loop, "full && !single_fail") : open_body(d.chrx_loop, "!single_fail", "xchr_ == (x_ == 1)", ""))
    << d.body << close_body(d.chrx_loop) << d.epilogue << "  }\n}\n";
  return s.str();
}

// "<lead> over F nuclear families[, conditioned on K member(s)], variant <variant>[, founder priors per site]": what a kernel of
// the sum-product family says of itself in its source's first line
std::string describe(const std::string &lead, const Graph &g, const std::string &variant, bool site_prior) {
  return lead + " over " + std::to_string(g.fam.size()) + " nuclear families" +
         (g.cut.empty() ? "" : ", conditioned on " + std::to_string(g.cut.size()) + " member(s)") + ", variant " + variant +
         (site_prior ? ", founder priors per site" : "");
}

Graph graph_or_throw(const Model &m) {
  Graph g;
  std::string why;
  if (!build_graph(m, g, &why)) throw std::runtime_error("elimination engine: " + why);
  return g;
}

// What every user of lane_shell starts from: the graph, the fence level f = variant (checked against the kernel's count), the
// emitter's options and a shell with the common rules set — entry famseq_<name>, the comment describe() makes of `lead`, the
// workgroup size, which fences and loops level f takes, and where the likelihoods live: from forty members on they are read
// from the lane's row at each use (lean, shell and emitter alike), as variant 8+ of famseq_elim does when asked: 3 N doubles of
// registers are the widest pedigrees' wall.  A kernel that deviates overrides behind the call and says why; each ends in its
// own `return lane_shell(m, d)`.
struct SideShell {
  Graph g;
  int f;
  EmitOptions eo;
  LaneShell d;
};
SideShell begin_side(const Model &m, const std::string &name, const std::string &lead, int variant, int n_variants, bool site_prior) {
  SideShell s{graph_or_throw(m), variant, {}, {}};
  if (variant < 0 || variant >= n_variants)
    throw std::runtime_error(name + "_source: variant must be 0.." + std::to_string(n_variants - 1));
  s.eo = emit_options(s.f, "pg", site_prior);
  s.d.lean = s.eo.lean = m.n_members >= 40;
  s.d.entry = "famseq_" + name;
  s.d.comment = describe(lead, s.g, std::to_string(s.f), site_prior);
  s.d.bt = elim_block_threads(m, false);
  s.d.fence_single = s.f >= 3, s.d.chrx_loop = s.f >= 1, s.d.site_prior = site_prior;
  return s;
}

// ---- Text that the epilogues share.
// the status byte of a kernel with the trio kernel's rules
std::string status_store() { return "    if (status_g) status_g[site] = single_fail ? 1 : (bn_fail ? 2 : 0);\n"; }
// `inner` for a site that failed
std::string fail_block(const std::string &inner) { return "    if (single_fail || bn_fail) {\n" + inner + "    }\n"; }
// ptr[0 .. count) = value under `guard` (the pointer itself where none is given: a null output is skipped), the loop
// `#pragma unroll 1`; `indent`: the guard's column (6 inside fail_block)
std::string fill(const std::string &ptr, const std::string &count, const std::string &value = "kNaN", const std::string &guard = "", int indent = 6) {
  const std::string in(indent, ' ');
  return in + "if (" + (guard.empty() ? ptr : guard) + ") {\n#pragma unroll 1\n" + in + "  for (int k = 0; k < " + count + "; ++k) " + ptr + "[k] = " + value +
         ";\n" + in + "}\n";
}
// a count argument clamped into 0 .. its define, once per workgroup (the host checks, the kernel clamps)
std::string clamp_count(const std::string &n, const std::string &arg, const std::string &max) {
  return "  const int " + n + " = " + arg + " < 0 ? 0 : (" + arg + " > " + max + " ? " + max + " : " + arg + ");\n";
}

// A per-pass product (Emitter::pass_loop), as far as its shell goes.  Such a kernel has the evidence kernel's rules and shell.
// Beyond the common arguments it takes a table and a count (1 .. its maximum; the host checks, the kernel clamps); its outputs
// per site are one value per row of the table and loglik, famseq_evidence's, from pass 0; either may be null, and without the
// first only pass 0 runs (last_).  A new one supplies this record, its table's arguments and staging, and an Emitter body that
// hands pass_loop what a pass does to the network.
struct PassProduct {
  const char *out_arg, *out;      // the per-pass output: the kernel's argument and the site's pointer into it
  const char *n_arg, *n, *n_max;  // the count: the kernel's argument, its clamped value, the define that bounds it
  const char *counter;            // the loop's variable
  const char *ll;                 // pass 0's log10 Z without the reference's 1e7: loglik
  const char *result = nullptr;   // what a later pass stores, of its Zp_; none: its log10 Z as pass 0's, not clamped
  bool z0 = false;                // pass 0's Zp_ is kept in Z0_ for `result`
  const char *result_im = nullptr;  // where given: a pass's result is two doubles, `result` and this one (16 bytes per pass)
};
// Fills in the shell's side of product p — the clamp (d.prologue), the output pointer and last_ (site_decls), the variables
// (site_vars), NaN for a failed site and the loglik store (epilogue) — and returns the `per_pass` text of its body: pass 0
// fails the site and leaves the loop where Zp_ is not a positive finite number, else keeps loglik; a later pass stores.
// `digits`: Emitter::evidence_scale_digits().  With `pass0`: that pass's check and keep go there (it fails the site without a
// loop to leave) and the later passes' store alone is returned.
std::string pass_product(const PassProduct &p, int digits, LaneShell &d, std::string *pass0 = nullptr) {
  const std::string out = p.out, n = p.n, ct = p.counter, ll = p.ll, log = "log10(Zp_) - " + std::to_string(digits) + ".0";
  const std::string wide = p.result_im ? "2 * " : "", ok = "Zp_ > 0 && Zp_ <= 1.79769313486231570815e308";
  const std::string keep = (p.z0 ? "Z0_ = Zp_; " : "") + ll + " = " + log + ";";
  d.prologue = clamp_count(n, p.n_arg, p.n_max);
  d.site_decls = "    double *" + out + " = " + p.out_arg + " ? " + p.out_arg + " + site * " + (p.result_im ? "(2 * " + n + ")" : n) + " : nullptr;\n"
                 "    const int last_ = " + out + " ? " + n + " : 0;\n";
  d.site_vars = "    double " + ll + " = kNaN" + (p.z0 ? ", Z0_ = 0" : "") + ";\n";
  d.epilogue = fail_block("      " + ll + " = kNaN;\n" + fill(out, wide + n)) +
               "    if (loglik_g) __builtin_nontemporal_store(" + ll + ", loglik_g + site);\n" + status_store();
  const std::string store =
      p.result_im ? "        __builtin_nontemporal_store(" + std::string(p.result) + ", " + out + " + 2 * (" + ct + " - 1));\n"
                    "        __builtin_nontemporal_store(" + p.result_im + ", " + out + " + 2 * (" + ct + " - 1) + 1);\n"
                  : "        __builtin_nontemporal_store(" + (p.result ? p.result : log) + ", " + out + " + (" + ct + " - 1));\n";
  if (pass0) {  // pass 0 stands apart, in front of a loop over the later passes alone (Emitter::charfn_body)
    *pass0 = "      if (!(" + ok + ")) bn_fail = true;\n      else { " + keep + " }\n";
    return store;
  }
  return "      if (" + ct + " == 0) {\n"
         "        if (!(" + ok + ")) { bn_fail = true; break; }\n"
         "        " + keep + "\n"
         "      } else {\n" + store +
         "      }\n";
}

}  // namespace

std::vector<int> trio_children(const Model &m) {
  std::vector<int> kids;
  for (int p = 0; p < m.n_members; ++p)
    if (m.mother[p] >= 0) kids.push_back(p);
  return kids;
}

// The trio kernel: no single posterior stored and no shortcut, every site that passes the single-posterior rule runs the full
// network.  Outputs per site: joint[27 K] and dnm[K] (either may be null), status.
std::string trio_source(const Model &m, int variant, int form, bool site_prior) {
  const bool want_dnm = form & 1, want_joint = form & 2;
  // (the fence level is the variant's low two bits: every value is taken; the output form is the kernel's own argument)
  auto [g, f, eo, d] = begin_side(m, "trio", "trio posteriors (" + std::string(want_dnm && want_joint ? "de novo + joint" : (want_dnm ? "de novo" : "joint")) + ")",
                                  variant & 3, 4, site_prior);
  if (form < 1 || form > 3) throw std::runtime_error("trio_source: form must be 1 (dnm), 2 (joint) or 3 (both)");
  const std::vector<int> kids = trio_children(m);
  // the de novo mask: where the mutation-free transmission table of the child is exactly 0 (model.cpp), [autosome, chrX][K][27]
  double a0[27], xf0[27], xm0[27];
  famseq_transmission_tables(0.0, a0, xf0, xm0);
  std::vector<std::vector<double>> mask(2, std::vector<double>(27 * kids.size()));
  for (size_t k = 0; k < kids.size(); ++k)
    for (int i = 0; i < 27; ++i) {
      mask[0][27 * k + i] = a0[i];
      mask[1][27 * k + i] = m.gender[kids[k]] == 1 ? xm0[i] : xf0[i];
    }
  d.outputs = "double *__restrict__ joint_g, double *__restrict__ dnm_g";
  d.defines = "#define NKID " + std::to_string(kids.size()) + "\n";
  // (an output this form does not write is a null constant: its stores fold away)
  d.site_decls = std::string(want_joint ? "    double *jg = joint_g ? joint_g + site * (27 * NKID) : nullptr;\n" : "    double *const jg = nullptr;\n") +
                 (want_dnm ? "    double *dg = dnm_g ? dnm_g + site * NKID : nullptr;\n" : "    double *const dg = nullptr;\n") +
                 "    (void)jg; (void)dg;\n";
  d.body = Emitter(m, g, eo).trio_body(kids, mask, want_joint);
  d.epilogue = fail_block(fill("dg", "NKID") + fill("jg", "27 * NKID")) + status_store();
  return lane_shell(m, d);
}

// The MAP kernel: the trio kernel's rules.  Outputs per site: map_gt[N] (int8), map_post (fp64), status; any may be null.  A
// lane's genotype row is N bytes at a stride of N bytes, which no lane can store in aligned words on its own: the rows of a
// workgroup's BT consecutive sites are staged in LDS (BT * N bytes) and written out together, a wave's stores contiguous —
// in 32-bit words where the block's first byte is 4-aligned, in bytes otherwise.
std::string map_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "map", "joint MAP configuration (max-product)", variant, kMapVariants, site_prior);
  const int N = m.n_members, nw = (N + 3) / 4;
  d.outputs = "signed char *__restrict__ gt_g, double *__restrict__ post_g";
  d.defines = "#define NMEM " + std::to_string(N) + "\n";
  d.shared = "  __shared__ unsigned s_gt[(BT * NMEM + 3) / 4];  // the workgroup's genotype rows, as they lie in map_gt\n"
             "  unsigned char *const s_gb = (unsigned char *)s_gt;\n";
  std::ostringstream vars, end;
  vars << "    double map_p = kNaN;\n    unsigned";
  for (int k = 0; k < nw; ++k) vars << (k ? ", " : " ") << "gw" << k << " = 0xffffffffu";
  vars << ";\n";
  d.site_vars = vars.str();
  d.body = Emitter(m, g, eo).map_body() +
           "      if (Z_ <= 0 || W_ <= 0) bn_fail = true;\n"
           "      else map_p = W_ / Z_;\n";
  end << "    if (single_fail || bn_fail) {\n      map_p = kNaN;\n     ";
  for (int k = 0; k < nw; ++k) end << " gw" << k << " = 0xffffffffu;";
  end << "\n    }\n"
      << "    if (post_g) __builtin_nontemporal_store(map_p, post_g + site);\n"
      << status_store()
      << "    if (gt_g) {\n";
  if (N % 4 == 0)
    for (int k = 0; k < nw; ++k) end << "      s_gt[tid * " << nw << " + " << k << "] = gw" << k << ";\n";
  else
    for (int p = 0; p < N; ++p) end << "      s_gb[tid * NMEM + " << p << "] = (unsigned char)(gw" << p / 4 << " >> " << 8 * (p % 4) << ");\n";
  end << "      LDS_BARRIER();\n"
      << "      const long left = n_sites - ch * BT;\n"
      << "      const int nb = (int)(left < BT ? left : BT) * NMEM;  // bytes of this block's rows that lie inside the batch\n"
      << "      signed char *dst = gt_g + ch * BT * NMEM;\n"
      << "      int done = 0;\n"
      << "      if (((unsigned long)dst & 3) == 0) {\n"
      << "        done = nb & ~3;\n"
      << "        for (int i = tid; i < (nb >> 2); i += BT) __builtin_nontemporal_store(s_gt[i], (unsigned *)dst + i);\n"
      << "      }\n"
      << "      for (int i = done + tid; i < nb; i += BT) dst[i] = (signed char)s_gb[i];\n"
      << "      LDS_BARRIER();\n"
      << "    }\n";
  d.epilogue = end.str();
  return lane_shell(m, d);
}

// The evidence kernel: the trio kernel's rules.  Outputs per site: loglik = log10 of the data's likelihood under the pedigree
// (the total weight without the reference's 1e7), pref = the posterior probability that every member is hom-ref, status; any
// may be null.  A total weight that is not a positive finite number fails the site (status 2); a hom-ref weight of 0 does not.
std::string evidence_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "evidence", "evidence and hom-ref posterior (sum pass)", variant, kEvidenceVariants, site_prior);
  d.outputs = "double *__restrict__ loglik_g, double *__restrict__ pref_g";
  d.site_vars = "    double ev_ll = kNaN, ev_p0 = kNaN;\n";
  Emitter e(m, g, eo);
  d.body = e.evidence_body() +
           "      if (!(Z_ > 0 && Z_ <= 1.79769313486231570815e308)) bn_fail = true;\n"
           "      else { ev_ll = log10(Z_) - " + std::to_string(e.evidence_scale_digits()) + ".0; ev_p0 = W0_ / Z_; }\n";
  d.epilogue = "    if (loglik_g) __builtin_nontemporal_store(ev_ll, loglik_g + site);\n"
               "    if (pref_g) __builtin_nontemporal_store(ev_p0, pref_g + site);\n" + status_store();
  return lane_shell(m, d);
}

// The leave-one-out kernel: the trio kernel's rules.  Outputs per site: loo[3 N] (member p's genotype distribution given every
// row but its own) and fit[N] (the predictive likelihood of p's row given the others, Z / Z_-p), status; any may be null (a
// null output's stores fold away).  Stored straight from the lane, as famseq_elim's variants 8..11 store post.  A cavity row
// whose sum is not a positive finite number fails the site (status 2); a total weight of 0 does not: every fit is 0.0 then.
std::string loo_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "loo", "leave-one-out posteriors and fit", variant, kLooVariants, site_prior);
  d.outputs = "double *__restrict__ loo_g, double *__restrict__ fit_g";
  d.defines = "#define NMEM " + std::to_string(m.n_members) + "\n";
  d.site_decls = "    double *og = loo_g ? loo_g + site * W3 : nullptr;\n"
                 "    double *fg = fit_g ? fit_g + site * NMEM : nullptr;\n"
                 "    (void)og; (void)fg;\n";
  d.body = Emitter(m, g, eo).loo_body();
  d.epilogue = fail_block(fill("og", "W3") + fill("fg", "NMEM")) + status_store();
  return lane_shell(m, d);
}

// The max-marginal kernel: the MAP kernel's rules.  Outputs per site: maxmarg[3 N] (member p's row max_{g: g_p = a} w(g) / Z) and
// top[2] (the best configuration's posterior, famseq_map's map_post bit for bit, and the runner-up's), status; any may be null (a
// null output's stores fold away).  The rows are stored straight from the lane as they are formed, as famseq_loo's; a site that
// fails is filled with NaN behind the body.  Where the likelihoods live is famseq_loo's rule (begin_side): this is that kernel's
// live set, a maximum in the place of an addition.
std::string maxmarg_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "maxmarg", "max-marginals and the runner-up (max-product, both directions)", variant, kMaxmargVariants, site_prior);
  d.outputs = "double *__restrict__ maxmarg_g, double *__restrict__ top_g";
  d.site_decls = "    double *mg = maxmarg_g ? maxmarg_g + site * W3 : nullptr;\n"
                 "    (void)mg;\n";
  d.site_vars = "    double mm_w = kNaN, mm_n = kNaN;\n";
  d.body = Emitter(m, g, eo).maxmarg_body();
  d.epilogue = fail_block("      mm_w = kNaN; mm_n = kNaN;\n" + fill("mg", "W3")) +
               "    if (top_g) {\n"
               "      __builtin_nontemporal_store(mm_w, top_g + 2 * site);\n"
               "      __builtin_nontemporal_store(mm_n, top_g + 2 * site + 1);\n"
               "    }\n" + status_store();
  return lane_shell(m, d);
}

// The pattern kernel: a per-pass product (PassProduct).  Beyond the common arguments: mask_g[n_patterns][N] (bit g of an entry
// set: genotype g is allowed to that member) and n_patterns (1 .. FAMSEQ_MAX_PATTERNS; the host checks, the kernel clamps).
// Outputs per site: ppost[n_patterns], pattern m's posterior Z_m / Z — a true division, so that a pattern that allows everything
// gives exactly 1.0 — and loglik, famseq_evidence's, from the unmasked pass; either may be null (without ppost only the unmasked
// pass runs).  No clamp: every term of the sum is non-negative and a masked pass runs the unmasked pass's statements on operands
// that are the same or zero, and rounding is monotonic, so Z_m <= Z holds in floating point as it does in exact arithmetic.
// Z_m = 0 gives 0.0, which is a result; only an unmasked Z that is not a positive finite number fails the site (status 2).
// Where the likelihoods live: in registers twice under forty members (the real rows and the pass's masked copy, which the
// compiler is free to form at its use instead), from forty on read from the lane's row at each use, as the evidence kernel does.
std::string pattern_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "pattern", "genotype-pattern posteriors (sum pass per pattern)", variant, kPatternVariants, site_prior);
  const int N = m.n_members, nmw = (N + 7) / 8;
  d.outputs = "double *__restrict__ ppost_g, double *__restrict__ loglik_g";
  d.more_args = ", const unsigned char *__restrict__ mask_g, int n_patterns";
  d.defines = "#define NMEM " + std::to_string(N) + "\n#define NMW " + std::to_string(nmw) + "\n#define MAXPAT " +
              std::to_string(FAMSEQ_MAX_PATTERNS) + "\n";
  d.shared = "  __shared__ unsigned s_mw[(MAXPAT + 1) * NMW];  // the passes' masks: four bits per member, row 0 (the unmasked pass) all ones\n";
  const PassProduct pass{"ppost_g", "pp", "n_patterns", "np_", "MAXPAT", "pt_", "pt_ll", "Zp_ / Z0_", /*z0=*/true};
  Emitter e(m, g, eo);
  const std::string per_pass = pass_product(pass, e.evidence_scale_digits(), d);
  d.prologue +=
      "  for (int i = tid; i < (np_ + 1) * NMW; i += BT) {\n"
      "    const int pt = i / NMW, w = i - pt * NMW;\n"
      "    unsigned v = 0;\n"
      "    for (int j = 0; j < 8 && 8 * w + j < NMEM; ++j) v |= (pt ? (unsigned)mask_g[(pt - 1) * NMEM + 8 * w + j] & 7u : 7u) << (4 * j);\n"
      "    s_mw[i] = v;\n"
      "  }\n";
  d.body = e.pattern_body(pass.counter, per_pass);
  return lane_shell(m, d);
}

// The relabelling kernel: a per-pass product (PassProduct).  Beyond the common arguments: assign_g[n_assign][N] (int32: which
// member's row member p is given; -1 "no data", and every other entry outside 0 .. N-1 is taken as -1, so nothing outside the
// site's row is ever read) and n_assign (1 .. FAMSEQ_MAX_RELABEL; the host checks, the kernel clamps).  Outputs per site:
// alt[n_assign], log10 Z_a without the reference's 1e7 — not clamped; -inf where Z_a is exactly 0, which is a result — and loglik,
// famseq_evidence's, from the identity pass; either may be null (without alt only the identity pass runs).  Only an identity Z
// that is not a positive finite number fails the site (status 2).
// Where the rows live: a pass indexes them by a run-time (wave-uniform) value, which registers do not allow.  Where BT lane rows
// of 3 (N + 1) doubles (odd stride: no bank conflicts) fit the 64 KB of static LDS beside the tables they sit there, read once
// per pass into the pass's registers; otherwise, and from forty members on as every lean kernel, the site's row in global memory
// is read again at each use.  FAMSEQ_RELABEL_LEAN=1 (a tuning aid) takes the second form at every size.
// That makes three forms, not two.  With 64-lane workgroups the budget ends at 37 members (64 936 bytes; 38 members need
// 65 960), not at 39: at 38 and 39 members the shell already reads global rows (d.lean) while the emitter is not lean yet
// (eo.lean, from forty on) and keeps its local factors in variables.  tests/test_edge_pedigrees.py pins the three from the
// emitted text (edge37, edge38 / edge39, edge40 of famseq_amd/prebuild_sets.py), tests/test_gpu_edge_pedigrees.py runs them.
std::string relabel_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "relabel", "relabelling evidence (sum pass per assignment)", variant, kRelabelVariants, site_prior);
  const int N = m.n_members, bits = N < 255 ? 8 : 16, per = 32 / bits, naw = (N + per - 1) / per;
  const size_t lds_bytes = size_t(d.bt) * ((3 * (N + 1)) | 1) * sizeof(double) + 432 * sizeof(double) +
                           size_t(FAMSEQ_MAX_RELABEL + 1) * naw * sizeof(unsigned);
  const bool lds_rows = N < 40 && lds_bytes <= (size_t(64) << 10) && env_int("FAMSEQ_RELABEL_LEAN", 0) == 0;
  d.lean = !lds_rows;  // (the shell's rows: the three forms above; the emitter stays lean from forty on)
  if (lds_rows) d.lds_from = 0, d.lds_extra = 3;
  d.outputs = "double *__restrict__ alt_g, double *__restrict__ loglik_g";
  d.more_args = ", const int *__restrict__ assign_g, int n_assign";
  d.defines = "#define NMEM " + std::to_string(N) + "\n#define NAW " + std::to_string(naw) + "\n#define MAXREL " +
              std::to_string(FAMSEQ_MAX_RELABEL) + "\n";
  d.shared = "  __shared__ unsigned s_aw[(MAXREL + 1) * NAW];  // the passes' assignments: " + std::to_string(bits) +
             " bits per member, row 0 (the identity pass) 0 .. N-1, NMEM for \"no data\"\n";
  const PassProduct pass{"alt_g", "ap", "n_assign", "na_", "MAXREL", "ps_", "rl_ll"};
  Emitter e(m, g, eo);
  const std::string per_pass = pass_product(pass, e.evidence_scale_digits(), d);
  d.prologue +=
      "  for (int i = tid; i < (na_ + 1) * NAW; i += BT) {\n"
      "    const int ps = i / NAW, w = i - ps * NAW;\n"
      "    unsigned v = 0;\n"
      "    for (int j = 0; j < " + std::to_string(per) + " && " + std::to_string(per) + " * w + j < NMEM; ++j) {\n"
      "      const int p = " + std::to_string(per) + " * w + j;\n"
      "      const int a = ps ? assign_g[(ps - 1) * NMEM + p] : p;\n"
      "      v |= (a >= 0 && a < NMEM ? (unsigned)a : (unsigned)NMEM) << (" + std::to_string(bits) + " * j);\n"
      "    }\n"
      "    s_aw[i] = v;\n"
      "  }\n";
  if (lds_rows) d.site_vars += "    lw[" + std::to_string(3 * N) + "] = 1.0; lw[" + std::to_string(3 * N + 1) + "] = 1.0; lw[" + std::to_string(3 * N + 2) + "] = 1.0;\n";
  d.body = e.relabel_body(pass.counter, per_pass, lds_rows, bits);
  return lane_shell(m, d);
}

// The mutation-rate kernel: a per-pass product (PassProduct), with the evidence kernel's LDS (the factor tables alone: a pass's
// table is read where it lies).  Beyond the common arguments: rt_g[n_rates][432], one factor table per rate, of which only the transmission
// entries are read (whatever they hold: nothing is indexed by them), and n_rates (1 .. FAMSEQ_MAX_RATES; the host checks, the
// kernel clamps).  Outputs per site: rate_ll[n_rates], log10 Z_r without the reference's 1e7 — not clamped; -inf where Z_r is
// exactly 0 (rate 0 on a Mendel-impossible row), which is a result — and loglik, famseq_evidence's, from the pass on the
// context's own table; either may be null (without rate_ll only that pass runs).  Only the context's own Z that is not a
// positive finite number fails the site (status 2).  The rows stay where famseq_evidence has them: registers, lean from forty.
std::string mutrate_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "mutrate", "mutation-rate likelihood profile (sum pass per rate)", variant, kMutrateVariants, site_prior);
  eo.t_from = "trt";
  d.chrx_loop = true;  // (variant 0 too: mutrate_body)
  d.outputs = "double *__restrict__ rate_ll_g, double *__restrict__ loglik_g";
  d.more_args = ", const double *__restrict__ rt_g, int n_rates";
  d.defines = "#define MAXRATES " + std::to_string(FAMSEQ_MAX_RATES) + "\n#define RTD " + std::to_string(FAMSEQ_RATE_TABLE_DOUBLES) + "\n";
  const PassProduct pass{"rate_ll_g", "rp", "n_rates", "nr_", "MAXRATES", "ps_", "mr_ll"};
  Emitter e(m, g, eo);
  d.body = e.mutrate_body(pass.counter, pass_product(pass, e.evidence_scale_digits(), d));
  return lane_shell(m, d);
}

// The weight kernel: a per-pass product (PassProduct), with the evidence kernel's LDS (the factor tables alone: a pass's
// weights are read where they lie).  Beyond the common arguments: wt_g[n_weights][N][3], one table of per-member genotype weights per pass (whatever
// they hold: nothing is indexed by them; the host entries admit finite numbers >= 0, above 1 included), and n_weights
// (1 .. FAMSEQ_MAX_WEIGHTS; the host checks, the kernel clamps).  Outputs per site: wt_ll[n_weights], log10 Z_m without the
// reference's 1e7, Z_m the network's total weight on the rows lk * w_m — not clamped; -inf where Z_m is exactly 0 and +inf where
// it overflows, which are results — and loglik, famseq_evidence's, from the pass on the rows as they are; either may be null
// (without wt_ll only that pass runs, and wt_g is not read).  Only the unweighted Z that is not a positive finite number fails
// the site (status 2).  The rows stay where famseq_evidence has them: registers (twice, as famseq_pattern: the real rows and
// the pass's weighted copy, which the compiler is free to form at its use instead), lean from forty.
std::string weight_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "weight", "per-member genotype weights (sum pass per weight table)", variant, kWeightVariants, site_prior);
  d.outputs = "double *__restrict__ wt_ll_g, double *__restrict__ loglik_g";
  d.more_args = ", const double *__restrict__ wt_g, int n_weights";
  d.defines = "#define MAXWT " + std::to_string(FAMSEQ_MAX_WEIGHTS) + "\n";
  const PassProduct pass{"wt_ll_g", "wp", "n_weights", "nw_", "MAXWT", "ps_", "wt_l0"};
  Emitter e(m, g, eo);
  d.body = e.weight_body(pass.counter, pass_product(pass, e.evidence_scale_digits(), d));
  return lane_shell(m, d);
}

// The characteristic-function kernel: a per-pass product (PassProduct) with the weight kernel's shell and rules, whose later
// passes are complex (Emitter::charfn_body).  Beyond the common arguments: cw_g[n_tables][N][3][2], one table of complex
// per-member genotype weights per pass (re, im; whatever they hold: nothing is indexed by them), and n_tables
// (1 .. FAMSEQ_MAX_CWEIGHTS; the host checks, the kernel clamps).  Outputs per site: cf[n_tables][2] = (Re Z_m / Z0, Im Z_m / Z0),
// true divisions, Z_m the network's total weight on the rows lk * w_m and Z0 on the rows as they are — not clamped; a Z_m of
// exactly 0 gives (0.0, 0.0), which is a result — and loglik, famseq_evidence's, from pass 0; either may be null (without cf only
// pass 0 runs, and cw_g is not read).  Only a Z0 that is not a positive finite number fails the site (status 2).
// Where the rows live: this product has a lean threshold of its own, 25 members (kCharfnLeanFrom; begin_side's is forty).  The
// complex messages double the pass's live set, and the register-resident form — rows in registers, a member's weighted pair
// formed where its local factor is — runs out of registers before forty: without scratch in every variant at 10, 20 and 24
// members, at 28 the site-prior form spills in every variant (24-128 B per lane) and the plain one in variant 0, at 32 both do
// (the site-prior form 164-372 B), at 39 every variant of both (84-644 B).  The lean form — rows read from the lane's row at each
// use, the weights by scalar loads beside them — keeps no scratch in any variant at 21, 32, 39, 40 and 64 members (variants 1-3
// at two to three waves per SIMD).  profiles/charfn/resources.txt holds both surveys.
constexpr int kCharfnLeanFrom = 25;
std::string charfn_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "charfn", "count characteristic function (real sum pass, then a complex sum pass per weight table)", variant, kCharfnVariants, site_prior);
  d.lean = eo.lean = m.n_members >= env_int("FAMSEQ_CHARFN_LEAN_FROM", kCharfnLeanFrom);  // (the variable: a tuning aid)
  d.outputs = "double *__restrict__ cf_g, double *__restrict__ loglik_g";
  d.more_args = ", const double *__restrict__ cw_g, int n_tables";
  d.defines = "#define MAXCW " + std::to_string(FAMSEQ_MAX_CWEIGHTS) + "\n#define CW6 " + std::to_string(6 * m.n_members) + "\n";
  const PassProduct pass{"cf_g", "cp", "n_tables", "nt_", "MAXCW", "ps_", "cf_l0", "Zp_r / Z0_", /*z0=*/true, "Zp_i / Z0_"};
  Emitter e(m, g, eo);
  std::string pass0;
  const std::string per_pass = pass_product(pass, e.evidence_scale_digits(), d, &pass0);
  d.body = e.charfn_body(pass.counter, pass0, per_pass);
  return lane_shell(m, d);
}

// The allele rows of famseq_origin: t(1 | g) = (mu, 1/2, 1 - mu) and t(0 | g) = (1 - mu, 1/2, mu) for a parent who hands one of
// two alleles on; a father's X reaches a daughter from a hemizygous genotype (the heterozygous column 0) and never reaches a son,
// whose row for "no allele" (0) is (1, 0, 1).  [chrX][child sex: 0 son, 1 daughter][parent: 0 mother, 1 father][allele][genotype].
void build_allele_tables(double mu, double *t) {
  const double u = 1.0 - mu;
  const double two[2][3] = {{u, 0.5, mu}, {mu, 0.5, u}}, hemi[2][3] = {{u, 0.0, mu}, {mu, 0.0, u}}, none[2][3] = {{1.0, 0.0, 1.0}, {0.0, 0.0, 0.0}};
  for (int x = 0; x < 2; ++x)
    for (int sex = 0; sex < 2; ++sex)
      for (int parent = 0; parent < 2; ++parent) {
        const double(*row)[3] = (x == 0 || parent == 0) ? two : (sex == 0 ? none : hemi);
        for (int a = 0; a < 2; ++a)
          for (int g = 0; g < 3; ++g) t[24 * x + 12 * sex + 6 * parent + 3 * a + g] = row[a][g];
      }
}

// The origin kernel: the trio kernel's rules and shell.  Beyond the common arguments: al_g[FAMSEQ_ALLELE_TABLE_DOUBLES],
// build_allele_tables' rows for the model's mutation rate.  Outputs per site: origin[K][4] and hettx[K][4] (Emitter::origin_body;
// either may be null: its stores are skipped), status.  Every variant takes the chrX loop, the fence-free one too (as
// famseq_mutrate does): the allele rows are read through the pass's wave-uniform pointer alx and cost no vector register.
std::string origin_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "origin", "phase by transmission (parental origin per child)", variant, kOriginVariants, site_prior);
  d.chrx_loop = true;  // (variant 0 too: alx, above)
  const std::vector<int> kids = trio_children(m);
  d.outputs = "double *__restrict__ origin_g, double *__restrict__ hettx_g";
  d.more_args = ", const double *__restrict__ al_g";
  d.defines = "#define NKID " + std::to_string(kids.size()) + "\n";
  d.site_decls = "    double *og = origin_g ? origin_g + site * (4 * NKID) : nullptr;\n"
                 "    double *hg = hettx_g ? hettx_g + site * (4 * NKID) : nullptr;\n"
                 "    (void)og; (void)hg;\n";
  d.body = Emitter(m, g, eo).origin_body(kids);
  d.epilogue = fail_block(fill("og", "4 * NKID") + fill("hg", "4 * NKID")) + status_store();
  return lane_shell(m, d);
}

// The allele-frequency kernel: the evidence kernel's rules and shell; the founders' prior is the unknown, so there is one form only.
// Beyond the common arguments: af0_g[n_sites], the start values, and n_iter (0 .. FAMSEQ_MAX_AF_ITER; the host checks, the kernel
// clamps).  Outputs per site: af = q after n_iter steps (8 bytes) and loglik[2] = log10 Z(q) and log10 Z(0) without the reference's
// 1e7 (16 bytes; -inf where the data exclude q = 0, which is a result), status; any may be null.  Status 1: the single posterior's
// rule under the start value's rows; 2: a start value outside [0, 1] (whatever the rows it gives say), a pass's total weight or a
// founder's row sum that is not a positive finite number.  Per-pass state: q, Z(q) and Z(0), three doubles in registers.
std::string af_source(const Model &m, int variant) {
  auto [g, f, eo, d] = begin_side(m, "af", "founder allele frequency by maximum likelihood (EM, a sum pass per step)", variant, kAfVariants, false);
  // the founders' prior is the kernel's own: the emitter reads the lane's pa_<g> / pm_<g> as with site priors, the shell has no
  // prior_g to read
  eo.site_prior = true, d.own_prior = true;
  d.comment += "\n// One step from q: the founders' rows are ((1-q)^2, 2q(1-q), q^2) and, male founders at a chrX site, (1-q, 0, q); with m_f the"
               "\n// marginal of founder f under them, q' = min(sum_f count_f / C, 1), count_f = (m_f1 + 2 m_f2) / (m_f0 + m_f1 + m_f2) (a male"
               "\n// founder at a chrX site: m_f2 / (m_f0 + m_f1 + m_f2)), C = 2 founders (chrX: 2 female founders + male founders), founders in"
               "\n// PED order.  n_iter steps from af0, no early exit: the result is a function of the inputs alone.";
  d.outputs = "double *__restrict__ af_g, double *__restrict__ loglik_g";
  d.more_args = ", const double *__restrict__ af0_g, int n_iter";
  d.defines = "#define MAXIT " + std::to_string(FAMSEQ_MAX_AF_ITER) + "\n";
  d.prologue = clamp_count("n_it_", "n_iter", "MAXIT");
  // the start value's rows, for the single posterior's rule (famseq_hwe_priors' expressions; a pass forms its own the same way)
  d.site_vars =
      "    double af_q = kNaN, af_l0 = kNaN, af_l1 = kNaN;\n"
      "    const double q0_ = af0_g[site];\n"
      "    const bool af_bad = !(q0_ >= 0.0 && q0_ <= 1.0);\n"
      "    const double qs_ = af_bad ? 0.5 : q0_;  // (what the passes of such a site run on: nothing of them is kept)\n"
      "    const bool xs_ = (fl & 2) != 0;\n"
      "    const double p0_ = 1 - q0_;\n"
      "    const double pa_0 = p0_ * p0_, pa_1 = 2 * q0_ * p0_, pa_2 = q0_ * q0_;\n"
      "    const double pm_0 = xs_ ? p0_ : pa_0, pm_1 = xs_ ? 0.0 : pa_1, pm_2 = xs_ ? q0_ : pa_2;\n";
  Emitter e(m, g, eo);
  const std::string digits = std::to_string(e.evidence_scale_digits()) + ".0";
  d.body = e.af_body() +
           "      if (!bn_fail) { af_q = q_; af_l0 = log10(Zq_) - " + digits + "; af_l1 = log10(Z0_) - " + digits + "; }\n";
  d.epilogue = "    if (af_bad || single_fail || bn_fail) af_q = af_l0 = af_l1 = kNaN;\n"
               "    if (af_g) __builtin_nontemporal_store(af_q, af_g + site);\n"
               "    if (loglik_g) {\n"
               "      __builtin_nontemporal_store(af_l0, loglik_g + 2 * site);\n"
               "      __builtin_nontemporal_store(af_l1, loglik_g + 2 * site + 1);\n"
               "    }\n"
               "    if (status_g) status_g[site] = af_bad ? 2 : (single_fail ? 1 : (bn_fail ? 2 : 0));\n";
  return lane_shell(m, d);
}

namespace {

// What a sampling kernel carries in front of its entry: the Philox text (philox_src.h, the one the host exports), a word as a
// uniform in (0, 1), and the decision among three and among nine non-negative terms (Emitter::sample_body).
#define FS_PHILOX_DEF(...) #__VA_ARGS__
const char kPhiloxText[] =
#include "philox_src.h"
    ;
#undef FS_PHILOX_DEF
const char kSampleHelpers[] = R"(
#define FS_U01(x) (((double)(x) + 0.5) * (1.0 / 4294967296.0))
static __device__ __forceinline__ unsigned fs_pick3(double u, double e0, double e1, double e2) {
  const double p1 = e0 + e1, s = p1 + e2, t = u * s;
  const unsigned last = e2 > 0.0 ? 2u : (e1 > 0.0 ? 1u : 0u);
  return t < e0 ? 0u : (t < p1 ? 1u : (t < s ? 2u : last));
}
static __device__ __forceinline__ unsigned fs_pick9(double u, const double *e) {
  double p[9];
  p[0] = e[0];
#pragma unroll
  for (int i = 1; i < 9; ++i) p[i] = p[i - 1] + e[i];
  const double t = u * p[8];
  unsigned pick = 0;
#pragma unroll
  for (int i = 1; i < 9; ++i) pick = e[i] > 0.0 ? (unsigned)i : pick;
#pragma unroll
  for (int i = 8; i >= 0; --i) pick = t < p[i] ? (unsigned)i : pick;  /* the partial sums do not decrease: the first such i */
  return pick;
}
)";

}  // namespace

// The sampling kernel: the MAP kernel's rules.  Beyond the common arguments: seed, site_base (the absolute index of the call's
// first site) and n_draws (1 .. FAMSEQ_MAX_DRAWS; the host checks, the kernel clamps).  Outputs per site: samp_gt[n_draws][N]
// (int8) and samp_post[n_draws] (fp64), status; any may be null.  A total weight that is not a positive finite number fails the
// site (status 2): every genotype -1, every samp_post NaN.
// The rows are stored from the lane as each draw ends — a loop pedigree's draw may be replaced by a later assignment, and K rows
// per lane do not fit a stage in LDS beside the messages — in 32-bit words where a row starts 4-aligned, in bytes otherwise:
// every store lies inside the site's n_draws * N bytes whatever the alignment of samp_gt.
std::string sample_source(const Model &m, int variant, bool site_prior) {
  auto [g, f, eo, d] = begin_side(m, "sample", "exact joint posterior draws (forward filtering, backward sampling)", variant, kSampleVariants, site_prior);
  const int N = m.n_members;
  Emitter e(m, g, eo);
  d.body = e.sample_body();
  const int vp = e.sample_row_doubles() | 1, D = e.sample_decisions();
  // (the factor tables, the rows and what the compiler keeps for itself within the CU's 160 KB)
  if (size_t(d.bt) * vp * sizeof(double) > size_t(150) << 10)
    throw std::runtime_error("sample_source: the messages of " + std::to_string(N) + " members do not fit the lanes' LDS rows");
  d.comment += "\n// Random numbers: Philox4x32-10, key (seed, seed >> 32), counter (i, i >> 32, draw, block), i the site's absolute index."
               "\n// Word w of a draw is element w % 4 of block w / 4; u = (word + 0.5) 2^-32 (one decision resolves 2^-32 of probability)."
               "\n// Decision d of a draw takes word d, d counting in the order the walk is written below: the root of every component, then the"
               "\n// families in reverse message order, in each the other parent or the parent pair, then its remaining children: D = " +
               std::to_string(D) + " words." +
               (g.cut.empty() ? "" : "\n// Assignment as_ of the conditioned members takes word D + as_ for its selection.");
  d.outputs = "signed char *__restrict__ gt_g, double *__restrict__ post_g";
  d.more_args = ", unsigned long seed, long site_base, int n_draws";
  d.defines = "#define NMEM " + std::to_string(N) + "\n#define MAXDRAW " + std::to_string(FAMSEQ_MAX_DRAWS) + "\n#define VP " + std::to_string(vp) +
              "\n#define FS_PHILOX_FN static __device__ __forceinline__\n" + kPhiloxText + "\n" + kSampleHelpers;
  d.shared = "  __shared__ double s_v[BT * VP];  // the member -> family messages of the collect pass, one padded row per lane\n";
  d.prologue = std::string() +
               "  const unsigned key0_ = (unsigned)seed, key1_ = (unsigned)(seed >> 32);\n" + clamp_count("nd_", "n_draws", "MAXDRAW") +
               "  double *const sw = s_v + tid * VP;\n" +
               // Read through a plain pointer.  Under forty members hipcc then turns a read at a genotype of 0..2 into three reads and
               // a select, forwards the stores, and keeps the messages in registers (the row takes no LDS at all); from forty on,
               // where the likelihoods are volatile reads, it leaves them in the row.  Measured against reads forced to LDS through
               // a volatile pointer, as lane_shell reads s_l (FAMSEQ_SAMPLE_ROWS=1, a tuning aid): the compiler's form is faster at
               // every size tried — K = 8 draws of 2 M 32-member sites 1.92 ms against 2.97 (K = 1: 0.44 against 0.66), 10 M
               // ten-member sites 2.35 against 2.46, 8 M trios 0.65 against 0.70 (profiles/sample/rate.txt).
               (env_int("FAMSEQ_SAMPLE_ROWS", 0) != 0
                    ? "  typedef const volatile __attribute__((address_space(3))) double smp_cvd;\n  smp_cvd *const sv = (smp_cvd *)sw;\n"
                    : "  const double *const sv = sw;\n");
  d.site_decls = "    signed char *gg = gt_g ? gt_g + site * nd_ * NMEM : nullptr;\n"
                 "    double *sp_ = post_g ? post_g + site * nd_ : nullptr;\n"
                 "    const unsigned long ai_ = (unsigned long)(site_base + site);\n"
                 "    const unsigned ilo_ = (unsigned)ai_, ihi_ = (unsigned)(ai_ >> 32);\n";
  d.epilogue = fail_block(fill("gg", "nd_ * NMEM", "(signed char)-1") + fill("sp_", "nd_")) + status_store();
  return lane_shell(m, d);
}

namespace {

// famseq_elim's variants 8..11 (the widest pedigrees): lane_shell's form of it, famseq_elim's rules
std::string direct_source(const Model &m, int variant, bool site_prior) {
  // (the fence level is the variant's low two bits: every value is taken)
  auto [g, f, eo, d] = begin_side(m, "elim", "exact sum-product", variant & 3, 4, site_prior);
  const int N = m.n_members;
  // (the comment names the kernel's variant, 8..11, and its form)
  d.comment = describe("exact sum-product", g, std::to_string(variant) + " (rows straight from and to global memory)", site_prior);
  // where the likelihoods live is this kernel's own rule: registers at every size unless asked, LDS rows for the last members
  d.lean = eo.lean = env_int("FAMSEQ_ELIM_LEAN", 0) != 0;  // tuning aid
  // members whose likelihoods live in the lane's LDS row rather than in registers: at four waves per CU a lane has 73 doubles
  // of LDS, 24 members.  Pays from the mid-fifties on, where the scratch it spares outweighs the LDS latency it adds (2 M
  // sites: 48 members 2.37-2.50 -> 2.55-2.59 ms, 64: 4.72-4.91 -> 4.25-4.44, 96: 10.3-10.5 -> 9.07; scratch 1276 -> 956 B at 64)
  const int n_lds = std::max(0, std::min(env_int("FAMSEQ_ELIM_LDSL", N >= 56 ? 24 : 0), N));  // (the variable: a tuning aid)
  d.lds_from = eo.lean_from = d.lean ? N : N - n_lds;
  d.outputs = "double *__restrict__ post_g, double *__restrict__ single_g";
  d.min_waves = std::max(1, env_int("FAMSEQ_ELIM_MINWAVES", 1));  // tuning aid
  d.shortcut = true;
  d.site_decls = "    double *pg = post_g + site * W3;\n"
                 "    double *row = single_g ? single_g + site * W3 : pg;  // where the single posterior goes\n";
  d.after_single =
      fill("row", "W3", "kNaN", "single_fail", 4) +
      // a site that does not take the full computation: its posterior IS the single posterior (family.cpp:793-878) or NaN
      fill("pg", "W3", "row[k]", "single_g && !(full && !single_fail)", 4);
  d.body = Emitter(m, g, eo).body() + fill("pg", "W3", "kNaN", "bn_fail");
  d.epilogue = "    if (status_g) status_g[site] = single_fail ? 1 : (!full ? 0x80 : (bn_fail ? 2 : 0));\n";
  return lane_shell(m, d);
}

std::string sum_product_source(const Model &m, int variant, bool call_mode, bool site_prior) {
  if (variant >= 8 && !call_mode) return direct_source(m, variant, site_prior);  // no LDS staging
  const Graph g = graph_or_throw(m);
  ShellOptions o;
  o.entry = site_prior ? "famseq_elim_prior" : "famseq_elim";
  o.bt = elim_block_threads(m, call_mode);
  o.min_waves = env_int("FAMSEQ_ELIM_MINWAVES", call_mode && m.n_members <= 10 ? 2 : 1);  // (the variable: a tuning aid)
  // From variant 1 on the transmission tables are read through scalar loads (measured: +9 % at 10
  // members where registers are tight, -7 % on the fence-free 5-member kernel, which keeps the LDS table).
  // variant 0: no compiler fences (most overlap between the message blocks; fits small pedigrees),
  //         1: a fence after every family->member message, 2: also after local factors and child
  //         summaries, 3: also between the members of the single posterior
  // Where the likelihoods live during the message passing: re-read from the lane's LDS row at each use (short live ranges:
  // what the narrow pedigrees' kernels want, they run at two or more waves per SIMD), or — registers-first — read once into
  // registers, the row then being the output stage (no q[] array, a tenth of the LDS reads, all of them issued together).
  o.regs_l = call_mode ? std::getenv("FAMSEQ_ELIM_CALL_REGS") != nullptr : variant >= 4;  // (the call path: r = 0 unless the tuning aid says otherwise)
  if (std::getenv("FAMSEQ_ELIM_REGS")) o.regs_l = env_int("FAMSEQ_ELIM_REGS", 0) != 0 && !call_mode;  // tuning aid
  o.call_ct_out = !(call_mode && (variant & 4));
  const int f = variant & 3;  // the fence level
  o.comment = describe("exact sum-product", g,
                       std::to_string(f + (call_mode ? (o.call_ct_out ? 0 : 4) : (o.regs_l ? 4 : 0))) + (o.regs_l ? " (likelihoods in registers)" : "") +
                           (call_mode ? ", call path" : ""),
                       site_prior);
  o.body = Emitter(m, g, emit_options(f, o.regs_l ? "row" : "q", site_prior)).body();
  o.fence_single = f >= 3, o.chrx_loop = f >= 1, o.call_mode = call_mode, o.site_prior = site_prior;
  return kernel_shell(m, o);
}

}  // namespace

std::string elim_source(const Model &m, int variant, bool call_mode) { return sum_product_source(m, variant, call_mode, false); }

// famseq_elim with the founders' prior given per site (famseq_bn_prior_batch): the same shells and the same statements in the
// same order, every founder-prior operand the lane's own pa_<g> / pm_<g> instead of an entry of the model's table.
std::string prior_source(const Model &m, int variant) { return sum_product_source(m, variant, false, true); }

}  // namespace famseq
