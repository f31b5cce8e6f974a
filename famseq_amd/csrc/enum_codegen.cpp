// enum_codegen.cpp — generates the lane-per-site 3^N enumeration kernel for one pedigree.
//
// Same computation as bn_enum_kernel (bn_kernel.hip) and as the reference's odometer
// (/root/reference/src/family.cpp:894-941, :1014-1106): every one of the 3^N joint genotype
// weights 1e7 * prod_m f_m is formed and added to the marginals.  What changes is the mapping:
// here ONE LANE owns a whole site, so there is no cross-lane reduction, no workgroup barrier in
// the hot loop and no per-step table traffic — everything a site needs lives in registers.
//   * "outer" members (ancestors) are walked by ordinary nested loops; the loop digits are the
//     same in every lane, so their table offsets are scalar;
//   * the last <= 6 members in descent order ("unrolled" set U, closed under children) form a
//     fully unrolled block of 3^|U| configurations whose factor tables (indexed by the unrolled
//     parents' digits) are rebuilt in registers once per outer step;
//   * inside the block prefix products are shared level by level; the deepest 2-3 levels (the
//     "super-leaf") are multiplied once per outer step into a table W, and every configuration
//     costs exactly one FMA, prefix * W[c] into the accumulator of its super-leaf digits c; those
//     3^sl accumulators run over the whole site and are summed into the super-leaf members'
//     marginals at the end; the other unrolled members receive block sums (Q) per prefix, the
//     looped ones block totals kept in the lane's LDS row.
//   * where the super-leaf table depends on no prefix digit and a cost model agrees (lane_form), the same step is taken one
//     level further out: the innermost looped member joins the block, prefix tables that mention no loop digit are built once
//     per site into the lane's LDS row, and the prefix members' marginals are formed after the loops (OnceEmitter, "The
//     once-per-site form"): lane variants 4-7 (enum_codegen.h); FAMSEQ_LANE_HOIST=0 keeps the per-prefix text there too.
//   * where a founder and its leaf children can be that super-leaf, with their other parent as the outermost loop, the table mentions
//     one loop digit and is built three times per site (outer_leaf_shape, "The outer-leaf plan"): lane variants 8-11, where a cost
//     model takes it; FAMSEQ_LANE_OUTER=0 keeps the text of 4-7.  Loops are then no longer parents first (BlockPlan::factor_pos).
// BlockPlan holds what is decided about a block shape, row_layout the lane's LDS row per form, Emitter the text both forms
// share; lane_form chooses between PrefixEmitter and OnceEmitter.
// The generic team-per-site kernel remains the fallback (small batches, no compiler at run time).
#include "enum_codegen.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "kernel_shell.h"

namespace famseq {

namespace {

std::string num(int x) { return std::to_string(x); }

struct Shape {
  int N = 0;
  std::vector<int> outer, unrolled;  // both in parents-before-children order (outer: unless loops_as_given)
  std::vector<int> upos;             // member -> level in `unrolled` or -1
  bool loops_as_given = false;       // the outer-leaf plan: `outer` is the loop order, and its first member may enclose its parents
};

int kind_of(const Model &m, int p) {
  const bool male = m.gender[p] == 1;
  return m.mother[p] < 0 ? (male ? 0 : 1) : (male ? 2 : 3);
}

Shape choose_shape(const Model &m, int cap) {
  const int N = m.n_members;
  std::vector<std::vector<int>> kids(N);
  for (int i = 0; i < N; ++i)
    if (m.mother[i] >= 0) {
      kids[m.mother[i]].push_back(i);
      kids[m.father[i]].push_back(i);
    }
  // depth = longest chain of ancestors; sorting by it gives a parents-before-children order
  std::vector<int> depth(N, 0);
  for (int pass = 0; pass < N; ++pass)
    for (int i = 0; i < N; ++i)
      if (m.mother[i] >= 0) depth[i] = std::max(depth[i], 1 + std::max(depth[m.mother[i]], depth[m.father[i]]));
  std::vector<int> order(N);
  for (int i = 0; i < N; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return depth[a] < depth[b]; });
  std::vector<char> inU(N, 0);
  int nu = 0;
  // (four members at most: 60 — two founders and two children of both are 3 + 3 + 27 + 27 — so that a quad is ONE unrolled block of
  // 81 configurations instead of a three-step loop over 27: 0.556 -> 0.512 ms per 8 M sites; five members all unrolled need 120 and
  // run at half the waves, 0.70 -> 0.88)
  const int table_budget = env_int("FAMSEQ_LANE_TABLE_BUDGET", N <= 4 ? 60 : 48);  // (the variable: a tuning aid)
  auto table_doubles = [&]() {
    int t = 0;
    for (int i = 0; i < N; ++i)
      if (inU[i]) {
        int e = 3;
        if (m.mother[i] >= 0) e *= (inU[m.mother[i]] ? 3 : 1) * (inU[m.father[i]] ? 3 : 1);
        t += e;
      }
    return t;
  };
  // children first: a member may join U only when all its children already have
  for (int k = N - 1; k >= 0 && nu < cap; --k) {
    const int i = order[k];
    bool ok = true;
    for (int c : kids[i]) ok = ok && inU[c];
    if (!ok) continue;
    inU[i] = 1;
    if (table_doubles() > table_budget) {  // register budget for the block's factor tables
      inU[i] = 0;
      continue;
    }
    ++nu;
  }
  Shape s;
  s.N = N;
  s.upos.assign(N, -1);
  for (int i : order)
    if (!inU[i]) s.outer.push_back(i);
  // Unrolled members in depth-first order (parents before children, each subtree contiguous):
  // the block sums below a level then depend on as few upper digits as possible.
  std::function<void(int)> place = [&](int i) {
    if (!inU[i] || s.upos[i] >= 0) return;
    if (m.mother[i] >= 0)
      for (int par : {m.mother[i], m.father[i]})
        if (inU[par] && s.upos[par] < 0) return;  // placed later, from its other parent
    s.upos[i] = (int)s.unrolled.size();
    s.unrolled.push_back(i);
    for (int c : kids[i]) place(c);
  };
  for (int i : order) place(i);
  return s;
}

int pow3(int e) {
  int r = 1;
  while (e-- > 0) r *= 3;
  return r;
}

// What a generator of the block has to know about (Model, Shape, fixed), computed once and never changed: the digits the
// block sums depend on, the super-leaf depth, the looped members in loop order and where each level's statements go.
// fixed: the `fixed` outermost looped members do not loop — their digits come from the lane's position in its group
// (fx0, fx1, ...: lanes-per-site mode, 3^fixed lanes share a site).
struct BlockPlan {
  const Model &m;
  const Shape s;
  const int fixed, nu;
  std::vector<std::vector<int>> dep;  // dep[k]: unrolled levels < k whose digits the block sums of levels >= k depend on
  // Super-leaf: the deepest sl levels are walked together.  Their factors are multiplied once per outer step into a
  // combined table W (3^sl entries per combination of the upper digits they depend on), so each of the 3^sl
  // configurations below a prefix costs exactly one FMA and no products are formed inside the block for these levels.
  int sl = 1;
  std::vector<int> outer;    // looped members, outermost first
  std::vector<int> entries;  // doubles in level k's factor table
  // Loop level (index into outer, -1 = before all loops) at which level k's factor table has to be rebuilt — that of its
  // innermost looped parent — and at which its block sums have to be
  std::vector<int> wb, qb;

  BlockPlan(const Model &model, const Shape &shape, int fixed_digits = 0)
      : m(model), s(shape), fixed(fixed_digits), nu((int)shape.unrolled.size()), outer(shape.outer) {
    dep.assign(nu + 1, {});
    for (int k = nu - 1; k >= 0; --k) {
      std::vector<char> in(nu, 0);
      for (int j = k; j < nu; ++j) {
        const int p = s.unrolled[j];
        if (m.mother[p] < 0) continue;
        for (int par : {m.mother[p], m.father[p]})
          if (s.upos[par] >= 0 && s.upos[par] < k) in[s.upos[par]] = 1;
      }
      for (int l = 0; l < k; ++l)
        if (in[l]) dep[k].push_back(l);
    }
    for (int t = std::min(3, nu); t >= 2 && sl == 1; --t) {
      const int d = (int)dep[nu - t].size();
      int doubles = pow3(t + d);
      for (int j = 0; j + 1 < t; ++j) doubles += pow3(j + 1 + d);
      if (doubles <= 45) sl = t;
    }
    for (int k = 0; k < nu; ++k) {
      const int p = s.unrolled[k];
      entries.push_back(m.mother[p] < 0 ? 3 : 3 * (s.upos[m.mother[p]] >= 0 ? 3 : 1) * (s.upos[m.father[p]] >= 0 ? 3 : 1));
    }
    if (!s.loops_as_given) order_outer_loops();
    wb.assign(nu, -1);
    qb.assign(nu + 1, -1);
    for (int k = nu - 1; k >= 0; --k) {
      const int p = s.unrolled[k];
      if (m.mother[p] >= 0)
        for (int par : {m.mother[p], m.father[p]})
          if (s.upos[par] < 0) wb[k] = std::max(wb[k], outer_pos(par));
      qb[k] = std::max(qb[k + 1], wb[k]);
    }
  }

  int np() const { return nu - sl; }  // prefix levels: unrolled levels above the super-leaf
  int outer_pos(int member) const {
    for (size_t k = 0; k < outer.size(); ++k)
      if (outer[k] == member) return (int)k;
    return -1;
  }
  // Loop level at which looped member p's own factor can be formed: the deepest of its own and its parents'.  Its own level,
  // while loops run parents first; in the outer-leaf plan the outermost member's factor waits for its parents' digits.
  int factor_pos(int p) const {
    int k = outer_pos(p);
    if (m.mother[p] >= 0) k = std::max(k, std::max(outer_pos(m.mother[p]), outer_pos(m.father[p])));
    return k;
  }
  int looped_tables() const {  // unrolled members with a looped parent
    return (int)std::count_if(wb.begin(), wb.end(), [](int b) { return b >= 0; });
  }

  // The innermost looped member, if it may join the unrolled block as its outermost prefix level: its digit feeds
  // only factor tables of prefix levels (none of the super-leaf's), another loop remains outside it, and the block
  // stays at seven members.  -1: none.
  int joinable_member() const {
    // (an explicit FAMSEQ_LANE_CAP bounds the block whichever way it grows)
    if ((int)outer.size() - fixed < 2 || nu + 1 > std::min(7, env_int("FAMSEQ_LANE_CAP", 7)) || sl < 2) return -1;
    const int c = outer.back();
    for (int k = np(); k < nu; ++k) {
      const int p = s.unrolled[k];
      if (m.mother[p] >= 0 && (m.mother[p] == c || m.father[p] == c)) return -1;
    }
    return c;
  }

  // The once-per-site form (OnceEmitter) applies where the super-leaf table depends on no prefix digit.
  bool once_applies() const { return fixed == 0 && sl >= 2 && np() >= 1 && dep[np()].empty(); }

 private:
  // The per-step tables are plain expressions of the loop digits, so the compiler hoists each one
  // to the outermost loop whose digit it mentions.  Put the member whose digit feeds the most
  // table entries outermost (among members of equal depth, parents still enclose children).
  void order_outer_loops() {
    const int N = s.N;
    std::vector<int> depth(N, 0), cost(N, 0);
    for (int pass = 0; pass < N; ++pass)
      for (int i = 0; i < N; ++i)
        if (m.mother[i] >= 0) depth[i] = std::max(depth[i], 1 + std::max(depth[m.mother[i]], depth[m.father[i]]));
    for (int o : outer) {
      bool below = false;  // does any level >= k depend on o?
      for (int k = nu - 1; k >= 0; --k) {
        const int p = s.unrolled[k];
        if (m.mother[p] >= 0 && (m.mother[p] == o || m.father[p] == o)) {
          cost[o] += entries[k];
          below = true;
        }
        if (below) cost[o] += pow3((int)dep[k].size());                                       // Q<k>
        if (below && sl >= 2 && k == nu - sl) cost[o] += pow3(sl + (int)dep[k].size()) * 3 / 2;  // W, X
      }
    }
    std::stable_sort(outer.begin(), outer.end(), [&](int a, int b) {
      if (depth[a] != depth[b]) return depth[a] < depth[b];
      return cost[a] > cost[b];
    });
  }
};

// The lane's LDS row, as the body uses it between the single-posterior store and the final write-back: slots 3k.. hold looped
// member k's marginal accumulators; then come, in the per-prefix form, the looped members' likelihoods (all or none) and the
// likelihoods of unrolled members whose tables are rebuilt inside the loops; in the once-per-site form the constant prefix
// tables, those unrolled members' likelihoods and the looped members' own behind them (all or none).
struct RowLayout {
  bool fits = true;  // (once-per-site form) false: no room, or more than two digits in the tables rebuilt per step
  bool l_in_lds = false;
  int lik_base = 0;                            // first slot of the looped members' likelihoods
  std::vector<std::pair<int, int>> lik_slots;  // unrolled member, first of its 3 slots: in the order the body fills them
  std::set<int> before_loops;                  // unrolled members whose tables are built once per site, ahead of all loops
  std::vector<int> tslot;  // prefix level -> first slot of its table, where the table mentions no loop digit ("constant"); else -1
  std::vector<int> D;      // prefix levels whose digits the tables rebuilt per step mention, ascending
};

RowLayout row_layout(const BlockPlan &p, int row_len, bool once) {
  RowLayout L;
  const int no = (int)p.outer.size();
  L.tslot.assign(p.nu, -1);
  int next = 3 * no;
  if (once) {
    std::set<int> d;
    for (int k = 0; k < p.np(); ++k) {
      if (p.wb[k] < 0) {
        L.tslot[k] = next;
        next += p.entries[k];
        continue;
      }
      d.insert(k);
      const int mem = p.s.unrolled[k];
      for (int par : {p.m.mother[mem], p.m.father[mem]})
        if (p.s.upos[par] >= 0) d.insert(p.s.upos[par]);
    }
    if (next > row_len || d.size() > 2) {  // (3^|D| values per step)
      L.fits = false;
      return L;
    }
    L.D.assign(d.begin(), d.end());
  } else {
    L.l_in_lds = 6 * no <= row_len;
    L.lik_base = next;
    next = (L.l_in_lds ? 6 : 3) * no;
  }
  // The unrolled members' likelihoods are needed only where their tables are rebuilt (outer loop levels).  What is left
  // of the row holds them for the members whose tables sit in the deepest loops (read 3^depth times per site: +3 % on
  // ped10), deepest loop first, while there is room.  Either way 6 registers per member stay free for the block.
  std::vector<int> order;
  for (int k = 0; k < p.nu; ++k)
    if (p.wb[k] >= 0) order.push_back(k);
    else L.before_loops.insert(p.s.unrolled[k]);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.wb[a] > p.wb[b]; });
  for (int k : order) {
    if (next + 3 > row_len) break;
    L.lik_slots.push_back({p.s.unrolled[k], next});
    next += 3;
  }
  if (once) {
    L.l_in_lds = next + 3 * no <= row_len;
    L.lik_base = next;
    std::sort(L.lik_slots.begin(), L.lik_slots.end());  // (this form fills them in member order)
  }
  return L;
}

// Lanes-per-site mode, last step (the group's first lane, after the column sums): normalise,
// failure rule (family.cpp:943-954).
std::string reduce_body() {
  std::ostringstream o;
  o << "#pragma unroll 1\n      for (int k = 0; k < W3; k += 3) {\n"
    << "        const double t0 = row[k], t1 = row[k + 1], t2 = row[k + 2];\n"
    << "        const double s = (t0 + t1) + t2; if (s <= 0) bn_fail = true;\n"
    << "        if (s < 1e-290) { asm volatile(\"\" ::: \"memory\"); row[k] = t0 / s; row[k + 1] = t1 / s; row[k + 2] = t2 / s; }\n"
    << "        else { const double r = 1.0 / s; row[k] = t0 * r; row[k + 1] = t1 * r; row[k + 2] = t2 * r; }\n      }\n";
  return o.str();
}

// What both forms of the body are made of: the outer loops with their prefetch, the factor-table statements, the super-leaf
// table and its FMAs, the marginals from the joint accumulators and the row normalisation.  A form supplies the block.
class Emitter {
 public:
  // late: the small-pedigree form — the lane's row keeps the input likelihoods (the shell reads them from
  // LDS and turns them into the single posterior only after this body), so the body's scratch slots live
  // behind them (srow = row + W3) and the normalised marginals go to registers q[] instead of the row
  // scalar_t: the children's transmission entries come from tcx[] (wave-uniform pointer: scalar loads, no LDS
  // instruction, no VGPR) and the founders' priors are folded into their likelihood slots once per site;
  // prefetch 1: the entries the innermost loop's tables need are loaded one step ahead (loop-carried SGPRs), 2: so are
  // that loop's LDS reads — everything the next step's table statements wait for is in flight during this step's block;
  // 0 is the text without any of it
  Emitter(const BlockPlan &plan, const RowLayout &layout, bool late, bool scalar_t, int prefetch)
      : p_(plan), L_(layout), m_(plan.m), s_(plan.s), nu_(plan.nu), sl_(plan.sl), joint_(plan.sl >= 2), fixed_(plan.fixed),
        S_(late ? "srow" : "row"), O_(late ? "q" : "row"), outer_(plan.outer), st_(scalar_t && !plan.outer.empty()),
        pre_(scalar_t && plan.fixed < (int)plan.outer.size() ? prefetch : 0) {}
  virtual ~Emitter() = default;

  std::string body() {
    const int no = (int)outer_.size();
    o_ << "      // outer (looped) members:";
    for (int p : outer_) o_ << " " << p;
    o_ << " | unrolled block:";
    for (int p : s_.unrolled) o_ << " " << p;
    o_ << " (" << pow3(nu_) << " configurations per outer step)\n";
    // The lane's LDS row is idle between the single-posterior store and the final write-back:
    // the looped members' marginal accumulators (touched once per iteration of their own loop)
    // and, when they fit, their likelihoods live there instead of in registers, which keeps the
    // unrolled block free of scratch traffic (RowLayout).
    for (int k = 0; k < no; ++k)
      if (folded(outer_[k]))  // the founder's prior goes into its likelihood once per site (the product the loop would form each time)
        for (int g = 0; g < 3; ++g)
          o_ << "      const double pl" << outer_[k] << "_" << g << " = tcf[" << kind_of(m_, outer_[k]) * 27 + 9 * g << "] * l" << outer_[k] << "_" << g << ";\n";
    for (int k = 0; k < no; ++k)
      for (int g = 0; g < 3; ++g) {
        o_ << "      " << S_ << "[" << 3 * k + g << "] = 0;\n";
        if (L_.l_in_lds) o_ << "      " << S_ << "[" << L_.lik_base + 3 * k + g << "] = " << l_name(outer_[k], g) << ";\n";
      }
    for (const auto &ms : L_.lik_slots)
      for (int g = 0; g < 3; ++g) o_ << "      " << S_ << "[" << ms.second + g << "] = l" << ms.first << "_" << g << ";\n";
    for (int k = 0; k < fixed_; ++k)  // this lane's digits of the members that do not loop
      o_ << "      const int fx" << k << " = (sub / " << pow3(k) << ") % 3;\n";
    for (int k = site_levels_; k < (joint_ ? nu_ - sl_ : nu_); ++k) {
      const int p = s_.unrolled[k];
      o_ << "      double b" << p << "_0 = 0, b" << p << "_1 = 0, b" << p << "_2 = 0;\n";
    }
    std::vector<int> dig(nu_, 0);
    if (joint_)
      for (int c = 0; c < pow3(sl_); ++c) o_ << "      double " << s_name(c, dig) << " = 0;\n";
    o_ << "      const double P_root = 10000000.0;\n";  // family.cpp:911
    tables();
    o_ << bucket_[0];
    before_loops();
    outer_level(0, "P_root", "");
    after_loops();
    for (int k = 0; k < no; ++k)
      o_ << "      const double b" << outer_[k] << "_0 = " << S_ << "[" << 3 * k << "], b" << outer_[k] << "_1 = " << S_ << "[" << 3 * k + 1
         << "], b" << outer_[k] << "_2 = " << S_ << "[" << 3 * k + 2 << "];\n";
    if (joint_)  // the super-leaf members' marginals: sums of the joint accumulators over the other digits
      for (int j = 0; j < sl_; ++j)
        for (int g = 0; g < 3; ++g) {
          std::string e;
          for (int c = 0; c < pow3(sl_); ++c) {
            int cc = c, mine = 0;
            for (int t = sl_ - 1; t >= 0; --t) {
              if (t == j) mine = cc % 3;
              cc /= 3;
            }
            if (mine != g) continue;
            const std::string n = s_name(c, dig);
            e = e.empty() ? n : "(" + e + " + " + n + ")";
          }
          o_ << "      const double b" << s_.unrolled[nu_ - sl_ + j] << "_" << g << " = " << e << ";\n";
        }
    if (fixed_ > 0) {  // this lane's share of the marginals, unnormalised: reduce_body() sums the group's
      for (int p = 0; p < s_.N; ++p)
        for (int g = 0; g < 3; ++g) o_ << "      row[" << 3 * p + g << "] = b" << p << "_" << g << ";\n";
      return o_.str();
    }
    // One division per row and three products (the sums differ from the reference's in their last bits already, by
    // summation order).  A row sum in the subnormal range, whose reciprocal overflows, keeps the three divisions behind
    // a real branch.
    for (int p = 0; p < s_.N; ++p) {
      auto out = [&](int g) { return O_ + "[" + std::to_string(3 * p + g) + "]"; };
      const std::string b = "b" + std::to_string(p);
      o_ << "      { const double s = (" << b << "_0 + " << b << "_1) + " << b << "_2; if (s <= 0) bn_fail = true;\n"
         << "        if (s < 1e-290) { asm volatile(\"\" ::: \"memory\"); " << out(0) << " = " << b << "_0 / s; " << out(1) << " = " << b
         << "_1 / s; " << out(2) << " = " << b << "_2 / s; }\n"
         << "        else { const double r = 1.0 / s; " << out(0) << " = " << b << "_0 * r; " << out(1) << " = " << b << "_1 * r; " << out(2)
         << " = " << b << "_2 * r; } }\n";
    }
    return o_.str();
  }

 protected:
  const BlockPlan &p_;
  const RowLayout &L_;
  const Model &m_;
  const Shape &s_;
  const int nu_, sl_;
  const bool joint_;  // super-leaf marginals from 3^sl joint accumulators (see superleaf())
  const int fixed_;
  const std::string S_, O_;  // the body's scratch array and where the normalised marginals go
  const std::vector<int> &outer_;
  const bool st_;  // see the constructor
  const int pre_;
  int site_levels_ = 0;  // prefix levels that get no accumulators and no block sums per prefix: the form sums them once per site
  std::string prologue_, prefetch_;  // (pre_) before the innermost loop / inside it, between its table statements and the block
  std::map<std::string, std::string> tq_;  // (pre_) table entry (index text with the innermost digit as '@') -> its loop-carried variable
  std::ostringstream o_;
  int uid_ = 0;

  // The unrolled block of one outer step: P the prefix product of the looped members, acc_parent the innermost loop's total.
  virtual void block(const std::string &P, const std::string &acc_parent) = 0;
  virtual void before_loops() {}
  virtual void after_loops() {}
  // an unrolled member's likelihood, where the row has no slot for it and its table is rebuilt inside the loops
  virtual std::string unplaced_likelihood(int p, int g) const = 0;
  // does a loop level read its marginal slot where its step begins (and not where it adds to it)?
  virtual bool slot_read_ahead() const { return false; }
  virtual void claim_carried(const std::string &) {}  // the innermost loop, after the next step's loads have been issued

  // table offset of member p's factor for child genotype expression `gc` ("2" or "g7"): literal
  // part + digits of outer parents (runtime, uniform) — unrolled parents are added by the caller
  // `dm`, `dexpr`: the digit of looped member dm is spelled dexpr instead of g<dm> (the prefetch's next digit)
  std::string t_index(int p, const std::string &gc, int um, int uf, int dm = -1, const std::string &dexpr = "") const {
    auto dig = [&](int q) { return q == dm ? dexpr : "g" + num(q); };
    std::string e = num(kind_of(m_, p) * 27) + " + 9 * " + gc;
    if (m_.mother[p] >= 0) {
      e += um >= 0 ? " + " + num(3 * um) : " + 3 * " + dig(m_.mother[p]);
      e += uf >= 0 ? " + " + num(uf) : " + " + dig(m_.father[p]);
    }
    return e;
  }
  // the table a member's factor entries are read from: the lane's LDS copy (flag-selected: Known picks the founders'
  // priors), or — scalar_t, children only — the wave-uniform pointer of the body's chrX pass
  std::string t_tab(int p) const { return st_ && m_.mother[p] >= 0 ? "tcx" : "tcf"; }
  // founder with its prior folded into the likelihood (scalar_t): pl<p>_<g>, formed once per site
  bool folded(int p) const { return st_ && m_.mother[p] < 0; }
  std::string l_name(int p, int g) const { return (folded(p) && p_.outer_pos(p) >= 0 ? "pl" : "l") + num(p) + "_" + num(g); }
  int inner_pos() const { return (int)outer_.size() - 1; }
  // (pre_) the loop-carried variable holding table entry `idx` ('@' = the innermost looped member's digit): loaded for
  // digit 0 ahead of the innermost loop, for the next digit inside it once this digit's table statements are done
  std::string carried_entry(const std::string &tab, const std::string &idx) {
    const std::string key = tab + "[" + idx + "]";
    auto it = tq_.find(key);
    if (it != tq_.end()) return it->second;
    const std::string v = "tq" + num((int)tq_.size()), gi = "g" + num(outer_[inner_pos()]);
    auto spell = [&](const std::string &d) {
      std::string e = key;
      for (size_t k; (k = e.find('@')) != std::string::npos;) e.replace(k, 1, d);
      return e;
    };
    prologue_ += "            double " + v + " = " + spell("0") + ";\n";
    prefetch_ += "              " + v + " = " + spell(gi + "n") + ";\n";
    tq_[key] = v;
    return v;
  }

  void outer_level(size_t k, const std::string &P, const std::string &acc_parent) {
    if (k == outer_.size()) {
      block(P, acc_parent);
      return;
    }
    const int p = outer_[k];
    const std::string g = "g" + num(p), ind(6 + 2 * k, ' ');
    const std::string lk_g = L_.l_in_lds ? S_ + "[" + num(L_.lik_base + 3 * (int)k) + " + " + g + "]"
                                         : "(" + g + " == 0 ? " + l_name(p, 0) + " : (" + g + " == 1 ? " + l_name(p, 1) + " : " + l_name(p, 2) + "))";
    const bool inner = pre_ > 0 && (int)k == inner_pos();
    const bool carried_l = inner && pre_ >= 2 && L_.l_in_lds;
    const bool early_acc = slot_read_ahead() && !carried_l;
    std::string f_expr = carried_l ? "lq_" : lk_g;
    if (!folded(p) && p_.factor_pos(p) == (int)k)
      f_expr = (inner && m_.mother[p] >= 0 ? carried_entry("tcx", t_index(p, "@", -1, -1, p, "@")) : t_tab(p) + "[" + t_index(p, g, -1, -1) + "]") + " * " + f_expr;
    // (the outer-leaf plan) a member looped outside a parent of its own: its transmission entry joins the product here, where the
    // last digit it mentions is known; its marginal slot is still added to where its own loop's step ends
    for (size_t j = 0; j < k; ++j)
      if (const int q = outer_[j]; m_.mother[q] >= 0 && p_.factor_pos(q) == (int)k)
        f_expr = (inner ? carried_entry("tcx", t_index(q, "g" + num(q), -1, -1, p, "@")) : t_tab(q) + "[" + t_index(q, "g" + num(q), -1, -1) + "]") + " * " + f_expr;
    if (inner) o_ << prologue_;
    if (carried_l)  // this loop's own LDS reads, one step ahead: the member's likelihood, its marginal slot
      o_ << ind << "double lq_ = " << S_ << "[" << L_.lik_base + 3 * (int)k << "], aq_ = " << S_ << "[" << 3 * (int)k << "];\n";
    if ((int)k < fixed_)
      o_ << ind << "{ const int " << g << " = fx" << k << ";  // one digit per lane of the group\n";
    else
      o_ << "#pragma unroll 1\n"  // keep the walk rolled: an unrolled outer loop triples the block's live state
         << ind << "for (int " << g << " = 0; " << g << " < 3; ++" << g << ") {\n";
    o_ << ind << "  const double f" << p << " = " << f_expr << ";\n"
       << ind << "  const double P" << p << " = " << P << " * f" << p << ";\n"
       << ind << "  double acc" << p << " = 0;\n"
       << bucket_[k + 1];
    if (inner) {
      o_ << ind << "  const int " << g << "n = " << g << " < 2 ? " << g << " + 1 : 2;\n" << prefetch_;
      if (carried_l) o_ << ind << "  const double lq_n = " << S_ << "[" << L_.lik_base + 3 * (int)k << " + " << g << "n];\n";
    }
    if (early_acc) o_ << ind << "  const double aq" << p << " = " << S_ << "[" << 3 * (int)k << " + " << g << "];\n";
    if (inner) {
      claim_carried(ind);
      o_ << ind << "  __builtin_amdgcn_sched_barrier(0);\n";
    }
    outer_level(k + 1, "P" + num(p), "acc" + num(p));
    if (carried_l)
      o_ << ind << "  " << S_ << "[" << 3 * (int)k << " + " << g << "] = aq_ + acc" << p << ";\n"
         << ind << "  lq_ = lq_n; aq_ = " << S_ << "[" << 3 * (int)k << " + " << g << "n];\n";
    else if (early_acc)
      o_ << ind << "  " << S_ << "[" << 3 * (int)k << " + " << g << "] = aq" << p << " + acc" << p << ";\n";
    else
      o_ << ind << "  " << S_ << "[" << 3 * (int)k << " + " << g << "] += acc" << p << ";\n";
    if (!acc_parent.empty()) o_ << ind << "  " << acc_parent << " += acc" << p << ";\n";
    o_ << ind << "}\n";
  }

  // name of table entry of unrolled level k for own digit g given the digits of the levels above
  std::string w_name(int k, int g, const std::vector<int> &dig) const {
    const int p = s_.unrolled[k];
    std::string n = "w" + num(p) + "_" + num(g);
    if (m_.mother[p] >= 0) {
      if (s_.upos[m_.mother[p]] >= 0) n += "m" + num(dig[s_.upos[m_.mother[p]]]);
      if (s_.upos[m_.father[p]] >= 0) n += "f" + num(dig[s_.upos[m_.father[p]]]);
    }
    return n;
  }
  std::string sl_name(const char *prefix, int upto, const std::vector<int> &dig) const {  // W / X entry
    const int k0 = nu_ - sl_;
    std::string n = prefix;
    for (int k = k0; k <= upto; ++k) n += "_" + num(dig[k]);
    for (int l : p_.dep[k0]) n += "_" + num(l) + "d" + num(dig[l]);
    return n;
  }
  // joint accumulator of super-leaf configuration c (most significant digit = shallowest member)
  std::string s_name(int c, std::vector<int> &dig) const {
    const int k0 = nu_ - sl_;
    for (int t = sl_ - 1; t >= 0; --t) {
      dig[k0 + t] = c % 3;
      c /= 3;
    }
    std::string n = "S";
    for (int k = k0; k < nu_; ++k) n += "_" + num(dig[k]);
    return n;
  }
  // Q<k>[digits of dep[k]] = sum over the configurations of levels k.. of prod w: the total
  // weight below a node, per unit of prefix.  Q<nu> = 1.
  std::string q_name(int k, const std::vector<int> &dig) const {
    if (k >= nu_) return "1.0";
    std::string n = "Q" + num(k);
    for (int l : p_.dep[k]) n += "_" + num(l) + "d" + num(dig[l]);
    return n;
  }

  // where the block's table statements read unrolled member p's likelihood from
  std::string lk_src(int p, int g) const {
    for (const auto &ms : L_.lik_slots)
      if (ms.first == p) return S_ + "[" + num(ms.second + g) + "]";
    if (L_.before_loops.count(p)) return "l" + num(p) + "_" + num(g);  // used once, ahead of all loops: still in registers
    return unplaced_likelihood(p, g);
  }

  // Table statements, bucketed by the innermost outer loop whose digit they mention
  // (index into outer_, -1 = none): each bucket is emitted at the top of that loop's body, so a
  // table is rebuilt only when a digit it depends on changes.
  std::vector<std::string> bucket_;  // [outer position + 1]

  void tables() {
    const std::string ind = "        ";
    bucket_.assign(outer_.size() + 1, "");
    const std::vector<int> &wb = p_.wb, &qb = p_.qb;
    const int innermost = (int)outer_.size() - 1;
    for (int k = 0; k < nu_; ++k) {
      std::ostringstream o;
      const int p = s_.unrolled[k];
      const bool has = m_.mother[p] >= 0;
      const bool mu = has && s_.upos[m_.mother[p]] >= 0, fu = has && s_.upos[m_.father[p]] >= 0;
      for (int gm = 0; gm < (mu ? 3 : 1); ++gm)
        for (int gf = 0; gf < (fu ? 3 : 1); ++gf) {
          std::string suffix;
          if (mu) suffix += "m" + num(gm);
          if (fu) suffix += "f" + num(gf);
          for (int g = 0; g < 3; ++g) {
            if (L_.tslot[k] >= 0) {  // built once per site, kept in the lane's LDS row
              o << "      " << S_ << "[" << L_.tslot[k] + ((gm * (fu ? 3 : 1) + gf) * 3 + g) << "] = " << t_tab(p) << "["
                << t_index(p, num(g), mu ? gm : -1, fu ? gf : -1) << "] * " << lk_src(p, g) << ";\n";
              continue;
            }
            o << ind << "const double w" << p << "_" << g << suffix << " = ";
            if (pre_ > 0 && has && wb[k] == innermost) {
              // rebuilt in the innermost loop: the entry comes from the variable loaded a step ahead, the likelihood — the
              // same in every step — from a register filled ahead of the loop (prefetch 2) instead of a read per step
              const int pin = outer_[innermost];
              o << carried_entry("tcx", t_index(p, num(g), mu ? gm : -1, fu ? gf : -1, pin, "@")) << " * ";
              const std::string src = lk_src(p, g);
              if (pre_ >= 2 && src.compare(0, S_.size() + 1, S_ + "[") == 0) {
                const std::string v = "lq" + num(p) + "_" + num(g);
                if (prologue_.find(" " + v + " =") == std::string::npos) prologue_ += "            const double " + v + " = " + src + ";\n";
                o << v << ";\n";
              } else {
                o << src << ";\n";
              }
            } else {
              o << t_tab(p) << "[" << t_index(p, num(g), mu ? gm : -1, fu ? gf : -1) << "] * " << lk_src(p, g) << ";\n";
            }
          }
        }
      bucket_[wb[k] + 1] += o.str();
    }
    // block sums, deepest level first
    for (int k = nu_ - 1; k >= site_levels_; --k) {
      std::ostringstream o;
      const int nd = (int)p_.dep[k].size();
      std::vector<int> dig(nu_, 0);
      for (int code = 0; code < pow3(nd); ++code) {
        int c = code;
        for (int l : p_.dep[k]) {
          dig[l] = c % 3;
          c /= 3;
        }
        std::string e;
        for (int g = 0; g < 3; ++g) {
          dig[k] = g;
          const std::string w = w_name(k, g, dig), q = q_name(k + 1, dig);
          if (q == "1.0") e = e.empty() ? w : "(" + e + " + " + w + ")";
          else e = e.empty() ? "(" + w + " * " + q + ")" : "__builtin_fma(" + w + ", " + q + ", " + e + ")";
        }
        o << ind << "const double " << q_name(k, dig) << " = " << e << ";\n";
      }
      bucket_[qb[k] + 1] += o.str();
    }
    if (sl_ < 2) return;
    // super-leaf tables: running products over the sl levels, per combination of the upper digits
    std::ostringstream o;
    const int k0 = nu_ - sl_, nd = (int)p_.dep[k0].size();
    std::vector<int> dig(nu_, 0);
    for (int code = 0; code < pow3(nd); ++code) {
      int c = code;
      for (int l : p_.dep[k0]) {
        dig[l] = c % 3;
        c /= 3;
      }
      std::function<void(int, const std::string &)> walk = [&](int k, const std::string &prod) {
        for (int g = 0; g < 3; ++g) {
          dig[k] = g;
          const std::string w = w_name(k, g, dig);
          std::string here = w;
          if (!prod.empty()) {
            here = sl_name(k == nu_ - 1 ? "W" : "X", k, dig);
            o << ind << "const double " << here << " = " << prod << " * " << w << ";\n";
          }
          if (k < nu_ - 1) walk(k + 1, here);
        }
      };
      walk(k0, "");
    }
    bucket_[qb[k0] + 1] += o.str();
  }

  // Every configuration: ONE FMA — its joint weight prefix * W is formed and added to the
  // accumulator of its super-leaf digits.  The 3^sl accumulators run over the whole site; the
  // marginals of all sl members are sums of them, taken once at the end (body()), and
  // the accumulators form 3^sl independent dependency chains.
  // (No pins here: the prefix products are pinned where they are formed, which is what keeps
  // hipcc from forming all of them up front; a pin per three FMAs cost an s_nop each, -5 %.)
  void superleaf(const std::string &P, std::vector<int> &dig, const std::string &ind) {
    for (int c = 0; c < pow3(sl_); ++c) {
      const std::string a = s_name(c, dig);  // sets dig[k0..]
      o_ << ind << a << " = __builtin_fma(" << P << ", " << sl_name("W", nu_ - 1, dig) << ", " << a << ");\n";
    }
  }

  // Where prefix products are formed the instruction order is pinned (left alone, hipcc forms the
  // products of the whole unrolled tree ahead of their uses and spills) by a scheduling barrier:
  // nothing is moved across, and no instruction is emitted.
  static std::string pin(const std::string &ind) { return ind + "__builtin_amdgcn_sched_barrier(0);\n"; }
};

// The per-prefix form: every prefix level adds prefix * (block sum below) to its member's marginal where the prefix
// product is formed, in every outer step.
class PrefixEmitter : public Emitter {
 public:
  using Emitter::Emitter;

 private:
  // (re-read from the site's own row in global memory: L2 hits)
  std::string unplaced_likelihood(int p, int g) const override { return "lg[" + num(3 * p + g) + "]"; }

  void level(int k, const std::string &P, std::vector<int> &dig, const std::string &ind) {
    const int p = s_.unrolled[k];
    if (sl_ >= 2 && k == nu_ - sl_) {
      superleaf(P, dig, ind);
      return;
    }
    if (k == nu_ - 1) {
      for (int g = 0; g < 3; ++g)
        o_ << ind << "b" << p << "_" << g << " = __builtin_fma(" << P << ", " << w_name(k, g, dig) << ", b" << p << "_" << g
           << ");\n";
      o_ << ind << "asm volatile(\"\" : \"+v\"(b" << p << "_0), \"+v\"(b" << p << "_1), \"+v\"(b" << p << "_2), \"+v\"(" << P
         << "));\n";
      return;
    }
    for (int g = 0; g < 3; ++g) {
      dig[k] = g;
      const std::string pg = "p" + num(uid_++);
      o_ << ind << "double " << pg << " = " << P << " * " << w_name(k, g, dig) << ";\n"
         << ind << "b" << p << "_" << g << " = __builtin_fma(" << pg << ", " << q_name(k + 1, dig) << ", b" << p << "_" << g
         << ");\n"
         << pin(ind);
      level(k + 1, pg, dig, ind);
      o_ << pin(ind);
    }
  }

  void block(const std::string &P, const std::string &acc_parent) override {
    const std::string ind(6 + 2 * outer_.size(), ' '), in2 = ind + "  ";
    std::vector<int> dig(nu_, 0);
    o_ << ind << "{\n" << in2 << "double Pb = " << P << ";\n";
    if (!acc_parent.empty()) o_ << in2 << acc_parent << " += Pb * " << q_name(0, dig) << ";\n";
    level(0, "Pb", dig, in2);
    o_ << ind << "}\n";
  }
};

// The once-per-site form.
// Every weight of an outer step is P x (product of the prefix levels' table entries) x W[c].  Where the
// super-leaf table W depends on no prefix digit (BlockPlan::once_applies), everything but the 3^N configuration
// FMAs factors:
//   * a prefix level whose table mentions no loop digit ("constant": a founder, or a child of unrolled
//     members only) has the same entries in every step: they are formed once per site and chrX pass, kept in
//     the lane's LDS row and read where a prefix product is formed (one group of reads ahead of their use);
//   * the block total of a step is P Q sum_c v_c C_c: Q the sum of W, v_c the product of the tables that ARE
//     rebuilt per step (c: the digits they mention, D), C_c the sum of the constant tables' products over the
//     other prefix digits — taken once per site, ahead of the loops;
//   * the prefix members' marginals need no per-step work beyond U_c += P Q v_c: after the loops one walk of
//     the prefix tree with U_c in the place of the per-step tables yields all of them (site_walk).
// Sums of non-negative terms in the order written here: results differ from the per-prefix form's in their
// last bits and are bit-reproducible.
// It honours prefetch too: 1 the same carried entries, 2 the likelihoods those entries multiply are read ahead of the
// innermost loop and every loop level reads its marginal slot where its step begins (one wave per SIMD: a wait right
// behind its load is time nobody else fills).
class OnceEmitter : public Emitter {
 public:
  OnceEmitter(const BlockPlan &plan, const RowLayout &layout, bool scalar_t, int prefetch)
      : Emitter(plan, layout, false, scalar_t, prefetch), np_(plan.np()), D_(layout.D) {
    if (!layout.fits || !plan.once_applies()) throw std::logic_error("enumeration codegen: the once-per-site form does not fit this shape");
    site_levels_ = np_;
    // read groups: the entries that become known at a node of the prefix tree, in walk order; a group opens only once
    // configuration FMAs lie between it and the one before (the root's entries and the first subtree's are one group)
    std::vector<int> dig(nu_, 0);
    bool work_since = true;
    std::function<void(int)> node = [&](int j) {  // node at level j (-1: the root), its digits in dig
      std::vector<std::pair<int, int>> here;
      for (int k = j + 1; k < np_; ++k)
        if (constant(k) && max_prefix_parent(k) == j)
          for (int g = 0; g < 3; ++g) here.push_back({k, t_off(k, g, dig)});
      if (!here.empty()) {
        if (work_since) {
          consumer_[node_key(j, dig)] = (int)groups_.size();
          groups_.push_back({});
          work_since = false;
        }
        groups_.back().insert(groups_.back().end(), here.begin(), here.end());
      }
      if (j == np_ - 1) {
        work_since = true;
        return;
      }
      for (int g = 0; g < 3; ++g) {
        dig[j + 1] = g;
        node(j + 1);
      }
    };
    node(-1);
  }

 private:
  const int np_;              // prefix levels
  const std::vector<int> &D_;  // prefix levels whose digits the per-step tables mention, ascending
  std::vector<std::vector<std::pair<int, int>>> groups_;  // table entries (level, offset) read together, in walk order
  std::map<std::string, int> consumer_;                   // tree node (its digits; "" = root) below which a group is first used

  bool constant(int k) const { return L_.tslot[k] >= 0; }
  // (this form has the registers: nothing is re-read from global memory)
  std::string unplaced_likelihood(int p, int g) const override { return "l" + num(p) + "_" + num(g); }
  // a level's marginal slot is read where the step begins: the sum at its end waits for nothing
  bool slot_read_ahead() const override { return pre_ >= 2; }
  // The entries loaded a step ahead are claimed here, a table's worth of statements after their issue, by an empty statement
  // that names them — scalar loads return out of order, so while one is in flight every wait inside the block, the counted
  // ones of its read groups too, is for all that is outstanding, the group just requested included.
  void claim_carried(const std::string &ind) override {
    std::vector<std::string> v;
    for (const auto &kv : tq_) v.push_back(kv.second);
    std::sort(v.begin(), v.end(), [](const std::string &a, const std::string &b) { return a.size() != b.size() ? a.size() < b.size() : a < b; });
    for (size_t i = 0; i < v.size(); i += 24) {  // (an asm statement takes thirty operands)
      o_ << ind << "  asm volatile(\"\" ::";
      for (size_t j = i; j < std::min(v.size(), i + 24); ++j) o_ << (j > i ? ", " : " ") << "\"s\"(" << v[j] << ")";
      o_ << ");\n";
    }
  }

  int t_off(int k, int g, const std::vector<int> &dig) const {  // the order tables() writes a level's entries in
    const int p = s_.unrolled[k];
    int o = 0;
    if (m_.mother[p] >= 0) {
      if (s_.upos[m_.mother[p]] >= 0) o = dig[s_.upos[m_.mother[p]]];
      if (s_.upos[m_.father[p]] >= 0) o = 3 * o + dig[s_.upos[m_.father[p]]];
    }
    return 3 * o + g;
  }
  std::string t_var(int k, int off) const { return "t" + num(s_.unrolled[k]) + "_" + num(off); }
  static std::string node_key(int k, const std::vector<int> &dig) {
    std::string n;
    for (int j = 0; j <= k; ++j) n += char('0' + dig[j]);
    return n;
  }
  int dcode(const std::vector<int> &dig) const {
    int c = 0;
    for (size_t i = D_.size(); i-- > 0;) c = 3 * c + dig[D_[i]];
    return c;
  }
  int max_prefix_parent(int k) const {  // deepest prefix level whose digit level k's table mentions, -1: none
    const int p = s_.unrolled[k];
    int j = -1;
    if (m_.mother[p] >= 0)
      for (int par : {m_.mother[p], m_.father[p]}) j = std::max(j, s_.upos[par]);
    return j;
  }

  void fetch_group(int i, const std::string &ind) {
    // (the clobber: these reads are repeated in every step on purpose — left to itself the compiler may keep the
    // tables in registers across the block instead)
    o_ << ind << "asm volatile(\"\" ::: \"memory\");\n";
    for (const auto &e : groups_[i]) o_ << ind << t_var(e.first, e.second) << " = " << S_ << "[" << L_.tslot[e.first] + e.second << "];\n";
  }

  // product of the per-step tables' entries for combination c of the digits in D_ (a table entry, or a new variable)
  std::string step_value(int c, const std::string &ind) {
    std::vector<int> dig(nu_, 0);
    for (int l : D_) {
      dig[l] = c % 3;
      c /= 3;
    }
    std::string v;
    for (int k = 0; k < np_; ++k) {
      if (constant(k)) continue;
      const std::string w = w_name(k, dig[k], dig);
      if (v.empty()) {
        v = w;
        continue;
      }
      const std::string n = "v" + num(uid_++);
      o_ << ind << "const double " << n << " = " << v << " * " << w << ";\n";
      v = n;
    }
    return v.empty() ? "1.0" : v;
  }

  // One walk of the prefix tree over the constant tables (read from the LDS row), outside the loops.
  // final = false: C_c += the product, per combination c of the digits in D_.
  // final = true : U_c joins the product at the deepest level of D_; every prefix member's marginal receives the sum
  //                of the weights below each of its digits (sums of three, level by level).
  void site_walk(bool final) {
    const std::string ind = "      ";
    const int at = D_.empty() ? 0 : D_.back();
    std::vector<int> dig(nu_, 0);
    std::function<std::string(int, const std::string &)> walk = [&](int k, const std::string &P) -> std::string {
      const int p = s_.unrolled[k];
      std::string sub[3];
      for (int g = 0; g < 3; ++g) {
        dig[k] = g;
        std::string cur = P;
        auto times = [&](const std::string &f) {
          if (cur.empty()) {
            cur = f;
            return;
          }
          const std::string n = "h" + num(uid_++);
          o_ << ind << "const double " << n << " = " << cur << " * " << f << ";\n";
          cur = n;
        };
        if (final && k == at) times("U_" + num(dcode(dig)));
        if (constant(k)) times(S_ + "[" + num(L_.tslot[k] + t_off(k, g, dig)) + "]");
        if (k < np_ - 1) sub[g] = walk(k + 1, cur);
        else {
          sub[g] = cur.empty() ? "1.0" : cur;
          if (!final) o_ << ind << "C_" << dcode(dig) << " = C_" << dcode(dig) << " + " << sub[g] << ";\n";
        }
        if (final) o_ << ind << "b" << p << "_" << g << " = b" << p << "_" << g << " + " << sub[g] << ";\n";
      }
      if (!final) return "";
      const std::string n = "h" + num(uid_++);
      o_ << ind << "const double " << n << " = (" << sub[0] << " + " << sub[1] << ") + " << sub[2] << ";\n";
      return n;
    };
    walk(0, "");
  }

  void before_loops() override {
    for (int c = 0; c < pow3((int)D_.size()); ++c) o_ << "      double C_" << c << " = 0, U_" << c << " = 0;\n";
    site_walk(false);
    std::set<std::string> declared;  // (an entry belongs to several groups where its table skips a level's digit)
    for (const auto &grp : groups_)
      for (const auto &e : grp)
        if (declared.insert(t_var(e.first, e.second)).second) o_ << "      double " << t_var(e.first, e.second) << ";\n";
    if (!groups_.empty()) fetch_group(0, "      ");
  }

  void after_loops() override {
    for (int k = 0; k < np_; ++k) {
      const int p = s_.unrolled[k];
      o_ << "      double b" << p << "_0 = 0, b" << p << "_1 = 0, b" << p << "_2 = 0;\n";
    }
    site_walk(true);
  }

  // a prefix level: the product, nothing else — the members' marginals are formed after the loops
  void level(int k, const std::string &P, std::vector<int> &dig, const std::string &ind) {
    if (k == np_) {
      superleaf(P, dig, ind);
      return;
    }
    for (int g = 0; g < 3; ++g) {
      dig[k] = g;
      const std::string pg = "p" + num(uid_++);
      o_ << ind << "double " << pg << " = " << P << " * " << (constant(k) ? t_var(k, t_off(k, g, dig)) : w_name(k, g, dig)) << ";\n" << pin(ind);
      const auto it = consumer_.find(node_key(k, dig));
      if (it != consumer_.end()) fetch_group((it->second + 1) % (int)groups_.size(), ind);
      level(k + 1, pg, dig, ind);
      o_ << pin(ind);
    }
  }

  // The block's total and the prefix members' marginals, once per step: every weight of the step is
  // (P Q) x (product of the prefix tables), Q the sum of the super-leaf table.  The tables built per step
  // enter through v_c (one value per combination c of the digits they mention); the others are the same in
  // every step of the site, so the sums of P Q v_c over the steps (U_c) are all the prefix members need.
  void block(const std::string &P, const std::string &acc_parent) override {
    const std::string ind(6 + 2 * outer_.size(), ' '), in2 = ind + "  ";
    std::vector<int> dig(nu_, 0);
    o_ << ind << "{\n" << in2 << "const double PQ = " << P << " * " << q_name(np_, dig) << ";\n";
    std::string z;
    for (int c = 0; c < pow3((int)D_.size()); ++c) {
      const std::string v = step_value(c, in2);
      o_ << in2 << "U_" << c << " = __builtin_fma(PQ, " << v << ", U_" << c << ");\n";
      z = z.empty() ? "(" + v + " * C_" + num(c) + ")" : "__builtin_fma(" + v + ", C_" + num(c) + ", " + z + ")";
    }
    if (!acc_parent.empty()) o_ << in2 << acc_parent << " += PQ * " << z << ";\n";
    o_ << in2 << "double Pb = " << P << ";\n" << pin(in2);
    if (consumer_.count("")) fetch_group((consumer_[""] + 1) % (int)groups_.size(), in2);
    level(0, "Pb", dig, in2);
    o_ << ind << "}\n";
  }
};

}  // namespace
namespace {

// fp64 statements of a generated body per site, each weighted by 3^(digit loops around it): what the kernel's time follows
// (DESIGN.md 2.1).  Counted from the text: index expressions (in brackets) and integer statements are left out.
double fp64_statements(const std::string &body) {
  double total = 0, weight = 1;
  int depth = 0;
  std::vector<int> loop_depth;
  std::istringstream in(body);
  for (std::string line; std::getline(in, line);) {
    const bool loop = line.find("for (int g") != std::string::npos;
    if (!loop && line.find("int ") == std::string::npos && line.find("asm") == std::string::npos && line.find("//") == std::string::npos) {
      int in_index = 0, ops = 0;
      for (size_t i = 0; i < line.size(); ++i) {
        const char ch = line[i];
        if (ch == '[') ++in_index;
        else if (ch == ']') --in_index;
        else if (in_index == 0 && (ch == '*' || ch == '/' || (ch == '+' && line[i + 1 < line.size() ? i + 1 : i] != '+' && (i == 0 || line[i - 1] != '+')))) ++ops;
        else if (in_index == 0 && line.compare(i, 14, "__builtin_fma(") == 0) ++ops;
      }
      total += ops * weight;
    }
    for (char ch : line) {
      if (ch == '{') {
        ++depth;
      } else if (ch == '}') {
        if (!loop_depth.empty() && loop_depth.back() == depth) {
          loop_depth.pop_back();
          weight /= 3;
        }
        --depth;
      }
    }
    if (loop && line.find('{') != std::string::npos) {  // the loop's own brace was counted just above
      loop_depth.push_back(depth);
      weight *= 3;
    }
  }
  return total;
}

// Doubles per lane (an odd count) that fit in the 160 KB of LDS with `bt` lanes per workgroup and `w` workgroups per CU,
// each workgroup also holding the 432-double transmission table (the call-path form: a byte per member and lane and two
// small tables as well) — and the unrolled members with a looped parent, whose likelihoods want a place there.
struct LdsRoom {
  int fit, looped_tables;
};
LdsRoom lds_room(const BlockPlan &p, int bt, int w, bool call_mode) {
  const int x = (160 * 1024 / w - 432 * 8 - (call_mode ? bt * p.m.n_members + 256 + 2064 : 0)) / (bt * 8);
  return {(x - 1) | 1, p.looped_tables()};
}

// The lane's LDS row: 3N doubles padded to an odd count, plus — while two workgroups per CU still
// fit — room for the likelihoods of unrolled members whose tables are rebuilt inside
// the loops (otherwise re-read from global memory there: L2 misses that show up as HBM traffic).
int lane_row_len(const BlockPlan &p, int bt, bool call_mode) {
  const LdsRoom room = lds_room(p, bt, 2, call_mode);
  const int row_len = (3 * p.m.n_members) | 1, no = (int)p.outer.size();
  const int want = ((6 * no <= row_len ? 6 : 3) * no + 3 * room.looped_tables) | 1;
  return want > row_len ? std::min(want, std::max(row_len, room.fit)) : row_len;
}

// LDS row of the once-per-site form (row_layout): what it would like, cut to what four one-wave workgroups per CU leave;
// 0: not even the output row fits.
int once_row_len(const BlockPlan &p, int bt) {
  int want = 6 * (int)p.outer.size();
  for (int k = 0; k < p.nu; ++k) want += p.wb[k] >= 0 ? 3 : p.entries[k];
  const int w3 = 3 * p.m.n_members, fit = lds_room(p, bt, 4, false).fit;
  return fit < (w3 | 1) ? 0 : std::min(std::max(want, w3) | 1, fit);
}

struct LaneForm {
  bool once = false, late = false, outer_leaf = false;
  Shape shape;  // of the form taken
  int row_len = 0;
  bool scalar_t = false;
  std::string body;                       // (empty where it was not asked for and the cost model did not need it)
  double fp64_parent = 0, fp64_once = 0;  // the cost model's counts (once: 0 where the form does not apply)
  double fp64_outer = 0;                  // ... and the outer-leaf plan's (0 where it does not apply or was not asked for)
};

// The outer-leaf plan (lane variants 8-11): the once-per-site form cut elsewhere.  Where a founder f has one or two children, all
// leaves and all by the same other parent r, the super-leaf table of {f, children} mentions one digit outside itself, r's.
// With r the OUTERMOST loop the table is built three times per site instead of once per step; everything else is the
// once-per-site form as it is.  r then encloses its own parents' loops: its factor joins the product at the innermost of their
// levels (BlockPlan::factor_pos).  From the once-per-site form's shape `h`: r first in the loops, f and its children last in
// the block, every other member where it was.  false: no such cut at f.
bool outer_leaf_shape(const Model &m, const Shape &h, int f, Shape *out) {
  const int N = m.n_members;
  if (m.mother[f] >= 0) return false;
  std::vector<int> kids;
  int r = -1;
  for (int i = 0; i < N; ++i) {
    if (m.mother[i] < 0 || (m.mother[i] != f && m.father[i] != f)) continue;
    const int other = m.mother[i] == f ? m.father[i] : m.mother[i];
    if (r >= 0 && other != r) return false;
    r = other;
    kids.push_back(i);
  }
  if (kids.empty() || kids.size() > 2 || r == f) return false;
  std::vector<char> leaf(N, 0), looped(N, 0);
  leaf[f] = 1;
  for (int c : kids) leaf[c] = 1;
  for (int i = 0; i < N; ++i)
    if (m.mother[i] >= 0 && (std::count(kids.begin(), kids.end(), m.mother[i]) || std::count(kids.begin(), kids.end(), m.father[i]))) return false;
  Shape s;
  s.N = N, s.loops_as_given = true;
  s.outer.push_back(r);
  for (int p : h.outer)
    if (p != r && !leaf[p]) s.outer.push_back(p);
  for (int p : h.unrolled)
    if (p != r && !leaf[p]) s.unrolled.push_back(p);
  s.unrolled.push_back(f);
  s.unrolled.insert(s.unrolled.end(), kids.begin(), kids.end());
  if (s.unrolled.size() > 7 || s.outer.size() < 2) return false;
  for (int p : s.outer) looped[p] = 1;
  for (int p : s.outer)  // a looped member's factor mentions loop digits only
    if (m.mother[p] >= 0 && !(looped[m.mother[p]] && looped[m.father[p]])) return false;
  s.upos.assign(N, -1);
  for (size_t k = 0; k < s.unrolled.size(); ++k) s.upos[s.unrolled[k]] = (int)k;
  *out = s;
  return true;
}

// Shape, form, row length and body of the one-lane-per-site kernel (group_digits = 0) for the block shape `s`.
// may_once (variants 4-7, not the call path: that form keeps the per-prefix text, and its posteriors differ from the
// once-per-site form's in their last bits): the once-per-site form (OnceEmitter) where it applies, fits four workgroups
// per CU and executes fewer fp64 statements per site than the per-prefix form; FAMSEQ_LANE_HOIST=0 (tuning aid) keeps the latter.
// may_outer (variants 8-11): beyond that, the outer-leaf plan where it applies and the cost model takes it (below).
LaneForm lane_form(const Model &m, const Shape &s, bool call_mode, bool may_once, bool need_body = true, bool may_outer = false) {
  LaneForm f;
  f.shape = s;
  if (s.unrolled.empty()) return f;
  const int bt = enumgen_block_threads(m, 0), no = (int)s.outer.size();
  const BlockPlan plan(m, s);
  f.row_len = lane_row_len(plan, bt, call_mode);
  const int prefetch = env_int("FAMSEQ_LANE_PRE", 2);  // tuning aid: 0 none, 1 table entries, 2 and LDS reads (both forms: see Emitter)
  // An experiment that is OFF (FAMSEQ_LANE_LATE=1 turns it on): the sum-product kernel's order of phases for
  // the enumeration too — the whole computation first (marginals to registers), the next chunk requested,
  // then the two outputs — instead of single posterior / store / enumeration / store: one barrier fewer and
  // the prefetch in flight through both output phases; the row keeps the likelihoods until the end, scratch
  // slots follow them.  Measured slower (8 M sites, tools/kernel_bench, two runs): trio 0.368-0.374 -> 0.385-0.392 ms,
  // quad 0.604-0.613 -> 0.640-0.655, 5 members 0.805-0.816 -> 0.827-0.829 (identical binaries differ by +-4 %
  // between runs on these boxes).
  if (env_int("FAMSEQ_LANE_LATE", 0) != 0) {  // tuning aid
    const LdsRoom room = lds_room(plan, bt, 2, call_mode);
    const int w3 = 3 * m.n_members, behind = room.fit - w3;
    if (behind >= 3 * no) {  // (else not even the looped members' accumulators fit behind the row)
      const int scratch_len = std::min(behind, (6 * no <= behind ? 6 : 3) * no + 3 * room.looped_tables);
      f.late = true, f.row_len = (w3 + scratch_len) | 1;
      const RowLayout layout = row_layout(plan, std::max(scratch_len, 1), false);
      f.body = PrefixEmitter(plan, layout, true, false, prefetch).body();
      return f;
    }
  }
  // Transmission entries through scalar loads, and the innermost loop's loads one step ahead (see Emitter): the one-lane-per-site
  // forms of pedigrees that have looped members; the lanes-per-site forms keep the per-lane LDS table.  Round 3, measured
  // with tools/kernel_bench on one box (profiles/r03a/exp_scalar_tables.txt): ten members 10.40 -> 10.13-10.20 ms per 4 M sites,
  // fifteen 139.2 -> 138.4 ms per 262 k; the innermost loop loses 36 of its 39 LDS reads and 10 of its 11 waits (885 -> 881
  // instructions per 729 configurations) — the waits were a small part of what one wave per SIMD loses: at 1.21 instructions
  // per configuration in that loop and 1.33 overall the kernel runs at the issue rate a single wave sustains.
  f.scalar_t = env_int("FAMSEQ_LANE_ST", 1) != 0 && no > 0;  // (the variable: a tuning aid)
  may_once = may_once && f.scalar_t && env_int("FAMSEQ_LANE_HOIST", 1) != 0;
  if (need_body || may_once) {
    const RowLayout layout = row_layout(plan, f.row_len, false);
    f.body = PrefixEmitter(plan, layout, false, f.scalar_t, prefetch).body();
  }
  if (!may_once) return f;
  f.fp64_parent = fp64_statements(f.body);
  Shape h = s;
  if (const int join = plan.joinable_member(); join >= 0) {  // part 1: the innermost looped member becomes the block's outermost prefix level
    h.outer.clear();
    for (int p : plan.outer)
      if (p != join) h.outer.push_back(p);
    h.unrolled.insert(h.unrolled.begin(), join);
    for (size_t k = 0; k < h.unrolled.size(); ++k) h.upos[h.unrolled[k]] = (int)k;
  }
  const BlockPlan hplan(m, h);
  const int hrow = hplan.once_applies() ? once_row_len(hplan, bt) : 0;
  if (hrow == 0) return f;
  const RowLayout hlayout = row_layout(hplan, hrow, true);
  if (!hlayout.fits) return f;
  std::string body = OnceEmitter(hplan, hlayout, f.scalar_t, prefetch).body();
  f.fp64_once = fp64_statements(body);
  if (f.fp64_once >= f.fp64_parent) return f;
  f.once = true, f.shape = h, f.row_len = hrow, f.body = std::move(body);
  if (!may_outer || env_int("FAMSEQ_LANE_OUTER", 1) == 0) return f;  // (the variable: a tuning aid; 0 keeps the once-per-site text)
  // The outer-leaf plan: every founder that allows the cut is a candidate; the lowest count wins, on a tie the lowest founder.
  // Taken only where it executes at least 1 % fewer fp64 statements than the once-per-site form: below that a second text,
  // with last bits of its own, is not worth having (a condition, not a prediction).
  LaneForm best;
  for (int fo = 0; fo < m.n_members; ++fo) {
    Shape c;
    if (!outer_leaf_shape(m, h, fo, &c)) continue;
    const BlockPlan cplan(m, c);
    // the super-leaf is the founder and its children, and its table mentions the outermost loop digit and no other
    if (!cplan.once_applies() || cplan.qb[cplan.np()] != 0 || cplan.s.unrolled[cplan.np()] != fo) continue;
    const int crow = once_row_len(cplan, bt);
    if (crow == 0) continue;
    const RowLayout clayout = row_layout(cplan, crow, true);
    if (!clayout.fits) continue;
    std::string cbody = OnceEmitter(cplan, clayout, f.scalar_t, prefetch).body();
    const double count = fp64_statements(cbody);
    if (best.fp64_outer > 0 && count >= best.fp64_outer) continue;
    best.fp64_outer = count, best.shape = c, best.row_len = crow, best.body = std::move(cbody);
  }
  if (best.fp64_outer <= 0) return f;
  f.fp64_outer = best.fp64_outer;
  if (best.fp64_outer > 0.99 * f.fp64_once) return f;
  f.outer_leaf = true, f.shape = best.shape, f.row_len = best.row_len, f.body = std::move(best.body);
  return f;
}

Shape variant_shape(const Model &m, const LaneVariant &v) { return choose_shape(m, env_int("FAMSEQ_LANE_CAP", v.cap)); }  // (the variable: a tuning aid)

}  // namespace

LaneVariant enumgen_variant(int variant, int group_digits) {
  LaneVariant v;
  v.once = variant >= 4 && group_digits == 0;
  v.outer_leaf = variant >= 8 && group_digits == 0;
  v.plain = variant < 0 ? variant : variant & 3;
  v.cap = group_digits == 0 && (v.plain == 0 || v.plain == 1) ? 7 : 6;
  v.fence_single = v.plain > 0 && (v.plain & 1);
  return v;
}

std::string enumgen_describe(const Model &m, int variant) {
  const LaneVariant v = enumgen_variant(variant);
  const LaneForm f = lane_form(m, variant_shape(m, v), false, v.once, /*need_body=*/false, v.outer_leaf);
  std::string d = "looped members [";
  for (size_t k = 0; k < f.shape.outer.size(); ++k) d += (k ? " " : "") + num(f.shape.outer[k]);
  d += "], unrolled block [";
  for (size_t k = 0; k < f.shape.unrolled.size(); ++k) d += (k ? " " : "") + num(f.shape.unrolled[k]);
  d += "] = " + num(pow3((int)f.shape.unrolled.size())) + " configurations per step";
  if (f.once) {
    char buf[160];
    std::snprintf(buf, sizeof buf, ", prefix tables and marginals once per site (%.0f fp64 statements per site against %.0f)", f.fp64_once,
                  f.fp64_parent);
    d += buf;
  }
  if (f.outer_leaf) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "; outer-leaf plan: the super-leaf table once per step of member %d's loop (%.0f fp64 statements per site against %.0f)",
                  f.shape.outer[0], f.fp64_outer, f.fp64_once);
    d += buf;
  }
  return d;
}

// One lane per site: workgroups of ONE wave, and no register cap (`__launch_bounds__(64, 1)`).  A wave that
// shares its workgroup with nobody waits at no real barrier, so the waves of a CU drift apart and one's memory phases
// overlap another's arithmetic (five members 0.724 -> 0.683 ms per 8 M sites, quads 0.570 -> 0.537); and where the
// arithmetic needs more than 256 registers the compiler now takes one wave per SIMD with its overflow in AGPRs —
// the ten-member kernel: 24 of them instead of 108 bytes of scratch per lane, an LDS row of 43 instead of 37 doubles
// (a quarter of the lanes per CU: no likelihood is re-read from global memory any more), 10.21 -> 9.78 ms per 4 M sites
// (profiles/r02c/exp_block_sizes_*.txt).  The lanes-per-site forms keep wide workgroups: a site's 81 lanes span waves.
int enumgen_block_threads(const Model &m, int group_digits) {
  return env_int("FAMSEQ_LANE_BT", group_digits == 0 ? 64 : (m.n_members <= 10 ? 256 : 128));  // (the variable: a tuning aid)
}

// (asked of the call-path form: its LDS row has less room than the plain form's, so it may re-read members
// the plain form keeps in LDS — and it is the form that can be fed packed PLs, with no fp64 rows to read)
bool enumgen_reads_global_rows(const Model &m, int variant) {
  return enumgen_source(m, variant, 0, /*call_mode=*/true).find("lg[") != std::string::npos;
}

int enumgen_max_group_digits(const Model &m) {
  return std::min<int>(kEnumMaxGroupDigits, (int)variant_shape(m, enumgen_variant(0, 1)).outer.size());
}

int enumgen_sites_per_chunk(const Model &m, int group_digits) { return enumgen_block_threads(m, group_digits) / pow3(group_digits); }

namespace {

// Shell of the lanes-per-site mode (small batches): G = 3^d consecutive lanes share a site, each
// walks the digits (fx0, fx1, ...) of the d outermost looped members given by its position in the
// group, i.e. 1/G of the enumeration; the partial marginals meet in the lanes' LDS rows, the group
// adds them column by column in lane order, its first lane normalises and applies the failure rule.  A site's
// latency drops by G and G times as many lanes are busy, which is what a batch too small to give
// every lane of the chip a site of its own needs (one lane per site: 0.17 ms for anything up to 131 k
// 10-member sites).  I/O is a plain strided walk — this shell never sees a large batch.
std::string grouped_shell(const Model &m, const std::string &comment, const std::string &body, const std::string &reduce,
                          int bt, int min_waves, bool fence_single, int row_doubles, int group) {
  const int N = m.n_members, W3 = 3 * N, ROW = (row_doubles > 0 ? row_doubles : W3) | 1;
  std::ostringstream s;
  s << source_head(m, comment, bt, ROW, "#define G " + std::to_string(group) + "\n#define SPC (BT / G)\n")
    // rows of the groups' first lanes -> global, coalesced
    << "#define STAGE_OUT(Gp) { double *g_ = (Gp) + site0 * W3; \\\n"
    << "  for (int e = tid; e < ns * W3; e += BT) { const int s_ = e / W3; g_[e] = s_io[s_ * G * ROW + (e - s_ * W3)]; } }\n"
    << kernel_signature("famseq_enum_lane", min_waves, "double *__restrict__ post_g, double *__restrict__ single_g")
    << "  __shared__ double s_io[BT * ROW];  // one padded row per lane\n"
    << "  __shared__ double s_tc[432];\n"
    << "  const int tid = threadIdx.x;\n"
    << "  for (int i = tid; i < 432; i += BT) s_tc[i] = tc_g[i];\n"
    << "  const int sidx = tid / G, sub = tid - sidx * G;  // site within the chunk, lane within the group\n"
    << "  const long chunks = (n_sites + SPC - 1) / SPC;\n"
    << chunk_range("  // q or q + 1 chunks each: no idle workgroup")
    << "  const double kNaN = __builtin_nan(\"\");\n"
    << "  double *row = s_io + tid * ROW;\n"
    << "  for (long ch = c_lo; ch < c_hi; ++ch) {\n"
    << "    const long site0 = ch * SPC;\n"
    << "    const int ns = n_sites - site0 < SPC ? (int)(n_sites - site0) : SPC;\n"
    << "    const bool act = sidx < ns;  // lanes beyond the chunk's sites compute on its first site and store nothing\n"
    << "    const long site = site0 + (act ? sidx : 0);\n"
    << "    const double *lg = lk_g + site * W3;\n"
    << "    LDS_BARRIER();  // the previous chunk's rows have been stored; the table is in LDS\n"
    << "    const int fl = flags_g ? (flags_g[site] & 3) : 0;\n"
    << "    const double *tcf = s_tc + fl * 108;\n"
    << "    bool single_fail = false, full = false, bn_fail = false;\n";
  for (int p = 0; p < N; ++p)
    for (int gt = 0; gt < 3; ++gt) s << "    const double l" << p << "_" << gt << " = lg[" << 3 * p + gt << "];\n";
  SingleOptions so;
  so.fence = fence_single;
  s << single_posterior_statements(m, so)
    << "    if (!act) full = false;\n"
    << "    if (single_fail) for (int k = 0; k < W3; ++k) row[k] = kNaN;\n"
    << "    LDS_BARRIER();\n"
    << "    if (single_g) { STAGE_OUT(single_g); }\n"
    << "    LDS_BARRIER();  // single rows are stored; sites that need the full computation overwrite theirs\n"
    << "    if (full && !single_fail) {\n"
    << body
    << "    }\n"
    << "    LDS_BARRIER();  // every lane's share of the marginals is in its row\n"
    // column sums over the group's rows, the columns dealt round the group's lanes (3N / G + 1 of them
    // each), every column in lane order 0..G-1 (bit-reproducible); the sums land in the first lane's row
    << "    if (full && !single_fail) {\n"
    << "      double *lead = row - sub * ROW;\n"
    << "#pragma unroll 1\n"
    << "      for (int k = sub; k < W3; k += G) {\n"
    << "        double t = lead[k];\n"
    << "#pragma unroll 1\n"
    << "        for (int j = 1; j < G; ++j) t += lead[j * ROW + k];\n"
    << "        lead[k] = t;\n      }\n    }\n"
    << "    LDS_BARRIER();\n"
    << "    if (full && !single_fail && sub == 0) {\n"
    << reduce
    << "      if (bn_fail) for (int k = 0; k < W3; ++k) row[k] = kNaN;\n"
    << "    }\n"
    << "    LDS_BARRIER();\n"
    << "    STAGE_OUT(post_g);\n"
    << "    if (status_g && act && sub == 0) status_g[site] = single_fail ? 1 : (!full ? 0x80 : (bn_fail ? 2 : 0));\n"
    << "  }\n}\n";
  return s.str();
}

}  // namespace

bool enumgen_has_once_form(const Model &m) {
  for (int v : {4, 6})  // the 7-member cap and the 6-member cap
    if (lane_form(m, variant_shape(m, enumgen_variant(v)), false, true, /*need_body=*/false).once) return true;
  return false;
}

bool enumgen_has_outer_leaf(const Model &m, int variant) {
  const LaneVariant v = enumgen_variant(8 + (variant & 3));
  return lane_form(m, variant_shape(m, v), false, true, /*need_body=*/false, true).outer_leaf;
}

std::string enumgen_source(const Model &m, int variant_asked, int group_digits, bool call_mode, bool call_ct_out) {
  // variants 4-7: variants 0-3 with the block's prefix levels in the once-per-site form, where the cost model takes it (lane_form);
  // where it does not — and in the lanes-per-site forms — they are the text of 0-3; variants 8-11: 4-7 in the outer-leaf plan
  // under the same rule
  const LaneVariant v = enumgen_variant(variant_asked, group_digits);
  const Shape s = variant_shape(m, v);
  if (s.unrolled.empty()) throw std::runtime_error("enumeration codegen: empty unrolled set");
  if (group_digits < 0 || group_digits > std::min<int>(kEnumMaxGroupDigits, (int)s.outer.size()))
    throw std::runtime_error("enumeration codegen: more group digits than looped members");
  const int bt = enumgen_block_threads(m, group_digits), group = pow3(group_digits);
  // (the call-path form of a small pedigree's kernel: two waves per SIMD at least — with 512 registers to fill, its output stages'
  // batched loads took the five-member kernel from two waves to one, 0.156 -> 0.203 ms per 1 M sites; bounded, the variant
  // contest sees the spill and takes the leaner stage-out)
  const int min_waves = env_int("FAMSEQ_LANE_MINWAVES", group_digits == 0 ? (call_mode && m.n_members <= 6 ? 2 : 1) : bt / 128);  // tuning aid
  if (group > 1) {
    if (call_mode) throw std::runtime_error("enumeration codegen: the lanes-per-site form has no call path");
    const std::string what = "3^N enumeration, " + std::to_string(group) + " lanes per site (" + std::to_string(group_digits) + " of " +
                             std::to_string(s.outer.size()) + " looped members' digits on lanes), " + std::to_string(s.unrolled.size()) +
                             " unrolled members, variant " + std::to_string(v.plain);
    const BlockPlan plan(m, s, group_digits);
    const int row_len = lane_row_len(plan, bt, false);
    const RowLayout layout = row_layout(plan, row_len, false);
    const std::string body = PrefixEmitter(plan, layout, false, false, 0).body();
    return grouped_shell(m, what, body, reduce_body(), bt, min_waves, v.fence_single, row_len, group);
  }
  LaneForm f = lane_form(m, s, call_mode, v.once && !call_mode, true, v.outer_leaf && !call_mode);
  ShellOptions o;
  o.entry = "famseq_enum_lane";
  o.comment = "3^N enumeration, lane per site, " + std::to_string(f.shape.outer.size()) + " looped + " + std::to_string(f.shape.unrolled.size()) +
              " unrolled members, variant " + std::to_string(f.outer_leaf ? variant_asked : f.once ? 4 + v.plain : v.plain);
  if (f.once) o.comment += ", prefix tables and marginals once per site";
  if (f.outer_leaf) o.comment += ", super-leaf table once per step of the outermost loop (member " + std::to_string(f.shape.outer[0]) + ")";
  if (f.shape.unrolled.size() > s.unrolled.size()) o.comment += " (looped member " + std::to_string(f.shape.unrolled[0]) + " unrolled ahead of the block)";
  if (call_mode) o.comment += ", call path";
  if (f.late) o.comment += ", compute-first shell";
  o.body = std::move(f.body);
  o.bt = bt, o.min_waves = min_waves, o.row_doubles = f.row_len;
  // registers-first (LDS-resident likelihoods measured 17 % slower) unless the late experiment asks for the shell's compute-first flow
  o.regs_l = !f.late, o.lane_body = f.late;
  // variant 0: the members of the single posterior overlap, 1: fenced one from the other (fewer registers)
  o.fence_single = v.fence_single, o.chrx_loop = f.scalar_t, o.call_mode = call_mode, o.call_ct_out = call_ct_out;
  return kernel_shell(m, o);
}

}  // namespace famseq
