// enum_codegen.h — source generator of the lane-per-site 3^N enumeration kernel.
#ifndef FAMSEQ_ENUM_CODEGEN_H_
#define FAMSEQ_ENUM_CODEGEN_H_

#include <string>

#include "famseq_hip.h"
#include "model.h"

namespace famseq {

// HIP source of `extern "C" __global__ famseq_enum_lane(lk, flags, post, single, status, n_sites, tc, lc)`.
// Variants of the one-lane-per-site kernel, tried in this order by jit_pick_variant (the first that does not
// spill wins, else the one that spills least): 0, 1 = a 7-member unrolled block (2187 configurations per outer
// step: fewer table rebuilds; measured +1.9 % at 15 members, where it does not spill; at 10 members it spills
// more than the 6-member block and loses the pick), 2, 3 = a 6-member block; odd = the members of the single
// posterior fenced one from the other (fewer registers).  The lanes-per-site forms always use the 6-member block.
// 4-7 = 0-3 with the block's prefix tables and marginals formed once per site (enum_codegen.cpp, "The once-per-site form"),
// for the pedigrees on which the generator's cost model takes that form; for every other pedigree they are the text of 0-3.
// Where the form exists the contest starts at 4 (enumgen_first_variant).
// 8-11 = 4-7 in the outer-leaf plan (enum_codegen.cpp, outer_leaf_shape): a founder and its children as the super-leaf, their
// other parent as the outermost loop, so that the super-leaf table is built three times per site; for every pedigree without such
// a cut, or where the cost model does not take it, they are the text of 4-7.  No contest ranges over them (kEnumContestVariants):
// they serve large one-lane-per-site batches through a slot of their own (kernels.cpp, K_LANE_BULK), or an explicit pick.
constexpr int kEnumVariants = 12;
constexpr int kEnumContestVariants = 8;
// What a variant index means (the one decoder): the block's member cap, whether the single posterior is fenced, whether the
// once-per-site form is asked for, whether the outer-leaf plan is, and the index without that request (0-3; -1, no variant chosen yet: the 6-member form).
struct LaneVariant {
  int plain, cap;
  bool fence_single, once, outer_leaf;
};
LaneVariant enumgen_variant(int variant, int group_digits = 0);
// The call-path kernel has variants 0-3 only (it keeps the per-prefix text): the one with plain variant `lane`'s block shape.
inline int enumgen_call_variant(int lane, bool fence_single) { return (enumgen_variant(lane < 0 ? 0 : lane).plain & 2) + (fence_single ? 1 : 0); }
// group_digits = d > 0: lanes-per-site mode for small batches — 3^d consecutive lanes share a site, each
// taking one combination of the d outermost looped members' digits (d <= enumgen_max_group_digits)
constexpr int kEnumMaxGroupDigits = 4;
// call_ct_out (call path only): the stage-out walk with the row width as a constant (see kElimCallVariants)
std::string enumgen_source(const Model &m, int variant, int group_digits = 0, bool call_mode = false, bool call_ct_out = true);
bool enumgen_has_once_form(const Model &m);  // does any of variants 4-7 differ from 0-3 for this pedigree?
inline int enumgen_first_variant(const Model &m) { return enumgen_has_once_form(m) ? 4 : 0; }
// Does variant 8 + b differ from 4 + b (b = variant & 3) for this pedigree: has the outer-leaf plan been taken for that block shape?
bool enumgen_has_outer_leaf(const Model &m, int variant);
int enumgen_max_group_digits(const Model &m);
// true when the call-path form of the one-lane-per-site kernel re-reads some members' likelihoods from the
// fp64 rows in global memory inside its loops (wide pedigrees whose LDS row cannot hold them): such a kernel
// must be given fp64 input (lk_g non-null), never packed PLs
bool enumgen_reads_global_rows(const Model &m, int variant);
int enumgen_sites_per_chunk(const Model &m, int group_digits);  // sites a workgroup handles per chunk
int enumgen_block_threads(const Model &m, int group_digits = 0);
// One-line description of the lane kernel's tiling (which members are looped / unrolled).
std::string enumgen_describe(const Model &m, int variant = -1);  // shape of the one-lane-per-site kernel of that variant

}  // namespace famseq
#endif
