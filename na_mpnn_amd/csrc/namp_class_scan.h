// Class scan (namp_class_mutations, include/namp.h): the group scan of namp_group_scan.h with the combine of the tied
// score (tied_combine_kernel, namp_tied.h) — the members of a unit speak through CLASS TABLES, so a unit may be a base pair, a wobble
// pair, a group with token maps or a pair joined with symmetry groups.  Everything in front of the units is the group scan's as it
// stands: the tied base stream of S, the plan on the keys, the items with edge kinds (a member's token comes from the variant through
// mut_token; edge kinds do not depend on tables), the whole-row head, the unit kernels.  What is new is their Combine.  With row_t the member's log_softmax
// row (the variant's where it has one in U_3(site), else the base row), C_t its table and b the bias of the LAST listed member's table,
//   total[c] = sum over the members t, listed order, of weight_t * row_t[C_t[c]]  +  b[c]     (classes c < n_classes every member has
//              a token for, else -inf; every product and sum rounded once, from 0)
//   clp = log_softmax(total);   unit = logsumexp of clp[c] over {c : C_t[c] == token of member t, for every t}, -inf if there is none
// and a member's token is the variant's where the site holds it, else S.  class_unit_row is the one device function the base units and
// the variants' units come from.  With identity tables and zero bias one lane matches and the unit is clp[token] + log(1): the bits of
// group_unit_row.  One wave per row, plain stores, bounded walks, every index read from a section or a table is clamped and every load
// is unconditional on its clamped index.
#pragma once
#include "namp_group_scan.h"

struct ClassScanArgs {
  const int32_t* table_idx; // [N] input section: the member's class table
  const int32_t* tables;    // [n_tables][64] input section: entry c = the member's token under class c, below 0: no such class
  const float* bias;        // [n_tables][64] input section: the class bias, read through the last listed member's table index
  int n_tables, n_classes;
};

// lane = class: the unit whose listed-first member is `first` -> its value under the tokens tok_of(member) (the same in every lane).
// A unit of one (grouped == false) is its own entry.  var_row(j): the row of member j other than its base row, or nullptr.
template <class VarRow, class TokOf>
__device__ __forceinline__ float class_unit_row(const MutPlanArgs& a, const GroupScanArgs& g, const ClassScanArgs& c, const float* __restrict__ base_lp,
                                                const int first, const bool grouped, const int lane, VarRow var_row, TokOf tok_of) {
  if (!grouped) {                                             // (wave-uniform)
    const float* vr = var_row(first);
    return (vr ? vr : base_lp + (long)first * a.vocab)[loo_clamp(tok_of(first), a.vocab)];
  }
  const int cl = lane < c.n_classes ? lane : 0;
  bool have = lane < c.n_classes, match = lane < c.n_classes;
  float z = 0.f;
  int cur = first, last = first;
  for (int step = 0; step < NAMP_LOO_GROUP_MAX; ++step) {
    const float* vr = var_row(cur);
    const int tk = loo_clamp(tok_of(cur), a.vocab);
    const int e = c.tables[loo_clamp(c.table_idx[cur], c.n_tables) * 64 + cl];
    have = have && e >= 0;
    match = match && e == tk;
    const float x = (vr ? vr : base_lp + (long)cur * a.vocab)[loo_clamp(e, a.vocab)];
    z = __fadd_rn(z, __fmul_rn(g.weight[cur], x));
    last = cur;
    cur = loo_clamp(g.next[cur], a.N);
    if (cur == first) break;
  }
  z = __fadd_rn(z, c.bias[loo_clamp(c.table_idx[last], c.n_tables) * 64 + cl]);
  if (!have) z = -INFINITY;
  const float mx = tied_wave_max(z);
  if (!(mx > -INFINITY)) return -INFINITY;                    // (wave-uniform: no class every member has, or a total that is no number)
  const float ex = tied_wave_sum(have ? expf(z - mx) : 0.f);
  const float clp = (z - mx) - logf(ex);
  const float x = (have && match) ? clp : -INFINITY;
  const float m2 = tied_wave_max(x);
  if (!(m2 > -INFINITY)) return -INFINITY;                    // (wave-uniform: the tokens break the tie)
  return m2 + logf(tied_wave_sum(x > -INFINITY ? expf(x - m2) : 0.f));
}

// the Combine of group_unit_kernel / group_base_unit_kernel (namp_group_scan.h) for the class scan: class_unit_row (`own` is not read:
// every member's token goes through its table)
struct ClassCombine {
  ClassScanArgs c;
  template <class VarRow, class TokOf>
  __device__ __forceinline__ float unit(const MutPlanArgs& a, const GroupScanArgs& g, const float* __restrict__ base_lp, const int first,
                                        const bool grouped, const int lane, const int, VarRow var_row, TokOf tok_of) const {
    return class_unit_row(a, g, c, base_lp, first, grouped, lane, var_row, tok_of);
  }
};
