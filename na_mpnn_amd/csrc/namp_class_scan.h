// Class scan (namp_class_mutations, include/namp.h): the group scan of namp_group_scan.h with the combine of the tied
// score (tied_combine_kernel, namp_tied.h) — the members of a unit speak through CLASS TABLES, so a unit may be a base pair, a wobble
// pair, a group with token maps or a pair joined with symmetry groups.  Everything in front of the units is the group scan's as it
// stands: the tied base stream of S, the plan on the keys, gmut_items_kernel (a member's token comes from the variant through
// mut_token; edge kinds do not depend on tables), the whole-row head.  What is new is the combine.  With row_t the member's log_softmax
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

// one wave per residue; the wave of a unit's listed-first member combines the base rows under S and stores the unit at every member's
// slot (an ungrouped residue: its own entry at its own slot)
static __global__ __launch_bounds__(256) void class_base_unit_kernel(const MutPlanArgs a, const GroupScanArgs g, const ClassScanArgs c,
                                                                      const float* __restrict__ base_lp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;                                       // (wave-uniform)
  const bool grouped = g.gl[i] >= 0;
  if (grouped && g.gl[i] != i) return;                        // (wave-uniform)
  const float unit = class_unit_row(a, g, c, base_lp, i, grouped, lane, [](int) -> const float* { return nullptr; },
                                    [&](const int j) -> int { return a.S[j]; });
  int cur = i;
  for (int step = 0; step < NAMP_LOO_GROUP_MAX; ++step) {
    if (lane == 0) g.base_unit[cur] = unit;
    if (!grouped) break;
    cur = loo_clamp(g.next[cur], a.N);
    if (cur == i) break;
  }
}

// one wave per layer-3 item row: the leader rule and the stores of group_unit_kernel, the units through class_unit_row
static __global__ __launch_bounds__(256) void class_unit_kernel(const MutPlanArgs a, const StateScanArgs s, const GroupScanArgs g,
                                                                 const ClassScanArgs c) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.icap[2]) return;                                 // (wave-uniform)
  const int32_t* io = a.ioff[2];
  bool lead = a.n_var > 0 && r < io[a.n_var];
  const int v = lead ? mut_variant_of(io, a.n_var, (int)r) : 0;
  const int site = a.n_var > 0 ? mut_site_of(a, v) : 0;
  const int b = a.n_var > 0 ? a.loff[2][site] : 0, e = a.n_var > 0 ? a.loff[2][site + 1] : 0;
  const int row0 = a.n_var > 0 ? io[v] : 0, row1 = a.n_var > 0 ? io[v + 1] : 0;
  const int f = loo_clamp(s.ctr[r], a.N);
  const bool grouped = g.gl[f] >= 0;
  const int first = grouped ? loo_clamp(g.gl[f], a.N) : f;
  auto var_row = [&](const int j) -> const float* {
    const int p = mut_find(a.list[2], b, e, j);
    const int row = row0 + (p - b);
    return (p >= 0 && row < row1) ? s.rows + (long)row * 64 : nullptr;
  };
  lead = lead && a.mask[f] != 0;
  if (grouped) {
    int cur = first;
    for (int step = 0; step < NAMP_LOO_GROUP_MAX; ++step) {
      if (cur == f) break;
      if (var_row(cur) != nullptr) lead = false;
      cur = loo_clamp(g.next[cur], a.N);
    }
  }
  if (!lead) {                                                // (wave-uniform)
    if (lane == 0) { s.term[r] = 0.f; s.unit_res[r] = -1; s.unit_lp[r] = 0.f; }
    return;
  }
  const float unit_v = class_unit_row(a, g, c, s.base_lp, first, grouped, lane, var_row,
                                      [&](const int j) -> int { return a.n_var > 0 ? mut_token(a, v, site, j) : a.S[j]; });
  const float unit_b = class_unit_row(a, g, c, s.base_lp, first, grouped, lane, [](int) -> const float* { return nullptr; },
                                      [&](const int j) -> int { return a.S[j]; });
  if (lane == 0) {
    s.term[r] = __fmul_rn(a.w[first], __fsub_rn(unit_v, unit_b));
    s.unit_res[r] = first;
    s.unit_lp[r] = unit_v;
  }
}
