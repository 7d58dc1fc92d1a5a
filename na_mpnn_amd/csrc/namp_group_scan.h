// Group scan (namp_group_mutations, include/namp.h): the mutational scan of namp_mutations.h under the TIED stream of
// namp_tied.h on one backbone, where a point mutation of a symmetry group is a site of all its members with one token (identity maps).
// The base stream is the tied stream of S run as items over all N residues (tied_item_stream at n_chunk = 1) with every layer's
// tables kept: centres, rows projected with the token at j and without it at N + j of ONE table, Pfw, states, log_softmax rows.  The
// plan is that of namp_mutations.h, unchanged, with the KEYS of tied_keys_kernel as its ranks: "key(j) < key(i) and (j in the site or
// level(j) < l)" — a hidden-backward edge counts like a backward one, a superset of the rows that can differ.  The items are
// mut_items_kernel's with the edge kinds of GroupScanArgs: for key(j) < key(i)
//   backward (leader[j] != leader[i])   the variant's with-token row (LOO_OV | r) if j has one in U_{l-1}(site), else base row j
//   hidden, layer 1                     Pfw_1[j]                    (the encoder state: no token, the same in every variant)
//   hidden, layers 2 and 3              the variant's without-token row (LOO_OV | R_{l-1} + r), else base row N + j
// so dec_items_kernel (namp_loo.h, unchanged) reads five sources through its three tables.  Behind layer 3 state_head_kernel keeps the
// whole row; group_unit_kernel combines the members of a unit in listed order through its Combine — GroupCombine here (group_unit_row),
// ClassCombine in namp_class_scan.h: the one device function the base units come from too, every product and sum rounded once — and
// state_delta_kernel sums the leader terms.  Plain stores, one wave owns a row, bounded loops, every index read from a section or a
// table is clamped.
#pragma once
#include "namp_state_scan.h"
#include "namp_tied.h"

struct GroupScanArgs {
  const int32_t* next;      // [N] input section: the successor cycle in listed order
  const float* weight;      // [N] input section: the member's weight in the combine
  const int32_t* gl;        // [N] loo_groups_kernel: listed-first member of the residue's valid group, or -1
  const uint32_t* key;      // [N] tied_keys_kernel
  const int32_t* leader;    // [N] tied_keys_kernel: the listed-first member of the residue's unit
  float* base_unit;         // [N] output section: the unit of S at every member

  // mut_items_kernel's Edges: j lies behind i by its key; the code by the edge's kind (pj: j's row in U_{l-1}(site), or -1)
  __device__ __forceinline__ bool behind(const MutPlanArgs&, const int j, const int i) const { return key[j] < key[i]; }
  __device__ __forceinline__ int code(const MutPlanArgs& a, const int l, const int j, const int i, const int pj) const {
    const bool hid = leader[j] == leader[i];
    if (l == 0) return hid ? (LOO_FW | j) : (pj >= 0 ? (LOO_OV | pj) : j);
    return pj >= 0 ? (LOO_OV | (hid ? mut_pick(a.icap, l - 1) + pj : pj)) : (hid ? a.N + j : j);
  }
};

// one wave per residue: the base stream's log_softmax row from its layer-3 state (state_head_kernel's arithmetic)
static __global__ __launch_bounds__(256) void group_base_head_kernel(const float* __restrict__ h3, const float* __restrict__ head_w,
                                                                      const float* __restrict__ head_b, float* __restrict__ log_probs,
                                                                      const int N, const int vocab) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;                                         // (wave-uniform)
  const float lp = mut_head_row(h3 + r * NAMP_H, head_w, head_b, vocab, lane);
  if (lane < vocab) log_probs[r * vocab + lane] = lp;
}

// lane = token: the unit whose listed-first member is `first` -> its log_softmax row, log_softmax(sum over the members in listed
// order of weight_t * row_t) (lanes >= vocab: -inf); a unit of one (grouped == false) is its own row.  var_row(j): the row of member j
// other than its base row, or nullptr.  The walk is bounded by NAMP_LOO_GROUP_MAX steps and every successor is clamped.
template <class VarRow>
__device__ __forceinline__ float group_unit_row(const MutPlanArgs& a, const GroupScanArgs& g, const float* __restrict__ base_lp, const int first,
                                                const bool grouped, const int lane, VarRow var_row) {
  const int t = lane < a.vocab ? lane : 0;
  if (!grouped) {                                             // (wave-uniform)
    const float* vr = var_row(first);
    const float x = (vr ? vr : base_lp + (long)first * a.vocab)[t];
    return lane < a.vocab ? x : -INFINITY;
  }
  float z = 0.f;
  int cur = first;
  for (int step = 0; step < NAMP_LOO_GROUP_MAX; ++step) {
    const float* vr = var_row(cur);
    const float x = (vr ? vr : base_lp + (long)cur * a.vocab)[t];
    z = __fadd_rn(z, __fmul_rn(g.weight[cur], x));
    cur = loo_clamp(g.next[cur], a.N);
    if (cur == first) break;
  }
  return mut_wave_log_softmax(lane < a.vocab ? z : -INFINITY, lane < a.vocab);
}

// A Combine gives the value of the unit whose listed-first member is `first`, the same in every lane: unit(a, g, base_lp, first, grouped,
// lane, own, var_row, tok_of) with var_row(j) as above, tok_of(j) the token of member j and `own` the token that picks the entry where
// the members speak without tables.  The symmetric scan's: the entry of group_unit_row at `own` (identity maps: one token per unit)
struct GroupCombine {
  template <class VarRow, class TokOf>
  __device__ __forceinline__ float unit(const MutPlanArgs& a, const GroupScanArgs& g, const float* __restrict__ base_lp, const int first,
                                        const bool grouped, const int lane, const int own, VarRow var_row, TokOf) const {
    return __shfl(group_unit_row(a, g, base_lp, first, grouped, lane, var_row), loo_clamp(own, a.vocab));
  }
};

// one wave per residue; the wave of a unit's listed-first member combines the base rows under S and stores the unit, at the token of
// that member, at every member's slot (an ungrouped residue: its own entry at its own slot)
template <class Combine>
static __global__ __launch_bounds__(256) void group_base_unit_kernel(const MutPlanArgs a, const GroupScanArgs g, const Combine c,
                                                                      const float* __restrict__ base_lp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;                                       // (wave-uniform)
  const bool grouped = g.gl[i] >= 0;
  if (grouped && g.gl[i] != i) return;                        // (wave-uniform)
  const float unit = c.unit(a, g, base_lp, i, grouped, lane, a.S[i], [](int) -> const float* { return nullptr; },
                            [&](const int j) -> int { return a.S[j]; });
  int cur = i;
  for (int step = 0; step < NAMP_LOO_GROUP_MAX; ++step) {
    if (lane == 0) g.base_unit[cur] = unit;
    if (!grouped) break;
    cur = loo_clamp(g.next[cur], a.N);
    if (cur == i) break;
  }
}

// one wave per layer-3 item row.  The row LEADS its unit if it is unmasked and no earlier-listed member of its validated cycle has a
// row in the site's list_3 segment within the variant's capacity.  The leader walks the cycle from the listed-first member, takes the
// variant's row where the member has one, else the base row, and stores w * (unit_v - unit) at its row and the unit into the sparse
// units (unit_res: the listed-first member); every other row stores 0 and -1
template <class Combine>
static __global__ __launch_bounds__(256) void group_unit_kernel(const MutPlanArgs a, const StateScanArgs s, const GroupScanArgs g, const Combine c) {
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
  const float unit_v = c.unit(a, g, s.base_lp, first, grouped, lane, s.tok[r], var_row,
                              [&](const int j) -> int { return a.n_var > 0 ? mut_token(a, v, site, j) : a.S[j]; });
  const float unit_b = c.unit(a, g, s.base_lp, first, grouped, lane, a.S[first], [](int) -> const float* { return nullptr; },
                              [&](const int j) -> int { return a.S[j]; });
  if (lane == 0) {
    s.term[r] = __fmul_rn(a.w[first], __fsub_rn(unit_v, unit_b));
    s.unit_res[r] = first;
    s.unit_lp[r] = unit_v;
  }
}
