// Group scan (namp_group_mutations, include/namp.h): the mutational scan of namp_mutations.h under the TIED stream of
// namp_tied.h on one backbone, where a point mutation of a symmetry group is a site of all its members with one token (identity maps).
// The base stream is the tied stream of S run as items over all N residues (tied_item_stream at n_chunk = 1) with every layer's
// tables kept: centres, rows projected with the token at j and without it at N + j of ONE table, Pfw, states, log_softmax rows.  The
// plan is that of namp_mutations.h, unchanged, with the KEYS of tied_keys_kernel as its ranks: "key(j) < key(i) and (j in the site or
// level(j) < l)" — a hidden-backward edge counts like a backward one, a superset of the rows that can differ.  gmut_items_kernel is
// mut_items_kernel with edge kinds: for key(j) < key(i)
//   backward (leader[j] != leader[i])   the variant's with-token row (LOO_OV | r) if j has one in U_{l-1}(site), else base row j
//   hidden, layer 1                     Pfw_1[j]                    (the encoder state: no token, the same in every variant)
//   hidden, layers 2 and 3              the variant's without-token row (LOO_OV | R_{l-1} + r), else base row N + j
// so dec_items_kernel (namp_loo.h, unchanged) reads five sources through its three tables.  Behind layer 3 state_head_kernel keeps the
// whole row; group_unit_kernel combines the members of a unit in listed order through group_unit_row — the one device function the
// base units come from too, every product and sum rounded once — and state_delta_kernel sums the leader terms.  Plain stores, one
// wave owns a row, bounded loops, every index read from a section or a table is clamped.
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
};

// the index tables of layer l's items: mut_items_kernel with edge kinds (a.rank holds the keys); one thread per (item row, edge)
static __global__ __launch_bounds__(256) void gmut_items_kernel(const MutPlanArgs a, const GroupScanArgs g, const MutItemTables t, const int l) {
  const long R = mut_pick(a.icap, l);
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= R * a.K) return;
  const int r = (int)(u / a.K);
  const int e = (int)(u - (long)r * a.K);
  const int32_t* io = mut_pick(a.ioff, l);
  const bool on = a.n_var > 0 && r < io[a.n_var];
  const int v = on ? mut_variant_of(io, a.n_var, r) : 0;
  const int site = a.n_var > 0 ? mut_site_of(a, v) : 0;
  const int i = on ? loo_clamp(mut_pick(a.list, l)[mut_pick(a.loff, l)[site] + (r - io[v])], a.N) : 0;
  const int Rprev = l ? mut_pick(a.icap, l - 1) : 0;
  auto prev_row = [&](const int j) -> int {                      // (mut_items_kernel's)
    if (!on) return -1;
    if (l == 0) { const int q = mut_edit(a, site, j); return q >= 0 ? v * MUT_E + q : -1; }
    const int32_t* lo = mut_pick(a.loff, l - 1);
    const int32_t* po = mut_pick(a.ioff, l - 1);
    const int p = mut_find(mut_pick(a.list, l - 1), lo[site], lo[site + 1], j);
    if (p < 0) return -1;
    const int row = po[v] + (p - lo[site]);
    return row < po[v + 1] ? row : -1;
  };
  const int j = loo_clamp(a.E_idx[(long)i * a.K + e], a.N);
  int code = LOO_FW | j;
  if (g.key[j] < g.key[i]) {
    const bool hid = g.leader[j] == g.leader[i];
    const int pj = prev_row(j);
    if (l == 0) code = hid ? (LOO_FW | j) : (pj >= 0 ? (LOO_OV | pj) : j);
    else code = pj >= 0 ? (LOO_OV | (hid ? Rprev + pj : pj)) : (hid ? a.N + j : j);
  }
  t.esrc[u] = code;
  if (e == 0) {
    const int pi = l ? prev_row(i) : -1;
    t.act[r] = on ? 1 : 0;
    t.ctr[r] = i;
    t.cen[r] = pi >= 0 ? (LOO_CEN_OV | pi) : i;
    t.msk[r] = a.mask[i];
    t.tok[r] = on ? mut_token(a, v, site, i) : a.S[i];
  }
}

// one wave per residue: the base stream's log_softmax row from its layer-3 state (state_head_kernel's arithmetic)
static __global__ __launch_bounds__(256) void group_base_head_kernel(const float* __restrict__ h3, const float* __restrict__ head_w,
                                                                      const float* __restrict__ head_b, float* __restrict__ log_probs,
                                                                      const int N, const int vocab) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;                                         // (wave-uniform)
  const float lp = state_head_row(h3 + r * NAMP_H, head_w, head_b, vocab, lane);
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
  if (lane >= a.vocab) z = -INFINITY;
  float mx = z;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float ex = (lane < a.vocab) ? expf(z - mx) : 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) ex += __shfl_xor(ex, o);
  return (z - mx) - logf(ex);
}

// one wave per residue; the wave of a unit's listed-first member combines the base rows and stores the unit, at the token of that
// member, at every member's slot (an ungrouped residue: its own entry at its own slot)
static __global__ __launch_bounds__(256) void group_base_unit_kernel(const MutPlanArgs a, const GroupScanArgs g, const float* __restrict__ base_lp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;                                       // (wave-uniform)
  const bool grouped = g.gl[i] >= 0;
  if (grouped && g.gl[i] != i) return;                        // (wave-uniform)
  const float row = group_unit_row(a, g, base_lp, i, grouped, lane, [](int) -> const float* { return nullptr; });
  const float unit = __shfl(row, loo_clamp(a.S[i], a.vocab));
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
static __global__ __launch_bounds__(256) void group_unit_kernel(const MutPlanArgs a, const StateScanArgs s, const GroupScanArgs g) {
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
  const float uv = group_unit_row(a, g, s.base_lp, first, grouped, lane, var_row);
  const float ub = group_unit_row(a, g, s.base_lp, first, grouped, lane, [](int) -> const float* { return nullptr; });
  const float unit_v = __shfl(uv, loo_clamp(s.tok[r], a.vocab));
  const float unit_b = __shfl(ub, loo_clamp(a.S[first], a.vocab));
  if (lane == 0) {
    s.term[r] = __fmul_rn(a.w[first], __fsub_rn(unit_v, unit_b));
    s.unit_res[r] = first;
    s.unit_lp[r] = unit_v;
  }
}
