// Specificity scan (namp_state_mutations, include/namp.h): the mutational scan of namp_mutations.h on the FLATTENED graph
// of M backbone states of L residues (flat residue m * L + i, block-diagonal E_idx: no edge runs between two copies of a residue), where
// a point mutation of shared residue i is a site of its M copies.  The plan, the item tables and dec_items_kernel run as they stand; what
// is new sits behind layer 3.  With present(j) = mask[j] != 0 on the flat graph and u = unit_w (w_m where the copy is present),
//   unit[i]    = log_softmax(sum over the present copies j = m L + i, m ascending, of u_j * row_j)[token of i],  row_j = log_softmax row
//   delta[v]   = sum over the LEADER rows of v, in list order, of w * (unit_v - unit)        (a variant's rows replace the base rows)
//   state_delta[v][m] = sum over the rows of v in block m, in list order, of w * (own entry - base own entry)
// A row LEADS its shared residue if it is present and no present copy of a lower state lies in the site's list_3 segment.  Every product
// and every sum of the combine is rounded once (no contraction) in one device function, so the base-unit kernel and the unit kernel
// agree bit for bit on a base unit.  Plain stores, one wave owns a row, every index read from a section or a table is clamped.
#pragma once
#include "namp_mutations.h"

struct StateScanArgs {
  const int32_t* ctr;       // [icap_3] layer-3 item tables: the row's flat residue
  const int32_t* tok;       // [icap_3] ... and its token in the variant
  const float* base_lp;     // [N][vocab] the base stream's log_softmax rows
  const float* unit_w;      // [N] input section: w_m where the copy is present, else 0
  float* rows;              // [icap_3][64] the variants' log_softmax rows
  float* term;              // [icap_3] w * (unit_v - unit) at leader rows, else 0
  int32_t* row_res;         // [icap_3] output section: flat residue of the row, -1: no item
  float* row_lp;            // [icap_3] ... the variant's own entry there
  int32_t* unit_res;        // [icap_3] ... shared residue the row leads, -1: none
  float* unit_lp;           // [icap_3] ... the variant's unit there
  float* base_unit;         // [L]
  float* delta;             // [n_var]
  float* state_delta;       // [n_var][n_states]
  int n_states, L;
};

// lane = token: the combine of the copies of shared residue i -> the unit's log_softmax row (lanes >= vocab: -inf).  var_row(m): the
// row of copy m other than its base row, or nullptr; solo: no copy is present (copy 0 speaks alone with weight 1).
template <class VarRow>
__device__ __forceinline__ float state_unit_row(const MutPlanArgs& a, const StateScanArgs& s, const int i, const int lane, const bool solo,
                                                VarRow var_row) {
  const int t = lane < a.vocab ? lane : 0;
  float z = 0.f;
  for (int m = 0; m < s.n_states; ++m) {
    const int j = m * s.L + i;
    const float* vr = var_row(m);
    const float x = (vr ? vr : s.base_lp + (long)j * a.vocab)[t];
    const float u = solo ? (m == 0 ? 1.f : 0.f) : s.unit_w[j];
    if (solo ? m == 0 : a.mask[j] != 0) z = __fadd_rn(z, __fmul_rn(u, x));
  }
  return mut_wave_log_softmax(lane < a.vocab ? z : -INFINITY, lane < a.vocab);
}

// one wave per shared residue: unit[i] of S from the base rows, at the token of the first present copy (none present: copy 0's)
static __global__ __launch_bounds__(256) void state_base_unit_kernel(const MutPlanArgs a, const StateScanArgs s) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= s.L) return;                                       // (wave-uniform)
  int seat = -1;
  for (int m = s.n_states - 1; m >= 0; --m)
    if (a.mask[m * s.L + i] != 0) seat = m;
  const float row = state_unit_row(a, s, i, lane, seat < 0, [](int) -> const float* { return nullptr; });
  const int tk = loo_clamp(a.S[(seat < 0 ? 0 : seat) * s.L + i], a.vocab);
  if (lane == tk) s.base_unit[i] = row;
}

// one wave per layer-3 item row: mut_head_kernel's row (mut_head_row), the whole log_softmax row kept beside the own entry
static __global__ __launch_bounds__(256) void state_head_kernel(const MutPlanArgs a, const StateScanArgs s, const float* __restrict__ h3,
                                                                 const float* __restrict__ head_w, const float* __restrict__ head_b) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.icap[2]) return;                                 // (wave-uniform)
  if (a.n_var == 0 || r >= a.ioff[2][a.n_var]) {              // (wave-uniform)
    s.rows[r * 64 + lane] = 0.f;
    if (lane == 0) { s.row_res[r] = -1; s.row_lp[r] = 0.f; }
    return;
  }
  const float lp = mut_head_row(h3 + r * NAMP_H, head_w, head_b, a.vocab, lane);
  s.rows[r * 64 + lane] = lane < a.vocab ? lp : 0.f;
  if (lane == loo_clamp(s.tok[r], a.vocab)) s.row_lp[r] = lp;
  if (lane == 0) s.row_res[r] = s.ctr[r];
}

// one wave per layer-3 item row: the leader of a shared residue combines its copies (the variant's row where the copy has one) and
// stores w * (unit_v - unit) at its row and the unit into the sparse units; every other row stores 0 and -1
static __global__ __launch_bounds__(256) void state_unit_kernel(const MutPlanArgs a, const StateScanArgs s) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.icap[2]) return;                                 // (wave-uniform)
  const int32_t* io = a.ioff[2];
  bool lead = a.n_var > 0 && r < io[a.n_var];
  const int v = lead ? mut_variant_of(io, a.n_var, (int)r) : 0;
  const int site = a.n_var > 0 ? mut_site_of(a, v) : 0;
  const int b = a.n_var > 0 ? a.loff[2][site] : 0, e = a.n_var > 0 ? a.loff[2][site + 1] : 0;
  const int f = loo_clamp(s.ctr[r], a.N);
  const int m0 = f / s.L, i = f - m0 * s.L;
  lead = lead && a.mask[f] != 0;
  for (int m = 0; m < s.n_states; ++m)
    if (m < m0 && a.mask[m * s.L + i] != 0 && mut_find(a.list[2], b, e, m * s.L + i) >= 0) lead = false;
  if (!lead) {                                                // (wave-uniform)
    if (lane == 0) { s.term[r] = 0.f; s.unit_res[r] = -1; s.unit_lp[r] = 0.f; }
    return;
  }
  const int row0 = io[v], row1 = io[v + 1];
  const float uv = state_unit_row(a, s, i, lane, false, [&](const int m) -> const float* {
    const int p = mut_find(a.list[2], b, e, m * s.L + i);
    const int row = row0 + (p - b);
    return (p >= 0 && row < row1) ? s.rows + (long)row * 64 : nullptr;
  });
  const float ub = state_unit_row(a, s, i, lane, false, [](int) -> const float* { return nullptr; });
  const float unit_v = __shfl(uv, loo_clamp(s.tok[r], a.vocab));
  const float unit_b = __shfl(ub, loo_clamp(a.S[f], a.vocab));
  if (lane == 0) {
    s.term[r] = __fmul_rn(a.w[f], __fsub_rn(unit_v, unit_b));
    s.unit_res[r] = i;
    s.unit_lp[r] = unit_v;
  }
}

// one thread per variant: the fp32 recursive sum of its leader terms in list order (mut_delta_kernel's rounding)
static __global__ __launch_bounds__(256) void state_delta_kernel(const MutPlanArgs a, const StateScanArgs s) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.n_var) return;
  float acc = 0.f;
  for (int r = a.ioff[2][v]; r < a.ioff[2][v + 1]; ++r) acc = __fadd_rn(acc, s.term[r]);
  s.delta[v] = acc;
}

// one thread per (variant, state): sum over the rows of block m (ascending flat residues: a contiguous range), in list order, of
// w * (own entry - base own entry)
static __global__ __launch_bounds__(256) void state_block_delta_kernel(const MutPlanArgs a, const StateScanArgs s) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= (long)a.n_var * s.n_states) return;
  const int v = (int)(u / s.n_states), m = (int)(u - (long)v * s.n_states);
  float acc = 0.f;
  for (int r = a.ioff[2][v]; r < a.ioff[2][v + 1]; ++r) {
    const int f = loo_clamp(s.row_res[r], a.N);
    if (f / s.L != m) continue;
    const float d = __fsub_rn(s.row_lp[r], s.base_lp[(long)f * a.vocab + loo_clamp(a.S[f], a.vocab)]);
    acc = __fadd_rn(acc, __fmul_rn(a.w[f], d));
  }
  s.state_delta[u] = acc;
}
