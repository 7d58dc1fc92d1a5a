// Mutational scan (namp_mutations, include/namp.h): the change of the joint log-likelihood of score() under every VARIANT of a list,
// where a variant replaces the tokens of one SITE — 1 to NAMP_MUT_MAX_EDITS distinct residues — and keeps S everywhere else.  The
// sets are those of namp_library.h with var = the site: act_l(site) and U_l(site) = act_l(site) + site, and a variant differs from
// the base stream on U_3(site) only.  Where the library has ONE plan, the scan has one PER SITE, shared by the site's variants:
//   level[site][i]   the first layer l = 1..3 with act_l(site)[i] (act_{l-1} is a subset of act_l), 4 = never; bit 7: i is in the site
//   sizes[site][l]   |U_l(site)|;  list_l: the residues of U_l(site), ascending, the sites' segments laid end to end (loff_l)
//   ioff_l[v]        where the items (variant v, row of U_l(site of v)) of layer l begin: prefix sums over the variants
// All of it is integer work in a fixed order (flag passes per site as lib_flag_kernel's, span sums as lib_compact_kernel's): no
// atomics, nothing depends on scheduling.  An item's index tables are those of lib_items_kernel, but the variant of an item row and
// the position of a neighbour in U_{l-1}(site) come from binary searches in ioff_l and in the site's sorted segment — there is no
// [N] table per site.  dec_items_kernel (namp_loo.h) runs the items unchanged; behind layer 3 mut_head_kernel keeps the variant's own
// entry per item (lib_head_kernel's arithmetic on a sparse row) and mut_delta_kernel sums w_i (entry - base entry) per variant in
// list order.  Plain stores, every item owns its rows: two calls give identical bits, and a variant's bits depend neither on its chunk
// nor on its neighbours in the call.  The sections are device data: everything read from them is clamped (see include/namp.h).
#pragma once
#include "namp_loo.h"

#define MUT_E NAMP_MUT_MAX_EDITS

struct MutPlanArgs {
  const int32_t* E_idx;     // [N][K]
  const int32_t* rank;      // [N]
  const int32_t* mask;      // [N]
  const int32_t* S;         // [N] base tokens
  const int32_t* sites;     // [n_sites][MUT_E]        input section: residues, < 0 = no edit
  const int32_t* variants;  // [n_var][1 + MUT_E]      input section: site index, tokens
  const float* w;           // [N]                     input section: weight of the residue in delta
  uint8_t* level;           // [n_sites][N]
  int32_t* sizes;           // [n_sites][3]            output section: |U_l(site)|
  int32_t* loff[3];         // [n_sites + 1] segment of the site in list_l, cut at lcap[l]
  int32_t* list[3];         // [lcap[l]]
  int32_t* ioff[3];         // [n_var + 1] item rows of the variant in layer l, cut at icap[l]
  int N, K, n_sites, n_var, vocab;
  int lcap[3], icap[3];
};

template <typename T> __device__ __forceinline__ T* mut_pick(T* const (&p)[3], const int l) { return l == 0 ? p[0] : l == 1 ? p[1] : p[2]; }
__device__ __forceinline__ int mut_pick(const int (&p)[3], const int l) { return l == 0 ? p[0] : l == 1 ? p[1] : p[2]; }

// the edit of `site` that names residue i (the LAST one of several that clamp to it), or -1
__device__ __forceinline__ int mut_edit(const MutPlanArgs& a, const int site, const int i) {
  int q = -1;
  for (int e = 0; e < MUT_E; ++e) {
    const int r = a.sites[(long)site * MUT_E + e];
    if (r >= 0 && loo_clamp(r, a.N) == i) q = e;
  }
  return q;
}

__device__ __forceinline__ int mut_site_of(const MutPlanArgs& a, const int v) { return loo_clamp(a.variants[(long)v * (1 + MUT_E)], a.n_sites); }

__device__ __forceinline__ int mut_token(const MutPlanArgs& a, const int v, const int site, const int i) {
  const int q = mut_edit(a, site, i);
  return q >= 0 ? loo_clamp(a.variants[(long)v * (1 + MUT_E) + 1 + q], a.vocab) : a.S[i];
}

// exclusive offset of thread t's value among the 256 of the workgroup, and their total: integer sums in a fixed order
__device__ __forceinline__ long mut_span_offset(long* sh, const int t, const long mine, long* total) {
  __syncthreads();
  sh[t] = mine;
  __syncthreads();
  long off = 0, tot = 0;
  for (int q = 0; q < 256; ++q) {
    if (q < t) off += sh[q];
    tot += sh[q];
  }
  *total = tot;
  return off;
}

// ONE workgroup per site: the levels (three flag passes over [N][K], a barrier between them) and the three sizes
static __global__ __launch_bounds__(256) void mut_plan_kernel(const MutPlanArgs a) {
  __shared__ long sh[256];
  const int site = blockIdx.x, t = threadIdx.x;
  uint8_t* lv = a.level + (long)site * a.N;
  for (int i = t; i < a.N; i += 256) lv[i] = (uint8_t)((mut_edit(a, site, i) >= 0 ? 0x80 : 0) | 4);
  for (int l = 1; l <= 3; ++l) {
    __threadfence_block();
    __syncthreads();
    for (int i = t; i < a.N; i += 256) {
      const int mine = lv[i];
      if ((mine & 7) != 4 || a.mask[i] == 0) continue;
      const int rk = a.rank[i];
      bool on = false;
      for (int k = 0; k < a.K; ++k) {
        const int j = loo_clamp(a.E_idx[(long)i * a.K + k], a.N);
        const int lj = lv[j];                                   // (a level written in THIS pass is l: it fails the test as 4 does)
        if (a.rank[j] < rk && ((lj & 0x80) || (lj & 7) < l)) on = true;
      }
      if (on) lv[i] = (uint8_t)((mine & 0x80) | l);
    }
  }
  __threadfence_block();
  __syncthreads();
  const int per = (a.N + 255) / 256;
  const int i0 = t * per, i1 = (i0 + per < a.N) ? i0 + per : a.N;
  for (int l = 1; l <= 3; ++l) {
    int n = 0;
    for (int i = i0; i < i1; ++i) n += ((lv[i] & 0x80) || (lv[i] & 7) <= l) ? 1 : 0;
    long tot;
    mut_span_offset(sh, t, n, &tot);
    if (t == 0) a.sizes[site * 3 + l - 1] = (int)tot;
  }
}

// ONE workgroup: the prefix sums — list segments over the sites, item rows over the variants —, each cut at its capacity
static __global__ __launch_bounds__(256) void mut_offsets_kernel(const MutPlanArgs a) {
  __shared__ long sh[256];
  const int t = threadIdx.x;
  for (int l = 0; l < 3; ++l) {
    {
      int32_t* off = mut_pick(a.loff, l);
      const int cap = mut_pick(a.lcap, l);
      const int per = (a.n_sites + 255) / 256;
      const int s0 = t * per, s1 = (s0 + per < a.n_sites) ? s0 + per : a.n_sites;
      long n = 0;
      for (int s = s0; s < s1; ++s) n += loo_clamp(a.sizes[s * 3 + l], a.N + 1);
      long tot;
      long o = mut_span_offset(sh, t, n, &tot);
      for (int s = s0; s < s1; ++s) {
        off[s] = (int)(o < cap ? o : cap);
        o += loo_clamp(a.sizes[s * 3 + l], a.N + 1);
      }
      if (t == 0) off[a.n_sites] = (int)(tot < cap ? tot : cap);
    }
    __threadfence_block();
    __syncthreads();
    {
      const int32_t* lo = mut_pick(a.loff, l);
      int32_t* off = mut_pick(a.ioff, l);
      const int cap = mut_pick(a.icap, l);
      const int per = (a.n_var + 255) / 256;
      const int v0 = t * per, v1 = (v0 + per < a.n_var) ? v0 + per : a.n_var;
      long n = 0;
      for (int v = v0; v < v1; ++v) { const int s = mut_site_of(a, v); n += lo[s + 1] - lo[s]; }
      long tot;
      long o = mut_span_offset(sh, t, n, &tot);
      for (int v = v0; v < v1; ++v) {
        const int s = mut_site_of(a, v);
        off[v] = (int)(o < cap ? o : cap);
        o += lo[s + 1] - lo[s];
      }
      if (t == 0) off[a.n_var] = (int)(tot < cap ? tot : cap);
    }
  }
}

// ONE workgroup per site: its segment of every list, ascending (what lies beyond the segment the capacity left is dropped)
static __global__ __launch_bounds__(256) void mut_lists_kernel(const MutPlanArgs a) {
  __shared__ long sh[256];
  const int site = blockIdx.x, t = threadIdx.x;
  const uint8_t* lv = a.level + (long)site * a.N;
  const int per = (a.N + 255) / 256;
  const int i0 = t * per, i1 = (i0 + per < a.N) ? i0 + per : a.N;
  for (int l = 1; l <= 3; ++l) {
    const int32_t* lo = mut_pick(a.loff, l - 1);
    int32_t* list = mut_pick(a.list, l - 1);
    const int b = lo[site], e = lo[site + 1];
    int n = 0;
    for (int i = i0; i < i1; ++i) n += ((lv[i] & 0x80) || (lv[i] & 7) <= l) ? 1 : 0;
    long tot;
    int o = b + (int)mut_span_offset(sh, t, n, &tot);
    for (int i = i0; i < i1; ++i)
      if ((lv[i] & 0x80) || (lv[i] & 7) <= l) {
        if (o < e) list[o] = i;
        ++o;
      }
  }
}

// position of residue i in the ascending segment list[b .. e), or -1
__device__ __forceinline__ int mut_find(const int32_t* list, int b, int e, const int i) {
  while (b < e) {
    const int m = (b + e) >> 1;
    const int r = list[m];
    if (r == i) return m;
    if (r < i) b = m + 1; else e = m;
  }
  return -1;
}

// the variant whose item rows hold row r: the last v with off[v] <= r (off ascending, off[n] > r)
__device__ __forceinline__ int mut_variant_of(const int32_t* off, const int n, const int r) {
  int b = 0, e = n;
  while (e - b > 1) {
    const int m = (b + e) >> 1;
    if (off[m] <= r) b = m; else e = m;
  }
  return b;
}

// layer 1's override rows, one per (variant, edit): Pfw_1[residue] + tok_1[token]
static __global__ __launch_bounds__(256) void mut_token_rows_kernel(const MutPlanArgs a, const float* __restrict__ Pfw, const float* __restrict__ tok,
                                                                     float* __restrict__ out) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  const long rows = (long)a.n_var * MUT_E;
  if (u >= rows * (NAMP_H / 4)) return;
  const long r = u / (NAMP_H / 4);
  const int c = (int)(u - r * (NAMP_H / 4)) * 4;
  const int v = (int)(r / MUT_E), e = (int)(r - (long)v * MUT_E);
  const int i = loo_clamp(a.sites[(long)mut_site_of(a, v) * MUT_E + e], a.N);
  const int tk = loo_clamp(a.variants[(long)v * (1 + MUT_E) + 1 + e], a.vocab);
  *(f4*)(out + r * NAMP_H + c) = *(const f4*)(Pfw + (long)i * NAMP_H + c) + *(const f4*)(tok + (long)tk * NAMP_H + c);
}

struct MutItemTables {
  int32_t* act;             // [R] item flags: the row lies inside the item rows of a variant
  int32_t* ctr;             // [R] the item's residue
  int32_t* cen;             // [R] centre code: the base row, or the override row of (variant, residue) in U_{l-1}
  int32_t* msk;             // [R] mask of the residue
  int32_t* tok;             // [R] token of the residue in the variant
  int32_t* esrc;            // [R][K] edge codes
};

// the plain scan's edges: j lies behind i by its rank; a backward edge reads the variant's row of j where U_{l-1}(site) holds one (pj),
// else base row j
struct MutPlainEdges {
  __device__ __forceinline__ bool behind(const MutPlanArgs& a, const int j, const int i) const { return a.rank[j] < a.rank[i]; }
  __device__ __forceinline__ int code(const MutPlanArgs&, const int, const int j, const int, const int pj) const {
    return pj >= 0 ? (LOO_OV | pj) : j;
  }
};

// the index tables of layer l's items (R = icap[l] rows, laid out by ioff_l); one thread per (item row, edge).  Edges: which edges lie
// behind their centre and the code of such an edge (MutPlainEdges; the group scan's kinds: GroupScanArgs, namp_group_scan.h)
template <class Edges>
static __global__ __launch_bounds__(256) void mut_items_kernel(const MutPlanArgs a, const Edges g, const MutItemTables t, const int l) {
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
  // U_{l-1}(site): the site's edits for layer 1 (override row v * MUT_E + edit), its segment of list_{l-1} behind it (the item row of
  // (v, residue) there, if the capacity left it one)
  auto prev_row = [&](const int j) -> int {
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
  t.esrc[u] = g.behind(a, j, i) ? g.code(a, l, j, i, prev_row(j)) : (LOO_FW | j);
  if (e == 0) {
    const int pi = l ? prev_row(i) : -1;                                     // (layer 1's input is the encoder state of every variant)
    t.act[r] = on ? 1 : 0;
    t.ctr[r] = i;
    t.cen[r] = pi >= 0 ? (LOO_CEN_OV | pi) : i;
    t.msk[r] = a.mask[i];
    t.tok[r] = on ? mut_token(a, v, site, i) : a.S[i];
  }
}

// lane = token: log_softmax of z over the lanes that are `on` (the others hold -inf).  The one copy every scan's head and combine goes
// through; called by all 64 lanes of a wave, never under a branch that splits it
__device__ __forceinline__ float mut_wave_log_softmax(const float z, const bool on) {
  const float mx = tied_wave_max(z);
  const float ex = tied_wave_sum(on ? expf(z - mx) : 0.f);
  return (z - mx) - logf(ex);
}

// lane = token: log_softmax(W_out . y + b) of one state row y [128] (lib_head_kernel's sums); lanes >= vocab hold -inf
__device__ __forceinline__ float mut_head_row(const float* __restrict__ y, const float* __restrict__ head_w, const float* __restrict__ head_b,
                                              const int vocab, const int lane) {
  float z = -INFINITY;
  if (lane < vocab) {
    const float* w = head_w + (long)lane * NAMP_H;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
    for (int c = 0; c < NAMP_H; c += 4) {
      const f4 wv = *(const f4*)(w + c);
      const f4 yv = *(const f4*)(y + c);
      s0 = fmaf(wv.x, yv.x, s0); s1 = fmaf(wv.y, yv.y, s1); s2 = fmaf(wv.z, yv.z, s2); s3 = fmaf(wv.w, yv.w, s3);
    }
    z = (s0 + s1) + (s2 + s3) + head_b[lane];
  }
  return mut_wave_log_softmax(z, lane < vocab);
}

// one wave per layer-3 item row: the log_softmax row of the item's state, of which the lane of the variant's own token stores its entry
// at the item's row; lane 0 stores the residue.  A row outside every variant: residue -1, entry 0
static __global__ __launch_bounds__(256) void mut_head_kernel(const MutPlanArgs a, const int32_t* __restrict__ ctr, const int32_t* __restrict__ tok,
                                                               const float* __restrict__ h3, const float* __restrict__ head_w,
                                                               const float* __restrict__ head_b, int32_t* __restrict__ row_res,
                                                               float* __restrict__ row_lp) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.icap[2]) return;                                 // (wave-uniform)
  if (a.n_var == 0 || r >= a.ioff[2][a.n_var]) {              // (wave-uniform)
    if (lane == 0) { row_res[r] = -1; row_lp[r] = 0.f; }
    return;
  }
  const float lp = mut_head_row(h3 + r * NAMP_H, head_w, head_b, a.vocab, lane);
  if (lane == loo_clamp(tok[r], a.vocab)) row_lp[r] = lp;
  if (lane == 0) row_res[r] = ctr[r];
}

// one thread per variant: delta = sum over its rows, in list order, of w_i * (entry - base entry); every product and every sum is
// rounded once (no contraction), so that the result is the fp32 recursive sum of the fp32 terms
static __global__ __launch_bounds__(256) void mut_delta_kernel(const MutPlanArgs a, const int32_t* __restrict__ row_res,
                                                                const float* __restrict__ row_lp, const float* __restrict__ base_lp,
                                                                float* __restrict__ delta) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.n_var) return;
  float acc = 0.f;
  for (int r = a.ioff[2][v]; r < a.ioff[2][v + 1]; ++r) {
    const int i = loo_clamp(row_res[r], a.N);
    const float d = __fsub_rn(row_lp[r], base_lp[(long)i * a.vocab + loo_clamp(a.S[i], a.vocab)]);
    acc = __fadd_rn(acc, __fmul_rn(a.w[i], d));
  }
  delta[v] = acc;
}
