// Library scoring (namp_library, include/namp.h): the token log-probs of n candidate sequences on ONE complex, where the candidates
// differ from the base sequence S at n_var listed positions only.  With the decoding order of score() the decoder state of row i at
// layer l depends on the candidate iff (model_utils.py:391-421: a row reads the token and the previous layer's state of its BACKWARD
// neighbours, its own previous state, and encoder states everywhere else)
//   act_l[i] = mask[i] and (act_{l-1}[i] or exists k: rank[E_idx[i,k]] < rank[i] and (var[E_idx[i,k]] or act_{l-1}[E_idx[i,k]])),   act_0 = 0
// (the neighbour's own mask is not consulted: the reference multiplies by the centre's mask only).  Every other row is the base
// stream's.  The kernels here are the PLAN — var / act_l flags, their compaction to row lists — and the index tables that turn
// (candidate, listed row) into an ITEM of dec_items_kernel (namp_loo.h, unchanged): which h_E rows, which centre state, and per edge a
// row of the base backward table, the base forward table or the per-candidate OVERRIDE table an earlier layer's items projected.
// The item set of layer l is U_l = act_l + var: a listed position outside act_l is evaluated too (at most n_var rows per layer, from
// base inputs), so that every row a later layer reads per candidate — state, W1a projection, W1v projection + ITS token — comes out of
// the one projection path and a backward edge needs one test, "is the neighbour in U_{l-1}" (U_0 = var: layer 1 reads
// Pfw_1[j] + tok_1[token], lib_token_rows_kernel).  Behind layer 3 lib_head_kernel applies W_out + log_softmax to the items' states
// and keeps the candidate's own entry; lib_fill_kernel has written every entry from the base rows before.
// Every item owns its rows, plain stores, separate launches: two calls give identical bits.  The section is device data: positions,
// tokens and list positions are clamped, a row beyond the caller's capacity rows_l is treated as not per-candidate.
#pragma once
#include "namp_loo.h"

struct LibPlanArgs {
  const int32_t* E_idx;     // [N][K]
  const int32_t* rank;      // [N]
  const int32_t* mask;      // [N]
  const int32_t* S;         // [N] base tokens
  const int32_t* positions; // [n_var]            input section
  const int32_t* tokens;    // [n_chunk][n_var]   input section
  int32_t* vpos;            // [N] column of the residue in `tokens` (the LAST listed position that clamps to it), or -1
  int32_t* flag[3];         // [N] act_1 .. act_3
  int32_t* pos[3];          // [N] position of the residue in list_l, or -1 (not in U_l, or beyond rows_l)
  int32_t* list[3];         // [rows_l] the residues of U_l, ascending
  int32_t* counts;          // [9]: |act_1..3|, |U_1..3|, min(|U_l|, rows_l)
  int N, K, n_var, n_chunk, vocab;
  int cap[3];               // rows_l: item rows per candidate the caller sized the workspace for
};

static __global__ __launch_bounds__(256) void lib_var_kernel(const LibPlanArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  int v = -1;
  for (int q = 0; q < a.n_var; ++q)
    if (loo_clamp(a.positions[q], a.N) == i) v = q;
  a.vpos[i] = v;
}

// one flag pass over [N][K] (layer l = 0, 1, 2 of the recurrence above; launches, not a barrier, separate the passes)
static __global__ __launch_bounds__(256) void lib_flag_kernel(const LibPlanArgs a, const int l) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int32_t* prev = l ? a.flag[l == 1 ? 0 : 1] : nullptr;
  bool on = prev && prev[i] != 0;
  const int rk = a.rank[i];
  for (int k = 0; k < a.K; ++k) {
    const int j = loo_clamp(a.E_idx[(long)i * a.K + k], a.N);
    if (a.rank[j] < rk && (a.vpos[j] >= 0 || (prev && prev[j] != 0))) on = true;
  }
  (l == 0 ? a.flag[0] : l == 1 ? a.flag[1] : a.flag[2])[i] = (on && a.mask[i] != 0) ? 1 : 0;
}

// ONE workgroup: the three lists in ascending residue order (thread t owns a contiguous span; its offset is the sum of the spans in
// front of it — integer sums in a fixed order), the counts
static __global__ __launch_bounds__(1024) void lib_compact_kernel(const LibPlanArgs a) {
  __shared__ int su[1024], sa[1024];
  const int t = threadIdx.x;
  const int per = (a.N + 1023) / 1024;
  const int i0 = t * per, i1 = (i0 + per < a.N) ? i0 + per : a.N;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int32_t* fl = l == 0 ? a.flag[0] : l == 1 ? a.flag[1] : a.flag[2];
    int32_t* pos = l == 0 ? a.pos[0] : l == 1 ? a.pos[1] : a.pos[2];
    int32_t* list = l == 0 ? a.list[0] : l == 1 ? a.list[1] : a.list[2];
    const int cap = l == 0 ? a.cap[0] : l == 1 ? a.cap[1] : a.cap[2];
    int nu = 0, na = 0;
    for (int i = i0; i < i1; ++i) {
      const bool f = fl[i] != 0;
      na += f ? 1 : 0;
      nu += (f || a.vpos[i] >= 0) ? 1 : 0;
    }
    su[t] = nu; sa[t] = na;
    __syncthreads();
    int off = 0, tot_u = 0, tot_a = 0;
    for (int q = 0; q < 1024; ++q) {
      if (q < t) off += su[q];
      tot_u += su[q]; tot_a += sa[q];
    }
    for (int i = i0; i < i1; ++i) {
      const bool u = fl[i] != 0 || a.vpos[i] >= 0;
      int p = -1;
      if (u) {
        if (off < cap) { p = off; list[off] = i; }
        ++off;
      }
      pos[i] = p;
    }
    if (t == 0) {
      a.counts[l] = tot_a; a.counts[3 + l] = tot_u; a.counts[6 + l] = tot_u < cap ? tot_u : cap;
    }
    __syncthreads();
  }
}

// layer 1's override rows, one per (candidate, listed position q): Pfw_1[position] + tok_1[token] — the backward table row of a residue
// whose state is the encoder's and whose token is the candidate's
static __global__ __launch_bounds__(256) void lib_token_rows_kernel(const LibPlanArgs a, const float* __restrict__ Pfw, const float* __restrict__ tok,
                                                                     float* __restrict__ out) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  const long rows = (long)a.n_chunk * a.n_var;
  if (u >= rows * (NAMP_H / 4)) return;
  const long r = u / (NAMP_H / 4);
  const int c = (int)(u - r * (NAMP_H / 4)) * 4;
  const int q = (int)(r % a.n_var);
  const int i = loo_clamp(a.positions[q], a.N);
  const int tk = loo_clamp(a.tokens[r], a.vocab);
  *(f4*)(out + r * NAMP_H + c) = *(const f4*)(Pfw + (long)i * NAMP_H + c) + *(const f4*)(tok + (long)tk * NAMP_H + c);
}

struct LibItemTables {
  int32_t* act;             // [R] item flags: list position < min(|U_l|, rows_l)
  int32_t* ctr;             // [R] the item's residue
  int32_t* cen;             // [R] centre code: the base row, or the override row of (candidate, residue) in U_{l-1}
  int32_t* msk;             // [R] mask of the residue
  int32_t* tok;             // [R] token of the residue in the candidate
  int32_t* esrc;            // [R][K] edge codes
};

__device__ __forceinline__ int lib_token(const LibPlanArgs& a, const long s, const int i) {
  const int v = a.vpos[i];
  return v >= 0 ? loo_clamp(a.tokens[s * a.n_var + v], a.vocab) : a.S[i];
}

// the index tables of layer l's items, row r = candidate * rows_l + list position; one thread per (item, edge)
static __global__ __launch_bounds__(256) void lib_items_kernel(const LibPlanArgs a, const LibItemTables t, const int l) {
  const int cap = l == 0 ? a.cap[0] : l == 1 ? a.cap[1] : a.cap[2];
  const long R = (long)a.n_chunk * cap;
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= R * a.K) return;
  const long r = u / a.K;
  const int e = (int)(u - r * a.K);
  const long s = r / cap;
  const int p = (int)(r - s * cap);
  const bool on = p < a.counts[6 + l];
  const int32_t* list = l == 0 ? a.list[0] : l == 1 ? a.list[1] : a.list[2];
  const int i = on ? loo_clamp(list[p], a.N) : 0;
  const int32_t* ppos = l == 0 ? a.vpos : l == 1 ? a.pos[0] : a.pos[1];     // position in U_{l-1} (U_0 = var: the token column)
  const long pcap = l == 0 ? a.n_var : l == 1 ? a.cap[0] : a.cap[1];
  const int j = loo_clamp(a.E_idx[(long)i * a.K + e], a.N);
  int code = LOO_FW | j;
  if (a.rank[j] < a.rank[i]) {
    const int pj = ppos[j];
    code = pj >= 0 ? (LOO_OV | (int)(s * pcap + pj)) : j;
  }
  t.esrc[u] = code;
  if (e == 0) {
    const int pi = l ? ppos[i] : -1;                                         // (layer 1's input is the encoder state of every candidate)
    t.act[r] = on ? 1 : 0;
    t.ctr[r] = i;
    t.cen[r] = pi >= 0 ? (LOO_CEN_OV | (int)(s * pcap + pi)) : i;
    t.msk[r] = a.mask[i];
    t.tok[r] = lib_token(a, s, i);
  }
}

// token_log_probs[s][i] = base_log_probs[i][token of i in candidate s], every entry (the rows of U_3 are overwritten by lib_head_kernel)
static __global__ __launch_bounds__(256) void lib_fill_kernel(const LibPlanArgs a, const float* __restrict__ base_lp, float* __restrict__ tlp) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= (long)a.n_chunk * a.N) return;
  const long s = u / a.N;
  const int i = (int)(u - s * a.N);
  tlp[u] = base_lp[(long)i * a.vocab + loo_clamp(lib_token(a, s, i), a.vocab)];
}

// one wave per layer-3 item: log_softmax(W_out . h + b) of the item's state (the sums of tail_head_row, namp_kernels.h), of which the
// lane of the candidate's own token stores its entry
static __global__ __launch_bounds__(256) void lib_head_kernel(const LibPlanArgs a, const float* __restrict__ h3, const float* __restrict__ head_w,
                                                               const float* __restrict__ head_b, float* __restrict__ tlp) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (long)a.n_chunk * a.cap[2]) return;                // (wave-uniform)
  const long s = r / a.cap[2];
  const int p = (int)(r - s * a.cap[2]);
  if (p >= a.counts[8]) return;                               // (wave-uniform)
  const int i = loo_clamp(a.list[2][p], a.N);
  const float* y = h3 + r * NAMP_H;
  float z = -INFINITY;
  if (lane < a.vocab) {
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
  float mx = z;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float ex = (lane < a.vocab) ? expf(z - mx) : 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) ex += __shfl_xor(ex, o);
  if (lane == loo_clamp(lib_token(a, s, i), a.vocab)) tlp[s * a.N + i] = (z - mx) - logf(ex);
}
