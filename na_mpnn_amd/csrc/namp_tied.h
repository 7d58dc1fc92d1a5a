// Tied score (namp_tied_score, include/namp.h): the joint log-likelihood of tie-consistent sequences under the
// distribution tied sample() draws from, every token teacher-forced.  A forced tied stream has no sequential dependency: with rank0
// the ranks of score() on the flattened graph, a residue's KEY is (min of rank0 over its group) << 4 | its listed position — groups
// are visited when the order reaches their first member, the members follow each other in listed order — and an edge i <- j is
//   forward          key(j) >= key(i)                       the encoder state, no token
//   hidden-backward  key(j) <  key(i), j in i's group       j's decoder state of the layer WITHOUT j's token
//   backward         otherwise                              j's decoder state plus the token of the sequence at j
// Every (sequence, residue) of a chunk is an item of every layer: dec_items_kernel (namp_loo.h, unchanged) runs them with the three
// edge tables T0 = the rows of the layer in front projected WITH the token, T1 = Pfw of the layer (per residue, shared by the
// sequences), T2 = the same rows projected WITHOUT the token (layer 1: a hidden-backward edge reads the encoder state, T1).  Behind
// layer 3 tied_head_kernel keeps the whole logits row per item and tied_combine_kernel sums the members' rows through their class
// tables (token maps without classes) in listed order.  Integer tables, plain stores, every item owns its rows, nothing is summed
// across items: two calls give equal bits, and a sequence's bits depend neither on its chunk nor on its place in it.  The sections
// are device data: everything read from them is clamped (see include/namp.h).
#pragma once
#include "namp_loo.h"

struct TiedArgs {
  const int32_t* E_idx;     // [N][K]
  const int32_t* rank;      // [N] rank0
  const int32_t* mask;      // [N]
  const int32_t* next;      // [N] input section: the successor cycle in listed order
  const int32_t* table_idx; // [N]
  const float* weight;      // [N]
  const int32_t* tables;    // [n_tables][64]
  const float* bias;        // [n_tables][64]
  const int32_t* seq;       // [n_chunk][N] the sequences
  const int32_t* gl;        // [N] loo_groups_kernel: leader of the residue's valid group, or -1
  const int32_t* gpos;      // [N] its listed position
  uint32_t* key;            // [N]
  int32_t* leader;          // [N] the listed-first member of the residue's unit (itself when ungrouped)
  int32_t* header;          // [64] output section: word 0 grouped residues, word 1 hidden-backward edges
  int N, K, n_tables, n_classes, n_chunk, vocab;
};

// one thread per residue: the key and the leader (the cycle was validated by loo_groups_kernel: every successor of a grouped
// residue lies inside [0, N) and the walk closes within NAMP_LOO_GROUP_MAX steps)
static __global__ __launch_bounds__(256) void tied_keys_kernel(const TiedArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.N) return;
  int mn = a.rank[g];
  const bool grouped = a.gl[g] >= 0;
  if (grouped) {
    int cur = g;
    for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
      cur = loo_clamp(a.next[cur], a.N);
      if (cur == g) break;
      const int r = a.rank[cur];
      mn = r < mn ? r : mn;
    }
  }
  a.key[g] = ((uint32_t)mn << 4) | (uint32_t)(grouped ? (a.gpos[g] & 15) : 0);
  a.leader[g] = grouped ? a.gl[g] : g;
}

__device__ __forceinline__ bool tied_hidden(const TiedArgs& a, const int i, const int j) {
  return a.key[j] < a.key[i] && a.leader[j] == a.leader[i];      // (equal leaders of two residues: one valid group)
}

// ONE workgroup: the header.  Integer sums in a fixed order (every thread's span, then the 256 spans by thread 0)
static __global__ __launch_bounds__(256) void tied_count_kernel(const TiedArgs a) {
  __shared__ int sg[256], sh[256];
  const int t = threadIdx.x;
  const int per = (a.N + 255) / 256;
  const int i0 = t * per, i1 = (i0 + per < a.N) ? i0 + per : a.N;
  int ng = 0, nh = 0;
  for (int i = i0; i < i1; ++i) {
    if (a.gl[i] < 0) continue;
    ++ng;
    for (int k = 0; k < a.K; ++k) nh += tied_hidden(a, i, loo_clamp(a.E_idx[(long)i * a.K + k], a.N)) ? 1 : 0;
  }
  sg[t] = ng; sh[t] = nh;
  __syncthreads();
  if (t == 0) {
    int tg = 0, th = 0;
    for (int q = 0; q < 256; ++q) { tg += sg[q]; th += sh[q]; }
    sg[0] = tg; sh[0] = th;
  }
  __syncthreads();
  if (t < 64) a.header[t] = t == 0 ? sg[0] : t == 1 ? sh[0] : 0;
}

struct TiedItemTables {
  int32_t* ctr;             // [R] the item's residue
  int32_t* msk;             // [R] its mask
  int32_t* tok;             // [R] its token in the item's sequence, clamped
  int32_t* cen[2];          // [R] centre codes of layer 1 (the encoder state) / of layers 2 and 3 (the item's own row in front)
  int32_t* esrc[2];         // [R][K] edge codes of layer 1 / of layers 2 and 3
};

// the index tables of the item rows r = k * N + i (R = n_chunk * N); one thread per (item row, edge)
static __global__ __launch_bounds__(256) void tied_items_kernel(const TiedArgs a, const TiedItemTables t) {
  const long R = (long)a.n_chunk * a.N;
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= R * a.K) return;
  const int r = (int)(u / a.K);
  const int e = (int)(u - (long)r * a.K);
  const int k = r / a.N, i = r - k * a.N;
  const int j = loo_clamp(a.E_idx[(long)i * a.K + e], a.N);
  const int rj = k * a.N + j;
  int c1 = LOO_FW | j, c2 = LOO_FW | j;
  if (a.key[j] < a.key[i]) {
    const bool hid = a.leader[j] == a.leader[i];
    c1 = hid ? (LOO_FW | j) : rj;
    c2 = hid ? (LOO_OV | rj) : rj;
  }
  t.esrc[0][u] = c1;
  t.esrc[1][u] = c2;
  if (e == 0) {
    t.ctr[r] = i;
    t.msk[r] = a.mask[i];
    t.tok[r] = loo_clamp(a.seq[r], a.vocab);
    t.cen[0][r] = i;
    t.cen[1][r] = LOO_CEN_OV | r;
  }
}

// layer 1's rows with token, one per item row (k, j): Pfw_1[j] + tok_1[S_k[j]]  (mut_token_rows_kernel's arithmetic)
static __global__ __launch_bounds__(256) void tied_token_rows_kernel(const TiedArgs a, const float* __restrict__ Pfw, const float* __restrict__ tok,
                                                                      float* __restrict__ out) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  const long R = (long)a.n_chunk * a.N;
  if (u >= R * (NAMP_H / 4)) return;
  const long r = u / (NAMP_H / 4);
  const int c = (int)(u - r * (NAMP_H / 4)) * 4;
  const int j = (int)(r % a.N);
  const int tk = loo_clamp(a.seq[r], a.vocab);
  *(f4*)(out + r * NAMP_H + c) = *(const f4*)(Pfw + (long)j * NAMP_H + c) + *(const f4*)(tok + (long)tk * NAMP_H + c);
}

// one wave per item row: logits = W_out . h + b of the item's layer-3 state (lib_head_kernel's sums), the whole row kept
static __global__ __launch_bounds__(256) void tied_head_kernel(const TiedArgs a, const float* __restrict__ h3, const float* __restrict__ head_w,
                                                                const float* __restrict__ head_b, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (long)a.n_chunk * a.N) return;                     // (wave-uniform)
  if (lane >= a.vocab) return;
  const float* y = h3 + r * NAMP_H;
  const float* w = head_w + (long)lane * NAMP_H;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
  for (int c = 0; c < NAMP_H; c += 4) {
    const f4 wv = *(const f4*)(w + c);
    const f4 yv = *(const f4*)(y + c);
    s0 = fmaf(wv.x, yv.x, s0); s1 = fmaf(wv.y, yv.y, s1); s2 = fmaf(wv.z, yv.z, s2); s3 = fmaf(wv.w, yv.w, s3);
  }
  logits[r * a.vocab + lane] = (s0 + s1) + (s2 + s3) + head_b[lane];
}

// ---- host: the three item launches of a forced tied stream over R = n_chunk * N item rows (namp_tied.hip, and the base stream of the
// group scan, namp_group_scan.h, at n_chunk = 1).  T0 = the rows of the layer in front projected WITH the token (layer 1: tokrows),
// T1 = Pfw of the layer, T2 = the same rows projected WITHOUT the token (layer 1: Pfw_1).  The caller says where every layer's
// outputs go: hO[l] the states, PaO / bwO / nbO [l] the next layer's centres and its rows with and without token (l = 0, 1).  One
// sequence of launches, hence one summation order, for every caller.
struct TiedStreamRows {
  const float* Pa1;                  // [N][128] layer 1's centres
  const float* Pfw[3];               // [N][128]
  const float* tokrows;              // [R][128] layer 1's rows with token
  float* hO[3];                      // [R][128]
  float *PaO[2], *bwO[2], *nbO[2];   // [R][128]
};

static inline int tied_item_stream(const NampModelW* w, const int prec, const float* h_V_enc, const float* h_E, const int K, const long R,
                                   const TiedItemTables& tab, const TiedStreamRows& b, hipStream_t s) {
  const float* cenPa[3] = {b.Pa1, b.PaO[0], b.PaO[1]};
  const float* cenH[3] = {h_V_enc, b.hO[0], b.hO[1]};
  const float* T0[3] = {b.tokrows, b.bwO[0], b.bwO[1]};
  const float* T2[3] = {b.Pfw[0], b.nbO[0], b.nbO[1]};
  for (int l = 0; l < 3; ++l) {
    const NampDecLayerW* D = &w->dec[l];
    const int q = l ? 1 : 0;
    LooItemArgs it = loo_items(D, prec, h_E, K, R, nullptr, tab.ctr, tab.cen[q], tab.esrc[q], b.Pa1, cenPa[l], h_V_enc, cenH[l], T0[l], b.Pfw[l],
                               T2[l]);
    loo_tail(it.tail, D, tab.msk, tab.tok, b.hO[l]);
    if (l < 2) {
      const NampDecLayerW* Dn = &w->dec[l + 1];
      loo_proj(it.tail, Dn->W1a_img, Dn->b1, nullptr, b.PaO[l]);
      loo_proj(it.tail, Dn->W1v_img, nullptr, Dn->tok, b.bwO[l]);
      loo_proj(it.tail, Dn->W1v_img, nullptr, nullptr, b.nbO[l]);
    }
    const int rc = launch_items(it, prec, s);
    if (rc) return rc;
  }
  return NAMP_OK;
}

// One wave per (sequence k, residue g), lane = class; only the wave of a unit's leader works.  It walks the cycle (an ungrouped
// residue is a cycle of one) in listed order: per member the own log-softmax of its logits row (its own entry -> member_lp, with
// k = 0 the row -> log_probs) and, in a group, total[c] = sum_t w_t z_t[C_t[c]] (fma chain) + b[c] through the table of the LAST
// listed member, -inf where a member has no token for c; clp = log_softmax(total); the unit's value is the logsumexp of clp over the
// classes c with C_t[c] == S_k[m_t] for every member (-inf where there is none: the sequence breaks the tie), stored at every
// member's slot.  A unit of one is its own entry.  Table indices, table entries and tokens are clamped; one address per lane.
static __global__ __launch_bounds__(256) void tied_combine_kernel(const TiedArgs a, const float* __restrict__ logits, float* __restrict__ unit_lp,
                                                                   float* __restrict__ member_lp, float* __restrict__ log_probs) {
  const int lane = threadIdx.x & 63;
  const long wv = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long)a.n_chunk * a.N) return;                    // (wave-uniform)
  const int k = (int)(wv / a.N), g = (int)(wv - (long)k * a.N);
  if (a.leader[g] != g) return;                               // (wave-uniform)
  const long r0 = (long)k * a.N;
  const bool grouped = a.gl[g] >= 0;
  const int c = lane < a.n_classes ? lane : 0;
  float tot = 0.f, own_first = 0.f;
  bool have = lane < a.n_classes, match = lane < a.n_classes;
  int cur = g, last = g;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    const float* z = logits + (r0 + cur) * a.vocab;
    const int tk = loo_clamp(a.seq[r0 + cur], a.vocab);
    // the member's own log-softmax
    const float zl = lane < a.vocab ? z[lane] : -INFINITY;
    const float mx = tied_wave_max(zl);
    const float ex = tied_wave_sum(lane < a.vocab ? expf(zl - mx) : 0.f);
    const float lsm = (zl - mx) - logf(ex);
    if (lane == tk) member_lp[r0 + cur] = lsm;
    if (k == 0 && lane < a.vocab) log_probs[(long)cur * a.vocab + lane] = lsm;
    if (t == 0) own_first = __shfl(lsm, tk);
    if (!grouped) break;
    const int e = a.tables[loo_clamp(a.table_idx[cur], a.n_tables) * 64 + c];
    have = have && e >= 0;
    match = match && e == tk;
    const float zc = z[loo_clamp(e, a.vocab)];
    tot = t == 0 ? a.weight[cur] * zc : fmaf(a.weight[cur], zc, tot);
    last = cur;
    cur = loo_clamp(a.next[cur], a.N);
    if (cur == g) break;
  }
  if (!grouped) {
    if (lane == 0) unit_lp[r0 + g] = own_first;
    return;
  }
  tot = have ? tot + a.bias[loo_clamp(a.table_idx[last], a.n_tables) * 64 + c] : -INFINITY;
  const float mx = tied_wave_max(tot);
  float unit = -INFINITY;
  if (mx > -INFINITY) {                                       // (wave-uniform; else no class every member has: the unit is -inf)
    const float ex = tied_wave_sum(have ? expf(tot - mx) : 0.f);
    const float clp = have ? (tot - mx) - logf(ex) : -INFINITY;
    const float x = (have && match) ? clp : -INFINITY;
    const float m2 = tied_wave_max(x);
    if (m2 > -INFINITY) unit = m2 + logf(tied_wave_sum(x > -INFINITY ? expf(x - m2) : 0.f));
  }
  cur = g;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    if (lane == 0) unit_lp[r0 + cur] = unit;
    cur = loo_clamp(a.next[cur], a.N);
    if (cur == g) break;
  }
}
