// Leave-one-out conditional log-probs (namp_decoder_loo, include/namp.h): log p(s_i | X, S_-i) for EVERY residue i of a complex —
// row i of the parallel decoder (model_utils.py:391-421) run with the decoding order of score() in which i is moved to the end.
//
// Stream i differs from the base stream (the plain score() order) only inside a small dependency cone around i:
//   phase 1  layer-1 outputs of the residues m that used to see i as decoded (i in N(m), rank[i] < rank[m], mask[m] = 1): one edge of m
//            flips from backward to forward.  Item = the directed edge, slot (m, k) with E_idx[m, k] = i: an [L, K] grid of items;
//   phase 2  layer-2 outputs of i's own neighbours q = E_idx[i, kq], slot (i, kq), where a phase-1 output feeds them;
//   own      residue i itself, layers 1..3 with every neighbour backward (the self edge stays forward), then W_out + log_softmax.
// loo_prepare_kernel / loo_edges_kernel turn (E_idx, rank, mask) into per-item INDEX tables — which residue's h_E rows, which centre
// state and, per edge, which table row (base backward / base forward / an override row written by an earlier phase) — and
// dec_items_kernel is the DecLayer message MLP + K-sum + residue tail (model_utils.py:636-657) over a grid of such items: the body of
// edge_mlp_kernel<MODE_DEC_MSG> with the rank comparison replaced by indirection.  Every item owns its output rows (no atomics, two
// runs are bit-identical); phases are separate launches (nothing waits on the device).
//
// Group conditionals (namp_loo_groups): a tied group (m_1, ..., m_n), n <= NAMP_LOO_GROUP_MAX, in LISTED order shares
// ONE stream, the order of score() with all members taken out and appended as ..., m_1, ..., m_n, every member's token hidden.  The
// second instantiation of the table kernels (LOO_TIE_GROUPS): loo_groups_kernel turns the caller's successor cycle into (leader,
// listed position) per residue; a slot belongs to the stream of its neighbour's (phase 1) or owner's (phase 2, own) group, edges to ANY
// member are forward there, and a residue that used to see several members as decoded has as many phase-1 slots that compute the
// same rows (each item still owns its rows; readers take the active slot that names the earliest-listed member).  Member t reads an
// earlier-listed member that is its neighbour without its token — layer 1 from Pfw[0], layers 2 / 3 from rows G + n of that layer's
// forward table, which hold W1v . (n's own-layer state): with an attachment the forward tables of layers 2 and 3 have 2 G rows and
// the own launches project the second half (dec_items_kernel itself is unchanged) — and a later-listed one forward.
// loo_group_combine_kernel then sums the members' head rows through their token maps and writes every member's row.
//
// Pair conditionals (namp_loo_pairs) are the groups of two: a base pair's partner table IS its successor cycle, and
// namp_loo_pairs attaches what namp_loo_groups does.
//
// Pair classes (namp_loo_classes): the members speak through class tables instead of token maps (G-U wobble).
// Nothing in front of the combine changes — the stream hides every member's token —; the attachment swaps loo_group_combine_kernel
// for loo_class_combine_kernel, which also writes the class rows into an output section of the workspace.
#pragma once
#include "namp_kernels.h"

// table row code of the index tables: bits 28-29 = table (edges: 0 base backward Pbw, 1 forward Pfw, 2 override; centres: 0 base,
// 1 override), bits 0-27 = row
#define LOO_ROW_BITS 28
#define LOO_ROW_MASK ((1 << LOO_ROW_BITS) - 1)
#define LOO_FW (1 << LOO_ROW_BITS)
#define LOO_OV (2 << LOO_ROW_BITS)
#define LOO_CEN_OV (1 << LOO_ROW_BITS)

struct LooPrepArgs {
  const int32_t* E_idx;   // [G][K] neighbour ids, local to the complex
  const int32_t* rank;    // [G]
  const int32_t* mask;    // [G]
  const int32_t* S;       // [G]
  const int32_t* pp;      // [G] GROUPS launches: the leader (listed-first member, global index) of the residue's valid group or -1,
                          //     from loo_groups_kernel
  const int32_t* lead;    // [G] GROUPS launches: the residue's listed position (0: the leader, or ungrouped)
  int32_t* rev;           // [R] edge (a, k) -> b: position of a in E_idx[b], or -1
  int32_t* act1;          // [R] phase-1 item (m, k) is active
  int32_t* act2;          // [R] phase-2 item (i, kq) is active
  int32_t* ctr1;          // [R] centre residue of a phase-1 item (also its centre-state code: base row m)
  int32_t* ctr2;          // [R] centre residue q of a phase-2 item
  int32_t* cen2;          // [R] its centre-state code
  int32_t* msk1; int32_t* S1; int32_t* msk2; int32_t* S2;   // [R] mask / token of the items' centres
  int32_t* eo1; int32_t* eo2; int32_t* eo3;                  // [R] = [G][K] edge codes of residue i's own layers 1..3
  int32_t* idG; int32_t* ovG;                                // [G] centre codes of the own items: base row g / override row g
  int32_t* esrc1; int32_t* esrc2;                            // [R][K] edge codes of the phase-1 / phase-2 items
  int32_t* gkey;          // [R] GROUPS launches: stream << 4 | listed position of the member an ACTIVE phase-1 slot names, else -1
  int G, N, K;
};

__device__ __forceinline__ int loo_clamp(const int v, const int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the wave's max / sum in every lane: one butterfly order (o = 1, 2, .. 32) for the tied score and every scan; all 64 lanes take part
__device__ __forceinline__ float tied_wave_max(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ float tied_wave_sum(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// The caller's table is device data, a successor cycle in LISTED order (next[g] = local index of the member listed after g, the last
// names the first) with first[g] = 1 on the listed-first member.  One thread per residue walks its cycle, at most NAMP_LOO_GROUP_MAX
// steps.  g is grouped only if the walk returns to it, every successor on the way is inside [0, N), exactly one member carries
// `first` and no member is masked; a self-loop, a tail that leads into a cycle, a longer cycle: ungrouped.  Every member of a cycle
// walks the same members and reaches the same verdict.  gl[g] = the leader (global index) or -1, gpos[g] = g's listed position.
static __global__ __launch_bounds__(256) void loo_groups_kernel(const int32_t* __restrict__ next, const int32_t* __restrict__ first,
                                                                 const int32_t* __restrict__ mask, int32_t* __restrict__ gl,
                                                                 int32_t* __restrict__ gpos, const int G, const int N) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const int b0 = (g / N) * N;
  int cur = g, n = 0, firsts = 0, at = 0, leader = g;
  bool ok = true, closed = false;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    const int nx = next[cur];
    ok = ok && nx >= 0 && nx < N && mask[cur] != 0;
    if (first[cur] != 0) { ++firsts; at = t; leader = cur; }
    ++n;
    cur = b0 + loo_clamp(nx, N);
    if (cur == g) { closed = true; break; }
  }
  ok = ok && closed && n >= 2 && firsts == 1;
  gl[g] = ok ? leader : -1;
  gpos[g] = ok ? (at == 0 ? 0 : n - at) : 0;                 // (the leader sits `at` steps behind g on the cycle)
}

#define LOO_TIE_NONE 0
#define LOO_TIE_GROUPS 1

// groups: the active phase-1 slot of residue x (global) that names the earliest-listed member of stream `sid` (the leader of a
// group, or the residue of a stream of one), or -1: one pass over the keys loo_prepare_kernel left.  Duplicate slots are bounded by
// the group size.
__device__ __forceinline__ int loo_group_override(const LooPrepArgs& a, const int x, const int sid) {
  int ov = -1, best = NAMP_LOO_GROUP_MAX;
  for (int q = a.K - 1; q >= 0; --q) {
    const long sl = (long)x * a.K + q;
    const int key = a.gkey[sl];
    if (key >= 0 && (key >> 4) == sid && (key & 15) <= best) { best = key & 15; ov = (int)sl; }
  }
  return ov;
}

// one thread per slot r = (g, k): reverse-edge index, phase-1 flag, the phase-1 items' centres
// (TIE = LOO_TIE_NONE is the code of a call without an attachment: no table of the caller's is read)
template <int TIE>
static __global__ __launch_bounds__(256) void loo_prepare_kernel(const LooPrepArgs a) {
  constexpr bool GROUPS = TIE == LOO_TIE_GROUPS;
  const long R = (long)a.G * a.K;
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int g = (int)(r / a.K), k = (int)(r - (long)g * a.K);
  const int b0 = (g / a.N) * a.N, m_loc = g - b0;
  const int i_loc = loo_clamp(a.E_idx[r], a.N), i = b0 + i_loc;
  int p = -1;
  for (int q = a.K - 1; q >= 0; --q)
    if (a.E_idx[(long)i * a.K + q] == m_loc) p = q;
  a.rev[r] = p;
  const int li = GROUPS ? a.pp[i] : -1;                     // m is not an item of its own group's stream
  const bool same = GROUPS && li >= 0 && li == a.pp[g];
  const bool on1 = i_loc != m_loc && !same && a.rank[i] < a.rank[g] && a.mask[g] != 0;
  a.act1[r] = on1 ? 1 : 0;
  if (GROUPS) a.gkey[r] = on1 ? (((li >= 0 ? li : i) << 4) | a.lead[i]) : -1;     // (a listed position is below NAMP_LOO_GROUP_MAX = 16)
  a.ctr1[r] = g; a.msk1[r] = a.mask[g]; a.S1[r] = a.S[g];
  if (k == 0) { a.idG[g] = g; a.ovG[g] = LOO_CEN_OV | g; }
}

// one wave per slot r: the edge codes of the phase-1 item (m, k) and of the phase-2 item (i, kq) that share the slot, the phase-2
// flag and centre, and the edge codes of the own layers (after loo_prepare_kernel: reads rev / act1 of other slots)
template <int TIE>
static __global__ __launch_bounds__(256) void loo_edges_kernel(const LooPrepArgs a) {
  constexpr bool GROUPS = TIE == LOO_TIE_GROUPS;
  const long R = (long)a.G * a.K;
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                                       // (wave-uniform)
  const int g = (int)(r / a.K);
  const int b0 = (g / a.N) * a.N, c_loc = g - b0;           // g = the slot's residue: m of the phase-1 item, i of the phase-2 item
  const int n_loc = loo_clamp(a.E_idx[r], a.N), n = b0 + n_loc;   // its k-th neighbour: i of the phase-1 item, q of the phase-2 item
  const int rk_g = a.rank[g], rk_n = a.rank[n];
  // groups: the stream of the phase-1 item is that of n's group, the stream of the phase-2 item and of the own layers that of g's
  // group; streams are named by their leaders (-1: the residue alone)
  const int lg = GROUPS ? a.pp[g] : -1, ln = GROUPS ? a.pp[n] : -1;
  const bool grouped = lg >= 0;
  const int sid = grouped ? lg : g;
  // n's layer-1 override in stream g: the slot of n that names g if it is active (groups: the active slot that names the
  // earliest-listed member)
  const int pf = a.rev[r];                                  // position of g in E_idx[n]
  int ovn = -1;
  if (GROUPS) {
    ovn = loo_group_override(a, n, sid);
  } else {
    if (pf >= 0 && a.act1[(long)n * a.K + (pf >= 0 ? pf : 0)] != 0) ovn = (int)((long)n * a.K + pf);
  }
  const bool cen_ov = ovn >= 0;                             // n's layer-1 state is overridden in stream g
  bool any = false;
  for (int e = lane; e < a.K; e += 64) {
    // phase 1, item (m = g, i = n): edge e of m; the edges to i and to every member of i's group are forward now
    const int j_loc = loo_clamp(a.E_idx[(long)g * a.K + e], a.N), j = b0 + j_loc;
    const bool j_tied = GROUPS && ln >= 0 && a.pp[j] == ln;
    a.esrc1[r * a.K + e] = (j_loc == n_loc || j_tied || !(a.rank[j] < rk_g)) ? (LOO_FW | j) : j;
    // phase 2, item (i = g, q = n): edge e of q
    const int m_loc = loo_clamp(a.E_idx[(long)n * a.K + e], a.N), mm = b0 + m_loc;
    const bool m_tied = GROUPS && grouped && a.pp[mm] == lg;
    int code = LOO_FW | mm;
    if (m_loc != c_loc && !m_tied && a.rank[mm] < rk_n) {
      code = mm;
      int ov = -1;
      if (GROUPS) {
        ov = loo_group_override(a, mm, sid);
      } else {
        int p1 = -1;
        for (int q = a.K - 1; q >= 0; --q)
          if (a.E_idx[(long)mm * a.K + q] == c_loc) p1 = q;
        if (p1 >= 0 && a.act1[(long)mm * a.K + p1] != 0) ov = (int)((long)mm * a.K + p1);
      }
      if (ov >= 0) { code = LOO_OV | ov; any = true; }
    }
    a.esrc2[r * a.K + e] = code;
  }
  // the slot's neighbour is another member of g's group: no item, and its own edge codes
  const bool part = GROUPS && grouped && ln == lg && n_loc != c_loc;
  const bool on2 = n_loc != c_loc && !part && a.mask[n] != 0 && (cen_ov || __any(any));
  if (lane == 0) {
    a.act2[r] = on2 ? 1 : 0;
    a.ctr2[r] = n; a.msk2[r] = a.mask[n]; a.S2[r] = a.S[n];
    a.cen2[r] = cen_ov ? (LOO_CEN_OV | ovn) : n;
    // residue i = g itself: every neighbour backward, the self edge forward.  In a group member t sees every later-listed member
    // forward and every earlier-listed one backward but without its token: Pfw[0] in layer 1, rows G + n of the forward tables in
    // layers 2, 3.
    const bool self = n_loc == c_loc;
    const bool later = !(GROUPS && part && a.lead[n] < a.lead[g]);
    const int pc = LOO_FW | (later ? n : a.G + n);
    a.eo1[r] = (self || part) ? (LOO_FW | n) : n;
    a.eo2[r] = self ? (LOO_FW | g) : part ? pc : cen_ov ? (LOO_OV | ovn) : n;
    a.eo3[r] = self ? (LOO_FW | g) : part ? pc : on2 ? (LOO_OV | (int)r) : n;
  }
}

// counts[0] / counts[1] = active phase-1 / phase-2 items (one workgroup; integer sums: the order does not matter)
static __global__ __launch_bounds__(1024) void loo_count_kernel(const int32_t* __restrict__ act1, const int32_t* __restrict__ act2,
                                                                 int32_t* __restrict__ counts, const long R) {
  __shared__ int s1[16], s2[16];
  int c1 = 0, c2 = 0;
  for (long r = threadIdx.x; r < R; r += 1024) { c1 += act1[r]; c2 += act2[r]; }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); }
  if ((threadIdx.x & 63) == 0) { s1[threadIdx.x >> 6] = c1; s2[threadIdx.x >> 6] = c2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t1 = 0, t2 = 0;
    for (int w = 0; w < 16; ++w) { t1 += s1[w]; t2 += s2[w]; }
    counts[0] = t1; counts[1] = t2;
  }
}

// The input section of a call with an attachment (include/namp.h): int32 words next[G], first[G], map_idx[G], weight[G] (float bits),
// maps[n_maps][64].  One wave per group LEADER: it walks the cycle twice, total[a] = sum_t w_t z_t[P_t[a]] over the members in listed
// order from their head rows (log-softmax rows: they differ from the logits by one constant per member, which cancels; the fma chain
// of dec_sample_kernel), then lp = log_softmax(total) and row_m[b] = lp[P_m[b]] for every member (the maps are involutions, so this
// gather IS row_m[P_m[a]] = lp[a]; it stays a plain in-bounds store per lane whatever the maps hold).  Cycles are disjoint (one
// successor per residue), every read of a group's rows precedes its first write, and every load is clamped.
static __global__ __launch_bounds__(256) void loo_group_combine_kernel(float* __restrict__ log_probs, const int32_t* __restrict__ gl,
                                                                        const int32_t* __restrict__ next, const int32_t* __restrict__ map_idx,
                                                                        const float* __restrict__ weight, const int32_t* __restrict__ maps,
                                                                        const int n_maps, const int vocab, const int G, const int N) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G || gl[g] != g) return;                          // (wave-uniform)
  const int b0 = (g / N) * N;
  const int a = lane < vocab ? lane : 0;
  float tot = 0.f;
  int cur = g;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    const int P = loo_clamp(maps[loo_clamp(map_idx[cur], n_maps) * 64 + a], vocab);
    const float z = log_probs[(long)cur * vocab + P];
    tot = t == 0 ? weight[cur] * z : fmaf(weight[cur], z, tot);
    cur = b0 + loo_clamp(next[cur], N);
    if (cur == g) break;
  }
  if (lane >= vocab) tot = -INFINITY;
  float mx = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float e = (lane < vocab) ? expf(tot - mx) : 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) e += __shfl_xor(e, o);
  const float lp = (tot - mx) - logf(e);
  cur = g;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    const int P = loo_clamp(maps[loo_clamp(map_idx[cur], n_maps) * 64 + a], vocab);
    const float row = __shfl(lp, P);
    if (lane < vocab) log_probs[(long)cur * vocab + lane] = row;
    cur = b0 + loo_clamp(next[cur], N);
    if (cur == g) break;
  }
}

// Pair classes (namp_loo_classes): the members speak through CLASS TABLES instead of token maps — tables[ti][c] = the
// member's token under class c, below 0: no such class — and the input section holds bias[n_tables][64] behind the tables.  One wave
// per residue, lane = class; a wave that is no leader of a valid group (gl, and the walk of loo_group_combine_kernel over the
// caller's successor cycle) writes a class row of -inf and ends.  The leader forms
//   total[c] = sum_t w_t z_t[C_t[c]] + b[c]   (listed order, the fma chain of the kernels above; b through the table index of the LAST
//                                              listed member, added once), -inf where some member has no token for c or c >= n_classes,
//   clp = log_softmax(total)                  (the butterfly of loo_group_combine_kernel: absent lanes add the zeros the lanes >= vocab add there),
//   row_m[t] = clp[C_m[t]], and for the classes c = vocab .. n_classes - 1 in ascending order with C_m[c] == t: log-add-exp(row_m[t], clp[c])
// (below the vocabulary a table is a token map, an involution: the one class with C_m[c] == t is c = C_m[t]), and writes every
// member's row and, at its own index, the class row [64].  Every read of a group's rows precedes its first write; every table index
// and entry is clamped, the fetch of an absent lane reads a clamped address and its sum is not used; plain stores, one address per
// lane.  A group none of whose classes is present keeps its leave-one-out rows.
static __global__ __launch_bounds__(256) void loo_class_combine_kernel(float* __restrict__ log_probs, const int32_t* __restrict__ gl,
                                                                        const int32_t* __restrict__ next,
                                                                        const int32_t* __restrict__ tab_idx, const float* __restrict__ weight,
                                                                        const int32_t* __restrict__ tables, const float* __restrict__ bias,
                                                                        float* __restrict__ cls, const int n_tables, const int n_classes,
                                                                        const int vocab, const int G, const int N) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                        // (wave-uniform)
  if (gl[g] != g) {
    cls[(long)g * 64 + lane] = -INFINITY;
    return;
  }
  const int b0 = (g / N) * N;
  const int c = lane < n_classes ? lane : 0;
  float tot = 0.f;
  bool have = lane < n_classes;
  int cur = g, last = g;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    const int e = tables[loo_clamp(tab_idx[cur], n_tables) * 64 + c];
    have = have && e >= 0;
    const float z = log_probs[(long)cur * vocab + loo_clamp(e, vocab)];
    tot = t == 0 ? weight[cur] * z : fmaf(weight[cur], z, tot);
    last = cur;
    cur = b0 + loo_clamp(next[cur], N);
    if (cur == g) break;
  }
  tot = have ? tot + bias[loo_clamp(tab_idx[last], n_tables) * 64 + c] : -INFINITY;
  float mx = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (!(mx > -INFINITY)) {                                   // (wave-uniform: no class, or nothing but -inf / NaN totals)
    cls[(long)g * 64 + lane] = -INFINITY;
    return;
  }
  float ex = have ? expf(tot - mx) : 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) ex += __shfl_xor(ex, o);
  const float clp = have ? (tot - mx) - logf(ex) : -INFINITY;
  cls[(long)g * 64 + lane] = clp;
  const int tk = lane < vocab ? lane : 0;
  cur = g;
  for (int t = 0; t < NAMP_LOO_GROUP_MAX; ++t) {
    const int32_t* tab = tables + loo_clamp(tab_idx[cur], n_tables) * 64;
    const int e_own = tab[tk];                               // the class below the vocabulary that gives this lane's token
    const int e_cls = tab[c];                                // the token this lane's class gives the member
    float row = __shfl(clp, loo_clamp(e_own, vocab));
    if (e_own < 0) row = -INFINITY;
    for (int k = vocab; k < n_classes; ++k) {
      const float x = __shfl(clp, k);
      const int tok = __shfl(e_cls, k);
      if (tok == lane && x > -INFINITY) {
        const float m = fmaxf(row, x);
        row = row > -INFINITY ? m + logf(expf(row - m) + expf(x - m)) : x;
      }
    }
    if (lane < vocab) log_probs[(long)cur * vocab + lane] = row;
    cur = b0 + loo_clamp(next[cur], N);
    if (cur == g) break;
  }
}

struct LooItemArgs {
  const float* hE;             // [G*K][128] encoder edge rows
  const int32_t* act;          // [R] item flags (null: every item is active)
  const int32_t* ctr;          // [R] residue whose h_E row block the item reads
  const int32_t* cen;          // [R] centre code: table 0 -> Pa0 / hV0, table 1 -> Pa1 / hV1
  const int32_t* esrc;         // [R][K] edge codes: table 0 -> T0, 1 -> T1, 2 -> T2
  const float* Pa0; const float* Pa1;     // W1a . (centre state) + b1
  const float* hV0; const float* hV1;     // centre state (the layer's input)
  const float* T0; const float* T1; const float* T2;   // base Pbw, Pfw, override Pbw rows of this layer
  const float* W1_img; const float* W2_img; const float* b2;   // per-edge images in the launch's precision
  const float* m3_img; const float* m3_b;                       // fp32 image of W3 (hoisted behind the K-sum), b3
  NodeTail tail;               // mask / S / outputs indexed by item row; hV and m3_img are not used (see cen, m3_img above)
  int R, K, TPN;
};

// 2 weight images | per-wave K-sums [12][128] + weight sums [16] | per-item K-sums [16][128] + weight sums [16] | active list [16] + count
#define LOO_ITEMS_LDS (2 * NAMP_IMG_BYTES + 12 * NAMP_H * 4 + 64 + 16 * NAMP_H * 4 + 64 + 128)
static_assert(NODE_TAIL_LDS <= 2 * NAMP_IMG_BYTES, "the residue tail re-uses the weight ring");

// Workgroup = 16 consecutive item rows (one 16-row tile of the residue tail), 12 waves.  The active items of the tile run the message
// MLP in rounds of 12 / TPN items (one 16-edge tile per wave, W1 / W2 resident in LDS across rounds); their K-sums meet in LDS and ONE
// residue tail (node_tail, the 16-row MFMA form) finishes the tile.  Rows of inactive items are written too (a zero message: never read).
template <int PREC>
__global__ __launch_bounds__(768) void dec_items_kernel(const LooItemArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool X3 = (PREC == PREC_X3);
  char* buf0 = smem;
  char* buf1 = smem + NAMP_IMG_BYTES;
  float* dpart = (float*)(smem + 2 * NAMP_IMG_BYTES);       // [12][128] per-wave tile sums of a round
  float* dws = dpart + 12 * NAMP_H;                          // [16]
  float* ksum = dws + 16;                                    // [16][128] per-item K-sums, by tile row
  float* kws = ksum + 16 * NAMP_H;                           // [16]
  int* list = (int*)(kws + 16);                              // [16] tile rows of the active items, [16] = their number
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwaves = blockDim.x >> 6;
  const int m = lane & 15, g = lane >> 4;
  const int bid = xcd_block_index(blockIdx.x, gridDim.x);
  const int row0 = bid * 16;

  if (wave == 0) {
    const int r = row0 + m;
    const int rc = r < a.R ? r : row0;
    const bool on = lane < 16 && r < a.R && (a.act == nullptr || a.act[rc] != 0);
    const unsigned long long bal = __ballot(on);
    if (on) list[__popcll(bal & ((1ull << lane) - 1ull))] = lane;
    if (lane == 0) list[16] = __popcll(bal);
  }
  for (int i = tid; i < 16 * NAMP_H + 16; i += (int)blockDim.x) ksum[i] = 0.f;
  __syncthreads();
  const int nact = list[16];
  if (nact == 0) return;                                     // (uniform)

  const int npw = nwaves / a.TPN;                            // items per round
  const int node_l = wave / a.TPN, kt = wave - node_l * a.TPN;
  const f4* w0 = (const f4*)buf0 + lane;
  const f4* w1 = (const f4*)buf1 + lane;
  f4 x[8], acc[8], pjv[8];
  bool first = true;
  for (int base = 0; base < nact; base += npw) {
    const int idx = base + node_l;
    const bool wact = node_l < npw && idx < nact;
    const int trow = list[wact ? idx : 0];
    const int row = row0 + trow;
    const int k = 16 * kt + m;
    const bool valid = wact && k < a.K;
    const int kc = valid ? k : 0;
    {
      const float* src = a.hE + ((long)a.ctr[row] * a.K + kc) * NAMP_H + 4 * g;
#pragma unroll
      for (int t = 0; t < 8; ++t) x[t] = *(const f4*)(src + 16 * t);
      const int cc = a.cen[row];
      const float* pa = ((cc >> LOO_ROW_BITS) ? a.Pa1 : a.Pa0) + (long)(cc & LOO_ROW_MASK) * NAMP_H + 4 * g;
      const int ec = a.esrc[(long)row * a.K + kc];
      const int et = ec >> LOO_ROW_BITS;
      const float* pj = (et == 0 ? a.T0 : et == 1 ? a.T1 : a.T2) + (long)(ec & LOO_ROW_MASK) * NAMP_H + 4 * g;
#pragma unroll
      for (int t = 0; t < 8; ++t) { acc[t] = *(const f4*)(pa + 16 * t); pjv[t] = *(const f4*)(pj + 16 * t); }
    }
    const float w_row = valid ? (1.0f / 30.0f) : 0.f;
    if (first) {
      // weight staging behind the first round's operand loads (the vector-memory counter retires in order)
      dma_to_lds(buf0, a.W1_img, 64, wave, nwaves, lane);
      dma_to_lds(buf1, a.W2_img, 64, wave, nwaves, lane);
      wait_dma_and_sync();
      first = false;
    }
    // layer 1 (T): Pa + W1e . h_E + table row; layer 2 (F): lane (m, g) gets rows 4g..4g+3 of channel 16t + m
    gemm128<X3, false, false>(acc, x, w0);
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] += pjv[t];
#pragma unroll
    for (int t = 0; t < 8; ++t) { const float b = a.b2[16 * t + m]; x[t] = (f4){b, b, b, b}; }
    gemm128<X3, true, true>(x, acc, w1);
    // K-sum of the layer-2 activations over the tile's 16 edges (layer 3 follows per item)
    float wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wr[r] = __shfl(w_row, 4 * g + r);
    float wsum = w_row;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) wsum += __shfl_xor(wsum, o);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const f4 v = gelu_prec<PREC>(x[t]);
      float s = (v.x * wr[0] + v.y * wr[1]) + (v.z * wr[2] + v.w * wr[3]);
      s = xg_sum(s);
      if (g == 0) dpart[wave * NAMP_H + 16 * t + m] = s;
    }
    if (lane == 0) dws[wave] = wsum;
    __syncthreads();
    // the round's items: tile sums -> the item's row (fixed order: two runs agree bit for bit)
    for (int u = tid; u < npw * NAMP_H; u += (int)blockDim.x) {
      const int il = u >> 7, ch = u & 127;
      if (base + il < nact) {
        float s = 0.f, ws = 0.f;
        for (int q = 0; q < a.TPN; ++q) { s += dpart[(il * a.TPN + q) * NAMP_H + ch]; ws += dws[il * a.TPN + q]; }
        const int tr = list[base + il];
        ksum[tr * NAMP_H + ch] = s;
        if (ch == 0) kws[tr] = ws;
      }
    }
    __syncthreads();
  }

  // ---- residue tail over the tile: x = centre state + W3 . K-sum + b3 * weight sum, then node_tail (LN1, FFN, LN2, mask, projections, head)
#pragma unroll
  for (int t = 0; t < 8; ++t) x[t] = *(const f4*)(ksum + m * NAMP_H + 16 * t + 4 * g);
  const float wsum_m = kws[m];
  float* ys = (float*)smem + 16 * FFN_LD;
  if (wave < 8) {
    f4 o[1] = {*(const f4*)(a.m3_b + 16 * wave + 4 * g) * wsum_m};
    chain_gemm_global<8, 1, false>(o, x, (const f4*)a.m3_img + wave * 64 + lane, 8);
    *(f4*)(ys + m * FFN_LD + 16 * wave + 4 * g) = o[0];
  }
  __syncthreads();
  {
    const int r = row0 + m;
    const int cc = a.cen[r < a.R ? r : row0];
    const float* hsrc = ((cc >> LOO_ROW_BITS) ? a.hV1 : a.hV0) + (long)(cc & LOO_ROW_MASK) * NAMP_H + 4 * g;
#pragma unroll
    for (int t = 0; t < 8; ++t) x[t] = *(const f4*)(hsrc + 16 * t) + *(const f4*)(ys + m * FFN_LD + 16 * t + 4 * g);
  }
  const int nrows = a.R - row0 < 16 ? a.R - row0 : 16;
  node_tail<false>(a.tail, x, 0.f, row0, nrows, a.R, (float*)smem, tid, wave, nwaves, lane);
}

// ---- host helpers of the translation units that launch dec_items_kernel (namp_loo.hip, namp_library.hip): each unit holds its own
// instances of the kernel, so each sets their attributes once
#include <cstdio>
#include <mutex>

__attribute__((visibility("hidden"))) int namp_internal_fail(int code, const char* msg);

static inline hipError_t loo_items_ready() {
  static std::once_flag once;
  static hipError_t err = hipSuccess;
  std::call_once(once, [] {
    auto set = [](const void* f) {
      hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LOO_ITEMS_LDS);
      if (e != hipSuccess) err = e;
    };
    set((const void*)dec_items_kernel<PREC_F32>);
    set((const void*)dec_items_kernel<PREC_X3>);
  });
  return err;
}

// what dec_items_kernel needs of the weights: three decoder layers of one precision (split-bf16 or exact fp32) with their images
static inline int loo_check_weights(const NampModelW* w, const char* who, int* prec_out) {
  char buf[256];
  auto bad = [&](const char* fmt, long v) {
    char f[224];
    snprintf(f, sizeof(f), "%s: %s", who, fmt);
    snprintf(buf, sizeof(buf), f, v);
    return namp_internal_fail(NAMP_EINVAL, buf);
  };
  if (w->n_dec != 3) return bad("the cone kernels walk three decoder layers (n_dec=%ld): use the L-stream form", w->n_dec);
  if (w->vocab < 1 || w->vocab > 64) return bad("vocab=%ld out of range", w->vocab);
  int prec = PREC_F32;
  for (int l = 0; l < 3; ++l) {
    const NampDecLayerW* D = &w->dec[l];
    if (D->flags & NAMP_FLAG_BF16) return bad("split-bf16 and exact fp32 evaluation only (layer %ld is bf16)", l);
    const int p = (D->flags & NAMP_FLAG_X3) ? PREC_X3 : PREC_F32;
    if (l && p != prec) return bad("the decoder layers must share one precision (layer %ld)", l);
    prec = p;
    const void* need[] = {D->W1a_img, D->W1e_img, D->W1v_img, D->b1, D->tok, D->W2_img, D->b2, D->W3_img, D->b3, D->Win_img, D->b_in,
                          D->Wout_img, D->b_out, D->ln1_g, D->ln1_b, D->ln2_g, D->ln2_b, p == PREC_X3 ? D->W1e_ximg : D->W1e_img,
                          p == PREC_X3 ? D->W2_ximg : D->W2_img};
    for (const void* q : need)
      if (!q || ((uintptr_t)q & 15u)) return bad("decoder layer %ld lacks a weight image (or it is misaligned)", l);
  }
  if (!w->Wout_w || !w->Wout_b) return bad("null output head (vocab=%ld)", w->vocab);
  *prec_out = prec;
  return NAMP_OK;
}

// the arguments of one launch over `rows` items of decoder layer D (the tail is filled by loo_tail / loo_proj)
static inline LooItemArgs loo_items(const NampDecLayerW* D, const int prec, const float* h_E, const int K, const long rows, const int32_t* act,
                                    const int32_t* ctr, const int32_t* cen, const int32_t* esrc, const float* Pa0, const float* Pa1,
                                    const float* hV0, const float* hV1, const float* T0, const float* T1, const float* T2) {
  LooItemArgs a = {};
  a.hE = h_E; a.act = act; a.ctr = ctr; a.cen = cen; a.esrc = esrc; a.Pa0 = Pa0; a.Pa1 = Pa1; a.hV0 = hV0; a.hV1 = hV1;
  a.T0 = T0; a.T1 = T1; a.T2 = T2;
  a.W1_img = prec == PREC_X3 ? D->W1e_ximg : D->W1e_img; a.W2_img = prec == PREC_X3 ? D->W2_ximg : D->W2_img; a.b2 = D->b2;
  a.m3_img = D->W3_img; a.m3_b = D->b3;
  a.R = (int)rows; a.K = K;
  return a;
}

static inline int launch_items(LooItemArgs a, int prec, hipStream_t s) {
  a.TPN = (a.K + 15) / 16;
  a.tail.m3_img = nullptr; a.tail.m3_b = nullptr; a.tail.hV = nullptr;
  const int grid = (a.R + 15) / 16;
  if (prec == PREC_X3) hipLaunchKernelGGL(dec_items_kernel<PREC_X3>, dim3(grid), dim3(768), LOO_ITEMS_LDS, s, a);
  else hipLaunchKernelGGL(dec_items_kernel<PREC_F32>, dim3(grid), dim3(768), LOO_ITEMS_LDS, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  return NAMP_OK;
}

static inline void loo_tail(NodeTail& t, const NampDecLayerW* D, const int32_t* mask, const int32_t* S, float* hV_out) {
  t = NodeTail{};
  t.mask = mask; t.S = S; t.hV_out = hV_out;
  t.ln1_g = D->ln1_g; t.ln1_b = D->ln1_b; t.Win_img = D->Win_img; t.b_in = D->b_in; t.Wout_img = D->Wout_img; t.b_out = D->b_out;
  t.ln2_g = D->ln2_g; t.ln2_b = D->ln2_b;
}

static inline void loo_proj(NodeTail& t, const float* img, const float* bias, const float* tok, float* out) {
  ProjDesc& p = t.p[t.nproj++];
  p.img = img; p.bias = bias; p.tok = tok; p.out = out;
}

// ---- the BASE STREAM of the calls that ride on namp_decoder_fwd with items on top (namp_library.hip, namp_mutations.hip; both include
// include/namp.h first): one pass over S at B = 1 through the library's own building blocks that keeps the tables and states of all
// three layers, with the head -> log_probs.  One sequence of launches, hence one summation order, for every such call.
struct LooBaseStream {
  float *Pa1, *Pbw1, *Pfw[3], *h1, *Pa2, *Pbw2, *h2, *Pa3, *Pbw3, *h3;     // [N][128] each
  float* partial;                                                          // [N][ceil(K / 16)][129] (+ 3) of the unfused form
};

static inline int loo_base_stream(const NampModelW* w, const LooBaseStream& b, const float* h_V_enc, const float* h_E, const int32_t* E_idx,
                                  const int32_t* S, const int32_t* mask, const int32_t* rank, float* log_probs, int N, int K, void* stream) {
  const NampDecLayerW *D0 = &w->dec[0], *D1 = &w->dec[1], *D2 = &w->dec[2];
  int rc;
  NampProj pf[5] = {{D0->W1v_img, nullptr, nullptr, b.Pfw[0]}, {D1->W1v_img, nullptr, nullptr, b.Pfw[1]}, {D2->W1v_img, nullptr, nullptr, b.Pfw[2]},
                    {D0->W1a_img, D0->b1, nullptr, b.Pa1}, {D0->W1v_img, nullptr, D0->tok, b.Pbw1}};
  if ((rc = namp_node_linear(h_V_enc, S, 1, 1, N, pf, 5, nullptr, stream))) return rc;
  const bool fused = N <= namp_fused_tail_max_residues();
  const float* Pa[3] = {b.Pa1, b.Pa2, b.Pa3};
  const float* Pbw[3] = {b.Pbw1, b.Pbw2, b.Pbw3};
  const float* hin[3] = {h_V_enc, b.h1, b.h2};
  float* hout[3] = {b.h1, b.h2, b.h3};
  for (int l = 0; l < 3; ++l) {
    const NampDecLayerW* D = &w->dec[l];
    const bool last = l == 2;
    NampProj pn[2] = {{}, {}};
    if (!last) {
      const NampDecLayerW* Dn = &w->dec[l + 1];
      pn[0] = {Dn->W1a_img, Dn->b1, nullptr, l ? b.Pa3 : b.Pa2};
      pn[1] = {Dn->W1v_img, nullptr, Dn->tok, l ? b.Pbw3 : b.Pbw2};
    }
    if (fused) {
      if ((rc = namp_dec_message_update(D, h_E, E_idx, rank, Pa[l], Pbw[l], b.Pfw[l], hin[l], mask, hout[l], pn, last ? 0 : 2, S,
                                        last ? w->Wout_w : nullptr, w->Wout_b, log_probs, nullptr, w->vocab, 1, 1, N, K, stream)))
        return rc;
    } else {
      if ((rc = namp_dec_message(D, h_E, E_idx, rank, Pa[l], Pbw[l], b.Pfw[l], b.partial, 1, 1, N, K, stream))) return rc;
      if ((rc = namp_node_update(D->ln1_g, D->ln1_b, D->Win_img, D->b_in, D->Wout_img, D->b_out, D->ln2_g, D->ln2_b, hin[l], b.partial,
                                 D->W3_img, D->b3, mask, hout[l], pn, last ? 0 : 2, S, N, K, stream)))
        return rc;
    }
  }
  if (!fused && (rc = namp_logits_log_softmax(w->Wout_w, w->Wout_b, b.h3, log_probs, nullptr, N, w->vocab, stream))) return rc;
  return NAMP_OK;
}

// ---- the ITEM LAYERS on top of the base stream (namp_library.hip, namp_mutations.hip): per layer the caller's table kernel, then one
// dec_items_kernel launch over R[l] items whose centre overrides and override rows come from the layer in front
struct LooItemRows {
  float* ov1;                        // layer 1's override rows (from the tokens)
  float *hO[3], *PaO[2], *ovO[2];    // [R_l][128] outputs of layer l's items: states, and the next layer's centre / override rows
};

// tables(l, R): enqueues the launch that fills tab[l] for R items.  An empty layer ends the walk (stop_at_empty) or is stepped over.
// both_rows: ovO[l] holds 2 R rows, the next layer's rows WITHOUT the token behind those with it (the group scan, namp_group_scan.h).
template <class Tables, class LaunchTables>
static inline int loo_item_layers(const NampModelW* w, int prec, const float* h_V_enc, const float* h_E, int K, const LooBaseStream& b,
                                  const LooItemRows& o, const Tables* tab, const long* R, bool stop_at_empty, hipStream_t s,
                                  LaunchTables tables, bool both_rows = false) {
  const float* Pa[3] = {b.Pa1, b.Pa2, b.Pa3};
  const float* Pbw[3] = {b.Pbw1, b.Pbw2, b.Pbw3};
  const float* hin[3] = {h_V_enc, b.h1, b.h2};
  const float* cenPa[3] = {b.Pa1, o.PaO[0], o.PaO[1]};
  const float* cenH[3] = {h_V_enc, o.hO[0], o.hO[1]};
  const float* ov[3] = {o.ov1, o.ovO[0], o.ovO[1]};
  for (int l = 0; l < 3; ++l) {
    if (R[l] == 0) {
      if (stop_at_empty) break;
      continue;
    }
    const NampDecLayerW* D = &w->dec[l];
    const Tables& t = tab[l];
    tables(l, R[l]);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
    LooItemArgs a = loo_items(D, prec, h_E, K, R[l], t.act, t.ctr, t.cen, t.esrc, Pa[l], cenPa[l], hin[l], cenH[l], Pbw[l], b.Pfw[l], ov[l]);
    loo_tail(a.tail, D, t.msk, t.tok, o.hO[l]);
    if (l < 2) {
      const NampDecLayerW* Dn = &w->dec[l + 1];
      loo_proj(a.tail, Dn->W1a_img, Dn->b1, nullptr, o.PaO[l]);
      loo_proj(a.tail, Dn->W1v_img, nullptr, Dn->tok, o.ovO[l]);
      if (both_rows) loo_proj(a.tail, Dn->W1v_img, nullptr, nullptr, o.ovO[l] + R[l] * NAMP_HIDDEN);
    }
    const int rc = launch_items(a, prec, s);
    if (rc) return rc;
  }
  return NAMP_OK;
}
