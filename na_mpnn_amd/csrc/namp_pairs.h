#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// ---- base-paired design: the plan of a design whose symmetry groups are all pairs (namp_pairs_plan / namp_pairs_work_lists, include/namp.h) ----
// Every stream of the call decodes ONE complex in ONE order (stream 0's, order0): a residue reached first in order0 emits its group — itself,
// or its pair in LISTED order (first[i] = 1: residue i is the pair's first listed member) — exactly what symmetry_visits() builds on the host
// from a Python loop over the L steps.  Here: one workgroup, every thread owns a run of consecutive steps, counts the visits its steps emit
// (0: the partner came earlier; 1: unpaired; 2: a pair), the counts are scanned over the workgroup and the visits written at their offsets.
// Plain stores, no atomics: two calls give identical arrays.
struct PairsPlan {
  const int32_t* partner;      // [L] the residue paired with residue i, -1: unpaired
  const int32_t* first;        // [L] 1: residue i is listed first in its pair
  const int32_t* order0;       // [L] the one decoding order
  const int32_t* rank0;        // [L] its inverse
  int32_t* order;              // [B_dec][L] residues by visit
  int32_t* rank;               // [B_dec][L] visit of a residue
  int32_t* group_first;        // [B_dec][L] by visit
  int32_t* group_last;         // [B_dec][L] by visit
  int B_dec, L;
};

static __global__ __launch_bounds__(1024) void pairs_plan_kernel(const PairsPlan p) {
  __shared__ int part[1024];
  const int tid = threadIdx.x, L = p.L;
  const int per = (L + 1023) / 1024;
  const int t0 = tid * per, t1 = min(L, t0 + per);
  // visits emitted at step t: the step's residue and, if it has one, its partner — unless the partner's step came first
  auto emits = [&](const int t, int& i, int& q) {
    i = p.order0[t];
    i = i < 0 ? 0 : (i >= L ? L - 1 : i);
    q = p.partner[i];
    if ((unsigned)q >= (unsigned)L || q == i) { q = -1; return 1; }
    return p.rank0[q] > t ? 2 : 0;
  };
  int sum = 0;
  for (int t = t0; t < t1; ++t) { int i, q; sum += emits(t, i, q); }
  part[tid] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int v0 = part[tid] - sum;
  for (int t = t0; t < t1; ++t) {
    int i, q;
    const int n = emits(t, i, q);
    if (n == 0 || v0 + n > L) continue;                         // (v0 + n <= L whenever partner is a proper pairing)
    const int a = (n == 2 && !p.first[i]) ? q : i, b2 = (n == 2) ? (a == i ? q : i) : -1;
    for (int b = 0; b < p.B_dec; ++b) {
      const long r = (long)b * L;
      p.order[r + v0] = a; p.rank[r + a] = v0; p.group_first[r + v0] = v0; p.group_last[r + v0] = n == 1;
      if (n == 2) { p.order[r + v0 + 1] = b2; p.rank[r + b2] = v0 + 1; p.group_first[r + v0 + 1] = v0; p.group_last[r + v0 + 1] = 1; }
    }
    v0 += n;
  }
}

// The level-sorted work lists of namp_decoder_sample_walk for groups kept as WHOLE items (level_work_lists(split = False) on the host: a
// stable argsort by level, bincounts, cumulative sums, and .nonzero() read back): level [L] by visit (namp_sample_levels_dep; the streams share
// one order and one graph, so row 0 holds every stream's levels), group_first [L] by visit.  An item is a group's first visit; inside a level
// the items run stream-major, then by visit: item (b, v) of level l sits at g[l] * B_dec + b * c[l] + (number of items of level l before v),
// g = the exclusive scan of the per-level counts c.  One workgroup; the counts through LDS atomics as in work_lists_kernel (integer adds:
// the result does not depend on their order), the place of an item among its level's by counting — no cursor, hence a stable sort.
#define PAIRS_LISTS_LDS(L) ((2 * (size_t)(L) + 2) * 4)
static __global__ __launch_bounds__(1024) void pairs_work_lists_kernel(const int32_t* __restrict__ level, const int32_t* __restrict__ group_first,
                                                                        int B_dec, int L, int32_t* __restrict__ work, int32_t* __restrict__ work_n,
                                                                        int32_t* __restrict__ level_off, int32_t* __restrict__ n_levels) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* lvh = (int*)smem;                    // [L] level of the item that starts at visit v, -1: no item starts there
  int* cnt = lvh + L;                       // [L + 2] items per level, then the offsets
  __shared__ int part[1024];
  __shared__ int nz;
  const int tid = threadIdx.x, nb = L + 1;
  for (int i = tid; i < nb + 1; i += 1024) cnt[i] = 0;
  if (tid == 0) nz = 0;
  __syncthreads();
  for (int v = tid; v < L; v += 1024) {
    const int l = level[v];
    const int lc = l < 0 ? 0 : (l > L ? L : l);
    const bool head = group_first[v] == v;
    lvh[v] = head ? lc : -1;
    if (head) atomicAdd(&cnt[lc], 1);
  }
  __syncthreads();
  // exclusive scan of cnt[0 .. nb): thread t owns entries [t * per, (t + 1) * per)
  const int per = (nb + 1023) / 1024;
  int sum = 0, mine_nz = 0;
  for (int q = 0; q < per; ++q) { const int i = tid * per + q; if (i < nb) { sum += cnt[i]; mine_nz += cnt[i] > 0; } }
  part[tid] = sum;
  if (mine_nz) atomicAdd(&nz, mine_nz);
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int q = 0; q < per; ++q) {
    const int i = tid * per + q;
    if (i < nb) { const int c = cnt[i]; cnt[i] = run; level_off[i] = run * B_dec; run += c; }
  }
  if (tid == 1023) { cnt[nb] = part[1023]; level_off[nb] = part[1023] * B_dec; }
  if (tid == 0) n_levels[0] = nz;
  __syncthreads();
  const int items = cnt[nb];
  for (int v = tid; v < L; v += 1024) {
    const int l = lvh[v];
    if (l < 0) continue;
    int place = 0;
    for (int u = 0; u < v; ++u) place += lvh[u] == l;
    int n = 1;
    while (v + n < L && group_first[v + n] == v) ++n;
    const int g = cnt[l], c = cnt[l + 1] - g;
    for (int b = 0; b < B_dec; ++b) {
      const int pos = g * B_dec + b * c + place;
      if (pos >= items * B_dec) continue;
      work[2 * pos] = b; work[2 * pos + 1] = v; work_n[pos] = n;
    }
  }
}
