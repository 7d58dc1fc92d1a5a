#pragma once
#include "namp_kernels.h"

// ---- tied states: the plan of one sequence sampled over M backbone states (namp_states_plan, include/namp.h) --------------------------------
// The M states of L residues are one symmetric design on the block-diagonal flattened graph of M * L residues (flat residue m * L + i;
// visit t * M + m = residue order0[t] of state m; the M copies of a residue are a symmetry group).  The group of residue i takes the level
// 1 + the highest level among the neighbours of ALL its members that are decoded before it — neighbour j of state m belongs to group j,
// and it comes earlier iff rank0[j] < t — so the levels live per residue, [L], and are the same for every sample stream.
//
// Workgroup 0: wave 0 walks the L steps (sample_levels_kernel walks M * L visits, with global loads of the ranks and of group_first /
// group_last on each).  The levels start at -1 = "not decoded yet": the walk is sequential, so at step t exactly the residues decoded
// before t hold a level, and a step is the maximum over the M * K look-ups lv[E_idx[m][i][k]] with no rank to compare.  The look-ups sit
// NPF per lane, addressed through per-lane offsets that do not change over the walk, and their neighbour indices are requested TWO steps
// ahead (two register sets, the loop handles two steps per turn): what stays on a step's chain is the LDS look-up and one wave maximum.
// The same lane-0 store that publishes a level also takes the step's place among the steps of its level (a counter per level in LDS):
// a stable counting sort with no atomics.  Then the whole workgroup scans the counters and writes the level-sorted lists in the layout
// level_work_lists() gives (stream-major inside a level, then by visit).  Workgroups 1 ..: the flattened arrays, grid-stride.
struct StatesPlan {
  const int32_t* E_idx;        // [M][L][K]
  const int32_t* order0;       // [L]
  const int32_t* rank0;        // [L]
  const float* w;              // [M]
  int32_t* E_flat;             // [M * L][K]
  int32_t* order;              // [B_dec][M * L]
  int32_t* rank;               // [B_dec][M * L]
  int32_t* group_first;        // [B_dec][M * L]
  int32_t* group_last;         // [B_dec][M * L]
  float* sym_w;                // [M * L]
  int32_t* work_n;             // [B_dec * M * L]
  int32_t* level;              // [L] by step
  int32_t* work;               // [B_dec * M * L][2]
  int32_t* level_off;          // [M * L + 2]
  int32_t* n_levels;           // [1]
  int32_t* close;              // [B_dec * L][2]
  int32_t* close_off;          // [M * L + 2]
  int B_dec, M, L, K;
};
#define STATES_PLAN_LDS(L) ((3 * (size_t)(L) + 2) * 4)

template <int NPF>
static __global__ __launch_bounds__(1024) void states_plan_kernel(const StatesPlan p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int M = p.M, L = p.L, K = p.K, N = M * L;
  if (blockIdx.x != 0) {
    const long g0 = (long)(blockIdx.x - 1) * 1024 + tid, stride = (long)(gridDim.x - 1) * 1024;
    const long LK = (long)L * K;
    for (long e = g0; e < (long)M * LK; e += stride) p.E_flat[e] = p.E_idx[e] + (int)(e / LK) * L;
    for (long e = g0; e < (long)p.B_dec * N; e += stride) {
      const int n = (int)(e % N);
      const int t = n / M, m = n - t * M;                        // as a visit
      p.order[e] = m * L + p.order0[t];
      p.group_first[e] = t * M;
      p.group_last[e] = (m == M - 1) ? 1 : 0;
      p.work_n[e] = 1;
      const int ms = n / L, i = n - ms * L;                      // as a flat residue
      p.rank[e] = p.rank0[i] * M + ms;
      if (e < N) p.sym_w[n] = p.w[ms];
    }
    return;
  }
  int* lv = (int*)smem;                     // [L] level of a residue's group; -1 until its step is done
  int* lp = lv + L;                         // [L] by step: level << 16 | place among the steps of its level   (L <= 8192)
  int* cnt = lp + L;                        // [L + 2] steps per level, then the offsets
  __shared__ int part[1024];
  const int nb = L + 1;
  for (int i = tid; i < nb + 1; i += 1024) cnt[i] = 0;
  for (int i = tid; i < L; i += 1024) lv[i] = -1;
  __syncthreads();
  if (tid < 64) {
    const int MK = M * K;
    int off[NPF];
#pragma unroll
    for (int q = 0; q < NPF; ++q) {
      const int e = q * 64 + lane, m = e / K;
      off[q] = e < MK ? m * L * K + (e - m * K) : -1;
    }
    // the residues of 128 consecutive steps sit one per lane in two registers and are handed out by v_readlane
    int base = 0;
    int blkA = p.order0[lane < L ? lane : L - 1], blkB = p.order0[64 + lane < L ? 64 + lane : L - 1];
    auto res_at = [&](int x) {                                   // base <= x < base + 128
      x = x < L ? x : L - 1;
      const int i = (x - base) < 64 ? __builtin_amdgcn_readlane(blkA, x & 63) : __builtin_amdgcn_readlane(blkB, x & 63);
      return i < 0 ? 0 : (i >= L ? L - 1 : i);
    };
    auto fetch = [&](int (&j)[NPF], const int i) {
#pragma unroll
      for (int q = 0; q < NPF; ++q) j[q] = off[q] >= 0 ? p.E_idx[off[q] + i * K] : -1;
    };
    int top = 0;
    auto step = [&](const int (&j)[NPF], const int t, const int i) {
      int d = -1;
#pragma unroll
      for (int q = 0; q < NPF; ++q) if ((unsigned)j[q] < (unsigned)L) d = max(d, lv[j[q]]);
      for (int e = NPF * 64 + lane; e < MK; e += 64) {           // (look-ups beyond 64 NPF per step: not requested ahead)
        const int m = e / K;
        const int jj = p.E_idx[(m * L + i) * K + (e - m * K)];
        if ((unsigned)jj < (unsigned)L) d = max(d, lv[jj]);
      }
      d = (int)wave_max64((float)d) + 1;                         // (levels < 2^24: exact in fp32)
      top = max(top, d);
      if (lane == 0) { const int c = cnt[d]; lv[i] = d; lp[t] = d << 16 | c; cnt[d] = c + 1; }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // LDS writes visible to the wave's next step (the requests made ahead stay in flight)
      __builtin_amdgcn_wave_barrier();
    };
    int jA[NPF], jB[NPF], jc[NPF];
    int iA = res_at(0), iB = res_at(1);
    fetch(jA, iA); fetch(jB, iB);
    for (int t = 0; t < L; t += 2) {
      if (t - base >= 64) { base += 64; blkA = blkB; blkB = p.order0[base + 64 + lane < L ? base + 64 + lane : L - 1]; }
      int ic = iA;
#pragma unroll
      for (int q = 0; q < NPF; ++q) jc[q] = jA[q];
      iA = res_at(t + 2); fetch(jA, iA);
      step(jc, t, ic);
      if (t + 1 < L) {
        ic = iB;
#pragma unroll
        for (int q = 0; q < NPF; ++q) jc[q] = jB[q];
        iB = res_at(t + 3); fetch(jB, iB);
        step(jc, t + 1, ic);
      }
    }
    if (tid == 0) p.n_levels[0] = top + 1;                      // (levels are contiguous from 0)
  }
  __syncthreads();
  // exclusive scan of cnt[0 .. nb): thread t owns entries [t * per, (t + 1) * per)
  const int per = (nb + 1023) / 1024;
  int sum = 0;
  for (int q = 0; q < per; ++q) { const int i = tid * per + q; if (i < nb) sum += cnt[i]; }
  part[tid] = sum;
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
    if (i < nb) { const int c = cnt[i]; cnt[i] = run; run += c; }
  }
  if (tid == 1023) cnt[nb] = part[1023];                         // (= L)
  __syncthreads();
  const int bs = p.B_dec;
  for (int l = tid; l < N + 2; l += 1024) {
    const int g = l <= nb ? cnt[l] : L;
    p.level_off[l] = g * bs * M; p.close_off[l] = g * bs;
  }
  for (int t = tid; t < L; t += 1024) p.level[t] = lp[t] >> 16;
  for (int x = tid; x < bs * L; x += 1024) {
    const int b = x / L, t = x - b * L;
    const int l = lp[t] >> 16, g = cnt[l], cl = cnt[l + 1] - g;
    const int ci = g * bs + b * cl + (lp[t] & 0xffff);
    p.close[2 * ci] = b; p.close[2 * ci + 1] = t * M + M - 1;
    const int wi = ci * M;
    for (int m = 0; m < M; ++m) { p.work[2 * (wi + m)] = b; p.work[2 * (wi + m) + 1] = t * M + m; }
  }
}
