// Training / validation metrics of the reference's loop (na_run.py:240-326; na_metric_manager.py accumulate; na_model_utils.py:148-166
// compute_canonical_base_pair_accuracy) as two launches per batch, with no host synchronisation and no atomics.
//
// metrics_partial_kernel: one workgroup of 128 threads per 128 consecutive tokens.  The block's log-prob rows are staged through LDS
// with coalesced loads (a wave's tokens are contiguous rows); each thread then evaluates its token — argmax, accuracy, the per-token
// label-smoothed loss (loss_smoothed_token of namp_train.h, the same arithmetic as namp_train_loss_smoothed), the canonical-pair hit
// with the partner's argmax read inline from global memory — and the products of its masks for every row.  Per-token values and row
// masks go to LDS, and thread p then sums cell p = (row, quantity) over the block's tokens in token order: partial[block][cell].
// MODE 2 writes the per-token canonical-pair accuracy instead and stops there.
// metrics_finish_kernel: one workgroup per cell sums the partial slabs in a fixed order (strided per thread, then an LDS tree) and
// adds the result into the caller's fp64 table.  The whole reduction is in fp64 and its order depends only on G.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "namp_train.h"

#define METRIC_TOK 128             // tokens (= threads) per workgroup of metrics_partial_kernel
#define METRIC_VMAX 64
#define METRIC_ROWS 12             // (1 + 3 polymer masks) x (1 + 2 interface masks)
#define METRIC_BASE_Q 5            // weights, canonical-pair weights, loss, accuracy, canonical-pair accuracy

struct MetricRef { const void* p; int dt; };

__device__ __forceinline__ double mref_f(const MetricRef r, long i) {
  switch (r.dt) {
    case NAMP_DT_BOOL: return (double)((const uint8_t*)r.p)[i];
    case NAMP_DT_I32: return (double)((const int32_t*)r.p)[i];
    case NAMP_DT_I64: return (double)((const long long*)r.p)[i];
    case NAMP_DT_F32: return (double)((const float*)r.p)[i];
    default: return ((const double*)r.p)[i];
  }
}
__device__ __forceinline__ long long mref_i(const MetricRef r, long i) {
  switch (r.dt) {
    case NAMP_DT_BOOL: return ((const uint8_t*)r.p)[i];
    case NAMP_DT_I32: return ((const int32_t*)r.p)[i];
    case NAMP_DT_I64: return ((const long long*)r.p)[i];
    case NAMP_DT_F32: return (long long)((const float*)r.p)[i];
    default: return (long long)((const double*)r.p)[i];
  }
}

struct MetricArgs {
  const float* log_probs;
  MetricRef S, mfl, cbp_mask, cbp_idx, pm[3], im[2];
  MetricRef loss, acc, cbp_acc, S_pred;                 // given mode
  MetricRef lpm[3], ppm_mask;                           // fused mode
  LossArgs la;                                          // restype tables, eps scales, 1 - weight, V
  long G; int L, V, npm, nim, nres, res[NAMP_METRIC_MAX_RES];
  unsigned long long pair_bits[METRIC_VMAX];
  double* partial; int32_t* err; long long* cbp_out;
};

struct MetricFinish {
  int row_of[METRIC_ROWS], col_of[METRIC_BASE_Q + 2 * NAMP_METRIC_MAX_RES];
  int Q, ncols, nblk, P;
};

// torch.argmax over one row: the first index of the maximum; a row holding NaN yields its first NaN
__device__ __forceinline__ int metric_argmax(const float* row, int V) {
  float best = row[0];
  int bi = 0;
  for (int v = 1; v < V; ++v) {
    if (best != best) break;
    const float x = row[v];
    if (x != x || x > best) { best = x; bi = v; }
  }
  return bi;
}

// MODE 0: from log_probs, 1: given per-token values, 2: per-token canonical-pair accuracy into a.cbp_out
template <int MODE>
__global__ __launch_bounds__(METRIC_TOK) void metrics_partial_kernel(const MetricArgs a) {
  __shared__ float lp_s[METRIC_TOK * METRIC_VMAX];
  __shared__ double m_s[METRIC_ROWS][METRIC_TOK];
  __shared__ double q_s[METRIC_BASE_Q][METRIC_TOK];
  __shared__ int st_s[METRIC_TOK], sp_s[METRIC_TOK];
  const int tid = threadIdx.x;
  const long i0 = (long)blockIdx.x * METRIC_TOK;
  const long i = i0 + tid;
  const int ntok = (int)min((long)METRIC_TOK, a.G - i0);
  if (MODE != 1) {
    const int n = ntok * a.V;
    const float* src = a.log_probs + i0 * a.V;
    for (int e = tid; e < n; e += METRIC_TOK) lp_s[e] = src[e];
    __syncthreads();
  }
  double qv[METRIC_BASE_Q] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double m[METRIC_ROWS];
#pragma unroll
  for (int r = 0; r < METRIC_ROWS; ++r) m[r] = 0.0;
  int s_true = -1, s_pred = -1;
  if (i < a.G) {
    s_true = (int)mref_i(a.S, i);
    double loss = 0.0, acc = 0.0, cbp_acc = 0.0;
    const double cbpm = mref_f(a.cbp_mask, i);
    if (MODE != 1) {
      const float* row = lp_s + tid * a.V;
      s_pred = metric_argmax(row, a.V);
      const long long idx = mref_i(a.cbp_idx, i);
      const bool ok = idx >= 0 && idx < a.L;
      if (!ok && a.err) a.err[0] = 1;
      double hit = 0.0;
      if (ok && cbpm != 0.0) {
        const long j = (i / a.L) * a.L + idx;
        const int s_j = metric_argmax(a.log_probs + j * a.V, a.V);
        hit = (double)((a.pair_bits[s_pred] >> s_j) & 1ull);
      }
      if (MODE == 2) {
        a.cbp_out[i] = hit != 0.0 ? mref_i(a.cbp_mask, i) : 0;
        return;
      }
      acc = (s_true == s_pred) ? 1.0 : 0.0;
      cbp_acc = hit * cbpm;
      const bool ppm = a.ppm_mask.p && mref_i(a.ppm_mask, i) != 0;
      loss = loss_smoothed_token(a.la, row, s_true, ppm ? a.la.aligned_ppm + i * a.V : nullptr, (float)mref_f(a.lpm[0], i),
                                 (float)mref_f(a.lpm[1], i), (float)mref_f(a.lpm[2], i));
    } else {
      loss = mref_f(a.loss, i); acc = mref_f(a.acc, i); cbp_acc = mref_f(a.cbp_acc, i);
      s_pred = (int)mref_i(a.S_pred, i);
    }
    qv[0] = 1.0; qv[1] = cbpm; qv[2] = loss; qv[3] = acc; qv[4] = cbp_acc * cbpm;
    const double mfl = mref_f(a.mfl, i);
    double ifac[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 2; ++k) if (k < a.nim) ifac[k] = mref_f(a.im[k], i);
#pragma unroll
    for (int pi = 0; pi < 4; ++pi) {
      const double mp = (pi && pi <= a.npm) ? mfl * mref_f(a.pm[pi ? pi - 1 : 0], i) : mfl;
#pragma unroll
      for (int ii = 0; ii < 3; ++ii) m[pi * 3 + ii] = ii ? mp * ifac[ii ? ii - 1 : 0] : mp;   // fixed slots: no dynamic register indexing
    }
  }
  if (MODE == 2) return;
#pragma unroll
  for (int pi = 0; pi < 4; ++pi)
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
      if (pi <= a.npm && ii <= a.nim) m_s[pi * (1 + a.nim) + ii][tid] = m[pi * 3 + ii];
#pragma unroll
  for (int q = 0; q < METRIC_BASE_Q; ++q) q_s[q][tid] = qv[q];
  st_s[tid] = s_true; sp_s[tid] = s_pred;
  __syncthreads();
  const int Q = METRIC_BASE_Q + 2 * a.nres, P = (1 + a.npm) * (1 + a.nim) * Q;
  for (int p = tid; p < P; p += METRIC_TOK) {
    const int r = p / Q, q = p - r * Q;
    double s = 0.0;
    if (q < METRIC_BASE_Q) {
      for (int t = 0; t < ntok; ++t) s += m_s[r][t] * q_s[q][t];
    } else {
      const int k = q - METRIC_BASE_Q;
      const int res = a.res[k < a.nres ? k : k - a.nres];
      const int* lab = k < a.nres ? st_s : sp_s;
      for (int t = 0; t < ntok; ++t) s += (double)(lab[t] == res) * m_s[r][t];
    }
    a.partial[(long)blockIdx.x * P + p] = s;
  }
}

__global__ __launch_bounds__(256) void metrics_finish_kernel(const double* __restrict__ partial, const MetricFinish f, double* __restrict__ table) {
  __shared__ double red[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int b = tid; b < f.nblk; b += 256) s += partial[(long)b * f.P + p];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const int r = p / f.Q, q = p - r * f.Q;
    const int c = f.col_of[q];
    if (c >= 0) table[(long)f.row_of[r] * f.ncols + c] += red[0];
  }
}
