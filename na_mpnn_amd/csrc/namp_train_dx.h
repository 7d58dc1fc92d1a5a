// Coordinate gradients of the edge featuriser: dL/dX18 from g_pre = dL/d(pre-LayerNorm edge embedding), the
// transpose of feat_wgrad_kernel's contraction.  For edge e = (i, k), j = E_idx[i, k], and atom pair (a, b) in column block q = 1 + 18a + b:
//     u[r]  = sum_o g_pre[e][o] * Wedge[o][16q + r]                                   (one fp32 MFMA chain: [16 edges x 128] . [128 x 16])
//     s_ab  = sum_r u[r] * (-2 (D - mu_r) / sigma^2) * exp(-((D - mu_r) / sigma)^2) * M18[i,a] * M18[j,b],   D = sqrt(|X18[i,a] - X18[j,b]|^2 + 1e-6)
//     gi[e][a] += s_ab (X18[i,a] - X18[j,b]) / D,     gj[e][b] -= the same
// with the RBFs regenerated from the atoms like the forward launch does.  Every edge's two rows gi / gj [18][3] go to scratch with plain
// stores; xgrad_reduce_kernel then adds, per residue, its K rows gi and the rows gj of its reverse adjacency in ascending edge order:
// no atomics, one summation order.  The launches read a CLAMPED copy of E_idx (xgrad_clamp_kernel), so that a malformed neighbour list
// gives the result of the clamped one and the counting sort of the reverse adjacency stays inside its counters.
#pragma once
#include "namp_device.h"

#define XG_ATOMS 18
#define XG_ROW (2 * XG_ATOMS * 3)   // floats per edge in scratch: gi [18][3] | gj [18][3]
#define XG_TILE 64                  // edges per workgroup = one presence tile (FEATW_TILE); a wave owns 16 of them (one MFMA row tile)
#define XG_LD 5200                  // row length of Wedge (FEATW_COLS)

static __global__ __launch_bounds__(256) void xgrad_clamp_kernel(const int32_t* __restrict__ E_idx, int32_t* __restrict__ out, long E, int L) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long)gridDim.x * blockDim.x) {
    int j = E_idx[e];
    j = j < 0 ? 0 : j;
    out[e] = j >= L ? L - 1 : j;
  }
}

// PK: packed atoms X18 [G][18][4] = (x, y, z, mask), M18 unused; otherwise X18 [G][18][3] and M18 [G][18].
// Grid: one workgroup per 64-edge tile.  A operand: lane (n, g) holds g_pre[edge n of the wave][32g .. 32g+31] in registers for the whole
// tile (MFMA step t contracts channel 32g + t in k-slot g: any order serves a sum, and this one makes the lane's A values 8 x 16 bytes);
// B operand: Wedge[32g + t][16q + n], 64 contiguous bytes per 16 lanes, from L2.  D[edge 4g + r][centre n] lands on lane (n, g), element r.
template <bool PK>
static __global__ __launch_bounds__(256) void feat_xgrad_kernel(const float* __restrict__ X18, const float* __restrict__ M18,
                                                                const int32_t* __restrict__ E_idx, const float* __restrict__ g_pre,
                                                                const float* __restrict__ Wedge, const int32_t* __restrict__ pres,
                                                                long E, int L, int K, float* __restrict__ rows) {
  __shared__ float acc_lds[4][16 * XG_ROW];
  constexpr int XS = PK ? 4 : 3;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const long tile = blockIdx.x;
  const long e0 = tile * XG_TILE + 16 * wave;                  // the wave's first edge
  float* mine = acc_lds[wave];
  for (int f = lane; f < 16 * XG_ROW; f += 64) mine[f] = 0.f;

  // A operand rows (clamped past the end: those edges' results are dropped)
  f4 av[8];
  {
    long er = e0 + n;
    er = er < E ? er : E - 1;
    const f4* src = (const f4*)(g_pre + er * NAMP_H + 32 * g);
#pragma unroll
    for (int t = 0; t < 8; ++t) av[t] = src[t];
  }
  // this lane's edge for the geometry and the accumulation: 4g + (n & 3) of the wave (lanes n < 4 accumulate; the others mirror them)
  const int el = 4 * g + (n & 3);
  const long eg = e0 + el;
  const bool eok = eg < E;
  const long ec = eok ? eg : E - 1;
  const int node = (int)(ec / K);
  const int j = node - node % L + E_idx[ec];
  const float mu = 2.0f + (float)n * (20.0f / 15.0f);
  const uint32_t pi = (uint32_t)__builtin_amdgcn_readfirstlane(pres[2 * tile]);
  const uint32_t pj = (uint32_t)__builtin_amdgcn_readfirstlane(pres[2 * tile + 1]);
  __syncthreads();

  for (int a = 0; a < XG_ATOMS; ++a) {
    if (((pi >> a) & 1u) == 0u) continue;
    const float* xi = X18 + ((long)node * 18 + a) * XS;
    const float xi0 = xi[0], xi1 = xi[1], xi2 = xi[2];
    const float mi = PK ? xi[XS - 1] : M18[(long)node * 18 + a];
    for (int b = 0; b < XG_ATOMS; ++b) {
      if (((pj >> b) & 1u) == 0u) continue;
      const float* xj = X18 + ((long)j * 18 + b) * XS;
      const float dx = xi0 - xj[0], dy = xi1 - xj[1], dz = xi2 - xj[2];
      const float mk = mi * (PK ? xj[XS - 1] : M18[(long)j * 18 + b]);
      const bool ok = eok && mk != 0.f;
      if (__ballot(ok) == 0ull) continue;                      // none of the wave's 16 edges has this pair
      const float D = sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
      const float dist = ok ? D : 1e30f;                        // absent pair: "infinitely far", RBF = 0 (as the forward launch)
      const float* wb = Wedge + (long)(32 * g) * XG_LD + 16 * (1 + 18 * a + b) + n;
      f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float b0 = wb[(4 * t + 0) * XG_LD], b1 = wb[(4 * t + 1) * XG_LD], b2 = wb[(4 * t + 2) * XG_LD], b3 = wb[(4 * t + 3) * XG_LD];
        acc = mfma4(av[t][0], b0, acc);
        acc = mfma4(av[t][1], b1, acc);
        acc = mfma4(av[t][2], b2, acc);
        acc = mfma4(av[t][3], b3, acc);
      }
      // acc[r] = u(edge 4g + r, centre n): times dRBF/dD, summed over the 16 centres of the lane row
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float de = __shfl(dist, 16 * g + r);               // lane (r, g) holds the geometry of edge 4g + r
        const float dm = de - mu;
        const float u = dm * 0.8f;
        float t_ = acc[r] * (-1.28f * dm) * __expf(-(u * u));     // -2 (D - mu) / sigma^2, sigma = 1.25
        t_ += __shfl_xor(t_, 1);
        t_ += __shfl_xor(t_, 2);
        t_ += __shfl_xor(t_, 4);
        t_ += __shfl_xor(t_, 8);
        s = (n == r) ? t_ : s;
      }
      if (n < 4 && ok) {
        const float c = s * mk / D;
        const float vx = c * dx, vy = c * dy, vz = c * dz;
        float* pi_ = mine + el * XG_ROW + 3 * a;
        float* pj_ = mine + el * XG_ROW + 3 * XG_ATOMS + 3 * b;
        pi_[0] += vx; pi_[1] += vy; pi_[2] += vz;
        pj_[0] -= vx; pj_[1] -= vy; pj_[2] -= vz;
      }
    }
  }
  __syncthreads();
  // the wave's 16 rows, contiguous in scratch
  for (int f = lane; f < 16 * XG_ROW; f += 64)
    if (e0 + f / XG_ROW < E) rows[e0 * XG_ROW + f] = mine[f];
}

// dX18[node][q] = sum_k gi[node K + k][q] + sum over the reverse adjacency of node (ascending edge number) of gj[edge][q],  q < 54
static __global__ __launch_bounds__(256) void xgrad_reduce_kernel(const float* __restrict__ rows, const int32_t* __restrict__ rev_off,
                                                                  const int32_t* __restrict__ rev_edge, long G, int K, float* __restrict__ dX) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G * (XG_ROW / 2)) return;
  const long node = idx / (XG_ROW / 2);
  const int q = (int)(idx - node * (XG_ROW / 2));
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += rows[(node * K + k) * XG_ROW + q];
  const int lo = rev_off[node], hi = rev_off[node + 1];
  for (int p = lo; p < hi; ++p) s += rows[(long)rev_edge[p] * XG_ROW + XG_ROW / 2 + q];
  dX[idx] = s;
}
