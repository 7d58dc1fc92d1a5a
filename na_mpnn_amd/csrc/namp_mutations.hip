// Translation unit of the mutational scan (namp_mutations.h): namp_mutations / namp_mutations_workspace_bytes / namp_mutations_in_offset /
// namp_mutations_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a scan.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the base stream as
// namp_library.hip runs it, the per-site plan, and per layer the index tables and one dec_items_kernel launch over
// (variant, row of U_l(site)) items.
#include "../../include/namp.h"
#include "namp_mutations.h"

#include <cstdio>

namespace {

int bfail(int code, const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return namp_internal_fail(code, buf);
}

struct MutDims { int N, K, n_sites, n_var, lcap[3], icap[3]; };

// the call's buffers, carved in one fixed order (base == nullptr: sizes only)
struct MutBuffers : LooBaseStream {                                                    // (the base stream's tables and states first)
  uint8_t* level;                                                                      // the plan
  int32_t *loff[3], *list[3], *ioff[3];
  int32_t* in;                                   // INPUT section: sites[n_sites][8], variants[n_var][9], w[N] (float bits)
  float* ov1;                                    // [n_var * 8][128] layer 1's override rows
  float *hO[3], *PaO[2], *ovO[2];                // [icap_l][128] outputs of layer l's items
  MutItemTables tab[3];
  int32_t* sizes;                                // OUTPUT section: int32 [n_sites][3], then
  float* delta;                                  // float [n_var], then
  int32_t* row_res;                              // int32 [icap_3], then
  float* row_lp;                                 // float [icap_3]
  size_t in_off, out_off, bytes;
};

MutBuffers mut_carve(void* base, const MutDims& d) {
  MutBuffers b;
  size_t off = 0;
  auto take = [&](size_t elems) {
    void* p = base ? (void*)((char*)base + off) : nullptr;
    off += (elems * 4 + 255) & ~size_t(255);
    return p;
  };
  const size_t N = (size_t)d.N, g128 = N * NAMP_HIDDEN, tpn = (d.K + 15) / 16, ns = (size_t)d.n_sites, nv = (size_t)d.n_var;
  float** gs[] = {&b.Pa1, &b.Pbw1, &b.Pfw[0], &b.Pfw[1], &b.Pfw[2], &b.h1, &b.Pa2, &b.Pbw2, &b.h2, &b.Pa3, &b.Pbw3, &b.h3};
  for (float** p : gs) *p = (float*)take(g128);
  b.partial = (float*)take(N * tpn * (NAMP_HIDDEN + 1) + 3);
  b.level = (uint8_t*)take((ns * N + 3) / 4 + 1);
  for (int l = 0; l < 3; ++l) {
    b.loff[l] = (int32_t*)take(ns + 1); b.list[l] = (int32_t*)take((size_t)d.lcap[l] + 1); b.ioff[l] = (int32_t*)take(nv + 1);
  }
  b.in_off = off;
  b.in = (int32_t*)take(ns * MUT_E + nv * (1 + MUT_E) + N);
  b.ov1 = (float*)take(nv * MUT_E * NAMP_HIDDEN + 4);
  for (int l = 0; l < 3; ++l) {
    const size_t R = (size_t)d.icap[l];
    b.hO[l] = (float*)take(R * NAMP_HIDDEN + 4);
    if (l < 2) { b.PaO[l] = (float*)take(R * NAMP_HIDDEN + 4); b.ovO[l] = (float*)take(R * NAMP_HIDDEN + 4); }
    MutItemTables& t = b.tab[l];
    t.act = (int32_t*)take(R + 1); t.ctr = (int32_t*)take(R + 1); t.cen = (int32_t*)take(R + 1); t.msk = (int32_t*)take(R + 1);
    t.tok = (int32_t*)take(R + 1); t.esrc = (int32_t*)take(R * d.K + 1);
  }
  b.out_off = off;
  b.sizes = (int32_t*)take(ns * 3 + 1);
  b.delta = (float*)take(nv + 1);
  b.row_res = (int32_t*)take((size_t)d.icap[2] + 1);
  b.row_lp = (float*)take((size_t)d.icap[2] + 1);
  b.bytes = off;
  return b;
}

bool mut_dims_ok(int N, int K, int n_dec, const int* m) {
  if (N < 1 || K < 1 || K > NAMP_MAX_K || K > N || n_dec != 3) return false;
  const long lim = 1L << LOO_ROW_BITS;                           // every table row code stays below 2^28
  if (m[0] < 0 || m[0] >= lim || m[1] < 0 || (long)m[1] * MUT_E >= lim || (m[1] > 0 && m[0] < 1) || N >= lim) return false;
  if ((long)m[0] * N >= (1L << 40)) return false;
  for (int q = 2; q < 8; ++q)
    if (m[q] < 0 || m[q] >= lim) return false;
  return true;
}

MutDims mut_dims(int N, int K, const int* m) { return MutDims{N, K, m[0], m[1], {m[2], m[3], m[4]}, {m[5], m[6], m[7]}}; }

// what the calling thread's NEXT namp_decoder_fwd call scans: taken, and cleared, by that call
struct MutAttachment { bool on; int dims[8]; };
thread_local MutAttachment g_mut_attached = {};

}  // namespace

// (for namp_decoder_fwd, namp.hip) the attachment of the calling thread, cleared
__attribute__((visibility("hidden"))) int namp_internal_mutations_take(int* dims) {
  const MutAttachment a = g_mut_attached;
  g_mut_attached = {};
  if (!a.on) return 0;
  for (int q = 0; q < 8; ++q) dims[q] = a.dims[q];
  return 1;
}

// the carrier's body with an attachment: base stream -> log_probs, the per-site plan -> sizes, the items -> sparse entries and deltas
__attribute__((visibility("hidden"))) int namp_internal_mutations_run(const NampModelW* w, const float* h_V_enc, const float* h_E, const int32_t* E_idx,
                                                                       const int32_t* S, const int32_t* mask, const int32_t* rank, float* log_probs,
                                                                       const float* logits, const float* h_V_dec, void* ws, size_t ws_bytes,
                                                                       int B_dec, int B_enc, int N, int K, const int* m, void* stream) {
  if (!w || !h_V_enc || !h_E || !E_idx || !S || !mask || !rank || !log_probs || !ws)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: null pointer argument (a mutational scan was attached; mask is required)");
  if (logits || h_V_dec) return bfail(NAMP_EINVAL, "namp_decoder_fwd: logits / h_V_dec are not written with a mutational scan attached");
  if (B_dec != 1 || B_enc != 1) return bfail(NAMP_EINVAL, "namp_decoder_fwd: a mutational scan runs on one complex (B_dec=%ld, B_enc=%ld)", B_dec, B_enc);
  if ((((uintptr_t)h_V_enc | (uintptr_t)h_E | (uintptr_t)ws | (uintptr_t)log_probs) & 15u) != 0)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: h_V_enc / h_E / log_probs / ws must be 16-byte aligned (a mutational scan was attached)");
  int prec = PREC_F32;
  int rc = loo_check_weights(w, "namp_decoder_fwd (mutational scan attached)", &prec);
  if (rc) return rc;
  if (!mut_dims_ok(N, K, w->n_dec, m))
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached mutational scan N=%ld K=%ld n_sites=%ld", N, K, m[0]);
  const MutDims d = mut_dims(N, K, m);
  MutBuffers b = mut_carve(ws, d);
  if (b.bytes > ws_bytes)                                        // (the sections are part of the call's arguments: include/namp.h)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: workspace too small for the attached mutational scan (%ld bytes, %ld needed)", (long)ws_bytes,
                 (long)b.bytes);
  const hipError_t ready = loo_items_ready();
  if (ready != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(ready));
  hipStream_t s = (hipStream_t)stream;
  const NampDecLayerW* D0 = &w->dec[0];
  const int n_sites = d.n_sites, n_var = d.n_var;

  // ---- base stream (namp_loo.h: the launches of namp_library.hip's, one summation order for every call that rides on this carrier)
  if ((rc = loo_base_stream(w, b, h_V_enc, h_E, E_idx, S, mask, rank, log_probs, N, K, stream))) return rc;
  const float* Pa[3] = {b.Pa1, b.Pa2, b.Pa3};
  const float* Pbw[3] = {b.Pbw1, b.Pbw2, b.Pbw3};
  const float* hin[3] = {h_V_enc, b.h1, b.h2};
  if (n_sites == 0) return NAMP_OK;

  // ---- the plan: levels and sizes per site, the prefix sums, the lists
  MutPlanArgs pa = {};
  pa.E_idx = E_idx; pa.rank = rank; pa.mask = mask; pa.S = S;
  pa.sites = b.in; pa.variants = b.in + (size_t)n_sites * MUT_E; pa.w = (const float*)(pa.variants + (size_t)n_var * (1 + MUT_E));
  pa.level = b.level; pa.sizes = b.sizes;
  for (int l = 0; l < 3; ++l) { pa.loff[l] = b.loff[l]; pa.list[l] = b.list[l]; pa.ioff[l] = b.ioff[l]; pa.lcap[l] = d.lcap[l]; pa.icap[l] = d.icap[l]; }
  pa.N = N; pa.K = K; pa.n_sites = n_sites; pa.n_var = n_var; pa.vocab = w->vocab;
  hipLaunchKernelGGL(mut_plan_kernel, dim3((unsigned)n_sites), dim3(256), 0, s, pa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  if (n_var == 0) return NAMP_OK;                                // (the sizes only: what the caller cuts its chunks by)
  hipLaunchKernelGGL(mut_offsets_kernel, dim3(1), dim3(256), 0, s, pa);
  hipLaunchKernelGGL(mut_lists_kernel, dim3((unsigned)n_sites), dim3(256), 0, s, pa);
  hipLaunchKernelGGL(mut_token_rows_kernel, dim3((unsigned)(((long)n_var * MUT_E * (NAMP_H / 4) + 255) / 256)), dim3(256), 0, s, pa, b.Pfw[0], D0->tok,
                     b.ov1);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));

  // ---- the items, layer by layer: centre overrides and override rows come from the layer in front
  const float* cenPa[3] = {b.Pa1, b.PaO[0], b.PaO[1]};
  const float* cenH[3] = {h_V_enc, b.hO[0], b.hO[1]};
  const float* ov[3] = {b.ov1, b.ovO[0], b.ovO[1]};
  for (int l = 0; l < 3; ++l) {
    const long R = d.icap[l];
    if (R == 0) continue;                                        // (an empty layer: whatever would read its rows finds none and reads base)
    const NampDecLayerW* D = &w->dec[l];
    const MutItemTables& t = b.tab[l];
    hipLaunchKernelGGL(mut_items_kernel, dim3((unsigned)((R * K + 255) / 256)), dim3(256), 0, s, pa, t, l);
    if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
    LooItemArgs a = loo_items(D, prec, h_E, K, R, t.act, t.ctr, t.cen, t.esrc, Pa[l], cenPa[l], hin[l], cenH[l], Pbw[l], b.Pfw[l], ov[l]);
    loo_tail(a.tail, D, t.msk, t.tok, b.hO[l]);
    if (l < 2) {
      const NampDecLayerW* Dn = &w->dec[l + 1];
      loo_proj(a.tail, Dn->W1a_img, Dn->b1, nullptr, b.PaO[l]);
      loo_proj(a.tail, Dn->W1v_img, nullptr, Dn->tok, b.ovO[l]);
    }
    if ((rc = launch_items(a, prec, s))) return rc;
  }
  if (d.icap[2] > 0)
    hipLaunchKernelGGL(mut_head_kernel, dim3((unsigned)((d.icap[2] + 3) / 4)), dim3(256), 0, s, pa, b.tab[2].ctr, b.tab[2].tok, b.hO[2], w->Wout_w,
                       w->Wout_b, b.row_res, b.row_lp);
  hipLaunchKernelGGL(mut_delta_kernel, dim3((unsigned)((n_var + 255) / 256)), dim3(256), 0, s, pa, b.row_res, b.row_lp, log_probs, b.delta);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  return NAMP_OK;
}

extern "C" {

size_t namp_mutations_workspace_bytes(int N, int K, int n_dec, int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2,
                                      int items3) {
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  if (!mut_dims_ok(N, K, n_dec, m)) return 0;
  return mut_carve(nullptr, mut_dims(N, K, m)).bytes;
}

size_t namp_mutations_in_offset(int N, int K, int n_dec, int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2,
                                int items3) {
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  if (!mut_dims_ok(N, K, n_dec, m)) return 0;
  return mut_carve(nullptr, mut_dims(N, K, m)).in_off;
}

size_t namp_mutations_out_offset(int N, int K, int n_dec, int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2,
                                 int items3) {
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  if (!mut_dims_ok(N, K, n_dec, m)) return 0;
  return mut_carve(nullptr, mut_dims(N, K, m)).out_off;
}

int namp_mutations(int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2, int items3) {
  g_mut_attached = {};
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  for (int v : m)
    if (v < 0) return bfail(NAMP_EINVAL, "namp_mutations: n_sites=%ld, n_variants=%ld and the capacities must not be negative", n_sites, n_variants);
  g_mut_attached.on = true;
  for (int q = 0; q < 8; ++q) g_mut_attached.dims[q] = m[q];
  return NAMP_OK;
}

}  // extern "C"
