// Translation unit of the mutational scan (namp_mutations.h): namp_mutations / namp_mutations_workspace_bytes / namp_mutations_in_offset /
// namp_mutations_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a scan.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the base stream as
// namp_library.hip runs it, the per-site plan, and per layer the index tables and one dec_items_kernel launch over
// (variant, row of U_l(site)) items.
#include "../../include/namp.h"
#include "namp_mutations.h"
#include "namp_attach.h"

namespace {

// the call's buffers, carved in one fixed order
struct MutBuffers : LooBaseStream, LooItemRows {                                       // (the base stream's tables and states first)
  uint8_t* level;                                                                      // the plan
  int32_t *loff[3], *list[3], *ioff[3];
  int32_t* in;                                   // INPUT section: sites[n_sites][8], variants[n_var][9], w[N] (float bits)
                                                 // (LooItemRows: [n_var * 8], [icap_l] rows)
  MutItemTables tab[3];
  int32_t* sizes;                                // OUTPUT section: int32 [n_sites][3], then
  float* delta;                                  // float [n_var], then
  int32_t* row_res;                              // int32 [icap_3], then
  float* row_lp;                                 // float [icap_3]
  size_t in_off, out_off, bytes;                 // (all 0: the dims are refused)
};

bool mut_dims_ok(int N, int K, int n_dec, const int* m) {
  if (N < 1 || K < 1 || K > NAMP_MAX_K || K > N || n_dec != 3) return false;
  const long lim = 1L << LOO_ROW_BITS;                           // every table row code stays below 2^28
  if (m[0] < 0 || m[0] >= lim || m[1] < 0 || (long)m[1] * MUT_E >= lim || (m[1] > 0 && m[0] < 1) || N >= lim) return false;
  if ((long)m[0] * N >= (1L << 40)) return false;
  for (int q = 2; q < 8; ++q)
    if (m[q] < 0 || m[q] >= lim) return false;
  return true;
}

// validates, then carves (base == nullptr: sizes only); m: n_sites, n_variants, list capacities [3], item capacities [3]
MutBuffers mut_layout(void* base, int N_, int K, int n_dec, const int* m) {
  MutBuffers b = {};
  if (!mut_dims_ok(N_, K, n_dec, m)) return b;
  WsCarver c(base);
  const int *lcap = m + 2, *icap = m + 5;
  const size_t N = (size_t)N_, g128 = N * NAMP_HIDDEN, tpn = (K + 15) / 16, ns = (size_t)m[0], nv = (size_t)m[1];
  float** gs[] = {&b.Pa1, &b.Pbw1, &b.Pfw[0], &b.Pfw[1], &b.Pfw[2], &b.h1, &b.Pa2, &b.Pbw2, &b.h2, &b.Pa3, &b.Pbw3, &b.h3};
  for (float** p : gs) *p = c.take<float>(g128);
  b.partial = c.take<float>(N * tpn * (NAMP_HIDDEN + 1) + 3);
  b.level = c.take<uint8_t>((ns * N + 3) / 4 + 1);
  for (int l = 0; l < 3; ++l) {
    b.loff[l] = c.take<int32_t>(ns + 1); b.list[l] = c.take<int32_t>((size_t)lcap[l] + 1); b.ioff[l] = c.take<int32_t>(nv + 1);
  }
  b.in_off = c.off;
  b.in = c.take<int32_t>(ns * MUT_E + nv * (1 + MUT_E) + N);
  b.ov1 = c.take<float>(nv * MUT_E * NAMP_HIDDEN + 4);
  for (int l = 0; l < 3; ++l) {
    const size_t R = (size_t)icap[l];
    b.hO[l] = c.take<float>(R * NAMP_HIDDEN + 4);
    if (l < 2) { b.PaO[l] = c.take<float>(R * NAMP_HIDDEN + 4); b.ovO[l] = c.take<float>(R * NAMP_HIDDEN + 4); }
    MutItemTables& t = b.tab[l];
    t.act = c.take<int32_t>(R + 1); t.ctr = c.take<int32_t>(R + 1); t.cen = c.take<int32_t>(R + 1); t.msk = c.take<int32_t>(R + 1);
    t.tok = c.take<int32_t>(R + 1); t.esrc = c.take<int32_t>(R * K + 1);
  }
  b.out_off = c.off;
  b.sizes = c.take<int32_t>(ns * 3 + 1);
  b.delta = c.take<float>(nv + 1);
  b.row_res = c.take<int32_t>((size_t)icap[2] + 1);
  b.row_lp = c.take<float>((size_t)icap[2] + 1);
  b.bytes = c.off;
  return b;
}

}  // namespace

// the carrier's body with an attachment: base stream -> log_probs, the per-site plan -> sizes, the items -> sparse entries and deltas
__attribute__((visibility("hidden"))) int namp_internal_mutations_run(const AttachedCall& c, const int* m) {
  const char* noun = ATTACH_NOUN[ATTACH_MUTATIONS];
  int prec = PREC_F32;
  int rc = attached_prologue(c, noun, &prec);
  if (rc) return rc;
  const NampModelW* w = c.w;
  const int N = c.N, K = c.K, n_sites = m[0], n_var = m[1], *lcap = m + 2, *icap = m + 5;
  MutBuffers b = mut_layout(c.ws, N, K, w->n_dec, m);
  if (!b.bytes) return namp_failf(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached mutational scan N=%ld K=%ld n_sites=%ld", N, K, n_sites);
  if ((rc = attached_ready(c, noun, b.bytes))) return rc;
  hipStream_t s = (hipStream_t)c.stream;

  // ---- base stream (namp_loo.h: the launches of namp_library.hip's, one summation order for every call that rides on this carrier)
  if ((rc = loo_base_stream(w, b, c.h_V_enc, c.h_E, c.E_idx, c.S, c.mask, c.rank, c.log_probs, N, K, c.stream))) return rc;
  if (n_sites == 0) return NAMP_OK;

  // ---- the plan: levels and sizes per site, the prefix sums, the lists
  MutPlanArgs pa = {};
  pa.E_idx = c.E_idx; pa.rank = c.rank; pa.mask = c.mask; pa.S = c.S;
  pa.sites = b.in; pa.variants = b.in + (size_t)n_sites * MUT_E; pa.w = (const float*)(pa.variants + (size_t)n_var * (1 + MUT_E));
  pa.level = b.level; pa.sizes = b.sizes;
  for (int l = 0; l < 3; ++l) { pa.loff[l] = b.loff[l]; pa.list[l] = b.list[l]; pa.ioff[l] = b.ioff[l]; pa.lcap[l] = lcap[l]; pa.icap[l] = icap[l]; }
  pa.N = N; pa.K = K; pa.n_sites = n_sites; pa.n_var = n_var; pa.vocab = w->vocab;
  hipLaunchKernelGGL(mut_plan_kernel, dim3((unsigned)n_sites), dim3(256), 0, s, pa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  if (n_var == 0) return NAMP_OK;                                // (the sizes only: what the caller cuts its chunks by)
  hipLaunchKernelGGL(mut_offsets_kernel, dim3(1), dim3(256), 0, s, pa);
  hipLaunchKernelGGL(mut_lists_kernel, dim3((unsigned)n_sites), dim3(256), 0, s, pa);
  hipLaunchKernelGGL(mut_token_rows_kernel, dim3((unsigned)(((long)n_var * MUT_E * (NAMP_H / 4) + 255) / 256)), dim3(256), 0, s, pa, b.Pfw[0],
                     w->dec[0].tok, b.ov1);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));

  // ---- the items, layer by layer (an empty layer is stepped over: whatever would read its rows finds none and reads base)
  const long R[3] = {icap[0], icap[1], icap[2]};
  rc = loo_item_layers(w, prec, c.h_V_enc, c.h_E, K, b, b, b.tab, R, false, s, [&](int l, long Rl) {
    hipLaunchKernelGGL(mut_items_kernel, dim3((unsigned)((Rl * K + 255) / 256)), dim3(256), 0, s, pa, b.tab[l], l);
  });
  if (rc) return rc;
  if (icap[2] > 0)
    hipLaunchKernelGGL(mut_head_kernel, dim3((unsigned)((icap[2] + 3) / 4)), dim3(256), 0, s, pa, b.tab[2].ctr, b.tab[2].tok, b.hO[2], w->Wout_w,
                       w->Wout_b, b.row_res, b.row_lp);
  hipLaunchKernelGGL(mut_delta_kernel, dim3((unsigned)((n_var + 255) / 256)), dim3(256), 0, s, pa, b.row_res, b.row_lp, c.log_probs, b.delta);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  return NAMP_OK;
}

extern "C" {

size_t namp_mutations_workspace_bytes(int N, int K, int n_dec, int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2,
                                      int items3) {
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  return mut_layout(nullptr, N, K, n_dec, m).bytes;
}

size_t namp_mutations_in_offset(int N, int K, int n_dec, int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2,
                                int items3) {
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  return mut_layout(nullptr, N, K, n_dec, m).in_off;
}

size_t namp_mutations_out_offset(int N, int K, int n_dec, int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2,
                                 int items3) {
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  return mut_layout(nullptr, N, K, n_dec, m).out_off;
}

int namp_mutations(int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2, int items3) {
  namp_internal_detach(ATTACH_MUTATIONS);
  const int m[8] = {n_sites, n_variants, list1, list2, list3, items1, items2, items3};
  for (int v : m)
    if (v < 0) return namp_failf(NAMP_EINVAL, "namp_mutations: n_sites=%ld, n_variants=%ld and the capacities must not be negative", n_sites, n_variants);
  namp_internal_attach(ATTACH_MUTATIONS, m, 8);
  return NAMP_OK;
}

}  // extern "C"
