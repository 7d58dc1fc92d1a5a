// Translation unit of the tied score (namp_tied.h): namp_tied_score / namp_tied_score_workspace_bytes / namp_tied_score_in_offset /
// namp_tied_score_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a tied score.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the per-residue tables of the
// encoder state, the keys, the item tables, per layer one dec_items_kernel launch over (sequence, residue) items, the head, the combine.
#include "../../include/namp.h"
#include "namp_tied.h"

#include <cstdio>

namespace {

int bfail(int code, const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return namp_internal_fail(code, buf);
}

struct TiedDims { int N, K, n_tables, n_classes, n_chunk; };

// the call's buffers, carved in one fixed order (base == nullptr: sizes only)
struct TiedBuffers {
  float *Pfw[3], *Pa1;                           // [N][128] W1v_l . h_V_enc, W1a_1 . h_V_enc + b1
  int32_t *gl, *gpos, *leader;                   // [N]
  uint32_t* key;                                 // [N]
  TiedItemTables tab;
  int32_t* in;                                   // INPUT section: next, first, table_idx, weight bits [N] each, tables and bias bits
                                                 // [n_tables][64] each, sequences [n_chunk][N]
  float* tokrows;                                // [R][128] layer 1's rows with token; layer 3's states afterwards
  float *hO[2], *PaO[2], *bwO[2], *nbO[2];       // [R][128] outputs of the items of layers 1, 2; hO[0] holds the logits rows at the end
  int32_t* header;                               // OUTPUT section: int32 [64], then
  float* unit_lp;                                // float [n_chunk][N], then
  float* member_lp;                              // float [n_chunk][N]
  size_t in_off, out_off, bytes;
};

TiedBuffers tied_carve(void* base, const TiedDims& d) {
  TiedBuffers b;
  size_t off = 0;
  auto take = [&](size_t elems) {
    void* p = base ? (void*)((char*)base + off) : nullptr;
    off += (elems * 4 + 255) & ~size_t(255);
    return p;
  };
  const size_t N = (size_t)d.N, R = (size_t)d.n_chunk * N, g128 = N * NAMP_HIDDEN, r128 = R * NAMP_HIDDEN + 4;
  for (int l = 0; l < 3; ++l) b.Pfw[l] = (float*)take(g128);
  b.Pa1 = (float*)take(g128);
  b.gl = (int32_t*)take(N); b.gpos = (int32_t*)take(N); b.leader = (int32_t*)take(N); b.key = (uint32_t*)take(N);
  b.tab.ctr = (int32_t*)take(R + 1); b.tab.msk = (int32_t*)take(R + 1); b.tab.tok = (int32_t*)take(R + 1);
  for (int q = 0; q < 2; ++q) { b.tab.cen[q] = (int32_t*)take(R + 1); b.tab.esrc[q] = (int32_t*)take(R * d.K + 1); }
  b.in_off = off;
  b.in = (int32_t*)take(4 * N + 128 * (size_t)d.n_tables + R);
  b.tokrows = (float*)take(r128);
  for (int l = 0; l < 2; ++l) {
    b.hO[l] = (float*)take(r128); b.PaO[l] = (float*)take(r128); b.bwO[l] = (float*)take(r128); b.nbO[l] = (float*)take(r128);
  }
  b.out_off = off;
  b.header = (int32_t*)take(64);
  b.unit_lp = (float*)take(R + 1);
  b.member_lp = (float*)take(R + 1);
  b.bytes = off;
  return b;
}

bool tied_dims_ok(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  if (N < 1 || K < 1 || K > NAMP_MAX_K || K > N || n_dec != 3 || n_chunk < 0) return false;
  if (n_tables < 1 || n_tables > 64 || n_classes < 1 || n_classes > 64) return false;
  // every table row code (sequence * N + residue) stays below 2^28
  return (long)(n_chunk > 0 ? n_chunk : 1) * N < (1L << LOO_ROW_BITS);
}

// what the calling thread's NEXT namp_decoder_fwd call scores: taken, and cleared, by that call
struct TiedAttachment { bool on; int dims[3]; };
thread_local TiedAttachment g_tied_attached = {};

}  // namespace

// (for namp_decoder_fwd, namp.hip) the attachment of the calling thread, cleared
__attribute__((visibility("hidden"))) int namp_internal_tied_take(int* dims) {
  const TiedAttachment a = g_tied_attached;
  g_tied_attached = {};
  if (!a.on) return 0;
  for (int q = 0; q < 3; ++q) dims[q] = a.dims[q];
  return 1;
}

// the carrier's body with an attachment; m: n_tables, n_classes, n_chunk
__attribute__((visibility("hidden"))) int namp_internal_tied_run(const NampModelW* w, const float* h_V_enc, const float* h_E, const int32_t* E_idx,
                                                                  const int32_t* S, const int32_t* mask, const int32_t* rank, float* log_probs,
                                                                  const float* logits, const float* h_V_dec, void* ws, size_t ws_bytes,
                                                                  int B_dec, int B_enc, int N, int K, const int* m, void* stream) {
  if (!w || !h_V_enc || !h_E || !E_idx || !S || !mask || !rank || !log_probs || !ws)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: null pointer argument (a tied score was attached; mask is required)");
  if (logits || h_V_dec) return bfail(NAMP_EINVAL, "namp_decoder_fwd: logits / h_V_dec are not written with a tied score attached");
  if (B_dec != 1 || B_enc != 1) return bfail(NAMP_EINVAL, "namp_decoder_fwd: a tied score runs on one complex (B_dec=%ld, B_enc=%ld)", B_dec, B_enc);
  if ((((uintptr_t)h_V_enc | (uintptr_t)h_E | (uintptr_t)ws | (uintptr_t)log_probs) & 15u) != 0)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: h_V_enc / h_E / log_probs / ws must be 16-byte aligned (a tied score was attached)");
  int prec = PREC_F32;
  int rc = loo_check_weights(w, "namp_decoder_fwd (tied score attached)", &prec);
  if (rc) return rc;
  if (!tied_dims_ok(N, K, w->n_dec, m[0], m[1], m[2]) || m[1] < w->vocab)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached tied score N=%ld K=%ld n_classes=%ld", N, K, m[1]);
  const TiedDims d = {N, K, m[0], m[1], m[2]};
  TiedBuffers b = tied_carve(ws, d);
  if (b.bytes > ws_bytes)                                        // (the sections are part of the call's arguments: include/namp.h)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: workspace too small for the attached tied score (%ld bytes, %ld needed)", (long)ws_bytes,
                 (long)b.bytes);
  const hipError_t ready = loo_items_ready();
  if (ready != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(ready));
  hipStream_t s = (hipStream_t)stream;
  const NampDecLayerW *D0 = &w->dec[0], *D1 = &w->dec[1], *D2 = &w->dec[2];
  const long R = (long)d.n_chunk * N;

  TiedArgs a = {};
  a.E_idx = E_idx; a.rank = rank; a.mask = mask;
  const int32_t* first = b.in + N;
  a.next = b.in; a.table_idx = b.in + 2 * (size_t)N; a.weight = (const float*)(b.in + 3 * (size_t)N);
  a.tables = b.in + 4 * (size_t)N; a.bias = (const float*)(a.tables + 64 * (size_t)d.n_tables); a.seq = a.tables + 128 * (size_t)d.n_tables;
  a.gl = b.gl; a.gpos = b.gpos; a.key = b.key; a.leader = b.leader; a.header = b.header;
  a.N = N; a.K = K; a.n_tables = d.n_tables; a.n_classes = d.n_classes; a.n_chunk = d.n_chunk; a.vocab = w->vocab;

  // ---- the plan: groups (the walk of the group conditionals, as is), keys and leaders, the header
  const unsigned gN = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(loo_groups_kernel, dim3(gN), dim3(256), 0, s, a.next, first, mask, b.gl, b.gpos, N, N);
  hipLaunchKernelGGL(tied_keys_kernel, dim3(gN), dim3(256), 0, s, a);
  hipLaunchKernelGGL(tied_count_kernel, dim3(1), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  if (d.n_chunk == 0) return NAMP_OK;                            // (the plan alone; log_probs is not written)

  // ---- what every sequence shares: the forward tables of the three layers and layer 1's centre, from the encoder state
  NampProj pf[4] = {{D0->W1v_img, nullptr, nullptr, b.Pfw[0]}, {D1->W1v_img, nullptr, nullptr, b.Pfw[1]}, {D2->W1v_img, nullptr, nullptr, b.Pfw[2]},
                    {D0->W1a_img, D0->b1, nullptr, b.Pa1}};
  if ((rc = namp_node_linear(h_V_enc, nullptr, 1, 1, N, pf, 4, nullptr, stream))) return rc;
  hipLaunchKernelGGL(tied_items_kernel, dim3((unsigned)((R * K + 255) / 256)), dim3(256), 0, s, a, b.tab);
  hipLaunchKernelGGL(tied_token_rows_kernel, dim3((unsigned)((R * (NAMP_H / 4) + 255) / 256)), dim3(256), 0, s, a, b.Pfw[0], D0->tok, b.tokrows);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));

  // ---- the items, layer by layer: T0 rows with token, T1 the layer's forward table, T2 rows without token
  float* hO[3] = {b.hO[0], b.hO[1], b.tokrows};                  // (layer 1 alone reads tokrows)
  const float* cenPa[3] = {b.Pa1, b.PaO[0], b.PaO[1]};
  const float* cenH[3] = {h_V_enc, b.hO[0], b.hO[1]};
  const float* T0[3] = {b.tokrows, b.bwO[0], b.bwO[1]};
  const float* T2[3] = {b.Pfw[0], b.nbO[0], b.nbO[1]};
  for (int l = 0; l < 3; ++l) {
    const NampDecLayerW* D = &w->dec[l];
    const int q = l ? 1 : 0;
    LooItemArgs it = loo_items(D, prec, h_E, K, R, nullptr, b.tab.ctr, b.tab.cen[q], b.tab.esrc[q], b.Pa1, cenPa[l], h_V_enc, cenH[l], T0[l],
                               b.Pfw[l], T2[l]);
    loo_tail(it.tail, D, b.tab.msk, b.tab.tok, hO[l]);
    if (l < 2) {
      const NampDecLayerW* Dn = &w->dec[l + 1];
      loo_proj(it.tail, Dn->W1a_img, Dn->b1, nullptr, b.PaO[l]);
      loo_proj(it.tail, Dn->W1v_img, nullptr, Dn->tok, b.bwO[l]);
      loo_proj(it.tail, Dn->W1v_img, nullptr, nullptr, b.nbO[l]);
    }
    if ((rc = launch_items(it, prec, s))) return rc;
  }
  float* lg = b.hO[0];                                           // (layer 1's states are read by layer 2 alone: [R][vocab <= 64] fits)
  hipLaunchKernelGGL(tied_head_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, a, hO[2], w->Wout_w, w->Wout_b, lg);
  hipLaunchKernelGGL(tied_combine_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, a, lg, b.unit_lp, b.member_lp, log_probs);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  return NAMP_OK;
}

extern "C" {

size_t namp_tied_score_workspace_bytes(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  if (!tied_dims_ok(N, K, n_dec, n_tables, n_classes, n_chunk)) return 0;
  return tied_carve(nullptr, TiedDims{N, K, n_tables, n_classes, n_chunk}).bytes;
}

size_t namp_tied_score_in_offset(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  if (!tied_dims_ok(N, K, n_dec, n_tables, n_classes, n_chunk)) return 0;
  return tied_carve(nullptr, TiedDims{N, K, n_tables, n_classes, n_chunk}).in_off;
}

size_t namp_tied_score_out_offset(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  if (!tied_dims_ok(N, K, n_dec, n_tables, n_classes, n_chunk)) return 0;
  return tied_carve(nullptr, TiedDims{N, K, n_tables, n_classes, n_chunk}).out_off;
}

int namp_tied_score(int n_tables, int n_classes, int n_chunk) {
  g_tied_attached = {};
  if (n_tables < 1 || n_tables > 64 || n_classes < 1 || n_classes > 64 || n_chunk < 0)
    return bfail(NAMP_EINVAL, "namp_tied_score: n_tables=%ld must be in [1, 64], n_classes=%ld in [1, 64] (the attached call refuses one below the vocabulary), n_chunk=%ld not negative", n_tables,
                 n_classes, n_chunk);
  g_tied_attached = {true, {n_tables, n_classes, n_chunk}};
  return NAMP_OK;
}

}  // extern "C"
