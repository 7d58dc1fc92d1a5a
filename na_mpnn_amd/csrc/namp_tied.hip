// Translation unit of the tied score (namp_tied.h): namp_tied_score / namp_tied_score_workspace_bytes / namp_tied_score_in_offset /
// namp_tied_score_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a tied score.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the per-residue tables of the
// encoder state, the keys, the item tables, per layer one dec_items_kernel launch over (sequence, residue) items, the head, the combine.
#include "../../include/namp.h"
#include "namp_tied.h"
#include "namp_attach.h"

namespace {

// the call's buffers, carved in one fixed order
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
  size_t in_off, out_off, bytes;                 // (all 0: the dims are refused)
};

bool tied_dims_ok(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  if (N < 1 || K < 1 || K > NAMP_MAX_K || K > N || n_dec != 3 || n_chunk < 0) return false;
  if (n_tables < 1 || n_tables > 64 || n_classes < 1 || n_classes > 64) return false;
  // every table row code (sequence * N + residue) stays below 2^28
  return (long)(n_chunk > 0 ? n_chunk : 1) * N < (1L << LOO_ROW_BITS);
}

// validates, then carves (base == nullptr: sizes only); m: n_tables, n_classes, n_chunk
TiedBuffers tied_layout(void* base, int N_, int K, int n_dec, const int* m) {
  TiedBuffers b = {};
  if (!tied_dims_ok(N_, K, n_dec, m[0], m[1], m[2])) return b;
  WsCarver c(base);
  const size_t N = (size_t)N_, R = (size_t)m[2] * N, g128 = N * NAMP_HIDDEN, r128 = R * NAMP_HIDDEN + 4;
  for (int l = 0; l < 3; ++l) b.Pfw[l] = c.take<float>(g128);
  b.Pa1 = c.take<float>(g128);
  b.gl = c.take<int32_t>(N); b.gpos = c.take<int32_t>(N); b.leader = c.take<int32_t>(N); b.key = c.take<uint32_t>(N);
  b.tab.ctr = c.take<int32_t>(R + 1); b.tab.msk = c.take<int32_t>(R + 1); b.tab.tok = c.take<int32_t>(R + 1);
  for (int q = 0; q < 2; ++q) { b.tab.cen[q] = c.take<int32_t>(R + 1); b.tab.esrc[q] = c.take<int32_t>(R * K + 1); }
  b.in_off = c.off;
  b.in = c.take<int32_t>(4 * N + 128 * (size_t)m[0] + R);
  b.tokrows = c.take<float>(r128);
  for (int l = 0; l < 2; ++l) {
    b.hO[l] = c.take<float>(r128); b.PaO[l] = c.take<float>(r128); b.bwO[l] = c.take<float>(r128); b.nbO[l] = c.take<float>(r128);
  }
  b.out_off = c.off;
  b.header = c.take<int32_t>(64);
  b.unit_lp = c.take<float>(R + 1);
  b.member_lp = c.take<float>(R + 1);
  b.bytes = c.off;
  return b;
}

}  // namespace

// the carrier's body with an attachment; m: n_tables, n_classes, n_chunk
__attribute__((visibility("hidden"))) int namp_internal_tied_run(const AttachedCall& c, const int* m) {
  const char* noun = ATTACH_NOUN[ATTACH_TIED];
  int prec = PREC_F32;
  int rc = attached_prologue(c, noun, &prec);
  if (rc) return rc;
  const NampModelW* w = c.w;
  const float *h_V_enc = c.h_V_enc, *h_E = c.h_E;
  const int32_t *E_idx = c.E_idx, *mask = c.mask, *rank = c.rank;
  float* log_probs = c.log_probs;
  void* stream = c.stream;
  const int N = c.N, K = c.K;
  struct { int n_tables, n_classes, n_chunk; } d = {m[0], m[1], m[2]};
  TiedBuffers b = tied_layout(c.ws, N, K, w->n_dec, m);
  if (!b.bytes || d.n_classes < w->vocab)
    return namp_failf(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached tied score N=%ld K=%ld n_classes=%ld", N, K, d.n_classes);
  if ((rc = attached_ready(c, noun, b.bytes))) return rc;
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
  const TiedStreamRows rows = {b.Pa1, {b.Pfw[0], b.Pfw[1], b.Pfw[2]}, b.tokrows, {b.hO[0], b.hO[1], b.tokrows},   // (layer 1 alone reads tokrows)
                               {b.PaO[0], b.PaO[1]}, {b.bwO[0], b.bwO[1]}, {b.nbO[0], b.nbO[1]}};
  if ((rc = tied_item_stream(w, prec, h_V_enc, h_E, K, R, b.tab, rows, s))) return rc;
  float* lg = b.hO[0];                                           // (layer 1's states are read by layer 2 alone: [R][vocab <= 64] fits)
  hipLaunchKernelGGL(tied_head_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, a, b.tokrows, w->Wout_w, w->Wout_b, lg);
  hipLaunchKernelGGL(tied_combine_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, a, lg, b.unit_lp, b.member_lp, log_probs);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  return NAMP_OK;
}

extern "C" {

size_t namp_tied_score_workspace_bytes(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  const int m[3] = {n_tables, n_classes, n_chunk};
  return tied_layout(nullptr, N, K, n_dec, m).bytes;
}

size_t namp_tied_score_in_offset(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  const int m[3] = {n_tables, n_classes, n_chunk};
  return tied_layout(nullptr, N, K, n_dec, m).in_off;
}

size_t namp_tied_score_out_offset(int N, int K, int n_dec, int n_tables, int n_classes, int n_chunk) {
  const int m[3] = {n_tables, n_classes, n_chunk};
  return tied_layout(nullptr, N, K, n_dec, m).out_off;
}

int namp_tied_score(int n_tables, int n_classes, int n_chunk) {
  namp_internal_detach(ATTACH_TIED);
  if (n_tables < 1 || n_tables > 64 || n_classes < 1 || n_classes > 64 || n_chunk < 0)
    return namp_failf(NAMP_EINVAL, "namp_tied_score: n_tables=%ld must be in [1, 64], n_classes=%ld in [1, 64] (the attached call refuses one below the vocabulary), n_chunk=%ld not negative", n_tables,
                      n_classes, n_chunk);
  const int m[3] = {n_tables, n_classes, n_chunk};
  namp_internal_attach(ATTACH_TIED, m, 3);
  return NAMP_OK;
}

}  // extern "C"
