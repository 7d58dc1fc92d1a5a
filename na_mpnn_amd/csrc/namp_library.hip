// Translation unit of library scoring (namp_library.h): namp_library / namp_library_workspace_bytes / namp_library_in_offset /
// namp_library_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a library.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the base stream through the
// library's own building blocks (as namp_decoder_loo runs it, plus the third layer and the head), the plan, and per layer the index
// tables and one dec_items_kernel launch over (candidate, listed row) items.
#include "../../include/namp.h"
#include "namp_library.h"

#include <cstdio>

namespace {

int bfail(int code, const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return namp_internal_fail(code, buf);
}

struct LibDims { int N, K, n_var, n_chunk, rows[3]; };

// the call's buffers, carved in one fixed order (base == nullptr: sizes only)
struct LibBuffers : LooBaseStream {                                                    // (the base stream's tables and states first)
  int32_t *vpos, *flag[3], *pos[3], *list[3];                                         // the plan
  int32_t* in;                                                                         // INPUT section: positions[n_var], tokens[n_chunk][n_var]
  float *ov1;                                                                          // [n_chunk * n_var][128] layer 1's override rows
  float *hO[3], *PaO[2], *ovO[2];                                                      // [n_chunk * rows_l][128] outputs of layer l's items
  LibItemTables tab[3];
  int32_t* counts;                                                                     // OUTPUT section: int32 [64] (9 used), then
  float* tlp;                                                                          // float [n_chunk][N]
  size_t in_off, out_off, bytes;
};

LibBuffers lib_carve(void* base, const LibDims& d) {
  LibBuffers b;
  size_t off = 0;
  auto take = [&](size_t elems) {
    void* p = base ? (void*)((char*)base + off) : nullptr;
    off += (elems * 4 + 255) & ~size_t(255);
    return p;
  };
  const size_t N = (size_t)d.N, g128 = N * NAMP_HIDDEN, tpn = (d.K + 15) / 16, nc = (size_t)d.n_chunk;
  float** gs[] = {&b.Pa1, &b.Pbw1, &b.Pfw[0], &b.Pfw[1], &b.Pfw[2], &b.h1, &b.Pa2, &b.Pbw2, &b.h2, &b.Pa3, &b.Pbw3, &b.h3};
  for (float** p : gs) *p = (float*)take(g128);
  b.partial = (float*)take(N * tpn * (NAMP_HIDDEN + 1) + 3);
  b.vpos = (int32_t*)take(N);
  for (int l = 0; l < 3; ++l) { b.flag[l] = (int32_t*)take(N); b.pos[l] = (int32_t*)take(N); b.list[l] = (int32_t*)take((size_t)d.rows[l] + 1); }
  b.in_off = off;
  b.in = (int32_t*)take((size_t)d.n_var + nc * d.n_var + 1);
  b.ov1 = (float*)take(nc * d.n_var * NAMP_HIDDEN + 4);
  for (int l = 0; l < 3; ++l) {
    const size_t R = nc * d.rows[l];
    b.hO[l] = (float*)take(R * NAMP_HIDDEN + 4);
    if (l < 2) { b.PaO[l] = (float*)take(R * NAMP_HIDDEN + 4); b.ovO[l] = (float*)take(R * NAMP_HIDDEN + 4); }
    LibItemTables& t = b.tab[l];
    t.act = (int32_t*)take(R + 1); t.ctr = (int32_t*)take(R + 1); t.cen = (int32_t*)take(R + 1); t.msk = (int32_t*)take(R + 1);
    t.tok = (int32_t*)take(R + 1); t.esrc = (int32_t*)take(R * d.K + 1);
  }
  b.out_off = off;
  b.counts = (int32_t*)take(64);
  b.tlp = (float*)take(nc * N + 1);
  b.bytes = off;
  return b;
}

bool lib_dims_ok(int N, int K, int n_dec, int n_var, int n_chunk, int r1, int r2, int r3) {
  if (N < 1 || K < 1 || K > NAMP_MAX_K || K > N || n_dec != 3 || n_var < 0 || n_var > N || n_chunk < 0) return false;
  const int rows[3] = {r1, r2, r3};
  long mx = n_var > N ? n_var : N;
  for (int r : rows) {
    if (r < 0 || r > N) return false;
  }
  // every table row code (candidate * rows + position, a residue) stays below 2^28, every item count inside an int
  if ((long)(n_chunk > 0 ? n_chunk : 1) * mx >= (1L << LOO_ROW_BITS)) return false;
  return true;
}

// what the calling thread's NEXT namp_decoder_fwd call scores: taken, and cleared, by that call
struct LibAttachment { bool on; int n_var, n_chunk, rows[3]; };
thread_local LibAttachment g_lib_attached = {};

}  // namespace

// (for namp_decoder_fwd, namp.hip) the attachment of the calling thread, cleared
__attribute__((visibility("hidden"))) int namp_internal_library_take(int* n_var, int* n_chunk, int* rows) {
  const LibAttachment a = g_lib_attached;
  g_lib_attached = {};
  if (!a.on) return 0;
  *n_var = a.n_var; *n_chunk = a.n_chunk;
  for (int l = 0; l < 3; ++l) rows[l] = a.rows[l];
  return 1;
}

// the carrier's body with an attachment: base stream -> log_probs, the plan -> counts, the items -> token log-probs
__attribute__((visibility("hidden"))) int namp_internal_library_run(const NampModelW* w, const float* h_V_enc, const float* h_E, const int32_t* E_idx,
                                                                     const int32_t* S, const int32_t* mask, const int32_t* rank, float* log_probs,
                                                                     const float* logits, const float* h_V_dec, void* ws, size_t ws_bytes,
                                                                     int B_dec, int B_enc, int N, int K, int n_var, int n_chunk, const int* rows,
                                                                     void* stream) {
  if (!w || !h_V_enc || !h_E || !E_idx || !S || !mask || !rank || !log_probs || !ws)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: null pointer argument (a library was attached; mask is required)");
  if (logits || h_V_dec) return bfail(NAMP_EINVAL, "namp_decoder_fwd: logits / h_V_dec are not written with a library attached");
  if (B_dec != 1 || B_enc != 1) return bfail(NAMP_EINVAL, "namp_decoder_fwd: a library is scored on one complex (B_dec=%ld, B_enc=%ld)", B_dec, B_enc);
  if ((((uintptr_t)h_V_enc | (uintptr_t)h_E | (uintptr_t)ws | (uintptr_t)log_probs) & 15u) != 0)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: h_V_enc / h_E / log_probs / ws must be 16-byte aligned (a library was attached)");
  int prec = PREC_F32;
  int rc = loo_check_weights(w, "namp_decoder_fwd (library attached)", &prec);
  if (rc) return rc;
  if (!lib_dims_ok(N, K, w->n_dec, n_var, n_chunk, rows[0], rows[1], rows[2]))
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached library N=%ld K=%ld n_var=%ld", N, K, n_var);
  const LibDims d = {N, K, n_var, n_chunk, {rows[0], rows[1], rows[2]}};
  LibBuffers b = lib_carve(ws, d);
  if (b.bytes > ws_bytes)                                        // (the sections are part of the call's arguments: include/namp.h)
    return bfail(NAMP_EINVAL, "namp_decoder_fwd: workspace too small for the attached library (%ld bytes, %ld needed)", (long)ws_bytes, (long)b.bytes);
  const hipError_t ready = loo_items_ready();
  if (ready != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(ready));
  hipStream_t s = (hipStream_t)stream;
  const NampDecLayerW* D0 = &w->dec[0];

  // ---- base stream: tables of every layer, the states behind layers 1 and 2, the head behind layer 3
  if ((rc = loo_base_stream(w, b, h_V_enc, h_E, E_idx, S, mask, rank, log_probs, N, K, stream))) return rc;
  const float* Pa[3] = {b.Pa1, b.Pa2, b.Pa3};
  const float* Pbw[3] = {b.Pbw1, b.Pbw2, b.Pbw3};
  const float* hin[3] = {h_V_enc, b.h1, b.h2};

  // ---- the plan
  LibPlanArgs pa = {};
  pa.E_idx = E_idx; pa.rank = rank; pa.mask = mask; pa.S = S;
  pa.positions = b.in; pa.tokens = b.in + n_var;
  pa.vpos = b.vpos; pa.counts = b.counts;
  for (int l = 0; l < 3; ++l) { pa.flag[l] = b.flag[l]; pa.pos[l] = b.pos[l]; pa.list[l] = b.list[l]; pa.cap[l] = rows[l]; }
  pa.N = N; pa.K = K; pa.n_var = n_var; pa.n_chunk = n_chunk; pa.vocab = w->vocab;
  const unsigned gN = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(lib_var_kernel, dim3(gN), dim3(256), 0, s, pa);
  for (int l = 0; l < 3; ++l) hipLaunchKernelGGL(lib_flag_kernel, dim3(gN), dim3(256), 0, s, pa, l);
  hipLaunchKernelGGL(lib_compact_kernel, dim3(1), dim3(1024), 0, s, pa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  if (n_chunk == 0) return NAMP_OK;                              // (the counts only: what the caller sizes rows_l by)

  // ---- every entry from the base rows, layer 1's override rows
  const long nc = n_chunk;
  hipLaunchKernelGGL(lib_fill_kernel, dim3((unsigned)((nc * N + 255) / 256)), dim3(256), 0, s, pa, log_probs, b.tlp);
  if (n_var)
    hipLaunchKernelGGL(lib_token_rows_kernel, dim3((unsigned)((nc * n_var * (NAMP_H / 4) + 255) / 256)), dim3(256), 0, s, pa, b.Pfw[0], D0->tok,
                       b.ov1);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));

  // ---- the items, layer by layer: centre overrides and override rows come from the layer in front
  const float* cenPa[3] = {b.Pa1, b.PaO[0], b.PaO[1]};
  const float* cenH[3] = {h_V_enc, b.hO[0], b.hO[1]};
  const float* ov[3] = {b.ov1, b.ovO[0], b.ovO[1]};
  for (int l = 0; l < 3; ++l) {
    const long R = nc * rows[l];
    if (R == 0) break;                                           // (rows_1 <= rows_2 <= rows_3 for the caller who read the counts; nothing reads an empty layer)
    const NampDecLayerW* D = &w->dec[l];
    const LibItemTables& t = b.tab[l];
    hipLaunchKernelGGL(lib_items_kernel, dim3((unsigned)((R * K + 255) / 256)), dim3(256), 0, s, pa, t, l);
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
  if (nc * rows[2] > 0 && nc * rows[1] > 0 && nc * rows[0] > 0) {
    hipLaunchKernelGGL(lib_head_kernel, dim3((unsigned)((nc * rows[2] + 3) / 4)), dim3(256), 0, s, pa, b.hO[2], w->Wout_w, w->Wout_b, b.tlp);
    if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  }
  return NAMP_OK;
}

extern "C" {

size_t namp_library_workspace_bytes(int N, int K, int n_dec, int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  if (!lib_dims_ok(N, K, n_dec, n_var, n_chunk, rows1, rows2, rows3)) return 0;
  return lib_carve(nullptr, LibDims{N, K, n_var, n_chunk, {rows1, rows2, rows3}}).bytes;
}

size_t namp_library_in_offset(int N, int K, int n_dec, int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  if (!lib_dims_ok(N, K, n_dec, n_var, n_chunk, rows1, rows2, rows3)) return 0;
  return lib_carve(nullptr, LibDims{N, K, n_var, n_chunk, {rows1, rows2, rows3}}).in_off;
}

size_t namp_library_out_offset(int N, int K, int n_dec, int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  if (!lib_dims_ok(N, K, n_dec, n_var, n_chunk, rows1, rows2, rows3)) return 0;
  return lib_carve(nullptr, LibDims{N, K, n_var, n_chunk, {rows1, rows2, rows3}}).out_off;
}

int namp_library(int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  g_lib_attached = {};
  if (n_var < 0 || n_chunk < 0 || rows1 < 0 || rows2 < 0 || rows3 < 0)
    return bfail(NAMP_EINVAL, "namp_library: n_var=%ld, n_chunk=%ld and the row capacities must not be negative", n_var, n_chunk);
  g_lib_attached = {true, n_var, n_chunk, {rows1, rows2, rows3}};
  return NAMP_OK;
}

}  // extern "C"
