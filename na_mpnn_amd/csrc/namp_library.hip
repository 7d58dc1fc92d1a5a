// Translation unit of library scoring (namp_library.h): namp_library / namp_library_workspace_bytes / namp_library_in_offset /
// namp_library_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a library.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the base stream through the
// library's own building blocks (as namp_decoder_loo runs it, plus the third layer and the head), the plan, and per layer the index
// tables and one dec_items_kernel launch over (candidate, listed row) items.
#include "../../include/namp.h"
#include "namp_library.h"
#include "namp_attach.h"

namespace {

// the call's buffers, carved in one fixed order
struct LibBuffers : LooBaseStream, LooItemRows {                                       // (the base stream's tables and states first)
  int32_t *vpos, *flag[3], *pos[3], *list[3];                                         // the plan
  int32_t* in;                                                                         // INPUT section: positions[n_var], tokens[n_chunk][n_var]
                                                                                       // (LooItemRows: [n_chunk * n_var], [n_chunk * rows_l] rows)
  LibItemTables tab[3];
  int32_t* counts;                                                                     // OUTPUT section: int32 [64] (9 used), then
  float* tlp;                                                                          // float [n_chunk][N]
  size_t in_off, out_off, bytes;                                                       // (all 0: the dims are refused)
};

bool lib_dims_ok(int N, int K, int n_dec, int n_var, int n_chunk, const int* rows) {
  if (N < 1 || K < 1 || K > NAMP_MAX_K || K > N || n_dec != 3 || n_var < 0 || n_var > N || n_chunk < 0) return false;
  long mx = n_var > N ? n_var : N;
  for (int l = 0; l < 3; ++l) {
    if (rows[l] < 0 || rows[l] > N) return false;
  }
  // every table row code (candidate * rows + position, a residue) stays below 2^28, every item count inside an int
  if ((long)(n_chunk > 0 ? n_chunk : 1) * mx >= (1L << LOO_ROW_BITS)) return false;
  return true;
}

// validates, then carves (base == nullptr: sizes only); m: n_var, n_chunk, row capacities [3]
LibBuffers lib_layout(void* base, int N_, int K, int n_dec, const int* m) {
  LibBuffers b = {};
  if (!lib_dims_ok(N_, K, n_dec, m[0], m[1], m + 2)) return b;
  WsCarver c(base);
  const int n_var = m[0], *rows = m + 2;
  const size_t N = (size_t)N_, g128 = N * NAMP_HIDDEN, tpn = (K + 15) / 16, nc = (size_t)m[1];
  float** gs[] = {&b.Pa1, &b.Pbw1, &b.Pfw[0], &b.Pfw[1], &b.Pfw[2], &b.h1, &b.Pa2, &b.Pbw2, &b.h2, &b.Pa3, &b.Pbw3, &b.h3};
  for (float** p : gs) *p = c.take<float>(g128);
  b.partial = c.take<float>(N * tpn * (NAMP_HIDDEN + 1) + 3);
  b.vpos = c.take<int32_t>(N);
  for (int l = 0; l < 3; ++l) { b.flag[l] = c.take<int32_t>(N); b.pos[l] = c.take<int32_t>(N); b.list[l] = c.take<int32_t>((size_t)rows[l] + 1); }
  b.in_off = c.off;
  b.in = c.take<int32_t>((size_t)n_var + nc * n_var + 1);
  b.ov1 = c.take<float>(nc * n_var * NAMP_HIDDEN + 4);
  for (int l = 0; l < 3; ++l) {
    const size_t R = nc * rows[l];
    b.hO[l] = c.take<float>(R * NAMP_HIDDEN + 4);
    if (l < 2) { b.PaO[l] = c.take<float>(R * NAMP_HIDDEN + 4); b.ovO[l] = c.take<float>(R * NAMP_HIDDEN + 4); }
    LibItemTables& t = b.tab[l];
    t.act = c.take<int32_t>(R + 1); t.ctr = c.take<int32_t>(R + 1); t.cen = c.take<int32_t>(R + 1); t.msk = c.take<int32_t>(R + 1);
    t.tok = c.take<int32_t>(R + 1); t.esrc = c.take<int32_t>(R * K + 1);
  }
  b.out_off = c.off;
  b.counts = c.take<int32_t>(64);
  b.tlp = c.take<float>(nc * N + 1);
  b.bytes = c.off;
  return b;
}

}  // namespace

// the carrier's body with an attachment: base stream -> log_probs, the plan -> counts, the items -> token log-probs
__attribute__((visibility("hidden"))) int namp_internal_library_run(const AttachedCall& c, const int* m) {
  const char* noun = ATTACH_NOUN[ATTACH_LIBRARY];
  int prec = PREC_F32;
  int rc = attached_prologue(c, noun, &prec);
  if (rc) return rc;
  const NampModelW* w = c.w;
  const int N = c.N, K = c.K, n_var = m[0], n_chunk = m[1], *rows = m + 2;
  LibBuffers b = lib_layout(c.ws, N, K, w->n_dec, m);
  if (!b.bytes) return namp_failf(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached library N=%ld K=%ld n_var=%ld", N, K, n_var);
  if ((rc = attached_ready(c, noun, b.bytes))) return rc;
  hipStream_t s = (hipStream_t)c.stream;

  // ---- base stream: tables of every layer, the states behind layers 1 and 2, the head behind layer 3
  if ((rc = loo_base_stream(w, b, c.h_V_enc, c.h_E, c.E_idx, c.S, c.mask, c.rank, c.log_probs, N, K, c.stream))) return rc;

  // ---- the plan
  LibPlanArgs pa = {};
  pa.E_idx = c.E_idx; pa.rank = c.rank; pa.mask = c.mask; pa.S = c.S;
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
  hipLaunchKernelGGL(lib_fill_kernel, dim3((unsigned)((nc * N + 255) / 256)), dim3(256), 0, s, pa, c.log_probs, b.tlp);
  if (n_var)
    hipLaunchKernelGGL(lib_token_rows_kernel, dim3((unsigned)((nc * n_var * (NAMP_H / 4) + 255) / 256)), dim3(256), 0, s, pa, b.Pfw[0],
                       w->dec[0].tok, b.ov1);
  if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));

  // ---- the items, layer by layer (rows_1 <= rows_2 <= rows_3 for the caller who read the counts; nothing reads an empty layer: the
  // walk ends there)
  const long R[3] = {nc * rows[0], nc * rows[1], nc * rows[2]};
  rc = loo_item_layers(w, prec, c.h_V_enc, c.h_E, K, b, b, b.tab, R, true, s, [&](int l, long Rl) {
    hipLaunchKernelGGL(lib_items_kernel, dim3((unsigned)((Rl * K + 255) / 256)), dim3(256), 0, s, pa, b.tab[l], l);
  });
  if (rc) return rc;
  if (R[2] > 0 && R[1] > 0 && R[0] > 0) {
    hipLaunchKernelGGL(lib_head_kernel, dim3((unsigned)((R[2] + 3) / 4)), dim3(256), 0, s, pa, b.hO[2], w->Wout_w, w->Wout_b, b.tlp);
    if ((e = hipGetLastError()) != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  }
  return NAMP_OK;
}

extern "C" {

size_t namp_library_workspace_bytes(int N, int K, int n_dec, int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  const int m[5] = {n_var, n_chunk, rows1, rows2, rows3};
  return lib_layout(nullptr, N, K, n_dec, m).bytes;
}

size_t namp_library_in_offset(int N, int K, int n_dec, int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  const int m[5] = {n_var, n_chunk, rows1, rows2, rows3};
  return lib_layout(nullptr, N, K, n_dec, m).in_off;
}

size_t namp_library_out_offset(int N, int K, int n_dec, int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  const int m[5] = {n_var, n_chunk, rows1, rows2, rows3};
  return lib_layout(nullptr, N, K, n_dec, m).out_off;
}

int namp_library(int n_var, int n_chunk, int rows1, int rows2, int rows3) {
  namp_internal_detach(ATTACH_LIBRARY);
  const int m[5] = {n_var, n_chunk, rows1, rows2, rows3};
  for (int v : m)
    if (v < 0) return namp_failf(NAMP_EINVAL, "namp_library: n_var=%ld, n_chunk=%ld and the row capacities must not be negative", n_var, n_chunk);
  namp_internal_attach(ATTACH_LIBRARY, m, 5);
  return NAMP_OK;
}

}  // extern "C"
