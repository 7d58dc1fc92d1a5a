// The attach-and-carry protocol of the scoring calls that ride on a decoder call, host code only: an entry point
// records a few integers for the calling thread, the caller fills an input section inside the workspace, and the thread's NEXT carrier
// call takes the record — cleared whatever becomes of that call —, carves the workspace in one fixed order, runs the route's launches
// and leaves its results in an output section.  Here: the error formatter, the workspace carver, the attachment table of
// namp_decoder_fwd's riders (namp_library.hip, namp_mutations.hip, namp_tied.hip) and the checks their bodies share.
// namp_decoder_loo's own attachment (namp_loo.hip) is a different carrier: it shares the formatter and the carver only.
#pragma once
#include "../../include/namp.h"

#include <cstdint>
#include <cstdio>

__attribute__((visibility("hidden"))) int namp_internal_fail(int code, const char* msg);      // namp.hip: sets namp_last_error()

// ---- (a) error text with up to three integers
static inline int namp_failf(int code, const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[320];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return namp_internal_fail(code, buf);
}

// ---- (b) bump allocator over the caller's workspace in 4-byte elements, every buffer rounded to 256 bytes; base == nullptr: sizes only
// (no bound: the caller compares `off` with ws_bytes once, behind the last take)
struct WsCarver {
  char* base;
  size_t off = 0;
  explicit WsCarver(void* p) : base((char*)p) {}
  template <class T>
  T* take(size_t elems) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += (elems * 4 + 255) & ~size_t(255);
    return p;
  }
};

// ---- (c) what the calling thread's NEXT namp_decoder_fwd call carries, per kind; dims: the integers of the kind's entry point
enum AttachKind { ATTACH_LIBRARY, ATTACH_MUTATIONS, ATTACH_TIED, ATTACH_STATE_MUTATIONS, ATTACH_KINDS };
constexpr int ATTACH_MAX_DIMS = 10;
struct Attachment { bool on; int dims[ATTACH_MAX_DIMS]; };
__attribute__((visibility("hidden"))) inline thread_local Attachment g_attached[ATTACH_KINDS] = {};

// an entry point clears its own kind first (bad arguments leave it cleared, the other kinds untouched), then attaches: the latest holds
static inline void namp_internal_detach(int kind) { g_attached[kind] = {}; }
static inline void namp_internal_attach(int kind, const int* dims, int n) {
  Attachment& a = g_attached[kind];
  a = {};
  a.on = true;
  for (int q = 0; q < n; ++q) a.dims[q] = dims[q];
}
// the carrier: every kind is taken and cleared, whatever becomes of the call -> bit k set where kind k was on
static inline unsigned namp_internal_take_attached(Attachment out[ATTACH_KINDS]) {
  unsigned on = 0;
  for (int k = 0; k < ATTACH_KINDS; ++k) {
    out[k] = g_attached[k];
    g_attached[k] = {};
    if (out[k].on) on |= 1u << k;
  }
  return on;
}
// what the messages call a kind
static const char* const ATTACH_NOUN[ATTACH_KINDS] = {"a library", "a mutational scan", "a tied score", "a state scan"};

// ---- (d) namp_decoder_fwd's arguments as a rider's body gets them; the bodies, one per kind
struct AttachedCall {
  const NampModelW* w;
  const float *h_V_enc, *h_E;
  const int32_t *E_idx, *S, *mask, *rank;
  float* log_probs;
  const float *logits, *h_V_dec;
  void* ws;
  size_t ws_bytes;
  int B_dec, B_enc, N, K;
  void* stream;
};
__attribute__((visibility("hidden"))) int namp_internal_library_run(const AttachedCall& c, const int* dims);       // n_var, n_chunk, row capacities [3]
__attribute__((visibility("hidden"))) int namp_internal_mutations_run(const AttachedCall& c, const int* dims);     // n_sites, n_variants, list [3] and item [3] capacities
__attribute__((visibility("hidden"))) int namp_internal_tied_run(const AttachedCall& c, const int* dims);          // n_tables, n_classes, n_chunk
__attribute__((visibility("hidden"))) int namp_internal_state_mutations_run(const AttachedCall& c, const int* dims);   // the scan's eight, n_states, L

#ifdef LOO_ROW_BITS      // (behind namp_loo.h: the units that launch dec_items_kernel)
// The checks every body starts with, in the order that decides which error a doubly-wrong call gets; noun: "a library", ...
// Behind them the body checks its dims, carves, and ends its own checks with attached_ready().
static inline int attached_prologue(const AttachedCall& c, const char* noun, int* prec) {
  char buf[192];
  auto bad = [&](const char* fmt, long a = 0, long b = 0) {
    snprintf(buf, sizeof(buf), fmt, noun);
    return namp_failf(NAMP_EINVAL, buf, a, b);
  };
  if (!c.w || !c.h_V_enc || !c.h_E || !c.E_idx || !c.S || !c.mask || !c.rank || !c.log_probs || !c.ws)
    return bad("namp_decoder_fwd: null pointer argument (%s was attached; mask is required)");
  if (c.logits || c.h_V_dec) return bad("namp_decoder_fwd: logits / h_V_dec are not written with %s attached");
  if (c.B_dec != 1 || c.B_enc != 1) return bad("namp_decoder_fwd: %s runs on one complex (B_dec=%%ld, B_enc=%%ld)", c.B_dec, c.B_enc);
  if ((((uintptr_t)c.h_V_enc | (uintptr_t)c.h_E | (uintptr_t)c.ws | (uintptr_t)c.log_probs) & 15u) != 0)
    return bad("namp_decoder_fwd: h_V_enc / h_E / log_probs / ws must be 16-byte aligned (%s was attached)");
  snprintf(buf, sizeof(buf), "namp_decoder_fwd (%s attached)", noun);
  return loo_check_weights(c.w, buf, prec);
}

// "workspace too small" (NAMP_EINVAL: the sections are part of the call's arguments, include/namp.h), then the item kernel's attributes
static inline int attached_ready(const AttachedCall& c, const char* noun, size_t need) {
  if (need > c.ws_bytes) {
    char buf[192];
    snprintf(buf, sizeof(buf), "namp_decoder_fwd: workspace too small for %s (%%ld bytes, %%ld needed)", noun);
    return namp_failf(NAMP_EINVAL, buf, (long)c.ws_bytes, (long)need);
  }
  const hipError_t ready = loo_items_ready();
  if (ready != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(ready));
  return NAMP_OK;
}
#endif
