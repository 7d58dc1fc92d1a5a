// Translation unit of the mutational scan (namp_mutations.h): namp_mutations / namp_mutations_workspace_bytes / namp_mutations_in_offset /
// namp_mutations_out_offset of include/namp.h, and the body namp_decoder_fwd runs when the calling thread has attached a scan.
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream: the base stream as
// namp_library.hip runs it, the per-site plan, and per layer the index tables and one dec_items_kernel launch over
// (variant, row of U_l(site)) items.  The four scans are ONE body (scan_run) and one layout (mut_layout) selected by a ScanKind:
// the specificity scan (namp_state_mutations, namp_state_scan.h) is the same call on the flattened graph of n_states backbone states
// with another output side, carved behind the scan's own and launched behind layer 3; the group scan (namp_group_mutations,
// namp_group_scan.h) runs the same plan on the keys of the tied stream over a tied base stream; the class scan (namp_class_mutations,
// namp_class_scan.h) is the group scan with class tables behind its input section and another combine.
#include "../../include/namp.h"
#include "namp_class_scan.h"
#include "namp_attach.h"

#include <initializer_list>

namespace {

// which scan: n_states != 0 the specificity scan on N = n_states * L flat residues; groups: the group scan; n_tables != 0: the class
// scan (groups with class tables); all zero: the plain scan
struct ScanKind {
  int n_states, L;
  bool groups;
  int n_tables, n_classes;
  // what the messages call it ("a group scan" / "a class scan" ride on the attach kind of the mutational scan: the carrier and its
  // table of kinds are unchanged, the messages of the body name them)
  const char* noun() const {
    return n_tables ? "a class scan" : groups ? "a group scan" : ATTACH_NOUN[n_states ? ATTACH_STATE_MUTATIONS : ATTACH_MUTATIONS];
  }
};

// the kind an attachment names.  dims: the scan's eight, then — ATTACH_STATE_MUTATIONS: n_states, L; ATTACH_MUTATIONS: 0 (namp_mutations),
// 1 (namp_group_mutations) or 2, n_tables | n_classes << 8 (namp_class_mutations; the table of attachments holds ten ints a kind).
// A class record without tables stays a class scan (n_tables -1), which the body refuses: it never decodes to a group scan
ScanKind scan_kind(int attach_kind, const int* m) {
  if (attach_kind == ATTACH_STATE_MUTATIONS) return {m[8], m[9], false, 0, 0};
  if (m[8] != 2) return {0, 0, m[8] == 1, 0, 0};
  return {0, 0, true, (m[9] & 0xff) ? m[9] & 0xff : -1, (m[9] >> 8) & 0xff};
}

// the call's buffers, carved in one fixed order
struct MutBuffers : LooBaseStream, LooItemRows {                                       // (the base stream's tables and states first)
  uint8_t* level;                                                                      // the plan
  int32_t *loff[3], *list[3], *ioff[3];
  int32_t* in;                                   // INPUT section: sites[n_sites][8], variants[n_var][9], w[N] (float bits)
                                                 // (states: unit_w[N] (float bits) behind them)
                                                 // (LooItemRows: [n_var * 8], [icap_l] rows)
  MutItemTables tab[3];
  int32_t* sizes;                                // OUTPUT section: int32 [n_sites][3], then
  float* delta;                                  // float [n_var], then
  int32_t* row_res;                              // int32 [icap_3], then
  float* row_lp;                                 // float [icap_3]
  float *rows, *term;                            // states only: the variants' whole rows [icap_3][64] and the leader terms [icap_3]
  float* state_delta;                            // states only, OUTPUT section behind delta: float [n_var][n_states]
  int32_t* unit_res;                             // ... behind row_lp: int32 [icap_3], then
  float *unit_lp, *base_unit;                    // float [icap_3], float [L]
  // the group scan (namp_group_scan.h) only.  Pbw2 / Pbw3 hold 2 N rows (without the token at N + j), ovO[l] 2 icap_l rows; the
  // input section carries next, first, weight bits [N] each behind w (the class scan: next, first, table_idx, weight bits [N] each,
  // tables and bias bits [n_tables][64] each); rows / term / unit_res / unit_lp as with states, base_unit [N]
  int32_t *gl, *gpos, *leader;                   // [N]
  uint32_t* key;                                 // [N]
  TiedItemTables ttab;                           // the base stream's item tables (R = N)
  int32_t* header;                               // OUTPUT section behind base_unit: int32 [64], namp_tied_score's
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
MutBuffers mut_layout(void* base, int N_, int K, int n_dec, const int* m, const ScanKind& k) {
  MutBuffers b = {};
  const bool groups = k.groups;
  if (!mut_dims_ok(N_, K, n_dec, m)) return b;
  if (k.n_states < 0 || k.n_states > MUT_E || (k.n_states && N_ % k.n_states != 0) || (groups && k.n_states)) return b;
  if (k.n_tables < 0 || k.n_tables > 64 || (k.n_tables && !groups)) return b;
  if (groups) {                                                  // two-part tables (codes N + j, R + r) and the keys as int32 ranks
    const long lim = 1L << (LOO_ROW_BITS - 1);
    if (N_ >= (1 << 27) || m[5] >= lim || m[6] >= lim) return b;
  }
  const size_t st = (size_t)k.n_states, two = groups ? 2 : 1;
  WsCarver c(base);
  const int *lcap = m + 2, *icap = m + 5;
  const size_t N = (size_t)N_, g128 = N * NAMP_HIDDEN, tpn = (K + 15) / 16, ns = (size_t)m[0], nv = (size_t)m[1];
  float** gs[] = {&b.Pa1, &b.Pbw1, &b.Pfw[0], &b.Pfw[1], &b.Pfw[2], &b.h1, &b.Pa2, &b.Pbw2, &b.h2, &b.Pa3, &b.Pbw3, &b.h3};
  for (float** p : gs) *p = c.take<float>((p == &b.Pbw2 || p == &b.Pbw3) ? two * g128 : g128);
  if (groups) {
    b.gl = c.take<int32_t>(N); b.gpos = c.take<int32_t>(N); b.leader = c.take<int32_t>(N); b.key = c.take<uint32_t>(N);
    b.ttab.ctr = c.take<int32_t>(N + 1); b.ttab.msk = c.take<int32_t>(N + 1); b.ttab.tok = c.take<int32_t>(N + 1);
    for (int q = 0; q < 2; ++q) { b.ttab.cen[q] = c.take<int32_t>(N + 1); b.ttab.esrc[q] = c.take<int32_t>(N * K + 1); }
  }
  b.partial = c.take<float>(N * tpn * (NAMP_HIDDEN + 1) + 3);
  b.level = c.take<uint8_t>((ns * N + 3) / 4 + 1);
  for (int l = 0; l < 3; ++l) {
    b.loff[l] = c.take<int32_t>(ns + 1); b.list[l] = c.take<int32_t>((size_t)lcap[l] + 1); b.ioff[l] = c.take<int32_t>(nv + 1);
  }
  b.in_off = c.off;
  b.in = c.take<int32_t>(ns * MUT_E + nv * (1 + MUT_E) + N + (st ? N : 0) + (groups ? 3 * N : 0) + (k.n_tables ? N + 128 * (size_t)k.n_tables : 0));
  b.ov1 = c.take<float>(nv * MUT_E * NAMP_HIDDEN + 4);
  for (int l = 0; l < 3; ++l) {
    const size_t R = (size_t)icap[l];
    b.hO[l] = c.take<float>(R * NAMP_HIDDEN + 4);
    if (l < 2) { b.PaO[l] = c.take<float>(R * NAMP_HIDDEN + 4); b.ovO[l] = c.take<float>(two * R * NAMP_HIDDEN + 4); }
    MutItemTables& t = b.tab[l];
    t.act = c.take<int32_t>(R + 1); t.ctr = c.take<int32_t>(R + 1); t.cen = c.take<int32_t>(R + 1); t.msk = c.take<int32_t>(R + 1);
    t.tok = c.take<int32_t>(R + 1); t.esrc = c.take<int32_t>(R * K + 1);
  }
  if (st || groups) { b.rows = c.take<float>((size_t)icap[2] * 64 + 4); b.term = c.take<float>((size_t)icap[2] + 1); }
  b.out_off = c.off;
  b.sizes = c.take<int32_t>(ns * 3 + 1);
  b.delta = c.take<float>(nv + 1);
  if (st) b.state_delta = c.take<float>(nv * st + 1);
  b.row_res = c.take<int32_t>((size_t)icap[2] + 1);
  b.row_lp = c.take<float>((size_t)icap[2] + 1);
  if (st || groups) {
    b.unit_res = c.take<int32_t>((size_t)icap[2] + 1);
    b.unit_lp = c.take<float>((size_t)icap[2] + 1);
    b.base_unit = c.take<float>((st ? N / st : N) + 1);
  }
  if (groups) b.header = c.take<int32_t>(64);
  b.bytes = c.off;
  return b;
}

// the last launch error, read and cleared (where nothing was launched since the last look: NAMP_OK, one harmless look more)
int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NAMP_OK : namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
}

// the base stream of the group and class scans: groups and keys (the kernels of the tied score as they stand, on the one sequence S),
// the header, then the TIED stream of S as items over all N residues with every layer's tables kept (with the token at j, without it at
// N + j) and its head -> log_probs.  wsec: the input section from w on.  Fills the arguments the kernels behind it take
int tied_base_stream(const AttachedCall& c, const MutBuffers& b, const ScanKind& k, const int32_t* wsec, int prec, GroupScanArgs* ga,
                     ClassScanArgs* ca) {
  const NampModelW* w = c.w;
  const NampDecLayerW* D0 = &w->dec[0];
  const int N = c.N, K = c.K;
  hipStream_t s = (hipStream_t)c.stream;
  int rc;
  TiedArgs ta = {};
  ta.E_idx = c.E_idx; ta.rank = c.rank; ta.mask = c.mask;
  ta.next = wsec + N; ta.weight = (const float*)(wsec + (k.n_tables ? 4 : 3) * (size_t)N); ta.seq = c.S;
  if (k.n_tables) {
    ca->table_idx = wsec + 3 * (size_t)N; ca->tables = wsec + 5 * (size_t)N; ca->bias = (const float*)(ca->tables + 64 * (size_t)k.n_tables);
    ca->n_tables = k.n_tables; ca->n_classes = k.n_classes;
  }
  ta.gl = b.gl; ta.gpos = b.gpos; ta.key = b.key; ta.leader = b.leader; ta.header = b.header;
  ta.N = N; ta.K = K; ta.n_tables = 1; ta.n_classes = w->vocab; ta.n_chunk = 1; ta.vocab = w->vocab;
  *ga = {ta.next, ta.weight, b.gl, b.key, b.leader, b.base_unit};
  const unsigned gN = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(loo_groups_kernel, dim3(gN), dim3(256), 0, s, ta.next, wsec + 2 * (size_t)N, c.mask, b.gl, b.gpos, N, N);
  hipLaunchKernelGGL(tied_keys_kernel, dim3(gN), dim3(256), 0, s, ta);
  hipLaunchKernelGGL(tied_count_kernel, dim3(1), dim3(256), 0, s, ta);
  if ((rc = launched())) return rc;
  NampProj pf[4] = {{D0->W1v_img, nullptr, nullptr, b.Pfw[0]}, {w->dec[1].W1v_img, nullptr, nullptr, b.Pfw[1]},
                    {w->dec[2].W1v_img, nullptr, nullptr, b.Pfw[2]}, {D0->W1a_img, D0->b1, nullptr, b.Pa1}};
  if ((rc = namp_node_linear(c.h_V_enc, nullptr, 1, 1, N, pf, 4, nullptr, c.stream))) return rc;
  hipLaunchKernelGGL(tied_items_kernel, dim3((unsigned)(((long)N * K + 255) / 256)), dim3(256), 0, s, ta, b.ttab);
  hipLaunchKernelGGL(tied_token_rows_kernel, dim3((unsigned)(((long)N * (NAMP_H / 4) + 255) / 256)), dim3(256), 0, s, ta, b.Pfw[0], D0->tok, b.Pbw1);
  if ((rc = launched())) return rc;
  const size_t g128 = (size_t)N * NAMP_HIDDEN;
  const TiedStreamRows rows = {b.Pa1, {b.Pfw[0], b.Pfw[1], b.Pfw[2]}, b.Pbw1, {b.h1, b.h2, b.h3},
                               {b.Pa2, b.Pa3}, {b.Pbw2, b.Pbw3}, {b.Pbw2 + g128, b.Pbw3 + g128}};
  if ((rc = tied_item_stream(w, prec, c.h_V_enc, c.h_E, K, N, b.ttab, rows, s))) return rc;
  hipLaunchKernelGGL(group_base_head_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, b.h3, w->Wout_w, w->Wout_b, c.log_probs, N, w->vocab);
  return NAMP_OK;
}

// the carrier's body with a scan attached: the base stream -> log_probs (the tied scans: on the keys, which are the plan's ranks) and
// the base units of S, the per-site plan -> sizes, the items -> sparse rows, then the kind's tail: own entries and deltas, or whole
// rows, units and the deltas of the leader terms
int scan_run(const AttachedCall& c, const int* m, const ScanKind& k) {
  const char* noun = k.noun();
  int prec = PREC_F32;
  int rc = attached_prologue(c, noun, &prec);
  if (rc) return rc;
  const NampModelW* w = c.w;
  const int N = c.N, K = c.K, n_sites = m[0], n_var = m[1], *lcap = m + 2, *icap = m + 5;
  if (k.n_states && (k.n_states < 1 || k.L < 1 || (long)k.n_states * k.L != N))
    return namp_failf(NAMP_EINVAL, "namp_decoder_fwd: bad dims for the attached state scan N=%ld n_states=%ld L=%ld", N, k.n_states, k.L);
  const bool cls = k.n_tables != 0, units = k.groups || k.n_states;
  const bool cls_ok = !cls || (k.n_tables >= 1 && k.n_tables <= 64 && k.n_classes >= w->vocab && k.n_classes <= 64);
  MutBuffers b = cls_ok ? mut_layout(c.ws, N, K, w->n_dec, m, k) : MutBuffers{};
  if (!b.bytes) {
    char fmt[128];
    snprintf(fmt, sizeof(fmt), "namp_decoder_fwd: bad dims for the attached %s N=%%ld K=%%ld n_sites=%%ld", noun + 2);   // (without the article)
    return namp_failf(NAMP_EINVAL, fmt, N, K, n_sites);
  }
  if ((rc = attached_ready(c, noun, b.bytes))) return rc;
  hipStream_t s = (hipStream_t)c.stream;
  const dim3 wg(256);

  // ---- base stream (namp_loo.h: the launches of namp_library.hip's, one summation order for every call that rides on this carrier;
  // the tied scans: the tied stream), then the arguments of everything behind it
  const int32_t* wsec = b.in + (size_t)n_sites * MUT_E + (size_t)n_var * (1 + MUT_E);
  GroupScanArgs ga = {};
  ClassCombine ca = {};
  if (k.groups) rc = tied_base_stream(c, b, k, wsec, prec, &ga, &ca.c);
  else rc = loo_base_stream(w, b, c.h_V_enc, c.h_E, c.E_idx, c.S, c.mask, c.rank, c.log_probs, N, K, c.stream);
  if (rc) return rc;
  MutPlanArgs pa = {};
  pa.E_idx = c.E_idx; pa.rank = k.groups ? (const int32_t*)b.key : c.rank; pa.mask = c.mask; pa.S = c.S;
  pa.sites = b.in; pa.variants = b.in + (size_t)n_sites * MUT_E; pa.w = (const float*)wsec;
  pa.level = b.level; pa.sizes = b.sizes;
  for (int l = 0; l < 3; ++l) { pa.loff[l] = b.loff[l]; pa.list[l] = b.list[l]; pa.ioff[l] = b.ioff[l]; pa.lcap[l] = lcap[l]; pa.icap[l] = icap[l]; }
  pa.N = N; pa.K = K; pa.n_sites = n_sites; pa.n_var = n_var; pa.vocab = w->vocab;
  StateScanArgs sa = {};
  sa.base_lp = c.log_probs; sa.rows = b.rows; sa.term = b.term; sa.row_res = b.row_res; sa.row_lp = b.row_lp; sa.unit_res = b.unit_res;
  sa.unit_lp = b.unit_lp; sa.delta = b.delta; sa.ctr = b.tab[2].ctr; sa.tok = b.tab[2].tok;
  sa.n_states = k.n_states ? k.n_states : 1; sa.L = N / sa.n_states;
  if (k.n_states) { sa.unit_w = (const float*)(wsec + N); sa.base_unit = b.base_unit; sa.state_delta = b.state_delta; }

  // ---- the units of S: every call leaves them, whatever its sites
  if (cls) hipLaunchKernelGGL(group_base_unit_kernel<ClassCombine>, dim3((unsigned)((N + 3) / 4)), wg, 0, s, pa, ga, ca, c.log_probs);
  else if (k.groups) hipLaunchKernelGGL(group_base_unit_kernel<GroupCombine>, dim3((unsigned)((N + 3) / 4)), wg, 0, s, pa, ga, GroupCombine{}, c.log_probs);
  else if (k.n_states) hipLaunchKernelGGL(state_base_unit_kernel, dim3((unsigned)((sa.L + 3) / 4)), wg, 0, s, pa, sa);
  if ((rc = launched())) return rc;
  if (n_sites == 0) return NAMP_OK;

  // ---- the plan: levels and sizes per site, the prefix sums, the lists
  hipLaunchKernelGGL(mut_plan_kernel, dim3((unsigned)n_sites), wg, 0, s, pa);
  if ((rc = launched())) return rc;
  if (n_var == 0) return NAMP_OK;                                // (the sizes only: what the caller cuts its chunks by)
  hipLaunchKernelGGL(mut_offsets_kernel, dim3(1), wg, 0, s, pa);
  hipLaunchKernelGGL(mut_lists_kernel, dim3((unsigned)n_sites), wg, 0, s, pa);
  hipLaunchKernelGGL(mut_token_rows_kernel, dim3((unsigned)(((long)n_var * MUT_E * (NAMP_H / 4) + 255) / 256)), wg, 0, s, pa, b.Pfw[0],
                     w->dec[0].tok, b.ov1);
  if ((rc = launched())) return rc;

  // ---- the items, layer by layer (an empty layer is stepped over: whatever would read its rows finds none and reads base)
  const long R[3] = {icap[0], icap[1], icap[2]};
  rc = loo_item_layers(w, prec, c.h_V_enc, c.h_E, K, b, b, b.tab, R, false, s, [&](int l, long Rl) {
    const dim3 grid((unsigned)((Rl * K + 255) / 256));
    if (k.groups) hipLaunchKernelGGL(mut_items_kernel<GroupScanArgs>, grid, wg, 0, s, pa, ga, b.tab[l], l);
    else hipLaunchKernelGGL(mut_items_kernel<MutPlainEdges>, grid, wg, 0, s, pa, MutPlainEdges{}, b.tab[l], l);
  }, k.groups);
  if (rc) return rc;

  // ---- the tail: the own entries and their deltas, or the whole rows, the units and the deltas of the leader terms
  const dim3 rows3((unsigned)((icap[2] + 3) / 4)), vars((unsigned)((n_var + 255) / 256));
  if (!units) {
    if (icap[2] > 0)
      hipLaunchKernelGGL(mut_head_kernel, rows3, wg, 0, s, pa, b.tab[2].ctr, b.tab[2].tok, b.hO[2], w->Wout_w, w->Wout_b, b.row_res, b.row_lp);
    hipLaunchKernelGGL(mut_delta_kernel, vars, wg, 0, s, pa, b.row_res, b.row_lp, c.log_probs, b.delta);
    return launched();
  }
  if (icap[2] > 0) {
    hipLaunchKernelGGL(state_head_kernel, rows3, wg, 0, s, pa, sa, b.hO[2], w->Wout_w, w->Wout_b);
    if (cls) hipLaunchKernelGGL(group_unit_kernel<ClassCombine>, rows3, wg, 0, s, pa, sa, ga, ca);
    else if (k.groups) hipLaunchKernelGGL(group_unit_kernel<GroupCombine>, rows3, wg, 0, s, pa, sa, ga, GroupCombine{});
    else hipLaunchKernelGGL(state_unit_kernel, rows3, wg, 0, s, pa, sa);
  }
  hipLaunchKernelGGL(state_delta_kernel, vars, wg, 0, s, pa, sa);
  if (k.n_states) hipLaunchKernelGGL(state_block_delta_kernel, dim3((unsigned)(((long)n_var * k.n_states + 255) / 256)), wg, 0, s, pa, sa);
  return launched();
}

// what the size functions of a family report: the layout without a workspace (bytes, in_off, out_off; all 0: the dims are refused)
MutBuffers scan_sizes(int N, int K, int n_dec, const ScanKind& k, std::initializer_list<int> m) { return mut_layout(nullptr, N, K, n_dec, m.begin(), k); }

bool class_dims_ok(int n_tables, int n_classes) { return n_tables >= 1 && n_tables <= 64 && n_classes >= 1 && n_classes <= 64; }

// an entry point: clears its kind, refuses negative counts, runs the family's own check (0, or the error it set) and attaches
// dims: the scan's eight, then the kind's (scan_kind)
template <class Check>
int scan_attach(const char* who, int attach_kind, std::initializer_list<int> dims, Check family) {
  namp_internal_detach(attach_kind);
  const int* m = dims.begin();
  for (int q = 0; q < 8; ++q)
    if (m[q] < 0) {
      char fmt[128];
      snprintf(fmt, sizeof(fmt), "%s: n_sites=%%ld, n_variants=%%ld and the capacities must not be negative", who);
      return namp_failf(NAMP_EINVAL, fmt, m[0], m[1]);
    }
  if (const int rc = family()) return rc;
  namp_internal_attach(attach_kind, m, (int)dims.size());
  return NAMP_OK;
}

}  // namespace

__attribute__((visibility("hidden"))) int namp_internal_mutations_run(const AttachedCall& c, const int* m) {
  return scan_run(c, m, scan_kind(ATTACH_MUTATIONS, m));
}
__attribute__((visibility("hidden"))) int namp_internal_state_mutations_run(const AttachedCall& c, const int* m) {
  return scan_run(c, m, scan_kind(ATTACH_STATE_MUTATIONS, m));
}

// the eight counts every entry point ends with (the full signatures: include/namp.h)
#define SCAN_COUNTS int n_sites, int n_variants, int list1, int list2, int list3, int items1, int items2, int items3
#define SCAN_M n_sites, n_variants, list1, list2, list3, items1, items2, items3

extern "C" {

size_t namp_mutations_workspace_bytes(int N, int K, int n_dec, SCAN_COUNTS) { return scan_sizes(N, K, n_dec, {}, {SCAN_M}).bytes; }
size_t namp_mutations_in_offset(int N, int K, int n_dec, SCAN_COUNTS) { return scan_sizes(N, K, n_dec, {}, {SCAN_M}).in_off; }
size_t namp_mutations_out_offset(int N, int K, int n_dec, SCAN_COUNTS) { return scan_sizes(N, K, n_dec, {}, {SCAN_M}).out_off; }
int namp_mutations(SCAN_COUNTS) {
  return scan_attach("namp_mutations", ATTACH_MUTATIONS, {SCAN_M}, [] { return 0; });
}

size_t namp_state_mutations_workspace_bytes(int N, int K, int n_dec, int n_states, SCAN_COUNTS) {
  return n_states < 1 ? 0 : scan_sizes(N, K, n_dec, {n_states}, {SCAN_M}).bytes;
}
size_t namp_state_mutations_in_offset(int N, int K, int n_dec, int n_states, SCAN_COUNTS) {
  return n_states < 1 ? 0 : scan_sizes(N, K, n_dec, {n_states}, {SCAN_M}).in_off;
}
size_t namp_state_mutations_out_offset(int N, int K, int n_dec, int n_states, SCAN_COUNTS) {
  return n_states < 1 ? 0 : scan_sizes(N, K, n_dec, {n_states}, {SCAN_M}).out_off;
}
int namp_state_mutations(int n_states, int L, SCAN_COUNTS) {
  return scan_attach("namp_state_mutations", ATTACH_STATE_MUTATIONS, {SCAN_M, n_states, L}, [&] {
    if (n_states >= 1 && n_states <= MUT_E && L >= 1) return 0;
    return namp_failf(NAMP_EINVAL, "namp_state_mutations: n_states=%ld must lie in [1, %ld] and L=%ld be positive", n_states, MUT_E, L);
  });
}

size_t namp_group_mutations_workspace_bytes(int N, int K, int n_dec, SCAN_COUNTS) { return scan_sizes(N, K, n_dec, {0, 0, true}, {SCAN_M}).bytes; }
size_t namp_group_mutations_in_offset(int N, int K, int n_dec, SCAN_COUNTS) { return scan_sizes(N, K, n_dec, {0, 0, true}, {SCAN_M}).in_off; }
size_t namp_group_mutations_out_offset(int N, int K, int n_dec, SCAN_COUNTS) { return scan_sizes(N, K, n_dec, {0, 0, true}, {SCAN_M}).out_off; }
int namp_group_mutations(SCAN_COUNTS) {
  return scan_attach("namp_group_mutations", ATTACH_MUTATIONS, {SCAN_M, 1}, [] { return 0; });
}

size_t namp_class_mutations_workspace_bytes(int N, int K, int n_dec, int n_tables, int n_classes, SCAN_COUNTS) {
  return class_dims_ok(n_tables, n_classes) ? scan_sizes(N, K, n_dec, {0, 0, true, n_tables, n_classes}, {SCAN_M}).bytes : 0;
}
size_t namp_class_mutations_in_offset(int N, int K, int n_dec, int n_tables, int n_classes, SCAN_COUNTS) {
  return class_dims_ok(n_tables, n_classes) ? scan_sizes(N, K, n_dec, {0, 0, true, n_tables, n_classes}, {SCAN_M}).in_off : 0;
}
size_t namp_class_mutations_out_offset(int N, int K, int n_dec, int n_tables, int n_classes, SCAN_COUNTS) {
  return class_dims_ok(n_tables, n_classes) ? scan_sizes(N, K, n_dec, {0, 0, true, n_tables, n_classes}, {SCAN_M}).out_off : 0;
}
int namp_class_mutations(int n_tables, int n_classes, SCAN_COUNTS) {
  return scan_attach("namp_class_mutations", ATTACH_MUTATIONS, {SCAN_M, 2, (n_tables & 0xff) | ((n_classes & 0xff) << 8)}, [&] {
    if (class_dims_ok(n_tables, n_classes)) return 0;
    return namp_failf(NAMP_EINVAL, "namp_class_mutations: n_tables=%ld must be in [1, 64], n_classes=%ld in [1, 64] (the attached call refuses one below the vocabulary)",
                      n_tables, n_classes);
  });
}

}  // extern "C"

#undef SCAN_COUNTS
#undef SCAN_M
