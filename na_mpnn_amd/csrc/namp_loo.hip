// Translation unit of the leave-one-out decoder (namp_loo.h): namp_loo_workspace_bytes / namp_decoder_loo of include/namp.h, and the
// group conditionals riding on it (namp_loo_groups_workspace_bytes / namp_loo_groups_offset / namp_loo_groups; the pair entry
// points namp_loo_pairs_workspace_bytes / namp_loo_pairs_offset / namp_loo_pairs attach the same thing), and pair classes on them
// (namp_loo_classes_workspace_bytes / namp_loo_classes_out_offset / namp_loo_classes).
// Host code only validates, carves the caller's workspace and enqueues launches on the caller's stream.  The base stream's
// per-layer states and tables come from the library's own building blocks (namp_node_linear, namp_dec_message_update, ...).
#include "../../include/namp.h"
#include "namp_loo.h"
#include "namp_attach.h"

namespace {

// the call's buffers, carved in one fixed order (base == nullptr: sizes only)
struct LooBuffers {
  float *Pa1, *Pbw1, *Pfw[3], *h1, *Pa2, *Pbw2, *h2, *Pa3, *Pbw3, *h1o, *Pa2o, *h2o, *Pa3o, *h3o, *partial;
  float *h1O, *Pa2O, *Pbw2O, *h2O, *Pbw3O;
  int32_t *rev, *act1, *act2, *ctr1, *ctr2, *cen2, *msk1, *S1, *msk2, *S2, *eo1, *eo2, *eo3, *idG, *ovG, *esrc1, *esrc2;
  size_t bytes;
  // with an attachment, behind everything above (so that a call without one carves exactly what it always did):
  int32_t *pin;            // the caller-filled input section: next[G], first[G], map_idx[G], weight[G], maps[n_maps][64] (classes: + bias[n_maps][64])
  int32_t *gl, *gpos;      // [G] leader / listed position of every residue (loo_groups_kernel)
  float *PfwQ[2];          // [2 G][128] the forward tables of layers 2 / 3: rows G.. = W1v . (own layer-1 / layer-2 state), no token — what
                           // a member reads for an earlier-listed one
  int32_t *gkey;           // [R] the stream and listed position an active phase-1 slot names
  size_t pin_off, group_bytes;
  // with pair classes, behind those, the OUTPUT section:
  float *cls;              // [G][64] the class row of every residue (-inf rows on all but the leaders of valid groups)
  size_t cls_off, cls_bytes;
};

LooBuffers loo_carve(void* base, long G, int K, int n_maps = 0, bool classes = false) {
  LooBuffers b;
  WsCarver c(base);
  const size_t g128 = (size_t)G * NAMP_HIDDEN, R = (size_t)G * K, r128 = R * NAMP_HIDDEN, tpn = (K + 15) / 16;
  float** gs[] = {&b.Pa1, &b.Pbw1, &b.Pfw[0], &b.Pfw[1], &b.Pfw[2], &b.h1, &b.Pa2, &b.Pbw2, &b.h2, &b.Pa3, &b.Pbw3,
                  &b.h1o, &b.Pa2o, &b.h2o, &b.Pa3o, &b.h3o};
  for (float** p : gs) *p = c.take<float>(g128);
  b.partial = c.take<float>((size_t)G * tpn * (NAMP_HIDDEN + 1) + 3);
  float** rs[] = {&b.h1O, &b.Pa2O, &b.Pbw2O, &b.h2O, &b.Pbw3O};
  for (float** p : rs) *p = c.take<float>(r128);
  int32_t** ri[] = {&b.rev, &b.act1, &b.act2, &b.ctr1, &b.ctr2, &b.cen2, &b.msk1, &b.S1, &b.msk2, &b.S2, &b.eo1, &b.eo2, &b.eo3};
  for (int32_t** p : ri) *p = c.take<int32_t>(R);
  b.idG = c.take<int32_t>((size_t)G); b.ovG = c.take<int32_t>((size_t)G);
  b.esrc1 = c.take<int32_t>(R * K); b.esrc2 = c.take<int32_t>(R * K);
  b.bytes = c.off;
  b.pin_off = c.off;
  b.pin = c.take<int32_t>((size_t)4 * G + (size_t)64 * n_maps * (classes ? 2 : 1));
  b.gl = c.take<int32_t>((size_t)G); b.gpos = c.take<int32_t>((size_t)G);
  b.PfwQ[0] = c.take<float>(2 * g128); b.PfwQ[1] = c.take<float>(2 * g128);
  b.gkey = c.take<int32_t>(R);
  b.group_bytes = c.off;
  b.cls_off = c.off;
  b.cls = c.take<float>((size_t)64 * G);
  b.cls_bytes = c.off;
  return b;
}

int loo_dims(long B, long N, long K) {
  if (B < 1 || N < 1 || K < 1 || K > NAMP_MAX_K || K > N) return namp_failf(NAMP_EINVAL, "namp_decoder_loo: bad dims B=%ld N=%ld K=%ld", B, N, K);
  if (B * N * K >= (1L << LOO_ROW_BITS)) return namp_failf(NAMP_EINVAL, "namp_decoder_loo: B*N*K=%ld exceeds 2^28 item rows", B * N * K);
  return NAMP_OK;
}

// what the calling thread's NEXT namp_decoder_loo call ties: taken, and cleared, by that call; the latest attachment holds
struct LooAttachment {
  int n_tables;            // token maps / class tables in the input section, 0: nothing attached
  int n_classes;           // namp_loo_classes: the classes the tables speak of, else 0
  bool as_pairs;           // attached through namp_loo_pairs / namp_loo_classes(..., 0): what the call's messages name
};
thread_local LooAttachment g_loo_attached = {};

}  // namespace

extern "C" {

size_t namp_loo_pairs_workspace_bytes(int B, int N, int K, int n_dec, int n_maps) {
  return namp_loo_groups_workspace_bytes(B, N, K, n_dec, n_maps);
}

size_t namp_loo_pairs_offset(int B, int N, int K, int n_dec) { return namp_loo_workspace_bytes(B, N, K, n_dec); }

int namp_loo_pairs(int n_maps) {
  g_loo_attached = {};
  if (n_maps < 1 || n_maps > 64) return namp_failf(NAMP_EINVAL, "namp_loo_pairs: n_maps=%ld must be in [1, 64]", n_maps);
  g_loo_attached = {n_maps, 0, true};
  return NAMP_OK;
}

size_t namp_loo_groups_workspace_bytes(int B, int N, int K, int n_dec, int n_maps) {
  if (namp_loo_workspace_bytes(B, N, K, n_dec) == 0 || n_maps < 1 || n_maps > 64) return 0;
  return loo_carve(nullptr, (long)B * N, K, n_maps).group_bytes;
}

size_t namp_loo_groups_offset(int B, int N, int K, int n_dec) { return namp_loo_workspace_bytes(B, N, K, n_dec); }

int namp_loo_group_max(void) { return NAMP_LOO_GROUP_MAX; }

int namp_loo_groups(int n_maps) {
  g_loo_attached = {};
  if (n_maps < 1 || n_maps > 64) return namp_failf(NAMP_EINVAL, "namp_loo_groups: n_maps=%ld must be in [1, 64]", n_maps);
  g_loo_attached = {n_maps, 0, false};
  return NAMP_OK;
}

// (pair classes: the input section grows by the biases, the output section lies behind the carve; `groups` only has to be valid)
size_t namp_loo_classes_workspace_bytes(int B, int N, int K, int n_dec, int n_tables, int groups) {
  if (namp_loo_groups_workspace_bytes(B, N, K, n_dec, n_tables) == 0 || groups < 0 || groups > 1) return 0;
  return loo_carve(nullptr, (long)B * N, K, n_tables, true).cls_bytes;
}

size_t namp_loo_classes_out_offset(int B, int N, int K, int n_dec, int n_tables, int groups) {
  if (namp_loo_groups_workspace_bytes(B, N, K, n_dec, n_tables) == 0 || groups < 0 || groups > 1) return 0;
  return loo_carve(nullptr, (long)B * N, K, n_tables, true).cls_off;
}

int namp_loo_classes(int n_tables, int n_classes, int groups) {
  g_loo_attached = {};
  if (n_tables < 1 || n_tables > 64) return namp_failf(NAMP_EINVAL, "namp_loo_classes: n_tables=%ld must be in [1, 64]", n_tables);
  if (n_classes < 1 || n_classes > 64) return namp_failf(NAMP_EINVAL, "namp_loo_classes: n_classes=%ld must be in [vocab, 64]", n_classes);
  if (groups < 0 || groups > 1) return namp_failf(NAMP_EINVAL, "namp_loo_classes: groups=%ld must be 0 (pairs) or 1 (groups)", groups);
  g_loo_attached = {n_tables, n_classes, groups == 0};
  return NAMP_OK;
}

size_t namp_loo_workspace_bytes(int B, int N, int K, int n_dec) {
  if (B < 1 || N < 1 || K < 1 || K > NAMP_MAX_K || n_dec != 3) return 0;
  return loo_carve(nullptr, (long)B * N, K).bytes;
}

int namp_decoder_loo(const NampModelW* w, const float* h_V_enc, const float* h_E, const int32_t* E_idx, const int32_t* S,
                     const int32_t* mask, const int32_t* rank, float* log_probs, int32_t* counts, void* ws, size_t ws_bytes,
                     int B, int N, int K, void* stream) {
  const LooAttachment att = g_loo_attached;
  g_loo_attached = {};                                           // (one call only, whatever becomes of it)
  const int n_maps = att.n_tables, n_classes = att.n_classes;
  if (!w || !h_V_enc || !h_E || !E_idx || !S || !mask || !rank || !log_probs || !counts || !ws)
    return namp_failf(NAMP_EINVAL, !n_maps        ? "namp_decoder_loo: null pointer argument"
                              : att.as_pairs ? "namp_decoder_loo: null pointer argument (pair tables were attached)"
                                             : "namp_decoder_loo: null pointer argument (group tables were attached)");
  if ((((uintptr_t)h_V_enc | (uintptr_t)h_E | (uintptr_t)ws | (uintptr_t)log_probs) & 15u) != 0)
    return namp_failf(NAMP_EINVAL, "namp_decoder_loo: h_V_enc / h_E / log_probs / ws must be 16-byte aligned");
  int prec = PREC_F32;
  int rc = loo_check_weights(w, "namp_decoder_loo", &prec);
  if (rc) return rc;
  if (n_classes && n_classes < w->vocab)
    return namp_failf(NAMP_EINVAL, "namp_decoder_loo: n_classes=%ld of the attached class tables is below vocab=%ld", n_classes, w->vocab);
  if ((rc = loo_dims(B, N, K))) return rc;
  const long G = (long)B * N, R = G * K;
  LooBuffers b = loo_carve(ws, G, K, n_maps, n_classes != 0);
  static_assert(NAMP_LOO_GROUP_MAX <= 16, "loo_prepare_kernel packs a listed position into 4 bits beside a residue index below 2^27");
  if (n_maps && 2 * G >= (1L << LOO_ROW_BITS)) return namp_failf(NAMP_EINVAL, "namp_decoder_loo: 2*B*N=%ld exceeds 2^28 table rows", 2 * G);
  const size_t need = n_classes ? b.cls_bytes : n_maps ? b.group_bytes : b.bytes;
  if (need > ws_bytes && n_classes)                              // (the class section is part of the call's arguments: include/namp.h)
    return namp_failf(NAMP_EINVAL, "namp_decoder_loo: workspace too small for the attached class tables (%ld bytes, %ld needed)", (long)ws_bytes, (long)need);
  if (need > ws_bytes) return namp_failf(NAMP_EWORKSPACE, "namp_decoder_loo: workspace too small (%ld bytes, %ld needed)", (long)ws_bytes, (long)need);
  const hipError_t ready = loo_items_ready();
  if (ready != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(ready));
  hipStream_t s = (hipStream_t)stream;
  const NampDecLayerW *D0 = &w->dec[0], *D1 = &w->dec[1], *D2 = &w->dec[2];

  // ---- index tables (they depend on the graph, the order and the mask only)
  LooPrepArgs pa = {};
  pa.E_idx = E_idx; pa.rank = rank; pa.mask = mask; pa.S = S;
  pa.rev = b.rev; pa.act1 = b.act1; pa.act2 = b.act2; pa.ctr1 = b.ctr1; pa.ctr2 = b.ctr2; pa.cen2 = b.cen2;
  pa.msk1 = b.msk1; pa.S1 = b.S1; pa.msk2 = b.msk2; pa.S2 = b.S2; pa.eo1 = b.eo1; pa.eo2 = b.eo2; pa.eo3 = b.eo3;
  pa.idG = b.idG; pa.ovG = b.ovG; pa.esrc1 = b.esrc1; pa.esrc2 = b.esrc2;
  pa.G = (int)G; pa.N = N; pa.K = K;
  const int32_t *p_first = b.pin + G, *p_map = b.pin + 2 * G, *p_maps = b.pin + 4 * G;
  const float* p_weight = (const float*)(b.pin + 3 * G);
  if (n_maps) {
    hipLaunchKernelGGL(loo_groups_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, b.pin, p_first, mask, b.gl, b.gpos, (int)G, N);
    pa.pp = b.gl; pa.lead = b.gpos; pa.gkey = b.gkey;
    b.Pfw[1] = b.PfwQ[0]; b.Pfw[2] = b.PfwQ[1];                   // (the same rows 0 .. G-1 at another address)
    hipLaunchKernelGGL(loo_prepare_kernel<LOO_TIE_GROUPS>, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, pa);
    hipLaunchKernelGGL(loo_edges_kernel<LOO_TIE_GROUPS>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, pa);
  } else {
    hipLaunchKernelGGL(loo_prepare_kernel<LOO_TIE_NONE>, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, pa);
    hipLaunchKernelGGL(loo_edges_kernel<LOO_TIE_NONE>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, pa);
  }
  hipLaunchKernelGGL(loo_count_kernel, dim3(1), dim3(1024), 0, s, b.act1, b.act2, counts, R);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));

  // ---- base stream (the order of score()): tables of every layer, states and tables behind layers 1 and 2
  NampProj pf[5] = {{D0->W1v_img, nullptr, nullptr, b.Pfw[0]}, {D1->W1v_img, nullptr, nullptr, b.Pfw[1]}, {D2->W1v_img, nullptr, nullptr, b.Pfw[2]},
                    {D0->W1a_img, D0->b1, nullptr, b.Pa1}, {D0->W1v_img, nullptr, D0->tok, b.Pbw1}};
  if ((rc = namp_node_linear(h_V_enc, S, B, B, N, pf, 5, nullptr, stream))) return rc;
  const bool fused = G <= namp_fused_tail_max_residues();
  for (int l = 0; l < 2; ++l) {
    const NampDecLayerW *D = &w->dec[l], *Dn = &w->dec[l + 1];
    const float* hin = l ? b.h1 : h_V_enc;
    float* out = l ? b.h2 : b.h1;
    const float *Pa = l ? b.Pa2 : b.Pa1, *Pbw = l ? b.Pbw2 : b.Pbw1;
    NampProj pn[2] = {{Dn->W1a_img, Dn->b1, nullptr, l ? b.Pa3 : b.Pa2}, {Dn->W1v_img, nullptr, Dn->tok, l ? b.Pbw3 : b.Pbw2}};
    if (fused) {
      if ((rc = namp_dec_message_update(D, h_E, E_idx, rank, Pa, Pbw, b.Pfw[l], hin, mask, out, pn, 2, S, nullptr, nullptr, nullptr, nullptr,
                                        w->vocab, B, B, N, K, stream)))
        return rc;
    } else {
      if ((rc = namp_dec_message(D, h_E, E_idx, rank, Pa, Pbw, b.Pfw[l], b.partial, B, B, N, K, stream))) return rc;
      if ((rc = namp_node_update(D->ln1_g, D->ln1_b, D->Win_img, D->b_in, D->Wout_img, D->b_out, D->ln2_g, D->ln2_b, hin, b.partial,
                                 D->W3_img, D->b3, mask, out, pn, 2, S, (int)G, K, stream)))
        return rc;
    }
  }

  // ---- the cone
  auto items = [&](const NampDecLayerW* D, long rows, const int32_t* act, const int32_t* ctr, const int32_t* cen, const int32_t* esrc,
                   const float* Pa0, const float* Pa1, const float* hV0, const float* hV1, const float* T0, const float* T1,
                   const float* T2) {
    return loo_items(D, prec, h_E, K, rows, act, ctr, cen, esrc, Pa0, Pa1, hV0, hV1, T0, T1, T2);
  };
  // phase 1: layer 1 at the residues that lose i from their decoded neighbours (tables of layer 2 for phase 2 and the own layer 2)
  LooItemArgs a = items(D0, R, b.act1, b.ctr1, b.ctr1, b.esrc1, b.Pa1, b.Pa1, h_V_enc, h_V_enc, b.Pbw1, b.Pfw[0], b.Pbw1);
  loo_tail(a.tail, D0, b.msk1, b.S1, b.h1O);
  loo_proj(a.tail, D1->W1a_img, D1->b1, nullptr, b.Pa2O);
  loo_proj(a.tail, D1->W1v_img, nullptr, D1->tok, b.Pbw2O);
  if ((rc = launch_items(a, prec, s))) return rc;
  // own layer 1 (the encoder states are every stream's layer-1 input: no override)
  a = items(D0, G, nullptr, b.idG, b.idG, b.eo1, b.Pa1, b.Pa1, h_V_enc, h_V_enc, b.Pbw1, b.Pfw[0], b.Pbw1);
  loo_tail(a.tail, D0, mask, S, b.h1o);
  loo_proj(a.tail, D1->W1a_img, D1->b1, nullptr, b.Pa2o);
  if (n_maps) loo_proj(a.tail, D1->W1v_img, nullptr, nullptr, b.PfwQ[0] + G * NAMP_HIDDEN);      // what a member reads for an earlier-listed one, layer 2
  if ((rc = launch_items(a, prec, s))) return rc;
  // phase 2: layer 2 at i's neighbours that a phase-1 output reaches (table of layer 3 for the own layer 3)
  a = items(D1, R, b.act2, b.ctr2, b.cen2, b.esrc2, b.Pa2, b.Pa2O, b.h1, b.h1O, b.Pbw2, b.Pfw[1], b.Pbw2O);
  loo_tail(a.tail, D1, b.msk2, b.S2, b.h2O);
  loo_proj(a.tail, D2->W1v_img, nullptr, D2->tok, b.Pbw3O);
  if ((rc = launch_items(a, prec, s))) return rc;
  // own layers 2 and 3, the output head behind the last
  a = items(D1, G, nullptr, b.idG, b.ovG, b.eo2, b.Pa2, b.Pa2o, b.h1, b.h1o, b.Pbw2, b.Pfw[1], b.Pbw2O);
  loo_tail(a.tail, D1, mask, S, b.h2o);
  loo_proj(a.tail, D2->W1a_img, D2->b1, nullptr, b.Pa3o);
  if (n_maps) loo_proj(a.tail, D2->W1v_img, nullptr, nullptr, b.PfwQ[1] + G * NAMP_HIDDEN);      // ... layer 3
  if ((rc = launch_items(a, prec, s))) return rc;
  a = items(D2, G, nullptr, b.idG, b.ovG, b.eo3, b.Pa3, b.Pa3o, b.h2, b.h2o, b.Pbw3, b.Pfw[2], b.Pbw3O);
  loo_tail(a.tail, D2, mask, S, b.h3o);
  a.tail.head_w = w->Wout_w; a.tail.head_b = w->Wout_b; a.tail.log_probs = log_probs; a.tail.logits = nullptr; a.tail.vocab = w->vocab;
  if ((rc = launch_items(a, prec, s)) || !n_maps) return rc;
  // every member's row -> the group's conditional, through the token maps; pair classes: through the class tables, with the class
  // rows into the output section
  const float* p_bias = (const float*)(p_maps + (size_t)64 * n_maps);
  if (n_classes)
    hipLaunchKernelGGL(loo_class_combine_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, s, log_probs, b.gl, b.pin, p_map, p_weight,
                       p_maps, p_bias, b.cls, n_maps, n_classes, (int)w->vocab, (int)G, N);
  else
    hipLaunchKernelGGL(loo_group_combine_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, s, log_probs, b.gl, b.pin, p_map, p_weight,
                       p_maps, n_maps, (int)w->vocab, (int)G, N);
  e = hipGetLastError();
  if (e != hipSuccess) return namp_internal_fail(NAMP_ELAUNCH, hipGetErrorString(e));
  return NAMP_OK;
}

}  // extern "C"
