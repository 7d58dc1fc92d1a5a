"""numpy restatement of the active phase-1 / phase-2 grids of the leave-one-out cone WITH PAIRS (na_mpnn_amd/csrc/namp_loo.h:
loo_pairs_kernel / loo_prepare_kernel / loo_edges_kernel), and a brute force of the same grids from the oracle's layer outputs, for
one complex.  Helper module of test_pair_conditional_host.py / test_gpu_pair_conditional.py (not a test)."""
import numpy as np


def pair_tables(L, pairs, mask, first=None):
    """The validated partner table of loo_pairs_kernel: partner [L] (-1: unpaired) and the listed-first flag [L], a pair with a masked
    member left out.  pairs: [(i, j)] in listed order."""
    partner, lead = np.full(L, -1, np.int64), np.zeros(L, bool)
    for i, j in pairs:
        if mask[i] and mask[j]:
            partner[i], partner[j], lead[i] = j, i, True
    return partner, lead


def pair_loo_grids(E_idx, rank, mask, partner, lead):
    """E_idx [L, K], rank [L], mask [L], partner / lead [L] -> act1 [L, K] (layer-1 item (m, k), n = E_idx[m, k]: m used to see n as
    decoded and is not n's partner; the item belongs to the stream of n's pair), act2 [L, K] (layer-2 item (g, kq), q = E_idx[g, kq]
    outside g's pair: q itself or one of its decoded neighbours has a layer-1 override in the stream of g's pair, through either
    member).  Without pairs these are loo_numpy.loo_grids' act1 / act2."""
    E_idx = np.asarray(E_idx, np.int64); rank = np.asarray(rank, np.int64); mask = np.asarray(mask)
    L, K = E_idx.shape
    ar = np.arange(L)
    sid = np.where((partner >= 0) & ~lead, partner, ar)                      # the stream of a residue: the listed-first member of its pair
    act1 = (E_idx != ar[:, None]) & (partner[E_idx] != ar[:, None]) & (rank[E_idx] < rank[:, None]) & (mask[:, None] != 0)
    has_ov = np.zeros((L, L), bool)                                          # [stream, m]: m has a layer-1 override in that stream
    mm, kk = np.nonzero(act1)
    has_ov[sid[E_idx[mm, kk]], mm] = True
    q = E_idx                                                                # [g, kq]
    s = sid[:, None]
    pg = partner[:, None]
    cen_ov = has_ov[s, q]
    nb = E_idx[q]                                                            # [g, kq, k']: neighbours of q
    bw = (nb != ar[:, None, None]) & (nb != pg[:, :, None]) & (rank[nb] < rank[q][..., None])
    ov = bw & has_ov[s[:, :, None], nb]
    act2 = (q != ar[:, None]) & (q != pg) & (mask[q] != 0) & (cen_ov | ov.any(-1))
    return act1, act2


def layer_states(w, h_V, h_E, E_idx, S, mask, order):
    """The parallel decoder of oracle.cpu_ref.decode_parallel (model_utils.py:406-421), the same calls in the same order, returning the
    state behind every decoder layer instead of the log-probs: [h_1, h_2, ...], each [B, L, H]."""
    import torch.nn.functional as F
    from oracle import cpu_ref as R
    m_att = R.backward_mask(order, E_idx)
    mask_1D = mask.view([mask.size(0), mask.size(1), 1, 1])
    mask_bw, mask_fw = mask_1D * m_att, mask_1D * (1. - m_att)
    h_S = F.embedding(S, w["W_s.weight"])
    h_ES = R.cat_neighbors_nodes(h_S, h_E, E_idx)
    h_EX_enc = R.cat_neighbors_nodes(h_S * 0, h_E, E_idx)
    fw = mask_fw * R.cat_neighbors_nodes(h_V, h_EX_enc, E_idx)
    out = []
    for l in range(R.n_layers(w, "decoder")):
        h_ESV = mask_bw * R.cat_neighbors_nodes(h_V, h_ES, E_idx) + fw
        h_V = R.dec_layer(w, f"decoder_layers.{l}.", h_V, h_ESV, mask)
        out.append(h_V)
    return out


def brute_force_cone(w64, enc64, S, mask, order0, members, tol=1e-10):
    """The residues outside `members` (one residue, or a pair (i, j) in listed order) whose layer-1 / layer-2 output in the stream
    that decodes `members` last differs from the base stream's by more than tol (fp64): (set1, set2)."""
    import torch
    h_V, h_E, E_idx = enc64
    keep = torch.ones_like(order0, dtype=torch.bool)
    for g in members:
        keep &= order0 != g
    order = torch.cat((order0[keep], order0.new_tensor(list(members))))
    base = layer_states(w64, h_V, h_E, E_idx, S.long(), mask, order0[None])
    strm = layer_states(w64, h_V, h_E, E_idx, S.long(), mask, order[None])
    sets = []
    for l in range(2):
        d = (base[l][0] - strm[l][0]).abs().amax(-1)
        sets.append({int(m) for m in torch.nonzero(d > tol)[:, 0].tolist() if m not in members})
    return sets
