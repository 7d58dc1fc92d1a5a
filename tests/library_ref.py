"""numpy restatement of the active-row sets of library scoring (ProteinMPNN.score_sequences, na_mpnn_amd/csrc/namp_library.h) and the
CPU oracle of the call: one encode, then score() per sequence, reduced to the token entries.  Helper module of
test_score_library_host.py / test_gpu_score_library*.py (not a test)."""
import numpy as np


def active_sets(E_idx, rank, mask, positions):
    """E_idx [L, K], rank [L], mask [L], positions (library positions) -> var [L] bool and [act_1, act_2, act_3] ([L] bool each):
    act_0 = 0, act_l[i] = mask[i] and (act_{l-1}[i] or exists k: rank[E_idx[i, k]] < rank[i] and (var or act_{l-1})[E_idx[i, k]]) —
    model_utils.py:391-421: row i reads the token and the previous layer's state of its BACKWARD neighbours and its own previous
    state; the neighbour's own mask is not consulted (the reference multiplies by the centre's mask only)."""
    E_idx = np.asarray(E_idx, np.int64); rank = np.asarray(rank, np.int64); mask = np.asarray(mask) != 0
    L = E_idx.shape[0]
    var = np.zeros(L, bool)
    var[np.asarray(positions, np.int64)] = True
    bw = rank[E_idx] < rank[:, None]                                          # [L, K]
    acts, prev = [], np.zeros(L, bool)
    for _ in range(3):
        prev = mask & (prev | (bw & (var | prev)[E_idx]).any(-1))
        acts.append(prev)
    return var, acts


def active_counts(E_idx, rank, mask, positions):
    return [int(a.sum()) for a in active_sets(E_idx, rank, mask, positions)[1]]


def full_sequences(S, positions, tokens):
    """S [L], positions [n_var], tokens [n, n_var] -> the full sequences [n, L] (numpy int64)."""
    out = np.repeat(np.asarray(S, np.int64)[None], len(tokens), 0)
    if len(positions):
        out[:, np.asarray(positions, np.int64)] = np.asarray(tokens, np.int64)
    return out


def random_library(rng, S, positions, n, protein, dna, rna):
    """n random sequences that differ from S at `positions` only, every residue inside its polymer's alphabet (synth.make_complex's
    ranges); tokens [n, n_var]."""
    positions = np.asarray(positions, np.int64)
    lo = np.where(protein[positions] != 0, 0, np.where(dna[positions] != 0, 21, 26))
    hi = np.where(protein[positions] != 0, 20, np.where(dna[positions] != 0, 25, 30))
    return rng.integers(lo[None], hi[None], (n, len(positions))).astype(np.int64)


_encoded = {}


def encoded(w, fd, top_k, key=None):
    """cpu_ref.encode of a CPU feature_dict, computed once per `key` and left unchanged."""
    from oracle import cpu_ref as R
    if key is None or key not in _encoded:
        val = R.encode(w, fd, top_k)
        if key is None:
            return val
        _encoded[key] = val
    return _encoded[key]


def oracle_library(w, fd, top_k, S_full, key=None):
    """The oracle of score_sequences: ONE cpu_ref.encode, then cpu_ref.score_from_encoded per sequence (feature_dict["S"] replaced,
    batch_size 1), reduced to the token's own entry.  -> token_log_probs [n, L] float32, decoding order [L], E_idx [L, K]."""
    import torch
    from oracle import cpu_ref as R
    h_V, h_E, E_idx = encoded(w, fd, top_k, key)
    rows, order = [], None
    for S_k in torch.as_tensor(np.asarray(S_full)).long():
        out = R.score_from_encoded(w, h_V, h_E, E_idx, S_k[None], fd["mask"], fd["chain_mask"], fd["randn"], 1)
        rows.append(out["log_probs"][0].gather(1, S_k[:, None])[:, 0])
        order = out["decoding_order"]
    return torch.stack(rows).float(), order, E_idx[0]


def oracle_decoder_states(w, fd, top_k, S_k, key=None):
    """The decoder states behind layers 1..3 of score() with feature_dict["S"] replaced by S_k: [3][L, 128] (decode_parallel of the
    oracle, layer by layer)."""
    import torch
    import torch.nn.functional as F
    from oracle import cpu_ref as R
    h_V, h_E, E_idx = encoded(w, fd, top_k, key)
    mask = fd["mask"]
    order = R.decoding_order_of(mask * fd["chain_mask"], fd["randn"])
    m_att = R.backward_mask(order, E_idx)
    mask_1D = mask.view([mask.size(0), mask.size(1), 1, 1])
    mask_bw, mask_fw = mask_1D * m_att, mask_1D * (1. - m_att)
    h_S = F.embedding(torch.as_tensor(np.asarray(S_k)).long()[None], w["W_s.weight"])
    h_ES = R.cat_neighbors_nodes(h_S, h_E, E_idx)
    h_EX = R.cat_neighbors_nodes(torch.zeros_like(h_S), h_E, E_idx)
    fw = mask_fw * R.cat_neighbors_nodes(h_V, h_EX, E_idx)
    states = []
    for i in range(R.n_layers(w, "decoder")):
        h_ESV = mask_bw * R.cat_neighbors_nodes(h_V, h_ES, E_idx) + fw
        h_V = R.dec_layer(w, f"decoder_layers.{i}.", h_V, h_ESV, mask)
        states.append(h_V[0])
    return states


def ranks_of(order):
    order = np.asarray(order, np.int64)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return rank


def make_case(name):
    """The cases of the library tests -> (k_neighbors, complex with its chain_mask / randn set, positions, tokens [n, n_var]).
    n97: the nucleic acid of a 97-residue complex designed, 12 random sequences and the native one (13: no multiple of the 16-row tile);
    crossing: the same with one designed residue decoded before the fixed ones (fixed rows become active); LltK: L < K;
    all: every residue designed (act_3 is nearly every row)."""
    from na_mpnn_amd import synth
    if name in ("n97", "crossing"):
        k, cx = 32, synth.make_complex(seed=497, n=97, missing_atom_frac=0.05, masked_frac=0.04)
    elif name == "LltK":
        k, cx = 48, synth.make_complex(seed=432, n=32)
    elif name == "all":
        k, cx = 32, synth.make_complex(seed=460, n=60)
    else:
        raise KeyError(name)
    na = (cx["dna_mask"] | cx["rna_mask"]) != 0
    cx["chain_mask"] = np.ones_like(cx["chain_mask"]) if name == "all" else na.astype(np.int32)
    if name == "crossing":
        first = int(np.nonzero(na & (cx["mask"] != 0))[0][0])
        cx["randn"] = cx["randn"].copy()
        cx["randn"][first] = 1e-7
    positions = np.nonzero((cx["mask"] * cx["chain_mask"]) != 0)[0]
    rng = np.random.default_rng(1234)
    n = {"n97": 12, "crossing": 6, "LltK": 5, "all": 4}[name]
    tokens = random_library(rng, cx["S"], positions, n, cx["protein_mask"], cx["dna_mask"], cx["rna_mask"])
    tokens = np.concatenate((tokens, cx["S"][positions][None].astype(np.int64)))          # the native sequence last
    return k, cx, positions, tokens
