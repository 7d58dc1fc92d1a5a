"""Reference of context states (ProteinMPNN.sample / score_tied with feature_dict["state_S"] / ["state_mask"] beside "state_weights":
per-state fixed tokens and per-state presence) built from the unchanged CPU oracle.  Per state m: cpu_ref.encode on the
state's own X and presence mask, cpu_ref.decode_parallel teacher-forced with the state's FULL token row (the design's tokens at
designable positions, state_S[m] elsewhere) under backward_mask(the one shared decoding order, E_idx_m), log_softmax.  Recombined in fp64:

    p_i = softmax((sum over the states m in which i is present of w_m log_probs_m[i] + bias_i) / T), special tokens removed, renormalised

(log_softmax differs from the logits by one constant per row, which the softmax drops)."""
import functools

import numpy as np
import torch

from na_mpnn_amd import synth
from oracle import cpu_ref
from tied_states_ref import make_states, state_fd, states_fd


def contexts_fd(cx, Xs, weights, bs, T, randn, state_S=None, state_mask=None, bias=None, sym=None):
    """tied_states_ref.states_fd plus the context keys.  state_S int [M, L]; state_mask {0, 1} [M, L]: the atoms of an absent residue
    are taken out of that state (X and X_m zero, as pdbio.parse_states(contexts=True) leaves them) and `mask` becomes the OR."""
    fd = states_fd(cx, Xs, weights, bs, T, randn, bias=bias, sym=sym)
    if state_S is not None:
        fd["state_S"] = torch.as_tensor(np.ascontiguousarray(state_S)).long()
    if state_mask is not None:
        sm = torch.as_tensor(np.ascontiguousarray(state_mask)).to(fd["mask"].dtype)
        fd["state_mask"] = sm
        fd["X"] = fd["X"] * sm[:, :, None, None].to(fd["X"].dtype)
        fd["X_m"] = fd["X_m"] * sm[:, :, None].to(fd["X_m"].dtype)
        fd["mask"] = (sm != 0).any(0, keepdim=True).to(fd["mask"].dtype)
    return fd


def contexts_of(fd):
    """(state_S int64 [M, L], state_mask [M, L]) with the defaults of the call: the shared row repeated."""
    M, L = fd["X"].shape[:2]
    sS = fd["state_S"].long() if fd.get("state_S") is not None else fd["S"].long().expand(M, L)
    sm = fd["state_mask"] if fd.get("state_mask") is not None else fd["mask"].expand(M, L)
    return sS, sm


def token_rows(fd, S):
    """S [n, L] -> the token every state's copy holds [n, M, L]: the design's token where mask * chain_mask != 0, state_S[m] elsewhere."""
    sS, _ = contexts_of(fd)
    cm = (fd["mask"] * fd["chain_mask"])[0] != 0
    return torch.where(cm[None, None, :], torch.as_tensor(S).long()[:, None, :], sS[None])


def context_state_fd(fd, m):
    """The feature_dict of state m alone: its coordinates, its presence as the mask, its tokens."""
    sS, sm = contexts_of(fd)
    out = state_fd(fd, m)
    out["mask"], out["S"] = sm[m:m + 1].to(fd["mask"].dtype), sS[m:m + 1].to(fd["S"].dtype)
    return out


def oracle_state_log_probs(weights_t, fd, K, S):
    """log_probs [n, M, L, V] of the per-state oracle teacher-forced with S [n, L] (every row of every state is computed: callers
    select) and the shared decoding order [L]."""
    M, L = fd["X"].shape[:2]
    rows = token_rows(fd, S)
    n = rows.shape[0]
    order = cpu_ref.decoding_order_of((fd["mask"] * fd["chain_mask"]), fd["randn"][:1])          # [1, L]
    lps = []
    rep = lambda t: t.repeat(n, *([1] * (t.dim() - 1)))
    for m in range(M):
        fdm = context_state_fd(fd, m)
        h_V, h_E, E_idx = cpu_ref.encode(weights_t, fdm, K)
        m_att = cpu_ref.backward_mask(order, E_idx)
        lp, _ = cpu_ref.decode_parallel(weights_t, rep(h_V), rep(h_E), rep(E_idx), rows[:, m].contiguous(), rep(fdm["mask"]).float(), m_att)
        lps.append(torch.log_softmax(lp.double(), -1))
    return torch.stack(lps, 1), order[0]


def context_probs(log_probs, fd, T=None, bias=None, special=cpu_ref.SPECIAL_TOKENS):
    """log_probs [n, M, L, V] per state -> the distribution every designable position draws from [n, L, V] (fp64; zero where
    mask * chain_mask is zero).  T / bias: other than the feature_dict's (score_tied: T = 1, no bias, special tokens kept)."""
    _, sm = contexts_of(fd)
    w = torch.tensor(fd["state_weights"], dtype=torch.float64)
    present = (sm != 0).double()
    z = (w[None, :, None, None] * present[None, :, :, None] * log_probs.double()).sum(1)       # [n, L, V]
    b = fd["bias"] if bias is None else bias
    z = z + b.double().expand(1, z.shape[1], z.shape[2])
    p = torch.softmax(z / (fd["temperature"] if T is None else T), -1)
    for tok in special:
        p[..., tok] = 0
    p = p / p.sum(-1, keepdim=True)
    cm = ((fd["mask"] * fd["chain_mask"])[0] != 0).double()
    return p * cm[None, :, None]


def oracle_contexts(weights_t, fd, K, S):
    """-> (log_probs [n, M, L, V] fp64, the drawn distribution [n, L, V] fp64, the shared decoding order [L])."""
    lp, order = oracle_state_log_probs(weights_t, fd, K, S)
    return lp, context_probs(lp, fd), order


def oracle_score_tied(weights_t, fd, K, S_lib):
    """score_tied() with contexts from the same oracle: token_log_probs [n, L] (the unit of present copies at T = 1, no bias, special
    tokens kept; where the present copies hold different tokens, only possible at fixed positions, -inf; a residue nowhere present: its
    state-0 own entry is not defined here and left nan), log_likelihood [n] over mask * chain_mask != 0, state_log_likelihood [n, M]."""
    S_lib = torch.as_tensor(S_lib).long()
    lp, _ = oracle_state_log_probs(weights_t, fd, K, S_lib)
    _, sm = contexts_of(fd)
    rows = token_rows(fd, S_lib)                                                   # [n, M, L]
    present = sm != 0
    w = torch.tensor(fd["state_weights"], dtype=torch.float64)
    z = (w[None, :, None, None] * present[None, :, :, None].double() * lp).sum(1)
    unit = torch.log_softmax(z, -1)                                                # [n, L, V]
    cm = (fd["mask"] * fd["chain_mask"])[0] != 0
    tlp = unit.gather(2, S_lib[:, :, None])[:, :, 0]
    own = lp.gather(3, rows[..., None])[..., 0]                                    # [n, M, L]
    counted = cm[None, None, :] & present[None]
    return {"token_log_probs": tlp, "log_likelihood": (tlp * cm[None].double()).sum(-1), "member_log_probs": own,
            "state_log_likelihood": (own * counted.double()).sum(-1)}


def write_models(path, models):
    """A multi-MODEL PDB file; models: per model the arguments of pdbio.write_pdb (X, X_m, resnames, chain_letters, R_idx, icodes)."""
    import os
    from na_mpnn_amd import pdbio
    tmp, body = str(path) + ".state", []
    for m, args in enumerate(models):
        pdbio.write_pdb(tmp, *args)
        body += ["MODEL     %4d" % (m + 1)] + [l for l in open(tmp).read().splitlines() if l != "END"] + ["ENDMDL"]
    os.remove(tmp)
    with open(path, "w") as fh:
        fh.write("\n".join(body + ["END"]) + "\n")


def model_of(cx, resnames, letters, rows=None, rename=None):
    """The write_pdb arguments of one model: the residues `rows` (all) of the complex `cx` (arrays per residue), residue names
    `resnames`, chain ids `letters`; rename: {row: residue name}."""
    rows = np.arange(len(resnames)) if rows is None else np.asarray(rows)
    names = [dict(rename or {}).get(int(i), resnames[int(i)]) for i in rows]
    return (cx["X"][rows], cx["X_m"][rows], names, [letters[int(i)] for i in rows], cx["R_idx"][rows], [""] * len(rows))


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------------------------------

def other_tokens(S, rows, rng):
    """Other protein tokens at `rows`: each differs from S there."""
    out = S.copy()
    out[rows] = (S[rows] + 1 + rng.integers(0, 19, len(rows))) % 20
    assert (out[rows] != S[rows]).all()
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (cx, CPU feature_dict, K).  Synthetic complexes with every residue resolved; the fixed residues are one block at the end (the
    partner); sum |w| / T <= 4 keeps the sampler's 1e-3 bar valid for the weighted sum (test_gpu_tied_states.case_fd)."""
    if name in ("tokens", "tokens_deformed", "tokens_equal_rows", "unbound"):
        L, K, M, bs = 60, 24, 2, 2
        T, w = (1.0, (1.0, -1.0)) if name == "unbound" else (0.5, (1.0, -0.5))
        fixed = np.arange(40, 60)
    elif name == "LltK":
        L, K, M, bs, T, w = 30, 48, 3, 3, 0.5, (0.6, 0.3, 0.1)
        fixed = np.arange(20, 30)
    else:
        raise KeyError(name)
    assert np.abs(w).sum() / T <= 4.0
    cx = synth.make_complex(seed=2100 + L, n=L)
    cx["mask"][:] = 1
    cx["chain_mask"][:] = 1
    cx["chain_mask"][fixed] = 0
    rng = np.random.default_rng(L + M)
    randn = rng.standard_normal((bs, L)).astype(np.float32)                    # (first: the cases of one shape share it)
    Xs = make_states(cx, M, seed=L + 7 * M)
    if name in ("tokens", "tokens_equal_rows"):
        Xs = np.stack([cx["X"].astype(np.float32)] * M)                        # the states share the backbone: they differ in tokens alone
    sS, sm = np.tile(cx["S"], (M, 1)), np.ones((M, L), np.int32)
    if name in ("tokens", "tokens_deformed"):
        sS[1] = other_tokens(cx["S"], fixed, rng)
    elif name == "unbound":
        sm[1, fixed] = 0
    elif name == "LltK":
        # everything present | the partner absent | the partner present with other tokens; designable residue 3 is absent in state 0
        # and 11 in the last state: the first and the closing member of a group absent
        sm[1, fixed] = 0
        sS[2] = other_tokens(cx["S"], fixed, rng)
        sm[0, 3] = 0
        sm[2, 11] = 0
    fd = contexts_fd(cx, Xs, w, bs, T, randn, state_S=sS, state_mask=sm)
    return cx, fd, K
