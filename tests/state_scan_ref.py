"""CPU reference of the specificity scan (ProteinMPNN.score_mutations with feature_dict["state_weights"]) and the cases
of its tests.  The reference is context_states_ref.oracle_score_tied, unchanged, on the explicit sequences of the variants with S itself
as the last row:

    delta[v] = log_likelihood[v] - log_likelihood[S],   state_delta[v, m] = state_log_likelihood[v, m] - state_log_likelihood[S, m]

mistaken_fd gives the same reference one of two mistakes — absent copies counted as present, the state weights dropped — so that the
host tests can show that the cases tell them apart.  Helper module (not a test)."""
import functools

import numpy as np
import torch

from na_mpnn_amd import synth
from oracle import cpu_ref
import context_states_ref as CR
import mutation_ref as MR
from tied_states_ref import make_states, states_fd

CASES = ("tokens_deformed", "unbound", "LltK", "plain", "cap8", "two_residue_sites", "single")


@functools.lru_cache(maxsize=None)
def weights_t():
    return cpu_ref.to_torch(synth.make_weights(0))


def _plain(L, K, w, seed):
    """Backbone states without contexts: every residue present everywhere, one block of fixed residues at the end."""
    M = len(w)
    cx = synth.make_complex(seed=seed, n=L)
    cx["mask"][:] = 1
    cx["chain_mask"][:] = 1
    cx["chain_mask"][L - L // 4:] = 0
    randn = np.random.default_rng(seed + 1).standard_normal((1, L)).astype(np.float32)
    Xs = make_states(cx, M, seed=seed + 2)
    return cx, states_fd(cx, Xs, w, 1, 1.0, randn), K


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (cx, CPU feature_dict, K, sites int64 [n_sites, s], site_tokens int64 [n, 1 + s]) over SHARED residues.  Per site three
    random tokens of the residue's alphabet and, for the first and the last site, the wild type."""
    if name in ("tokens_deformed", "unbound", "LltK"):
        cx, fd, K = CR.case(name)
    elif name == "plain":
        cx, fd, K = _plain(40, 16, (1.0, -0.5), 4016)
    elif name == "cap8":
        cx, fd, K = _plain(12, 8, (0.5, -0.5, 0.5, -0.5, 0.5, -0.5, 0.5, -0.5), 1208)
    elif name == "two_residue_sites":
        cx, fd, K = _plain(20, 16, (1.0, -0.5, 0.75, -0.25), 2016)
    elif name == "single":
        cx, fd, K = _plain(40, 16, (1.0,), 4016)
    else:
        raise KeyError(name)
    L = len(cx["S"])
    order = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"][:1])[0].tolist()
    cm = ((fd["mask"] * fd["chain_mask"])[0] != 0).tolist()
    designed = [i for i in order if cm[i]]
    if name == "two_residue_sites":
        groups = [[designed[0], designed[1]], [designed[len(designed) // 2], designed[-1]], [designed[2], designed[-2]]]
    else:
        picks = [designed[0], designed[1], designed[len(designed) // 2], designed[-1]]
        if name == "LltK":
            picks += [3, 11, 4]                                     # the designable residues absent in a state, and a neighbour
        groups = [[p] for p in dict.fromkeys(picks)]
    s = max(len(g) for g in groups)
    sites = np.full((len(groups), s), -1, np.int64)
    for q, g in enumerate(groups):
        sites[q, :len(g)] = g
    rng = np.random.default_rng(len(name) + L)
    rows = []
    for q, g in enumerate(groups):
        for _ in range(3):
            rows.append([q] + [int(rng.choice(list(MR.alphabet(cx, r)))) for r in g] + [0] * (s - len(g)))
    for q in (0, len(groups) - 1):
        rows.append([q] + [int(cx["S"][r]) for r in groups[q]] + [0] * (s - len(groups[q])))
    return cx, fd, K, sites, np.array(rows, np.int64)


def sequences(fd, sites, site_tokens):
    """The explicit sequences of the variants and S itself as the last row, int64 [n + 1, L]."""
    S = fd["S"][0].numpy()
    return torch.from_numpy(np.concatenate((MR.expand(S, sites, site_tokens).reshape(-1, len(S)), S[None].astype(np.int64))))


def reference(fd, K, sites, site_tokens):
    """oracle_score_tied on sequences() -> {"delta" [n], "state_delta" [n, M], "units" [n + 1, L] (the last row: S), "own" [n + 1, M, L],
    "log_probs" [n + 1, M, L, V] the per-state oracle rows}, fp64."""
    S_all = sequences(fd, sites, site_tokens)
    got = CR.oracle_score_tied(weights_t(), fd, K, S_all)
    lp, _ = CR.oracle_state_log_probs(weights_t(), fd, K, S_all)
    ll, sl = got["log_likelihood"], got["state_log_likelihood"]
    return {"delta": ll[:-1] - ll[-1], "state_delta": sl[:-1] - sl[-1:], "units": got["token_log_probs"], "own": got["member_log_probs"],
            "log_probs": lp}


def mistaken_fd(fd, mistake):
    """The feature_dict of a reference that makes one mistake: "absent_as_present" — every copy counts as present (state_mask all ones;
    the absent copies keep their zeroed atoms) —, "drop_weights" — every state weighs 1.  None where the case leaves nothing to get wrong."""
    if mistake == "absent_as_present":
        if fd.get("state_mask") is None or not bool((fd["state_mask"] == 0).any()):
            return None
        return dict(fd, state_mask=torch.ones_like(fd["state_mask"]))
    if mistake == "drop_weights":
        if all(float(v) == 1.0 for v in fd["state_weights"]):
            return None
        return dict(fd, state_weights=[1.0] * len(fd["state_weights"]))
    raise KeyError(mistake)


def flat_rows(fd, K, sites):
    """The per-site lists U_3 on the FLAT graph from the oracle's per-state neighbour lists: site_rows int64 [n_sites, 3] and, per site,
    the ascending flat residues of U_3.  A copy that is absent in its state is never active (mask 0) but is in the site."""
    M, L = fd["X"].shape[:2]
    _, sm = CR.contexts_of(fd)
    order = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"][:1])[0].numpy()
    rank = np.empty(L, np.int64)
    rank[order] = np.arange(L)
    E = np.concatenate([cpu_ref.encode(weights_t(), CR.context_state_fd(fd, m), K)[2][0].numpy() + m * L for m in range(M)])
    flat_sites = [[m * L + int(r) for r in row if r >= 0 for m in range(M)] for row in np.asarray(sites)]
    width = max(len(s) for s in flat_sites)
    st = np.full((len(flat_sites), width), -1, np.int64)
    for q, s in enumerate(flat_sites):
        st[q, :len(s)] = s
    return MR.site_rows(E, np.tile(rank, M), (sm != 0).numpy().astype(np.int64).reshape(-1), st)
