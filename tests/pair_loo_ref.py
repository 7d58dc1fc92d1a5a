"""Reference of the pair conditionals (ProteinMPNN.conditional_probs with feature_dict["paired_residues"]) built from the unchanged
CPU oracle: the PAIR STREAM — oracle.cpu_ref.decode_parallel run with score()'s decoding order from which the pair's residues i, j
are taken out and appended as ..., i, j, the true S teacher-forced, the token embedding of i HIDDEN (a zero row of h_S: an extra all-zero
row appended to W_s and S[i] pointing at it, so decode_parallel itself stays as it is) — and the combine

    total[a] = w_i z_i[P_i[a]] + w_j z_j[P_j[a]],   lp = log_softmax(total),   row_m[P_m[a]] = lp[a]   for m in (i, j)

in fp64.  Helper module of test_pair_conditional_host.py / test_gpu_pair_conditional.py (not a test)."""
import numpy as np
import torch

from na_mpnn_amd.model import mapped_groups
from oracle import cpu_ref
from loo_numpy import oracle_conditional


def pair_specs(fd, rti):
    """The pairs of a CPU feature_dict as conditional_probs() ties them: [(i, j, w_i, w_j, P_i, P_j)] in LISTED order (fixed=None:
    chain_mask does not reorder members), the pairs with a masked member left out."""
    L = fd["S"].shape[1]
    polymer = [1 if d else (2 if r else 0) for d, r in zip(fd["dna_mask"][0].tolist(), fd["rna_mask"][0].tolist())]
    mask = fd["mask"][0].tolist()
    for i, j in fd["paired_residues"]:                       # (a masked residue without a polymer flag: its partner's stands in)
        for r, q in ((i, j), (j, i)):
            if not mask[r] and polymer[r] == 0 and not fd["protein_mask"][0][r]:
                polymer[r] = polymer[q]
    g, w, m, _ = mapped_groups(L, rti, fd["paired_residues"], fd.get("paired_weights"), polymer, None)
    return [(gi[0], gi[1], wi[0], wi[1], mi[0], mi[1]) for gi, wi, mi in zip(g, w, m) if mask[gi[0]] and mask[gi[1]]]


def pair_stream_logits(w, enc, S, mask, order0, pairs, hide=True, chunk=16):
    """Logits of both members of every pair (i, j) in its pair stream -> [n, 2, vocab].  enc = (h_V, h_E, E_idx) of ONE complex
    (batch dimension 1), order0 [L] the order of score(); hide=False leaves i's token visible to j (what a build that forgets to hide
    it computes)."""
    h_V, h_E, E_idx = enc
    V = w["W_s.weight"].shape[0]
    w2 = dict(w)
    w2["W_s.weight"] = torch.cat((w["W_s.weight"], torch.zeros(1, w["W_s.weight"].shape[1], dtype=w["W_s.weight"].dtype)))
    out = []
    for p0 in range(0, len(pairs), chunk):
        part = pairs[p0:p0 + chunk]
        n = len(part)
        orders = torch.stack([torch.cat((order0[(order0 != i) & (order0 != j)], order0.new_tensor([i, j]))) for i, j in part])
        Sn = S.long().expand(n, -1).clone()
        if hide:
            for t, (i, _) in enumerate(part):
                Sn[t, i] = V
        rep = lambda t: t.expand(n, *t.shape[1:])
        E_rep = rep(E_idx).contiguous()
        _, logits = cpu_ref.decode_parallel(w2, rep(h_V), rep(h_E), E_rep, Sn, rep(mask), cpu_ref.backward_mask(orders, E_rep))
        for t, (i, j) in enumerate(part):
            out.append(torch.stack((logits[t, i], logits[t, j])))
    return torch.stack(out) if out else torch.zeros(0, 2, V)


def combine(z_i, z_j, w_i, w_j, P_i, P_j):
    """The pair's conditional from the two members' rows (logits, or log-softmax rows: one constant per member cancels), in fp64 ->
    (row_i, row_j), each in its member's alphabet."""
    P_i, P_j = torch.as_tensor(P_i), torch.as_tensor(P_j)
    total = float(w_i) * z_i.double()[P_i] + float(w_j) * z_j.double()[P_j]
    lp = torch.log_softmax(total, -1)
    row_i, row_j = torch.empty_like(lp), torch.empty_like(lp)
    row_i[P_i] = lp
    row_j[P_j] = lp
    return row_i, row_j


def oracle_pair_conditional(w, fd, top_k, rti):
    """conditional_probs() with pairs on the CPU oracle -> (log_probs [1, L, vocab] with the pair rows on the tied residues and the
    leave-one-out rows everywhere else, the same without pairs, the base order [1, L], E_idx, the tied specs)."""
    loo, order, E_idx = oracle_conditional(w, fd, top_k)
    specs = pair_specs(fd, rti)
    enc = cpu_ref.encode(w, fd, top_k)
    z = pair_stream_logits(w, enc, fd["S"], fd["mask"], order[0], [(s[0], s[1]) for s in specs])
    out = loo.clone()
    for (i, j, wi, wj, Pi, Pj), zz in zip(specs, z):
        ri, rj = combine(zz[0], zz[1], wi, wj, Pi, Pj)
        out[0, i], out[0, j] = ri.float(), rj.float()
    return out, loo, order, E_idx, specs


def neighbour_kinds(E_idx, pairs):
    """Per pair (i in N(j), j in N(i)) on E_idx [L, K]."""
    E = np.asarray(E_idx)
    return [(bool((E[j] == i).any()), bool((E[i] == j).any())) for i, j in pairs]
