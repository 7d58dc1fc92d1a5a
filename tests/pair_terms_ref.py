"""Reference of the compact pair terms (ProteinMPNN.sample with feature_dict["pair_terms"]) on top of the references of the ties: the
terms are computed in float64 from the FINAL sequence and the decoding order,

    term(i)[a] = sum over the slots d of i, sorted by partner, of tables[table[i][d]][a][tok(partner[i][d])]

— tok(j) the token of j if j's group was drawn before the group of i was reached, else PAD —, and enter the existing recombinations
(paired_ref.paired_probs, wobble_ref.class_probs, tied_states_ref.tied_probs) where the bias enters them: a group's addend

    add[a] = sum over the counted members m ("closing": the last listed one; "all": every member, in listed order) of term(m)[P_m[a]]

is folded into the bias row of the group's closing member (token maps: bias_c[P_c[a]] += add[a]) or into the group's class biases (class
tables, where several classes may share the closing member's token).  The terms depend on the sample, so the recombination runs once
per sample.  Log-probs come from the unchanged oracles (paired_ref.oracle_paired, wobble_ref.oracle_wobble, tied_states_ref)."""
import torch

from na_mpnn_amd import spec
import paired_ref
import tied_states_ref
import wobble_ref

V = len(spec.RESTYPES)
PAD = V - 1


def slots_of(pt, b, i, L):
    """The slots of residue i as the kernels sum them: (partner, table) sorted by partner, stable; absent slots dropped; tables clamped."""
    n_tab = len(pt["tables"])
    raw = [(int(j), int(k)) for j, k in zip(pt["partner"][b, i].tolist(), pt["table"][b, i].tolist())]
    keep = [(j, max(0, min(n_tab - 1, k))) for j, k in raw if 0 <= j < L and j != i]
    return sorted(keep, key=lambda s: s[0])


def steps_of(order0, groups, L):
    """The step at which every residue's group is reached: a group is emitted when the decoding order reaches its first member."""
    pos = [0] * L
    for t, r in enumerate(order0):
        pos[int(r)] = t
    step = list(pos)
    for g in groups:
        s = min(pos[r] for r in g)
        for r in g:
            step[r] = s
    return step


def term(pt, i, S_row, step, L, b=0):
    """term(i) [V] in float64 under the final sequence S_row."""
    tables = torch.as_tensor(pt["tables"]).double()
    out = torch.zeros(V, dtype=torch.float64)
    for j, k in slots_of(pt, b, i, L):
        tok = int(S_row[j]) if step[j] < step[i] else PAD
        out = out + tables[k][:, tok]
    return out


def group_add(pt, g, alphabets, S_row, step, L, lanes):
    """add [lanes] of group g: alphabets[m][a] the token of member m under group token / class a (negative: none, read as token 0)."""
    counted = list(g) if pt.get("members", "closing") == "all" else [g[-1]]
    add = torch.zeros(lanes, dtype=torch.float64)
    for m, P in zip(g, alphabets):
        if m in counted:
            add = add + term(pt, m, S_row, step, L)[torch.tensor(P[:lanes]).clamp(min=0)]
    return add


def _bias_with_terms(fd, pt, groups, alphabets, S_row, order0, fold_groups):
    """fd["bias"] [1, L, V] in float64 with the terms of every untied residue added, and — fold_groups — every group's addend on its
    closing member's row through that member's map; -> (bias, the groups' addends)."""
    L = fd["S"].shape[1]
    step = steps_of(order0, groups, L)
    bias = fd["bias"].double().expand(1, L, V).clone()
    tied = {i for g in groups for i in g}
    for i in range(L):
        if i not in tied:
            bias[0, i] += term(pt, i, S_row, step, L)
    adds = []
    for g, al in zip(groups, alphabets):
        lanes = len(al[-1])
        adds.append(group_add(pt, g, al, S_row, step, L, lanes))
        if fold_groups:
            extra = torch.zeros(V, dtype=torch.float64)
            extra[torch.tensor(al[-1])] = adds[-1]                            # bias_c[P_c[a]] += add[a]: P_c is a permutation
            bias[0, g[-1]] += extra
    return bias, adds


def plain_probs(log_probs, fd, pt, S, order, groups=None, group_weights=None, state_weights=None):
    """Untied residues, symmetry groups (identity maps) and states: log_probs [bs, L, V] or [bs, M, L, V] -> probabilities [bs, L, V]."""
    groups = [list(g) for g in (groups or []) if len(g)]
    weights = [list(w) for w in (group_weights or [])][:len(groups)]
    maps = [[list(range(V))] * len(g) for g in groups]
    out = []
    for b in range(S.shape[0]):
        bias, _ = _bias_with_terms(fd, pt, groups, maps, S[b].tolist(), order[b].tolist(), True)
        out.append(paired_ref.paired_probs(log_probs[b:b + 1], dict(fd, bias=bias), groups, weights, maps, state_weights=state_weights))
    return torch.cat(out)


def paired_probs(lp_groups, fd, pt, S, order, groups, weights, maps, state_weights=None):
    """paired_ref.paired_probs with the pair terms: lp_groups as oracle_paired returns them (the rows of fixed members kept)."""
    out = []
    for b in range(S.shape[0]):
        bias, _ = _bias_with_terms(fd, pt, groups, maps, S[b].tolist(), order[b].tolist(), True)
        out.append(paired_ref.paired_probs(lp_groups[b:b + 1], dict(fd, bias=bias), groups, weights, maps, state_weights=state_weights))
    return torch.cat(out)


def class_probs(lp_groups, fd, pt, S, order, groups, weights, tables, class_bias, state_weights=None):
    """wobble_ref.class_probs' rows with the pair terms: a group's addend joins its class biases."""
    rows = []
    for b in range(S.shape[0]):
        bias, adds = _bias_with_terms(fd, pt, groups, tables, S[b].tolist(), order[b].tolist(), False)
        cb = [(torch.tensor(c, dtype=torch.float64) + a).tolist() for c, a in zip(class_bias, adds)]
        rows.append(wobble_ref.class_probs(lp_groups[b:b + 1], dict(fd, bias=bias), groups, weights, tables, cb,
                                           state_weights=state_weights)[0])
    return torch.cat(rows).float()


def neighbour_terms(L, AA, members="closing", chain_of=None):
    """Residue i reads i - 1 through AA.t() and i + 1 through AA inside a chain (chain_of: chain id per residue; None: one chain)."""
    partner = torch.full((1, L, 2), -1, dtype=torch.int32)
    table = torch.zeros(1, L, 2, dtype=torch.int32)
    for i in range(L):
        if i > 0 and (chain_of is None or chain_of[i] == chain_of[i - 1]):
            partner[0, i, 0], table[0, i, 0] = i - 1, 1
        if i + 1 < L and (chain_of is None or chain_of[i] == chain_of[i + 1]):
            partner[0, i, 1] = i + 1
    AA = torch.as_tensor(AA).float()
    return {"partner": partner, "table": table, "tables": torch.stack((AA, AA.t())).contiguous(), "members": members}


__all__ = ["slots_of", "steps_of", "term", "group_add", "plain_probs", "paired_probs", "class_probs", "neighbour_terms", "tied_states_ref"]
