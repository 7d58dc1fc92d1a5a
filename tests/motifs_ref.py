"""Reference of the forbidden motifs (ProteinMPNN.sample with feature_dict["forbidden_motifs"]) by brute force, on top of the references
of the ties.  A motif OCCURS at residues r_0 .. r_{n-1} that are consecutive on one chain (same chain_labels, R_idx one apart), all present
(mask) and hold the motif's tokens.  When the group reached at a step draws, candidate `a` (a group token with maps, a class with class
tables) is banned if the following sequence holds an occurrence that covers a member of the group: every member holds the token the
sampler's assignment would write for it under `a` (forced and fixed members their own; with maps they also pass it on), every residue
whose group was drawn before holds its token of the FINAL sequence, every other residue is PAD.  For every draw and every candidate the
sequence is built and searched.  The ban is folded as -1e9 into the bias row of the group's closing member (token maps: bias_c[P_c[a]])
or into the group's class biases (class tables), and then goes through the existing recombinations (paired_ref.paired_probs,
wobble_ref.class_probs, with state_weights tied_states_ref's rule inside them) exactly as pair_terms_ref folds its terms; a ban that would
leave no candidate with p > 0 is skipped (found with a first recombination without bans).  Log-probs come from the unchanged oracles."""
import torch

from na_mpnn_amd import spec
import paired_ref
import wobble_ref
from pair_terms_ref import steps_of

V = len(spec.RESTYPES)
PAD = V - 1
IDENT = list(range(V))
BAN = -1e9


def next_ok(fd, b=0):
    """next_ok[i]: residues i and i + 1 are consecutive on one chain and both present."""
    cl, ri, mk = fd["chain_labels"][b].tolist(), fd["R_idx"][b].tolist(), fd["mask"][b].tolist()
    return [bool(cl[i] == cl[i + 1] and ri[i + 1] - ri[i] == 1 and mk[i] and mk[i + 1]) for i in range(len(cl) - 1)]


def occurrences(seq, nxt, motifs):
    """Every occurrence as (start, length)."""
    out, L = [], len(seq)
    for m in motifs:
        n = len(m)
        for s in range(L - n + 1):
            if all(nxt[s + q] for q in range(n - 1)) and all(int(seq[s + q]) == int(m[q]) for q in range(n)):
                out.append((s, n))
    return out


def hits(S, fd, motifs):
    """motif_hits: occurrences in every row of S [bs, L] (row r of complex r % B)."""
    B = fd["mask"].shape[0]
    return torch.tensor([len(occurrences(S[r].tolist(), next_ok(fd, r % B), motifs)) for r in range(S.shape[0])], dtype=torch.int64)


def member_tokens(g, alphabets, a, fixed_tok, forced_tok, classes):
    """The token every member of g holds under candidate a.  alphabets[m][a]: member m's token under group token / class a;
    fixed_tok[j] / forced_tok[j]: the member's own token if it is fixed / forced, else None.  Maps: the running group token starts as a;
    a forced, then a fixed member replaces it by the group token of its own token (P is an involution) and passes that on; the member
    holds P[running].  Class tables: a pinned member holds its own token and passes nothing on."""
    out, run = [], a
    for j, P in zip(g, alphabets):
        if classes:
            tok = P[a]
            if forced_tok[j] is not None:
                tok = forced_tok[j]
            if fixed_tok[j] is not None:
                tok = fixed_tok[j]
        else:
            if forced_tok[j] is not None:
                run = P[forced_tok[j]]
            if fixed_tok[j] is not None:
                run = P[fixed_tok[j]]
            tok = P[run]
        out.append(int(tok))
    return out


def banned(motifs, g, alphabets, lanes, S_row, step, nxt, fixed_tok, forced_tok, classes):
    """[lanes] bool: the candidates of group g that are banned under the final sequence S_row."""
    L = len(S_row)
    s_g = step[g[0]]
    base = [int(S_row[j]) if step[j] < s_g else PAD for j in range(L)]
    out = []
    for a in range(lanes):
        seq = list(base)
        for j, tok in zip(g, member_tokens(g, alphabets, a, fixed_tok, forced_tok, classes)):
            seq[j] = tok if 0 <= tok < V else PAD
        out.append(any(any(s <= j < s + n for j in g) for s, n in occurrences(seq, nxt, motifs)))
    return out


def _pins(fd, S_forced_b, S_true):
    L = fd["S"].shape[1]
    cm = (fd["mask"] * fd["chain_mask"])[0].bool().tolist()
    S_true = fd["S"][0].tolist() if S_true is None else [int(t) for t in S_true]
    fixed_tok = [None if cm[j] else S_true[j] for j in range(L)]
    forced_tok = [None if S_forced_b is None else int(S_forced_b[j]) for j in range(L)]
    return fixed_tok, forced_tok


def _free(fd):
    return dict(fd, mask=torch.ones_like(fd["mask"]), chain_mask=torch.ones_like(fd["chain_mask"]))


def paired_probs(lp_groups, fd, motifs, S, order, groups, weights, maps, state_weights=None, S_forced=None, S_true=None, info=None):
    """paired_ref.paired_probs under the motifs: lp_groups [bs, L, V] or [bs, M, L, V] as oracle_paired returns them (the rows of fixed
    members kept).  Untied residues are groups of one.  S_true: the tokens fixed residues hold where they differ from fd["S"] (context
    states: state 0's).  info (dict, optional): receives "bans" (draws with a banned candidate that had mass) and "skipped"."""
    L = fd["S"].shape[1]
    groups = [list(g) for g in groups if len(g)]
    tied = {i for g in groups for i in g}
    all_groups = groups + [[i] for i in range(L) if i not in tied]
    all_maps = [list(m) for m in maps][:len(groups)] + [[IDENT]] * (len(all_groups) - len(groups))
    nxt = next_ok(fd)
    p0 = paired_ref.paired_probs(lp_groups, _free(fd), groups, weights, maps, state_weights=state_weights).double()
    info = {} if info is None else info
    info.setdefault("bans", 0); info.setdefault("skipped", 0)
    out = []
    for b in range(S.shape[0]):
        step = steps_of(order[b].tolist(), groups, L)
        fixed_tok, forced_tok = _pins(fd, None if S_forced is None else S_forced[b], S_true)
        bias = fd["bias"].double().expand(1, L, V).clone()
        for g, al in zip(all_groups, all_maps):
            ban = banned(motifs, g, al, V, S[b].tolist(), step, nxt, fixed_tok, forced_tok, False)
            c, Pc = g[-1], al[-1]
            alive = [a for a in range(V) if float(p0[b, c, Pc[a]]) > 0]
            if not any(ban[a] for a in alive):
                continue
            if all(ban[a] for a in alive):
                info["skipped"] += 1
                continue
            info["bans"] += 1
            for a in range(V):
                if ban[a]:
                    bias[0, c, Pc[a]] += BAN
        out.append(paired_ref.paired_probs(lp_groups[b:b + 1], dict(fd, bias=bias), groups, weights, maps, state_weights=state_weights))
    return torch.cat(out)


def plain_probs(log_probs, fd, motifs, S, order, groups=None, group_weights=None, state_weights=None, S_forced=None, S_true=None, info=None):
    """Untied residues, symmetry groups (identity maps) and states."""
    groups = [list(g) for g in (groups or []) if len(g)]
    weights = [list(w) for w in (group_weights or [])][:len(groups)]
    maps = [[IDENT] * len(g) for g in groups]
    return paired_probs(log_probs, fd, motifs, S, order, groups, weights, maps, state_weights, S_forced, S_true, info)


def class_probs(lp_groups, fd, motifs, S, order, groups, weights, tables, class_bias, state_weights=None, S_forced=None, info=None):
    """wobble_ref.class_probs' rows under the motifs: a banned class gets -1e9 on its class bias, a banned token of an untied residue on
    its bias row."""
    L = fd["S"].shape[1]
    lanes = spec.N_CLASS_LANES
    nxt = next_ok(fd)
    _, draws0 = wobble_ref.class_probs(lp_groups, _free(fd), groups, weights, tables, class_bias, state_weights=state_weights)
    info = {} if info is None else info
    info.setdefault("bans", 0); info.setdefault("skipped", 0)
    rows = []
    for b in range(S.shape[0]):
        step = steps_of(order[b].tolist(), groups, L)
        fixed_tok, forced_tok = _pins(fd, None if S_forced is None else S_forced[b], None)
        bias = fd["bias"].double().expand(1, L, V).clone()
        cb = [list(c) for c in class_bias]
        for gi, (g, p_free, _) in enumerate(draws0):
            al = [list(t) for t in tables[gi]] if gi < len(groups) else [wobble_ref.IDENT]
            ban = banned(motifs, g, al, lanes, S[b].tolist(), step, nxt, fixed_tok, forced_tok, True)
            alive = [a for a in range(lanes) if float(p_free[b, a]) > 0]
            if not any(ban[a] for a in alive):
                continue
            if all(ban[a] for a in alive):
                info["skipped"] += 1
                continue
            info["bans"] += 1
            for a in range(lanes):
                if ban[a] and gi < len(groups):
                    cb[gi][a] += BAN
                elif ban[a] and a < V:
                    bias[0, g[0], a] += BAN
        rows.append(wobble_ref.class_probs(lp_groups[b:b + 1], dict(fd, bias=bias), groups, weights, tables, cb, state_weights=state_weights,
                                           S_forced=None if S_forced is None else S_forced[b:b + 1])[0])
    return torch.cat(rows).float()
