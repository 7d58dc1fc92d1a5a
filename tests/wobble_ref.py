"""Reference of base-paired design with G-U wobble (ProteinMPNN.sample with feature_dict["paired_wobble"]) built from the unchanged
CPU oracle in the way paired_ref is: oracle.cpu_ref.sample_symmetric runs with the pairs as plain symmetry groups, teacher-forced per
member with the sampled tokens, and the distribution over PAIR CLASSES is recombined from the members' log_probs rows in float64,

    total[c] = sum_j w_j * log_probs_j[C_j[c]] + bias_close[C_close[c]] + class_bias[c]     over the classes every member has a token for,
    p = softmax(total / T), the classes whose closing token is special zeroed, renormalised,

(C_j the class table of member j, `close` the last listed member), which equals the distribution of the logits' sum because log_softmax
differs from the logits by one constant per member.  The row of a member is the marginal of p in its own alphabet; the draw is from p
restricted by the pinned (fixed or forced) members in listed order, a restriction that would leave nothing being skipped."""
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import mapped_groups
from oracle import cpu_ref
import paired_ref

WOBBLE_KEYS = ("paired_wobble", "paired_wobble_bias")
V = len(spec.RESTYPES)
IDENT = list(range(V)) + [-1] * (spec.N_CLASS_LANES - V)


def groups_of(fd, rti):
    """The groups of a CPU feature_dict as the model builds them with wobble: (groups, weights, class tables, class biases)."""
    L = fd["S"].shape[1]
    polymer = [1 if d else (2 if r else 0) for d, r in zip(fd["dna_mask"][0].tolist(), fd["rna_mask"][0].tolist())]
    fixed = [not v for v in (fd["mask"] * fd["chain_mask"])[0].tolist()]
    g, w, t, _, cb = mapped_groups(L, rti, fd["paired_residues"], fd.get("paired_weights"), polymer, fixed, fd.get("symmetry_residues"),
                                   fd.get("symmetry_weights"), fd.get("symmetry_token_maps"), fd.get("paired_wobble", False),
                                   fd.get("paired_wobble_bias"))
    return g, w, t, cb


def with_singletons(L, groups, weights, tables, class_bias):
    """The groups, and behind them every residue that is in none as a group of its own (the identity table, no class bias)."""
    tied = {i for g in groups for i in g}
    rest = [i for i in range(L) if i not in tied]
    return (list(groups) + [[i] for i in rest], list(weights) + [[1.0]] * len(rest), list(tables) + [[IDENT]] * len(rest),
            list(class_bias) + [[0.0] * spec.N_CLASS_LANES] * len(rest))


def class_probs(log_probs, fd, groups, weights, tables, class_bias, special=cpu_ref.SPECIAL_TOKENS, state_weights=None, S_forced=None):
    """log_probs [bs, L, V] (or [bs, M, L, V] with state_weights [M]), teacher-forced per residue, the rows of fixed members kept ->
    (rows, draws): rows [bs, L, V] float64 the unrestricted marginal of every residue in its own alphabet, zero where mask *
    chain_mask is zero; draws: per group (members, p_restricted [bs, 64], its cumulative sum in class order [bs, 64]).
    Residues outside the groups count as groups of one."""
    lp = log_probs.double()
    if lp.dim() == 3:
        lp = lp[:, None]
    bs, M, L, _ = lp.shape
    sw = [1.0] * M if state_weights is None else [float(v) for v in state_weights]
    T = float(fd["temperature"])
    bias = fd["bias"].double().expand(1, L, V)[0]
    cm = (fd["mask"] * fd["chain_mask"])[0].bool().tolist()
    S_true = fd["S"][0].tolist()
    rows = torch.zeros(bs, L, V, dtype=torch.float64)
    draws = []
    for g, gw, gt, cb in zip(*with_singletons(L, groups, weights, tables, class_bias)):
        tabs = [torch.tensor(t) for t in gt]
        valid = torch.stack([t >= 0 for t in tabs]).all(0)
        cl = [t.clamp(min=0) for t in tabs]
        total = torch.zeros(bs, spec.N_CLASS_LANES, dtype=torch.float64)
        for m in range(M):
            for j, w_j, c_j in zip(g, gw, cl):
                total = total + sw[m] * float(w_j) * lp[:, m, j][:, c_j]
        total = total + bias[g[-1]][cl[-1]][None] + torch.tensor(cb, dtype=torch.float64)[None]
        total = torch.where(valid[None], total, torch.full_like(total, -float("inf")))
        p = torch.softmax(total / T, -1)
        p = p * torch.tensor([int(c) not in special for c in cl[-1]], dtype=torch.float64)[None] * valid[None]
        p = p / p.sum(-1, keepdim=True)
        for j, t_j in zip(g, tabs):
            if cm[j]:
                for c in range(spec.N_CLASS_LANES):                            # ascending class index
                    if int(t_j[c]) >= 0:
                        rows[:, j, int(t_j[c])] += p[:, c]
        pr = torch.zeros_like(p)
        for b in range(bs):
            keep = p[b] > 0
            for j, t_j in zip(g, tabs):
                tok = S_true[j] if not cm[j] else (int(S_forced[b, j]) if S_forced is not None else None)
                if tok is not None and bool((keep & (t_j == tok)).any()):
                    keep = keep & (t_j == tok)
            pr[b] = p[b] * keep / (p[b] * keep).sum()
        draws.append((g, pr, torch.cumsum(pr, -1)))
    return rows, draws


def drawn_class(pr, cdf, u):
    """The inverse CDF in ascending class index: the first class with mass whose cumulative sum exceeds u (the last with mass if none
    does) -> (class, the distance of u to the nearest boundary of the CDF)."""
    pos = pr > 0
    hit = pos & (cdf > u)
    c = int(hit.nonzero()[0]) if hit.any() else int(pos.nonzero()[-1])
    return c, float((cdf[pos] - u).abs().min())


def tokens_of(c, g, tables, fd, S_forced_b=None):
    """The tokens of the members of group g under class c: a fixed or forced member keeps its own."""
    cm = (fd["mask"] * fd["chain_mask"])[0].bool().tolist()
    out = []
    for j, t_j in zip(g, tables):
        if not cm[j]:
            out.append(int(fd["S"][0, j]))
        elif S_forced_b is not None:
            out.append(int(S_forced_b[j]))
        else:
            out.append(int(t_j[c]))
    return out


def oracle_wobble(weights_t, fd, K, S, rti, special=cpu_ref.SPECIAL_TOKENS, S_forced=None):
    """The oracle teacher-forced with S [bs, L] on the pairs of `fd` -> (log_probs [bs, L, V], rows [bs, L, V], draws, the oracle's
    decoding order, (groups, weights, tables, class_bias), the log_probs with the rows of fixed group members kept)."""
    plain = {k: v for k, v in fd.items() if k not in WOBBLE_KEYS}
    lp, _, order, (groups, weights, _), lp_groups = paired_ref.oracle_paired(weights_t, plain, K, S, rti, special)
    g2, w2, tables, cb = groups_of(fd, rti)
    assert g2 == groups and w2 == weights                                    # (wobble changes the tables, never the groups)
    rows, draws = class_probs(lp_groups, fd, groups, weights, tables, cb, special, S_forced=S_forced)
    return lp, rows, draws, order, (groups, weights, tables, cb), lp_groups


def pair_kind(a, b, rti):
    """'canonical', 'wobble' or None for the tokens (a, b) of a pair."""
    if (a, b) in set(spec.na_canonical_base_pair_ints(rti)):
        return "canonical"
    g, u = {rti["DG"], rti["G"]}, {rti["DT"], rti["U"]}
    if (a in g and b in u) or (a in u and b in g):
        return "wobble"
    return None
