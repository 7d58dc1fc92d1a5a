"""Reference of the group conditionals (ProteinMPNN.conditional_probs(tied=True)) built from the unchanged CPU oracle:
the GROUP STREAM — oracle.cpu_ref.decode_parallel run with score()'s decoding order from which the group's members are taken out and
appended as ..., m_1, ..., m_n (listed order), the true S teacher-forced, the token embedding of EVERY member hidden (a zero row of
h_S: an extra all-zero row appended to W_s and S[m_t] pointing at it, so decode_parallel itself stays as it is) — and the combine

    total[a] = sum_t w_t z_t[P_t[a]],   lp = log_softmax(total),   row_{m_t}[P_t[a]] = lp[a]

in fp64.  Tied states run on the block-diagonal flattened graph of M * L residues (flat residue m * L + i), every state encoded by
the oracle on its own.  Generalises pair_loo_ref.py; also the numpy restatement of the active grids with groups and the cases the
CPU and GPU tests share.  Helper module of test_group_conditional_host.py / test_gpu_group_conditional.py (not a test)."""
import functools

import numpy as np
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import mapped_groups
from oracle import cpu_ref
from loo_numpy import near_tie_rows, oracle_conditional
import paired_ref
import tied_states_ref as ts

GROUP_MAX = 16


def group_specs(fd, rti):
    """The groups of a CPU feature_dict as conditional_probs(tied=True) ties them: [(members, weights, maps)] in LISTED order
    (fixed=None), in flat indices m * L + i with states (state-major, weights w_m * w_member), every residue outside the listed
    groups a group across the states; groups of one and groups with a masked member left out."""
    L = fd["S"].shape[1]
    mask = fd["mask"][0].tolist()
    pairs = fd.get("paired_residues") or None
    sym = fd.get("symmetry_residues")
    sym = None if sym is None or len(sym) == 0 or (len(sym) == 1 and len(sym[0]) == 0) else sym
    polymer = None
    if pairs:
        polymer = [1 if d else (2 if r else 0) for d, r in zip(fd["dna_mask"][0].tolist(), fd["rna_mask"][0].tolist())]
    g, w, m = [], [], []
    if pairs or sym:
        g, w, m, _ = mapped_groups(L, rti, pairs, fd.get("paired_weights"), polymer, None, sym, fd.get("symmetry_weights") if sym else None,
                                   fd.get("symmetry_token_maps") if sym else None)
    sw = fd.get("state_weights")
    M = 1 if sw is None else len(sw)
    sw = [1.0] if sw is None else [float(v) for v in sw]
    if M > 1 or fd.get("state_weights") is not None:
        tied = {r for gi in g for r in gi}
        ident = list(range(len(spec.RESTYPES)))
        for i in range(L):
            if i not in tied:
                g.append([i]); w.append([1.0]); m.append([ident])
    out = []
    for gi, wi, mi in zip(g, w, m):
        if len(gi) * M < 2 or not all(mask[r] for r in gi):
            continue
        out.append(([r + s * L for s in range(M) for r in gi], [sw[s] * float(v) for s in range(M) for v in wi],
                    [list(P) for s in range(M) for P in mi]))
    return out


def flat_encoding(w, fd, top_k):
    """The oracle's encoding of the call's graph: (h_V, h_E, E_idx) of ONE complex — with states the block-diagonal flattened graph —,
    S and mask [1, N] and the base order [N] (score()'s order; with states step by step, the states of a residue side by side)."""
    if fd.get("state_weights") is None:
        enc = cpu_ref.encode(w, fd, top_k)
        order0 = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"])[0]
        return enc, fd["S"], fd["mask"], order0
    M, L = fd["X"].shape[:2]
    encs = [cpu_ref.encode(w, ts.state_fd(fd, s), top_k) for s in range(M)]
    enc = (torch.cat([e[0] for e in encs], 1), torch.cat([e[1] for e in encs], 1), torch.cat([e[2] + s * L for s, e in enumerate(encs)], 1))
    base = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"][:1])[0]
    order0 = (base[:, None] + L * torch.arange(M)[None, :]).reshape(-1)
    return enc, fd["S"].repeat(1, M), fd["mask"].repeat(1, M), order0


def group_stream_logits(w, enc, S, mask, order0, groups, hide=True, visible=(), chunk=8):
    """Logits of every member of every group in its group stream -> a list of [n_members, vocab].  enc = (h_V, h_E, E_idx) of ONE complex,
    order0 [N] the base order; hide=False leaves every member's token visible (what a build that forgets to hide them computes),
    `visible`: residues whose token stays visible although they are members."""
    h_V, h_E, E_idx = enc
    V = w["W_s.weight"].shape[0]
    w2 = dict(w)
    w2["W_s.weight"] = torch.cat((w["W_s.weight"], torch.zeros(1, w["W_s.weight"].shape[1], dtype=w["W_s.weight"].dtype)))
    out = []
    for p0 in range(0, len(groups), chunk):
        part = groups[p0:p0 + chunk]
        n = len(part)
        orders = []
        for g in part:
            keep = torch.ones_like(order0, dtype=torch.bool)
            for r in g:
                keep &= order0 != r
            orders.append(torch.cat((order0[keep], order0.new_tensor(list(g)))))
        orders = torch.stack(orders)
        Sn = S.long().expand(n, -1).clone()
        if hide:
            for t, g in enumerate(part):
                for r in g:
                    if r not in visible:
                        Sn[t, r] = V
        rep = lambda t: t.expand(n, *t.shape[1:])
        E_rep = rep(E_idx).contiguous()
        _, logits = cpu_ref.decode_parallel(w2, rep(h_V), rep(h_E), E_rep, Sn, rep(mask), cpu_ref.backward_mask(orders, E_rep))
        for t, g in enumerate(part):
            out.append(logits[t, list(g)])
    return out


def combine(zs, ws, Ps):
    """The group's conditional from the members' rows (logits, or log-softmax rows: one constant per member cancels), members in
    listed order, in fp64 -> one row per member, each in its member's alphabet."""
    Ps = [torch.as_tensor(P) for P in Ps]
    total = None
    for z, wt, P in zip(zs, ws, Ps):
        term = float(wt) * z.double()[P]
        total = term if total is None else total + term
    lp = torch.log_softmax(total, -1)
    rows = []
    for P in Ps:
        row = torch.empty_like(lp)
        row[P] = lp
        rows.append(row)
    return rows


def oracle_group_conditional(w, fd, top_k, rti, hide=True):
    """conditional_probs(tied=True) on the CPU oracle -> (log_probs [1, L, vocab] with the group rows on the tied residues and the
    leave-one-out rows — state 0's with states — everywhere else, the same without groups, the base order [N], the flat E_idx
    [N, K], the tied specs)."""
    enc, S, mask, order0 = flat_encoding(w, fd, top_k)
    L = fd["S"].shape[1]
    fd0 = fd if fd.get("state_weights") is None else ts.state_fd(fd, 0)
    loo = oracle_conditional(w, {k: v for k, v in fd0.items() if k not in ("paired_residues", "symmetry_residues")}, top_k)[0][:1]
    specs = group_specs(fd, rti)
    zs = group_stream_logits(w, enc, S, mask, order0, [s[0] for s in specs], hide=hide)
    out = loo.clone()
    for (g, gw, gm), z in zip(specs, zs):
        for r, row in zip(g, combine(z, gw, gm)):
            if r < L:
                out[0, r] = row.float()
    return out, loo, order0, enc[2][0], specs


def group_tables(N, groups, mask):
    """What loo_groups_kernel leaves: sid [N] the stream of a residue (the listed-first member of its group, itself when ungrouped) and
    pos [N] its listed position; a group with a masked member left out.  groups: lists of flat indices in listed order."""
    sid, pos = np.arange(N), np.zeros(N, np.int64)
    for g in groups:
        if len(g) >= 2 and all(mask[r] for r in g):
            for t, r in enumerate(g):
                sid[r], pos[r] = g[0], t
    return sid, pos


def group_loo_grids(E_idx, rank, mask, sid):
    """E_idx [N, K], rank [N], mask [N], sid [N] -> act1 [N, K] (layer-1 item (m, k), n = E_idx[m, k]: m used to see n as decoded and is
    not in n's group; the item belongs to the stream of n's group), act2 [N, K] (layer-2 item (g, kq), q = E_idx[g, kq] outside g's
    group: q itself or one of its decoded neighbours outside the group has a layer-1 override in the stream of g's group, through any
    member).  With groups of two these are pair_loo_numpy.pair_loo_grids' grids, without groups loo_numpy.loo_grids'."""
    E_idx = np.asarray(E_idx, np.int64); rank = np.asarray(rank, np.int64); mask = np.asarray(mask); sid = np.asarray(sid, np.int64)
    N, K = E_idx.shape
    act1 = (sid[E_idx] != sid[:, None]) & (rank[E_idx] < rank[:, None]) & (mask[:, None] != 0)
    has_ov = np.zeros((N, N), bool)                                          # [stream, m]: m has a layer-1 override in that stream
    mm, kk = np.nonzero(act1)
    has_ov[sid[E_idx[mm, kk]], mm] = True
    q = E_idx                                                                # [g, kq]
    s = sid[:, None]
    cen_ov = has_ov[s, q]
    nb = E_idx[q]                                                            # [g, kq, k']: neighbours of q
    bw = (sid[nb] != s[:, :, None]) & (rank[nb] < rank[q][..., None])
    ov = bw & has_ov[s[:, :, None], nb]
    act2 = (sid[q] != s) & (mask[q] != 0) & (cen_ov | ov.any(-1))
    return act1, act2


def flat_rank(rank, M):
    """The ranks the device reads on the flattened graph: the one order's ranks, repeated per state."""
    return np.tile(np.asarray(rank), M)


def neighbour_kinds(E_idx, group):
    """Per ordered member pair (t < u) of a group: (m_t in N(m_u), m_u in N(m_t)) on E_idx [N, K]."""
    E = np.asarray(E_idx)
    return [(bool((E[group[u]] == group[t]).any()), bool((E[group[t]] == group[u]).any()))
            for t in range(len(group)) for u in range(t + 1, len(group))]


# ---- the cases of the CPU and GPU tests -----------------------------------------------------------------------------------------
CASES = ("trimer_l24", "mixed_l12", "dimer_l48", "states_m3_l20", "states_pairs_m2_l32", "cap_m8_l16", "trimer_maps_l24")
K_CASE = 16


def _sym_case(L, seed, groups, weights=None, masked=()):
    _, fd, _ = paired_ref.make_case(L=L, bs=1, T=1.0, n_pairs=0, seed=seed, fixed_every=0)
    fd = {k: v for k, v in fd.items() if k != "paired_residues"}
    fd["mask"] = fd["mask"].clone()
    for r in masked:
        fd["mask"][0, r] = 0
    fd.update(symmetry_residues=groups, symmetry_weights=weights or [[1.0] * len(g) for g in groups])
    return fd


def _states_case(L, M, seed, state_w, n_pairs=0):
    cx, fdp, pairs = paired_ref.make_case(L=L, bs=1, T=1.0, n_pairs=n_pairs, seed=seed, fixed_every=0)
    Xs = ts.make_states(cx, M, seed + 5)
    fd = ts.states_fd(cx, Xs, state_w, 1, 1.0, fdp["randn"])
    if n_pairs:
        fd["paired_residues"] = pairs
    return fd


def case_inputs(name):
    """name -> the CPU feature_dict of a case (K = 16 everywhere):
    trimer_l24           L = 24: a 3 x 8 homo-trimer, eight groups (i, i + 8, i + 16) with weights (1, 0.5, 0.25); L is near K: of the 21
                         ordered member pairs of the seven tied groups 14 are mutual neighbours, 1 + 3 one-way, 3 none (K = 16 of 24
                         residues cannot make all of them neighbours); residue 11 is masked: the group of residue 3 is dropped;
    mixed_l12            L = 12 < K: listed groups of two (1, 7), four (2, 5, 8, 11) and ONE (4, with weight 0.5: a group of one is the
                         leave-one-out row and its weight is not applied), everything else alone;
    dimer_l48            L = 48: a 2 x 24 dimer, groups (i, i + 24): 2 copies are mutual neighbours, 3 + 1 one-way (only the second in
                         the first's list / only the first in the second's), 18 no neighbours at all;
    states_m3_l20        M = 3 states of 20 residues, weights (0.5, 0.3, 0.2), no pairs: members are never neighbours;
    states_pairs_m2_l32  M = 2 states of 32 residues with six base pairs: groups of four with maps, groups of two elsewhere;
    cap_m8_l16           M = 8 states of 16 residues with one base pair: a group at the cap of 16;
    trimer_maps_l24      trimer_l24 with symmetry_token_maps: the second member of every group speaks through the Watson-Crick map."""
    if name == "trimer_l24":
        return _sym_case(24, 11, [[i, i + 8, i + 16] for i in range(8)], [[1.0, 0.5, 0.25]] * 8, masked=(11,))
    if name == "mixed_l12":
        return _sym_case(12, 7, [[1, 7], [2, 5, 8, 11], [4]], [[1.0, 1.0], [1.0] * 4, [0.5]])
    if name == "dimer_l48":
        return _sym_case(48, 13, [[i, i + 24] for i in range(24)])
    if name == "states_m3_l20":
        return _states_case(20, 3, 13, [0.5, 0.3, 0.2])
    if name == "states_pairs_m2_l32":
        return _states_case(32, 2, 23, [0.6, 0.4], n_pairs=6)
    if name == "cap_m8_l16":
        return _states_case(16, 8, 29, [0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05], n_pairs=1)
    if name == "trimer_maps_l24":
        wc = spec.token_map(spec.restype_to_int(), "same")
        return dict(case_inputs("trimer_l24"), symmetry_token_maps=[[None, list(wc), None] for _ in range(8)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle's rows of a case, computed once and shared: (fd, rows with groups, leave-one-out rows, base order [N], E_idx [N, K],
    tied specs)."""
    fd = case_inputs(name)
    w = cpu_ref.to_torch(synth.make_weights(0))
    return (fd,) + oracle_group_conditional(w, fd, K_CASE, spec.restype_to_int())


@functools.lru_cache(maxsize=None)
def oracle_case_unhidden(name):
    """The rows of a build that forgets to hide the members' tokens."""
    fd = case_inputs(name)
    w = cpu_ref.to_torch(synth.make_weights(0))
    return oracle_group_conditional(w, fd, K_CASE, spec.restype_to_int(), hide=False)[0]


def left_out(name):
    fd, ref = oracle_case(name)[:2]
    return near_tie_rows(ref, fd["mask"])[1]
