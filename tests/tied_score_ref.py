"""Reference of the tied score (ProteinMPNN.score_tied) built from the unchanged CPU oracle.

* the numpy restatement of what the device plans — key(i) = (min of rank0 over i's group) << 4 | listed position, the leader, and the
  kind of every edge (forward / backward / hidden-backward) — and the brute force it must equal: dense visit ranks of
  model.symmetry_visits plus group membership;
* the PARALLEL form on the oracle's pieces (cpu_ref.dec_layer with per-edge token hiding) and the SEQUENTIAL oracles teacher-forced
  on the same sequences (cpu_ref.sample / cpu_ref.sample_symmetric, per state through tied_states_ref.oracle_tied), which it must
  reproduce;
* the combine in fp64 and the cases the CPU and GPU tests share.

Helper module of test_tied_score_host.py / test_gpu_tied_score*.py (not a test)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import symmetry_visits
from oracle import cpu_ref
import class_loo_ref
import group_loo_ref
import paired_ref
import tied_states_ref as ts

NEG = -float("inf")
FW, BW, HID = 0, 1, 2
TIE_KEYS = ("paired_residues", "paired_weights", "paired_wobble", "paired_wobble_bias", "symmetry_residues", "symmetry_weights",
            "symmetry_token_maps")


def wobble_asked(fd):
    w = fd.get("paired_wobble")
    w = w.tolist() if torch.is_tensor(w) else w
    return any(w) if isinstance(w, (list, tuple)) else bool(w)


def specs_of(fd, rti):
    """The units of more than one residue as score_tied ties them: [(members, weights, tables, class bias or None)] in LISTED order,
    flat indices; maps [vocab] without paired_wobble, class tables [64] with it."""
    if wobble_asked(fd):
        return [tuple(s) for s in class_loo_ref.class_specs(fd, rti, True)]
    return [tuple(s) + (None,) for s in group_loo_ref.group_specs(fd, rti)]


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def keys_and_leaders(rank0, groups):
    """rank0 [N], groups: the tied groups (flat indices, listed order) -> (key [N], leader [N])."""
    rank0 = np.asarray(rank0, np.int64)
    key, leader = rank0 << 4, np.arange(len(rank0))
    for g in groups:
        mn = min(int(rank0[r]) for r in g)
        for t, r in enumerate(g):
            key[r], leader[r] = (mn << 4) | t, g[0]
    return key, leader


def edge_kinds(E_idx, key, leader):
    """E_idx [N, K] -> kinds [N, K]: FW where key(j) >= key(i), HID where key(j) < key(i) in one group, BW otherwise."""
    E = np.asarray(E_idx, np.int64)
    kj, ki = key[E], key[:, None]
    return np.where(kj >= ki, FW, np.where(leader[E] == leader[:, None], HID, BW))


def edge_kinds_brute(E_idx, order0, groups):
    """The same from the visit plan of the sampler: dense visit ranks of symmetry_visits and group membership."""
    E = np.asarray(E_idx, np.int64)
    N = E.shape[0]
    visits = symmetry_visits(groups, [[1.0] * len(g) for g in groups], [int(v) for v in order0], N)[0]
    vr = np.empty(N, np.int64)
    vr[np.asarray(visits)] = np.arange(N)
    gid = -np.arange(1, N + 1)
    for q, g in enumerate(groups):
        gid[list(g)] = q
    out = np.empty(E.shape, np.int64)
    for i in range(N):
        for k, j in enumerate(E[i]):
            out[i, k] = FW if vr[j] >= vr[i] else (HID if gid[j] == gid[i] else BW)
    return out


def rank_of(order0):
    r = np.empty(len(order0), np.int64)
    r[np.asarray(order0)] = np.arange(len(order0))
    return r


# ---- the parallel form on the oracle's pieces -------------------------------------------------------------------------------------
def parallel_logits(w, enc, S, mask, kinds, hide=True):
    """enc = (h_V, h_E, E_idx) of ONE complex [1, N, ...], S [n, N], mask [1, N], kinds [N, K] -> logits [n, N, vocab] of the tied
    stream evaluated in parallel; hide=False treats hidden-backward edges as ordinary backward edges."""
    n = S.shape[0]
    rep = lambda t: t.expand(n, *t.shape[1:])
    h_V, h_E, E_idx = (rep(t) for t in enc)
    kinds = torch.as_tensor(kinds)
    m1 = rep(mask).float().view(n, -1, 1, 1)
    bw = (kinds == BW) | ((kinds == HID) if not hide else torch.zeros_like(kinds, dtype=torch.bool))
    hid = (kinds == HID) & hide
    sel = lambda b: m1 * b.float()[None, :, :, None]
    h_S = F.embedding(S.long(), w["W_s.weight"])
    h_ES = cpu_ref.cat_neighbors_nodes(h_S, h_E, E_idx)
    h_EX = cpu_ref.cat_neighbors_nodes(torch.zeros_like(h_S), h_E, E_idx)
    ctx_fw = sel(kinds == FW) * cpu_ref.cat_neighbors_nodes(h_V, h_EX, E_idx)
    for l in range(cpu_ref.n_layers(w, "decoder")):
        h_ESV = sel(bw) * cpu_ref.cat_neighbors_nodes(h_V, h_ES, E_idx) + sel(hid) * cpu_ref.cat_neighbors_nodes(h_V, h_EX, E_idx) + ctx_fw
        h_V = cpu_ref.dec_layer(w, f"decoder_layers.{l}.", h_V, h_ESV, rep(mask).float())
    return cpu_ref._lin(w, "W_out", h_V)


def sequential_rows(w, fd, top_k, S, specs):
    """The sequential oracle teacher-forced with S [n, L] (chain_mask all ones: score()'s order) -> log-softmax rows [n, N, vocab] of
    every residue (every state's copy), zero on masked residues."""
    n, L = S.shape
    groups0 = [[r for r in g if r < L] for g, *_ in specs]
    groups0 = [g for g in groups0 if len(g) > 1]
    fdo = {k: v for k, v in fd.items() if k not in TIE_KEYS}
    fdo.update(batch_size=n, temperature=1.0, bias=torch.zeros(1, L, len(spec.RESTYPES)), randn=fd["randn"][:1].repeat(n, 1),
               symmetry_residues=groups0 or [[]], symmetry_weights=[[1.0] * len(g) for g in groups0] or [[]])
    assert bool((fd["chain_mask"] == 1).all())
    if fd.get("state_weights") is not None:
        return ts.oracle_tied(w, fdo, top_k, S)[0].reshape(n, -1, len(spec.RESTYPES))
    ref = (cpu_ref.sample_symmetric if groups0 else cpu_ref.sample)(w, fdo, top_k, S_forced=S)
    assert torch.equal(ref["S"] * fd["mask"].long(), S * fd["mask"].long())
    return ref["log_probs"]


# ---- the combine ----------------------------------------------------------------------------------------------------------------
def unit_values(rows, S_flat, specs):
    """rows [n, N, vocab] (logits or log-softmax rows), S_flat [n, N] -> (unit log-probs [n, N], own entries [n, N]) in fp64."""
    own = torch.log_softmax(rows.double(), -1).gather(2, S_flat.long()[:, :, None])[:, :, 0]
    unit = own.clone()
    for g, gw, tabs, gb in specs:
        T = torch.tensor(tabs)
        width = T.shape[1]
        have = (T >= 0).all(0) & (torch.arange(width) < (spec.N_CLASSES if gb is not None else width))
        for k in range(rows.shape[0]):
            total = torch.zeros(width, dtype=torch.float64)
            for r, wt, C in zip(g, gw, T.clamp(min=0)):
                total = total + float(wt) * rows[k, r].double()[C]
            if gb is not None:
                total = total + torch.tensor(gb, dtype=torch.float64)
            clp = torch.log_softmax(torch.where(have, total, torch.full_like(total, NEG)), -1)
            match = have.clone()
            for r, C in zip(g, T):
                match &= C == int(S_flat[k, r])
            unit[k, list(g)] = torch.logsumexp(clp[match], 0) if bool(match.any()) else NEG
    return unit, own


def consistent_sequence(S, specs, L, pick=0):
    """S [L] -> a copy that satisfies every tie: the group's class is the pick-th one (cyclically) every member has a token for that
    keeps the listed-first member's token if there is one, else the pick-th valid class."""
    S = S.clone()
    for g, _, tabs, gb in specs:
        T = torch.tensor(tabs)
        have = (T >= 0).all(0) & (torch.arange(T.shape[1]) < (spec.N_CLASSES if gb is not None else T.shape[1]))
        valid = [c for c in range(T.shape[1]) if bool(have[c])]
        keep = [c for c in valid if int(T[0, c]) == int(S[g[0] % L])]
        c = (keep or valid)[pick % len(keep or valid)]
        for r, C in zip(g, T):
            S[r % L] = int(C[c])
    return S


# ---- the cases ------------------------------------------------------------------------------------------------------------------
GROUP_CASES = ("trimer_l24", "mixed_l12", "dimer_l48", "states_m3_l20", "states_pairs_m2_l32", "cap_m8_l16", "trimer_maps_l24")
CLASS_CASES = class_loo_ref.CASES          # l48_k16, l12_lt_k, hybrid (K = 24), states_pairs, cap16, 4oqu (a real structure, K = 32)
K_OF = dict({n: group_loo_ref.K_CASE for n in GROUP_CASES}, **{n: class_loo_ref.K_OF[n] for n in CLASS_CASES}, paired_l40=16, plain_l17=48,
            plain_l1=48, trimer_l24_k48=48)
# what the GPU tests run (each one encoder + a few decoder calls)
GPU_CASES = ("trimer_l24", "mixed_l12", "states_m3_l20", "states_pairs_m2_l32", "cap_m8_l16", "trimer_maps_l24", "l48_k16", "l12_lt_k",
             "states_pairs", "cap16", "hybrid", "4oqu", "trimer_l24_k48", "paired_l40", "plain_l17", "plain_l1")
N_SEQ = 3
SENSITIVE = "l48_k16"     # the paired case on which the oracle moves most when hidden-backward edges are read as backward edges


def case_inputs(name):
    """The cases of group_loo_ref / class_loo_ref, one paired_ref.make_case (paired_l40: 40 residues, five Watson-Crick pairs, 5 %
    masked), trimer_l24 again with k_neighbors = 48 (trimer_l24_k48: L = 24 < K) and two complexes without ties (plain_l17: 17 residues, K = 17 — one item tile and one row; plain_l1: one residue);
    chain_mask all ones, zero bias, T = 1."""
    if name in GROUP_CASES:
        fd = dict(group_loo_ref.case_inputs(name))
    elif name == "trimer_l24_k48":                       # L = 24 < K = 48: K clamps to 24, two edge tiles, every residue a neighbour of every other
        fd = dict(group_loo_ref.case_inputs("trimer_l24"))
    elif name in CLASS_CASES:
        fd = dict(class_loo_ref.case_inputs(name))
    elif name == "paired_l40":
        fd = dict(paired_ref.make_case(L=40, bs=1, T=1.0, n_pairs=5, seed=31, masked_frac=0.05, fixed_every=0)[1])
    elif name in ("plain_l17", "plain_l1"):
        L = 17 if name == "plain_l17" else 1
        cx = synth.make_complex(seed=5, n=L, n_chains=1, frac_protein=1.0, frac_dna=0.0)
        fd = {k: torch.from_numpy(np.ascontiguousarray(cx[k]))[None] for k in paired_ref.PER_RESIDUE}
        fd.update(symmetry_residues=[[]], symmetry_weights=[[]],
                  randn=torch.from_numpy(np.random.default_rng(9).standard_normal((1, L)).astype(np.float32)))
    else:
        raise KeyError(name)
    L = fd["S"].shape[1]
    fd.update(chain_mask=torch.ones_like(fd["chain_mask"]), bias=torch.zeros(1, L, len(spec.RESTYPES)), temperature=1.0, batch_size=1)
    fd["randn"] = fd["randn"][:1]
    return fd


def library(fd, specs, n=N_SEQ, seed=0):
    """n sequences [n, L]: tie-consistent variants of fd["S"] with random tokens outside the groups, and — with n >= 3 and a group to
    break — the LAST one with the listed-first member of the first group changed (it breaks that tie)."""
    L = fd["S"].shape[1]
    rng = np.random.default_rng(seed)
    prot = fd["protein_mask"][0].bool() & (fd["mask"][0] != 0)
    out = []
    for k in range(n):
        S = fd["S"][0].clone().long()
        if k:
            flip = torch.from_numpy(rng.random(L) < 0.3) & prot
            S[flip] = torch.from_numpy(rng.integers(0, 20, L))[flip]
        out.append(consistent_sequence(S, specs, L, pick=k))
    if n >= 3 and specs:
        r = specs[0][0][0]
        tabs = torch.tensor(specs[0][2])
        other = [int(t) for t in tabs[0].tolist() if t >= 0 and t != int(out[-1][r])]
        out[-1][r] = other[0]
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def oracle_case(name, hide=True):
    """Computed once and shared -> dict: fd, specs, S_lib [n, L], order0 [N], E_idx [N, K], kinds [N, K], mask [N], and from the PARALLEL form
    in fp32 with the fp64 combine: unit [n, N], own [n, N], logits [n, N, vocab]."""
    fd = case_inputs(name)
    rti = spec.restype_to_int()
    w = cpu_ref.to_torch(synth.make_weights(0))
    specs = specs_of(fd, rti)
    enc, S1, mask, order0 = group_loo_ref.flat_encoding(w, fd, K_OF[name])
    E = enc[2][0].numpy()
    key, leader = keys_and_leaders(rank_of(order0.numpy()), [s[0] for s in specs])
    kinds = edge_kinds(E, key, leader)
    L = fd["S"].shape[1]
    S_lib = library(fd, specs)
    S_flat = S_lib.repeat(1, mask.shape[1] // L)
    logits = parallel_logits(w, enc, S_flat, mask, kinds, hide=hide)
    unit, own = unit_values(logits, S_flat, specs)
    return dict(fd=fd, specs=specs, S_lib=S_lib, S_flat=S_flat, order0=order0, E_idx=E, kinds=kinds, key=key, leader=leader, mask=mask[0], unit=unit,
                own=own, logits=logits, w=w)


def counted_units(case):
    """bool [L]: the leaders of the distinct units that count (mask * chain_mask != 0; chain_mask is all ones)."""
    L = case["fd"]["S"].shape[1]
    counted = torch.zeros(L, dtype=torch.bool)
    counted[torch.as_tensor(case["leader"][:L])] = True
    return counted & (case["mask"][:L] != 0)
