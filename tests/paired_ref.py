"""Reference of base-paired design (ProteinMPNN.sample with feature_dict["paired_residues"] / "symmetry_token_maps") built from the
unchanged CPU oracle: oracle.cpu_ref.sample_symmetric runs with the mapped groups as plain symmetry groups, teacher-forced per member
with the sampled tokens (its S_forced is per member, so complementary tokens are fine) — that gives every residue's log_probs under the
same visit order — and the paired distribution is recombined from those rows,

    total[a] = sum_j w_j * log_probs_j[P_j[a]] + bias_c[P_c[a]],   p = softmax(total / T),   probs_j[P_j[a]] = p[a]

(c the last listed member), which equals the distribution of the logits' sum because log_softmax differs from the logits by one
constant per member; special tokens are zeroed and the rest renormalised."""
import numpy as np
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import mapped_groups
from oracle import cpu_ref

PER_RESIDUE = ("X", "X_m", "S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")


def special_tokens(rti):
    return tuple(sorted({int(rti[n]) for n in spec.SPECIAL_RESTYPES}))


def make_case(L, bs, T, n_pairs, seed, masked_frac=0.0, shared=False, want_cross=False, fixed_every=9):
    """(cx, fd, pairs): a synth.make_complex complex (40 % protein, 30 % DNA, 30 % RNA; re-chained into five chains) as a CPU feature_dict with
    `n_pairs` pairs of nucleic-acid residues of DIFFERENT chains, chosen by a seeded generator; want_cross: the first pair is a DNA
    residue with an RNA residue.  shared: the tokens of restype_to_int(na_shared_tokens=True) (RNA residues hold the DNA ids)."""
    cx = synth.make_complex(seed=seed, n=L, n_chains=4, frac_protein=0.4, frac_dna=0.3, masked_frac=masked_frac)
    # five chains: the protein, two DNA strands and two RNA strands (the generator's own chain breaks may leave one strand per polymer)
    n_prot, n_dna = int(round(0.4 * L)), int(round(0.3 * L))
    bounds = [n_prot, n_prot + n_dna // 2, n_prot + n_dna, n_prot + n_dna + (L - n_prot - n_dna) // 2]
    cx["chain_labels"] = np.searchsorted(bounds, np.arange(L), side="right").astype(np.int32)
    for c in range(5):
        sel = cx["chain_labels"] == c
        cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    if fixed_every:
        cx["chain_mask"][::fixed_every] = 0
    if shared:
        cx["S"] = np.where(cx["rna_mask"] == 1, cx["S"] - 5, cx["S"]).astype(np.int32)
    rng = np.random.default_rng(seed + 17)
    design = cx["mask"] * cx["chain_mask"]
    na_all = [i for i in range(L) if not cx["protein_mask"][i]]
    na = [i for i in range(L) if not cx["protein_mask"][i] and cx["mask"][i]]     # (a masked residue has no oracle log-probs to recombine)
    pairs, used = [], set()
    tries = 0
    while len(pairs) < n_pairs and tries < 100000:
        tries += 1
        i, j = (int(v) for v in rng.choice(na, 2, replace=False))
        if i in used or j in used or cx["chain_labels"][i] == cx["chain_labels"][j]:
            continue
        if want_cross and not pairs and cx["dna_mask"][i] == cx["dna_mask"][j]:
            continue
        if not (design[i] or design[j]):                                     # (both fixed: allowed, but nothing is tied)
            continue
        pairs.append((i, j)); used.update((i, j))
    assert len(pairs) == n_pairs, "the complex has too few nucleic-acid residues on different chains"
    fd = {k: torch.from_numpy(np.ascontiguousarray(cx[k]))[None] for k in PER_RESIDUE}
    # synthetic weights know no chemistry: the bias keeps a DNA residue on the DNA bases and an RNA residue on the RNA bases (what a
    # trained model does by itself), so that a pair of drawn tokens can be a canonical base pair at all
    rti = spec.restype_to_int(shared)
    bias = torch.zeros(1, L, 33)
    for i in na_all:
        allowed = [rti[n] for n in (("DA", "DC", "DG", "DT") if cx["dna_mask"][i] else ("A", "C", "G", "U"))]
        bias[0, i] = -1e8
        bias[0, i, allowed] = 0.0
    fd.update({"batch_size": bs, "temperature": T, "bias": bias, "symmetry_residues": [[]], "symmetry_weights": [[]],
               "randn": torch.from_numpy(np.random.default_rng(seed + 3).standard_normal((bs, L)).astype(np.float32)),
               "paired_residues": pairs})
    return cx, fd, pairs


def groups_of(fd, rti):
    """The mapped groups of a CPU feature_dict as the model builds them: (groups, weights, maps)."""
    L = fd["S"].shape[1]
    pairs = fd.get("paired_residues")
    polymer = [1 if d else (2 if r else 0) for d, r in zip(fd["dna_mask"][0].tolist(), fd["rna_mask"][0].tolist())]
    fixed = [not v for v in (fd["mask"] * fd["chain_mask"])[0].tolist()]
    g, w, m, _ = mapped_groups(L, rti, pairs, fd.get("paired_weights"), polymer if pairs else None, fixed if pairs else None,
                               fd.get("symmetry_residues"), fd.get("symmetry_weights"), fd.get("symmetry_token_maps"))
    return g, w, m


def paired_probs(log_probs, fd, groups, weights, maps, special=cpu_ref.SPECIAL_TOKENS, state_weights=None):
    """log_probs [bs, L, V] (or [bs, M, L, V] with state_weights [M]), teacher-forced per residue -> the sampling distribution of every
    residue in its own alphabet [bs, L, V], zero where mask * chain_mask is zero."""
    lp = log_probs.double()
    if lp.dim() == 3:
        lp = lp[:, None]
    sw = torch.ones(lp.shape[1], dtype=torch.float64) if state_weights is None else torch.tensor(state_weights, dtype=torch.float64)
    bs, M, L, V = lp.shape
    T = fd["temperature"]
    bias = fd["bias"].double().expand(1, L, V)

    def dist(total):
        p = torch.softmax(total / T, -1)
        for tok in special:
            p[..., tok] = 0
        return p / p.sum(-1, keepdim=True)

    out = dist((sw[None, :, None, None] * lp).sum(1) + bias)
    for g, gw, gm in zip(groups, weights, maps):
        total = torch.zeros(bs, V, dtype=torch.float64)
        for m in range(M):
            for j, w_j, P_j in zip(g, gw, gm):
                total = total + float(sw[m]) * float(w_j) * lp[:, m, j][:, P_j]
        total = total + bias[:, g[-1]][:, gm[-1]]
        p = dist(total)
        for j, P_j in zip(g, gm):
            row = torch.zeros_like(p)
            row[:, P_j] = p                                                   # row[P_j[a]] = p[a]
            out[:, j] = row
    cm = (fd["mask"] * fd["chain_mask"]).double()[0]
    return (out * cm[None, :, None]).float()


def oracle_paired(weights_t, fd, K, S, rti, special=cpu_ref.SPECIAL_TOKENS):
    """The oracle teacher-forced with S [bs, L] on the mapped groups -> (log_probs [bs, L, V], paired probabilities [bs, L, V],
    the oracle's decoding order [bs, L], (groups, weights, maps), the log_probs with the rows of fixed group members kept)."""
    groups, weights, maps = groups_of(fd, rti)
    fdo = {k: v for k, v in fd.items() if k not in ("paired_residues", "paired_weights", "symmetry_token_maps")}
    fdo["symmetry_residues"], fdo["symmetry_weights"] = (groups, weights) if groups else ([[]], [[]])
    fdo["randn"] = fd["randn"][:1].repeat(fd["batch_size"], 1)
    ref = cpu_ref.sample_symmetric(weights_t, fdo, K, special=special, S_forced=S)
    assert torch.equal(ref["S"], S), "S does not keep the fixed residues' tokens"
    lp = ref["log_probs"]
    cm = (fd["mask"] * fd["chain_mask"])[0]
    if any(not bool(cm[i]) for g in groups for i in g):
        # The oracle zeroes the log_probs row of a fixed residue, but a fixed member's logits count in its group's sum.  A second pass with
        # every unmasked residue designable — teacher-forced with the same S (masked residues hold S_true in it), in the same decoding order (a randn whose sort is that order) —
        # computes the same logits and keeps those rows.
        base = cpu_ref.decoding_order_of(cm[None], fd["randn"][:1])[0]
        randn2 = torch.empty(len(base)); randn2[base] = torch.arange(1, len(base) + 1, dtype=torch.float32)
        randn2 = torch.where(fd["mask"][0].bool(), randn2, randn2 * 1e4)      # (a masked residue's sort key is 1e-4 |randn|: t + 1 again)
        fd2 = dict(fdo, chain_mask=torch.ones_like(fd["chain_mask"]), randn=randn2[None].repeat(fd["batch_size"], 1))
        full = cpu_ref.sample_symmetric(weights_t, fd2, K, special=special, S_forced=S)
        assert torch.equal(full["decoding_order"], ref["decoding_order"])
        assert torch.allclose(full["log_probs"] * cm[None, :, None], lp, rtol=0, atol=1e-6)
        lp_groups = full["log_probs"]
    else:
        lp_groups = lp
    return lp, paired_probs(lp_groups, fd, groups, weights, maps, special), ref["decoding_order"], (groups, weights, maps), lp_groups


def to_dev(fd, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}
