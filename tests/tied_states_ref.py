"""Reference of tied-states sampling (ProteinMPNN.sample with feature_dict["state_weights"]) built from the unchanged CPU oracle:
every state is decoded by oracle.cpu_ref.sample / sample_symmetric on that state alone, teacher-forced with the one sequence, with
row 0 of `randn` repeated (the one decoding order), and the tied distribution is recombined from the per-state log-probs —

    softmax((sum_m w_m logits_m + bias) / T) == softmax((sum_m w_m log_softmax(logits_m) + bias) / T)

because log_softmax differs from the logits by one constant per row — with the special tokens zeroed and the rest renormalised."""
import numpy as np
import torch

from oracle import cpu_ref

SHARED = ("S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")


def make_states(cx, M, seed, amplitude=2.0, jitter=0.15):
    """X [M, L, A, 3]: state 0 is the complex itself; every other state is a seeded smooth deformation of it (a few low-frequency
    sine waves of the coordinates, up to `amplitude` Angstrom each, so that neighbour lists change) plus Gaussian jitter.  Absent
    atoms stay zero."""
    rng = np.random.default_rng(seed)
    X, X_m = cx["X"].astype(np.float64), cx["X_m"]
    out = [cx["X"].astype(np.float32)]
    scale = max(1.0, float(np.abs(X).max()))
    for _ in range(1, M):
        D = np.zeros_like(X)
        for _w in range(3):
            kvec = rng.standard_normal(3) * (2.5 / scale)
            amp = rng.standard_normal(3) * amplitude
            D += np.sin(X @ kvec + rng.uniform(0, 2 * np.pi))[..., None] * amp
        Y = X + D + jitter * rng.standard_normal(X.shape)
        out.append((Y * X_m[:, :, None]).astype(np.float32))
    return np.stack(out)


def states_fd(cx, Xs, weights, bs, T, randn, bias=None, sym=None):
    """CPU feature_dict of the tied-states call: X / X_m [M, L, ...], every other per-residue entry [1, L]."""
    M, L = Xs.shape[:2]
    fd = {k: torch.from_numpy(np.ascontiguousarray(cx[k]))[None] for k in SHARED}
    fd["X"] = torch.from_numpy(np.ascontiguousarray(Xs))
    fd["X_m"] = torch.from_numpy(np.ascontiguousarray(cx["X_m"]))[None].repeat(M, 1, 1)
    fd.update({"batch_size": bs, "temperature": T, "bias": torch.zeros(1, L, 33) if bias is None else bias,
               "symmetry_residues": sym[0] if sym else [[]], "symmetry_weights": sym[1] if sym else [[]],
               "randn": torch.as_tensor(randn, dtype=torch.float32), "state_weights": [float(v) for v in weights]})
    return fd


def state_fd(fd, m):
    """The feature_dict of state m alone (a plain sample() / score() input): row 0 of randn for every stream."""
    out = {k: v for k, v in fd.items() if k != "state_weights"}
    out["X"], out["X_m"] = fd["X"][m:m + 1], fd["X_m"][m:m + 1]
    out["randn"] = fd["randn"][:1].repeat(fd["batch_size"], 1)
    return out


def to_dev(fd, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def tied_probs(log_probs, fd, groups=None, group_weights=None):
    """log_probs [bs, M, L, V] (per state, teacher-forced) -> the tied sampling distribution [bs, L, V] on designable residues, zero
    elsewhere.  groups / group_weights: symmetry groups (all members designable) whose members share one distribution, with the bias
    of the LAST member (model_utils.py:300)."""
    w = torch.tensor(fd["state_weights"], dtype=torch.float64)
    lp = log_probs.double()
    z = (w[None, :, None, None] * lp).sum(1)                                    # [bs, L, V]
    bias = fd["bias"].double().expand(1, z.shape[1], z.shape[2])
    zt = z + bias
    for g, gw in zip(groups or [], group_weights or []):
        tot = sum(float(gw_i) * z[:, i] for i, gw_i in zip(g, gw)) + bias[:, g[-1]]
        for i in g:
            zt[:, i] = tot
    p = torch.softmax(zt / fd["temperature"], -1)
    for tok in cpu_ref.SPECIAL_TOKENS:
        p[..., tok] = 0
    p = p / p.sum(-1, keepdim=True)
    cm = (fd["mask"] * fd["chain_mask"]).double()[0]
    return (p * cm[None, :, None]).float()


def oracle_tied(weights_t, fd, K, S):
    """The per-state oracle teacher-forced with the one sequence S [bs, L] -> (log_probs [bs, M, L, V], tied probabilities [bs, L, V],
    decoding order [bs, L] as the oracle visits the residues)."""
    M = fd["X"].shape[0]
    sym = fd["symmetry_residues"]
    symmetric = not (len(sym) == 1 and len(sym[0]) == 0)
    cm = (fd["mask"] * fd["chain_mask"])[0]
    lps, order = [], None
    for m in range(M):
        fdm = state_fd(fd, m)
        if symmetric:
            assert all(bool(cm[i]) for g in sym for i in g), "the helper takes only groups whose members are all designable"
            ref = cpu_ref.sample_symmetric(weights_t, fdm, K, S_forced=S)
        else:
            ref = cpu_ref.sample(weights_t, fdm, K, S_forced=S)
        assert torch.equal(ref["S"], S)
        lps.append(ref["log_probs"])
        order = ref["decoding_order"]
    lp = torch.stack(lps, 1)
    return lp, tied_probs(lp, fd, sym if symmetric else None, fd["symmetry_weights"] if symmetric else None), order


def write_multimodel(path, src_pdb, M, seed, fmt="pdb", drop_last_residue_of_model=None):
    """A multi-model file made from a single-model one: `src_pdb` parsed, deformed per state (make_states) and written per state with
    pdbio.write_pdb between MODEL / ENDMDL lines (fmt "pdb"), or as one mmCIF `_atom_site` loop with M model numbers (fmt "cif").
    drop_last_residue_of_model: that model (1-based) loses its last residue — a file parse_states must refuse.  Returns X [M, L, 16, 3]."""
    import os
    from na_mpnn_amd import pdbio
    P = pdbio.parse_pdb(src_pdb)
    names = {}
    for a in pdbio.read_atoms(src_pdb):
        names.setdefault((a.chain, a.resnum, a.icode), a.resname)
    resnames = [names[k] for k in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    Xs = make_states(P, M, seed)
    tmp = str(path) + ".state"
    body = []
    for m in range(M):
        n = len(resnames) - (1 if drop_last_residue_of_model == m + 1 else 0)
        args = (Xs[m][:n], P["X_m"][:n], resnames[:n], P["chain_letters"][:n], P["R_idx"][:n], P["icodes"][:n])
        if fmt == "pdb":
            pdbio.write_pdb(tmp, *args)
            body += ["MODEL     %4d" % (m + 1)] + [l for l in open(tmp).read().splitlines() if l != "END"] + ["ENDMDL"]
        else:
            pdbio.write_mmcif(tmp, *args)
            lines = open(tmp).read().splitlines()
            head = [l for l in lines if not l.startswith("ATOM")][:-1]
            rows = [l.rsplit(" ", 1)[0] + " %d" % (m + 1) for l in lines if l.startswith("ATOM")]
            body = (head if m == 0 else body) + rows
    os.remove(tmp)
    with open(path, "w") as fh:
        fh.write("\n".join(body + (["END"] if fmt == "pdb" else ["#"])) + "\n")
    return Xs
