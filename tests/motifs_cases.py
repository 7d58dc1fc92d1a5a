"""The cases the forbidden-motif tests share between the CPU premises (test_motifs_host.py) and the GPU tests (test_gpu_motifs.py)."""
import numpy as np
import torch

from na_mpnn_amd import spec, synth
import paired_ref

V = 33
RTI = spec.restype_to_int()
A_, R_ = RTI["ALA"], RTI["ARG"]
# lengths 3, 5 and 8 over two tokens: under a +6 bias on both a free design is a random word over {A, R} and holds them
PLAIN_MOTIFS = [(A_, A_, A_), (A_, R_, A_, R_, A_), (R_, R_, A_, A_, R_, R_, A_, A_)]
NA_HOMOPOLYMERS = [(RTI[n],) * 3 for n in ("DA", "DC", "DG", "DT", "A", "C", "G", "U")]


def fd_of(cx, bs, T, seed):
    L = cx["S"].shape[0]
    fd = {k: torch.from_numpy(np.ascontiguousarray(cx[k]))[None] for k in paired_ref.PER_RESIDUE}
    fd.update({"batch_size": bs, "temperature": T, "bias": torch.zeros(1, L, V), "symmetry_residues": [[]], "symmetry_weights": [[]],
               "randn": torch.from_numpy(np.random.default_rng(seed).standard_normal((bs, L)).astype(np.float32))})
    return fd


def two_chain_complex(seed, L, split, gap_at=None):
    """An all-designable, all-present complex of two chains [0, split) and [split, L) with R_idx counting from 0 in each; gap_at: the
    numbering jumps by 3 in front of that residue (no chain break)."""
    cx = synth.make_complex(seed=seed, n=L, n_chains=2)
    cx["mask"][:] = 1
    cx["chain_mask"][:] = 1
    cx["chain_labels"] = (np.arange(L) >= split).astype(np.int32)
    cx["R_idx"] = np.where(np.arange(L) < split, np.arange(L), np.arange(L) - split).astype(np.int32)
    if gap_at is not None:
        same = cx["chain_labels"] == cx["chain_labels"][gap_at]
        cx["R_idx"][(np.arange(L) >= gap_at) & same] += 3
    return cx


def plain_case(L=40, bs=3, T=1.0, seed=4100):
    """L = 40, two chains (22 + 18) and one R_idx gap in front of residue 10, +6 on ALA and ARG everywhere -> (cx, fd, motifs)."""
    cx = two_chain_complex(seed, L, min(22, L // 2 + 1), gap_at=min(10, L // 3))
    fd = fd_of(cx, bs, T, seed + 1)
    fd["bias"][:, :, [A_, R_]] = 6.0
    return cx, fd, list(PLAIN_MOTIFS)


def most_banned_at_once(motifs):
    """An upper bound of the candidates ONE draw of an untied residue can lose: the distinct tokens over all motifs."""
    return len({t for m in motifs for t in m})
