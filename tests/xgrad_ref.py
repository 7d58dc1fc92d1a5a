"""Reference for the coordinate gradients of the edge featuriser.  Helper only (no tests in this file).

Two independent evaluations of dL/dX through y = Wedge . [E_pos | RBF] on GIVEN neighbour lists (the lists are constants):
  * the dense torch formulation (as tests/test_gpu_train.py::test_feature_weight_gradient writes it), differentiated by autograd in
    whatever dtype its inputs have — fp64 in the tests;
  * the closed form of the issue in numpy fp64:
        u[a,b,r] = sum_o g[o] Wedge[o][16 (1 + A a + b) + r],     s_ab = sum_r u[a,b,r] (-2 (D_ab - mu_r) / sigma^2) R(a,b,r),
        dX18[i,a] += s_ab (X18[i,a] - X18[j,b]) / D_ab,           dX18[j,b] -= the same.
A = 18 atoms (16 + virtual Cb + virtual N_na), or 17 for a weight of a model without the virtual N_na atom ([128 x 4640]).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import cpu_ref

SIGMA = 1.25
NUM_RBF = 16


def n_atoms_of(W):
    a = int(round(((W.shape[1] - 16) / 16) ** 0.5))
    assert 16 + 16 * a * a == W.shape[1], W.shape
    return a


def atom_frames(X, fd, n_atoms=18):
    """X [B,L,16,3] -> X18 [B,L,A,3] (16 atoms + Cb + N_na) and M18 [B,L,A], as oracle/cpu_ref.py::features builds them."""
    A = cpu_ref.ATOM
    Cb = cpu_ref._virtual_atom(X[:, :, A["N"]], X[:, :, A["CA"]], X[:, :, A["C"]], -0.58273431, 0.56802827, -0.54067466)
    Nna = cpu_ref._virtual_atom(X[:, :, A["O4'"]], X[:, :, A["C1'"]], X[:, :, A["C2'"]], -0.56967352, 0.51055973, -0.53122153)
    X18 = torch.cat((X, Cb[:, :, None], Nna[:, :, None]), -2)
    M18 = torch.cat((fd["X_m"], fd["protein_mask"][:, :, None], (fd["rna_mask"] + fd["dna_mask"])[:, :, None]), -1).to(X.dtype)
    return X18[:, :, :n_atoms], M18[:, :, :n_atoms]


def rbf_rows(W, X18, M18, E_idx):
    """The RBF part of the pre-LayerNorm edge embedding, dense: [B,L,K,128]."""
    B, L, A = X18.shape[:3]
    j = E_idx.long()
    bidx = torch.arange(B)[:, None, None]
    Xj, Mj = X18[bidx, j], M18[bidx, j]                       # [B,L,K,A,3], [B,L,K,A]
    D = torch.sqrt(((X18[:, :, None, :, None, :] - Xj[:, :, :, None, :, :]) ** 2).sum(-1) + 1e-6)
    mu = torch.linspace(2., 22., NUM_RBF, dtype=X18.dtype)
    rbf = torch.exp(-(((D[..., None] - mu) / SIGMA) ** 2)) * M18[:, :, None, :, None, None] * Mj[:, :, :, None, :, None]
    return rbf.reshape(B, L, j.shape[2], -1) @ W[:, 16:].to(X18.dtype).t()


def pos_rows(W, pos_w, pos_b, fd, E_idx):
    """The positional part (independent of the coordinates): [B,L,K,128]."""
    B = E_idx.shape[0]
    j = E_idx.long()
    bidx = torch.arange(B)[:, None, None]
    R_idx, ch = fd["R_idx"].long(), fd["chain_labels"].long()
    same = (ch[:, :, None] == ch[bidx, j]).long()
    d = torch.clip(R_idx[:, :, None] - R_idx[bidx, j] + 32, 0, 64) * same + (1 - same) * 65
    return (pos_w.t()[d] + pos_b) @ W[:, :16].t()


def dX_autograd(W, X, fd, E_idx, g):
    """d sum(g * y) / dX [B,L,16,3] by autograd through atom_frames and rbf_rows, in X's dtype."""
    Xr = X.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        X18, M18 = atom_frames(Xr, fd, n_atoms_of(W))
        (rbf_rows(W, X18, M18, E_idx) * g).sum().backward()
    return Xr.grad


def dX18_autograd(W, X18, M18, E_idx, g):
    Xr = X18.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (rbf_rows(W, Xr, M18, E_idx) * g).sum().backward()
    return Xr.grad


def dX18_closed_form(W, X18, M18, E_idx, g):
    """The issue's formulas, numpy fp64, complex by complex -> [B,L,A,3]."""
    W, X18, M18, g = (np.asarray(t, dtype=np.float64) for t in (W, X18, M18, g))
    E_idx = np.asarray(E_idx).astype(np.int64)
    B, L, A = X18.shape[:3]
    K = E_idx.shape[2]
    Wr = W[:, 16:].reshape(W.shape[0], A, A, NUM_RBF)
    mu = 2.0 + np.arange(NUM_RBF) * (20.0 / 15.0)
    out = np.zeros_like(X18)
    for b in range(B):
        j = E_idx[b]                                              # [L,K]
        diff = X18[b][:, None, :, None, :] - X18[b][j][:, :, None, :, :]        # [L,K,A,A,3]
        D = np.sqrt((diff ** 2).sum(-1) + 1e-6)
        R = np.exp(-(((D[..., None] - mu) / SIGMA) ** 2)) * M18[b][:, None, :, None, None] * M18[b][j][:, :, None, :, None]
        u = np.einsum("iko,oabr->ikabr", g[b], Wr)
        s = (u * (-2.0 * (D[..., None] - mu) / SIGMA ** 2) * R).sum(-1)           # [L,K,A,A]
        v = s[..., None] * diff / D[..., None]
        out[b] += v.sum(axis=(1, 3))                              # dX18[i,a]: over k and b
        np.subtract.at(out[b], j.reshape(-1), v.sum(axis=2).reshape(L * K, A, 3))  # dX18[j,b]: over a
    return out


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))
