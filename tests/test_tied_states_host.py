"""Host-side tests of multi-state design (one sequence tied across backbone states): the yardstick itself — the unchanged CPU oracle's
symmetric sampler on the block-diagonal flattened graph equals the per-state definition —, the multi-model readers of pdbio and the
argument checks of ProteinMPNN.sample that need no device."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import pdbio, spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
from tied_states_ref import make_states, oracle_tied, state_fd, states_fd, write_multimodel

torch.set_grad_enabled(False)


@pytest.mark.parametrize("n,K,M,bs,T", [(40, 16, 3, 2, 0.5), (30, 48, 2, 2, 1.0), (60, 24, 4, 1, 0.3)])
def test_flattened_oracle_equals_the_per_state_definition(weights_np, monkeypatch, n, K, M, bs, T):
    """oracle.cpu_ref.sample_symmetric on the flattened graph (h_V / h_E of the M states side by side, neighbour lists E_idx[m] + m L,
    groups {i, L + i, ...} with the state weights; cpu_ref.encode swapped for those encoder outputs) draws ONE sequence for all states,
    and — teacher-forced per state by cpu_ref.sample with that sequence — the per-state log-probs and the tied probabilities agree.
    Bounds: both sides evaluate the same fp32 expressions on differently shaped batches, so only summation order inside the CPU GEMMs
    may differ: 1e-5 on log-probs (|logp| < 20, a few hundred fp32 roundings of 6e-8 relative), 5e-6 on probabilities (<= 1, sharpened
    by sum |w| / T <= 4)."""
    w = cpu_ref.to_torch(weights_np)
    cx = synth.make_complex(seed=1200 + n, n=n)
    cx["chain_mask"][::8] = 0
    rng = np.random.default_rng(n)
    wts = rng.uniform(0.5, 1.5, M)
    wts = wts / wts.sum()
    fd = states_fd(cx, make_states(cx, M, seed=n + M), wts, bs, T, rng.standard_normal((bs, n)).astype(np.float32))
    enc = [cpu_ref.encode(w, state_fd(fd, m), K) for m in range(M)]
    assert any(not torch.equal(enc[0][2], e[2]) for e in enc[1:])                  # the states' neighbour lists differ
    flat = (torch.cat([e[0] for e in enc], 1), torch.cat([e[1] for e in enc], 1), torch.cat([e[2] + m * n for m, e in enumerate(enc)], 1))
    fdf = {"batch_size": bs, "temperature": T, "S": fd["S"].repeat(1, M), "mask": fd["mask"].repeat(1, M),
           "chain_mask": fd["chain_mask"].repeat(1, M), "bias": fd["bias"].repeat(1, M, 1), "randn": fd["randn"][:1].repeat(1, M),
           "symmetry_residues": [[i + m * n for m in range(M)] for i in range(n)], "symmetry_weights": [list(wts)] * n}
    monkeypatch.setattr(cpu_ref, "encode", lambda w_, fd_, k_, **kw: flat)
    torch.manual_seed(3)
    out = cpu_ref.sample_symmetric(w, fdf, K)
    monkeypatch.undo()
    S = out["S"].view(bs, M, n)
    assert all(torch.equal(S[:, 0], S[:, m]) for m in range(1, M))
    cm = (fd["mask"] * fd["chain_mask"])[0].bool()
    assert torch.equal(S[:, 0][:, ~cm], fd["S"][:, ~cm].long().expand(bs, -1))
    lp, probs, _ = oracle_tied(w, fd, K, S[:, 0])
    d_lp = float((out["log_probs"].view(bs, M, n, 33) - lp).abs().max())
    d_p = float((out["sampling_probs"].view(bs, M, n, 33)[:, 0] - probs).abs().max())
    print(f"flattened oracle n={n} K={K} M={M}: max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}")
    assert d_lp <= 1e-5 and d_p <= 5e-6


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli", "input.pdb")


def test_model_ids_and_parse_states_pdb(tmp_path):
    path = os.path.join(str(tmp_path), "ens.pdb")
    Xs = write_multimodel(path, GOLD, 3, seed=5)
    assert pdbio.model_ids(path) == [1, 2, 3] and pdbio.model_ids(GOLD) == [1]
    P0 = pdbio.parse_pdb(GOLD)
    P = pdbio.parse_states(path)
    assert P["model_ids"] == [1, 2, 3]
    assert P["X"].shape == (3,) + P0["X"].shape and P["X_m"].shape == (3,) + P0["X_m"].shape
    assert np.abs(P["X"] - Xs).max() < 1e-3 and all(np.array_equal(P["X_m"][m], P0["X_m"]) for m in range(3))
    assert np.abs(P["X"][0] - P["X"][1]).max() > 0.1                       # the states differ
    for k in ("S", "mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type"):
        assert np.array_equal(P[k], P0[k]), k
    assert P["chain_letters"] == P0["chain_letters"] and P["icodes"] == P0["icodes"]
    # the default still reads model 1; model= selects
    D = pdbio.parse_pdb(path)
    assert np.array_equal(D["X"], P["X"][0]) and np.array_equal(D["X"], pdbio.parse_pdb(path, model=1)["X"])
    assert np.array_equal(pdbio.parse_pdb(path, model=3)["X"], P["X"][2])
    n1 = sum(1 for _ in pdbio.read_atoms(path))
    assert n1 == sum(1 for _ in pdbio.read_atoms(path, model=2)) == int(P0["X_m"].sum())
    with pytest.raises(ValueError):
        pdbio.parse_pdb(path, model=7)


def test_parse_states_mmcif(tmp_path):
    path = os.path.join(str(tmp_path), "ens.cif")
    Xs = write_multimodel(path, GOLD, 2, seed=6, fmt="cif")
    assert pdbio.model_ids(path) == [1, 2]
    P = pdbio.parse_states(path)
    assert P["X"].shape[0] == 2 and np.abs(P["X"] - Xs).max() < 1e-3
    assert np.array_equal(pdbio.parse_pdb(path)["X"], P["X"][0]) and np.array_equal(pdbio.parse_pdb(path, model=2)["X"], P["X"][1])
    assert np.array_equal(P["S"], pdbio.parse_pdb(GOLD)["S"])


def test_parse_states_refuses_models_with_different_residues(tmp_path):
    path = os.path.join(str(tmp_path), "bad.pdb")
    write_multimodel(path, GOLD, 3, seed=7, drop_last_residue_of_model=2)
    with pytest.raises(ValueError, match="model 2"):
        pdbio.parse_states(path)
    assert len(pdbio.parse_pdb(path, model=2)["S"]) == len(pdbio.parse_pdb(path)["S"]) - 1


def _cpu_model(k=16):
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int()).eval()


def test_sample_argument_checks_with_states():
    """What sample() refuses with state_weights, before it touches a device."""
    n, M, bs = 20, 2, 2
    cx = synth.make_complex(seed=3, n=n)
    good = lambda: states_fd(cx, make_states(cx, M, 1), [0.5, 0.5], bs, 0.5, np.zeros((bs, n), np.float32))
    m = _cpu_model()
    fd = good(); fd["state_weights"] = [1.0, 1.0, 1.0]                     # three weights, two states
    with pytest.raises(ValueError, match="state_weights"):
        m.sample(fd)
    fd = good(); fd["X"] = fd["X"][0]                                      # no state dimension
    with pytest.raises(ValueError):
        m.sample(fd)
    fd = good(); fd["X_m"] = fd["X_m"][:1]
    with pytest.raises(ValueError, match="X_m"):
        m.sample(fd)
    for k in ("S", "mask", "chain_mask", "R_idx", "R_polymer_type"):
        fd = good(); fd[k] = fd[k].repeat(M, 1)                            # a shared entry given per state
        with pytest.raises(ValueError, match=k):
            m.sample(fd)
    fd = good(); fd["randn"] = fd["randn"][:1]
    with pytest.raises(ValueError, match="randn"):
        m.sample(fd)
    fd = good(); fd["S_forced"] = torch.zeros(1, n, dtype=torch.int64)
    with pytest.raises(ValueError, match="S_forced"):
        m.sample(fd)
    fd = good(); fd["bias"] = torch.zeros(M, n, 33)
    with pytest.raises(ValueError, match="bias"):
        m.sample(fd)
    fd = good(); fd["pair_bias"] = torch.zeros(1, n, 33, n, 33)
    with pytest.raises(NotImplementedError):
        m.sample(fd)
    big = 8001                                                             # 2 x 8001 residues: beyond the level lists' 16000
    fd = good()
    for k in list(fd):
        if isinstance(fd[k], torch.Tensor) and fd[k].dim() >= 2 and fd[k].shape[1] == n:
            fd[k] = torch.zeros((fd[k].shape[0], big) + tuple(fd[k].shape[2:]), dtype=fd[k].dtype)
    with pytest.raises(ValueError, match="16000"):
        m.sample(fd)
    with pytest.raises(RuntimeError, match="HIP device"):                  # well-formed input on the CPU: there is no CPU path
        m.sample(good())
