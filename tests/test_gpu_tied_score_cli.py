"""--score_tied on the command line: the keys and shapes of scores/<name>.npz on the tests/golden/cli input with tie
flags, and --score_fasta without the flag, which keeps its file and its refusals."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _setup(tmp_path, golden_dir):
    from na_mpnn_amd import pdbio
    gd = os.path.join(golden_dir, "cli")
    out = os.path.join(str(tmp_path), "out")
    pdb = os.path.join(gd, "input.pdb")
    P = pdbio.parse_pdb(pdb)
    enc = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    common = ["--mode", "design", "--pdb_path", pdb, "--out_folder", out, "--random_init_seed", "0", "--seed", "7"]
    return P, enc, out, common


def test_cli_score_tied(tmp_path, golden_dir):
    """Designs drawn under a symmetry group (three residues of chain A, weights 1 / 0.5 / 0.25) and a base pair are scored with
    --score_tied 1 under the same flags: the keys and shapes of the file, one value per group, the designs consistent, and the file
    equal to the Python call."""
    from na_mpnn_amd import cli, pdbio
    P, enc, out, common = _setup(tmp_path, golden_dir)
    a = [i for i, c in enumerate(P["chain_letters"]) if c == "A"][2:5]
    b = [i for i, c in enumerate(P["chain_letters"]) if c == "B"][-1]
    c = [i for i, c in enumerate(P["chain_letters"]) if c == "C"][0]
    ties = ["--symmetry_residues", ",".join(enc[i] for i in a), "--symmetry_weights", "1.0,0.5,0.25", "--paired_residues", f"{enc[b]}:{enc[c]}"]
    cli.main(common + ties + ["--batch_size", "3", "--output_pdbs", "0"])
    fa = os.path.join(out, "seqs", "input.fa")
    cli.main(common + ties + ["--score_fasta", fa, "--score_tied", "1"])
    z = np.load(os.path.join(out, "scores", "input.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["S", "token_log_probs", "leader", "log_likelihood", "member_log_probs", "consistent", "decoding_order",
                                      "chunks", "state_weights"])
    L = len(P["S"])
    n = z["S"].shape[0]
    assert n == 4 and z["S"].shape == (n, L) and z["token_log_probs"].shape == (n, L) and z["token_log_probs"].dtype == np.float32
    assert z["leader"].shape == (L,) and z["log_likelihood"].shape == (n,) and z["member_log_probs"].shape == (n, 1, L)
    assert z["consistent"].shape == (n,) and z["decoding_order"].shape == (L,) and z["state_weights"].tolist() == [1.0]
    want = np.arange(L); want[a[1]] = want[a[2]] = a[0]; want[c] = b
    assert np.array_equal(z["leader"], want)
    assert bool(z["consistent"][1:].all()) and np.isfinite(z["log_likelihood"][1:]).all()        # the designs satisfy the ties they were drawn under
    for g in (a, [b, c]):
        assert all(np.array_equal(z["token_log_probs"][:, g[0]], z["token_log_probs"][:, r]) for r in g)
    dev = torch.device("cuda:0")
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(True),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    m = m.to(dev).eval()
    fd = pdbio.to_feature_dict(P, np.ones(L, np.int32), dev)              # (no flag fixes a residue: every chain is designed)
    torch.manual_seed(7)
    fd.update(batch_size=1, randn=torch.randn(1, L, device=dev), symmetry_residues=[a], symmetry_weights=[[1.0, 0.5, 0.25]],
              paired_residues=[(b, c)])
    ref = m.score_tied(fd, torch.from_numpy(z["S"]).to(dev))
    assert ref["method"] == "items" and np.array_equal(ref["decoding_order"].cpu().numpy(), z["decoding_order"])
    assert np.array_equal(ref["token_log_probs"].cpu().numpy(), z["token_log_probs"])
    assert np.array_equal(ref["log_likelihood"].cpu().numpy(), z["log_likelihood"])
    with pytest.raises(ValueError, match="score_fasta"):
        cli.main(common + ["--score_tied", "1"])


def test_cli_score_fasta_without_the_flag_is_unchanged(tmp_path, golden_dir):
    """Without --score_tied the file of --score_fasta keeps its keys and holds the bits of score_sequences, and the tie flags stay refused."""
    from na_mpnn_amd import cli, pdbio
    P, enc, out, common = _setup(tmp_path, golden_dir)
    cli.main(common + ["--batch_size", "2", "--output_pdbs", "0"])
    fa = os.path.join(out, "seqs", "input.fa")
    cli.main(common + ["--score_fasta", fa])
    z = np.load(os.path.join(out, "scores", "input.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["token_log_probs", "loss", "sequences", "mask", "chain_mask", "decoding_order", "seed"])
    L = len(P["S"])
    dev = torch.device("cuda:0")
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(True),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    m = m.to(dev).eval()
    fd = pdbio.to_feature_dict(P, z["chain_mask"], dev)
    fd["batch_size"] = 1
    torch.manual_seed(7)
    fd["randn"] = torch.randn(1, L, device=dev)
    ref = m.score_sequences(fd, torch.from_numpy(z["sequences"]).to(dev))
    assert np.array_equal(ref["token_log_probs"].cpu().numpy(), z["token_log_probs"]) and np.array_equal(ref["loss"].cpu().numpy(), z["loss"])
    b = [i for i, c in enumerate(P["chain_letters"]) if c == "B"][-1]
    c = [i for i, c in enumerate(P["chain_letters"]) if c == "C"][0]
    with pytest.raises(ValueError, match="score_fasta"):
        cli.main(common + ["--score_fasta", fa, "--paired_residues", f"{enc[b]}:{enc[c]}"])
