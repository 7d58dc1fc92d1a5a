"""The CLI's specificity scan: --mutation_scan 1 --multi_state 1 --state_contexts 1 on a two-MODEL file (model 2: a renamed base and no
second strand, written with context_states_ref.write_models) writes mutations/<name>.npz with what ProteinMPNN.score_mutations returns
for the same feature_dict, bit for bit."""
import os

import numpy as np
import pytest
import torch

import real_structures
from context_states_ref import model_of, write_models
from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"


def test_cli_state_scan(tmp_path):
    from na_mpnn_amd import cli, pdbio
    cx = real_structures.variant("1am9_crop")
    letters = [real_structures.chain_letters("1am9")[i] for i in real_structures.rows_of_chains("1am9", real_structures.CROP_CHAINS)]
    names = [spec.RESTYPES[int(t)] for t in cx["S"]]
    rows = np.r_[0:12, 21:33, 38:68]
    keep = np.r_[0:12, 38:68]
    other = "DG" if names[5] != "DG" else "DA"
    path = os.path.join(str(tmp_path), "ctx.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(cx, names, letters, keep, rename={5: other})])
    out_dir = os.path.join(str(tmp_path), "out")
    cli.main(["--mode", "design", "--pdb_path", path, "--out_folder", out_dir, "--random_init_seed", "0", "--seed", "11", "--chains_to_design", "A",
              "--multi_state", "1", "--state_contexts", "1", "--state_weights", "1,-0.5", "--mutation_scan", "1"])
    z = np.load(os.path.join(out_dir, "mutations", "ctx.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["residues", "tokens", "delta", "base_loss", "wild_type_token", "site_rows", "state_delta", "state_weights",
                                      "base_state_log_likelihood"])
    P = pdbio.parse_states(path, contexts=True)
    L = len(P["S"])
    assert L == len(rows) and not P["state_mask"][1, 12:24].any() and P["state_S"][1, 5] != P["state_S"][0, 5]
    chain_mask = np.array([int(c == "A") for c in P["chain_letters"]], np.int32)
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in synth.make_weights(0).items()})
    m = m.to(DEV).eval()
    fd = pdbio.to_feature_dict(dict(P, X=P["X"][0], X_m=P["X_m"][0]), chain_mask, DEV)
    fd.update({"X": torch.as_tensor(P["X"], device=DEV), "X_m": torch.as_tensor(P["X_m"], dtype=torch.int32, device=DEV),
               "state_weights": [1.0, -0.5], "state_S": torch.as_tensor(P["state_S"], dtype=torch.int64, device=DEV),
               "state_mask": torch.as_tensor(P["state_mask"], dtype=torch.int32, device=DEV), "batch_size": 1})
    torch.manual_seed(11)
    fd["randn"] = torch.randn(1, L, device=DEV)
    out = m.score_mutations(fd)
    n_pos, n = len(out["positions"]), len(out["delta_log_likelihood"])
    assert n_pos == int(((P["mask"] * chain_mask) != 0).sum()) > 0
    assert z["delta"].shape == (n_pos, len(out["tokens"])) and z["state_delta"].shape == (n, 2) and z["state_delta"].dtype == np.float32
    assert np.array_equal(z["delta"], out["delta"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(z["state_delta"], out["state_delta"].cpu().numpy())
    assert np.array_equal(z["site_rows"], out["site_rows"].cpu().numpy())
    assert np.array_equal(z["base_state_log_likelihood"], out["base_state_log_likelihood"].cpu().numpy())
    assert z["state_weights"].tolist() == [1.0, -0.5] and float(z["base_loss"]) == float(out["base_loss"])
    assert np.array_equal(z["wild_type_token"], np.asarray(P["S"])[out["positions"].cpu().numpy()])
    wt = z["delta"][np.arange(n_pos), [out["tokens"].tolist().index(int(t)) for t in z["wild_type_token"]]]
    assert np.abs(wt).max() < 2e-4 * 2 * L                                   # the wild-type column changes nothing
    # other flag combinations keep their refusals
    with pytest.raises(ValueError, match="backbone states alone"):
        cli.main(["--mode", "design", "--pdb_path", path, "--out_folder", out_dir, "--multi_state", "1", "--mutation_scan", "1", "--symmetry_residues", "A1,A2"])
