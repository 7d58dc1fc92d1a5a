"""Host-side tests of context states (per-state fixed tokens and presence in tied design): the argument checks that
need no device, pdbio.parse_states(contexts=True) on multi-model files, and the premises of the oracle the GPU tests compare against
(context_states_ref)."""
import os

import numpy as np
import pytest
import torch

import real_structures
from context_states_ref import (context_probs, contexts_fd, model_of, oracle_contexts, oracle_score_tied, oracle_state_log_probs,
                                write_models)
from na_mpnn_amd import cli, pdbio, spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
from tied_states_ref import make_states

torch.set_grad_enabled(False)


def _cpu_model(k=16):
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int()).eval()


def _good(n=20, M=2, bs=2):
    cx = synth.make_complex(seed=3, n=n)
    cx["chain_mask"][::4] = 0
    sS = np.tile(cx["S"], (M, 1))
    sS[1, ::4] = (sS[1, ::4] + 1) % 20
    sm = np.tile(cx["mask"], (M, 1))
    sm[1, 4] = 0
    return contexts_fd(cx, make_states(cx, M, 1), [1.0, -0.5], bs, 0.5, np.zeros((bs, n), np.float32), state_S=sS, state_mask=sm)


def test_argument_checks_with_context_states():
    """What sample(), score_tied() and conditional_probs() refuse about state_S / state_mask before they touch a device."""
    m = _cpu_model()
    n, M = 20, 2
    for call in (m.sample, m.score_tied):
        fd = _good(); fd["state_S"] = fd["state_S"][:1]                        # one row for two states
        with pytest.raises(ValueError, match="state_S"):
            call(fd)
        fd = _good(); fd["state_mask"] = fd["state_mask"][:, :-1]
        with pytest.raises(ValueError, match="state_mask"):
            call(fd)
        fd = _good(); fd["state_S"] = fd["state_S"].float()
        with pytest.raises(ValueError, match="state_S"):
            call(fd)
        fd = _good(); fd["state_S"][1, 3] = 33                                 # not a token
        with pytest.raises(IndexError, match="state_S"):
            call(fd)
        fd = _good(); fd["state_S"][0, 0] = -1
        with pytest.raises(IndexError, match="state_S"):
            call(fd)
        fd = _good(); fd["state_mask"][1, 2] = 2
        with pytest.raises(ValueError, match="state_mask"):
            call(fd)
        fd = _good(); fd["state_mask"][:, 7] = 0                               # nowhere present, yet `mask` has it
        with pytest.raises(ValueError, match="OR"):
            call(fd)
        fd = _good(); fd["mask"] = fd["mask"].clone(); fd["mask"][0, 4] = 0; fd["state_mask"][1, 4] = 0    # present in state 0, `mask` lacks it
        with pytest.raises(ValueError, match="OR"):
            call(fd)
        for k in ("S", "mask"):                                               # the shared rows stay [1, L]: the new keys are the per-state ones
            fd = _good(); fd[k] = fd[k].repeat(M, 1)
            with pytest.raises(ValueError, match=k):
                call(fd)
        for only in ("state_S", "state_mask"):                                 # either key alone is a well-formed call: no CPU path
            fd = _good(); fd.pop(only)
            with pytest.raises(RuntimeError, match="HIP device"):
                call(fd)
        with pytest.raises(RuntimeError, match="HIP device"):
            call(_good())
    fd = _good(); fd.pop("state_weights")                                      # the keys mean nothing without states
    with pytest.raises(ValueError, match="state_weights"):
        m.score_tied(dict(fd, X=fd["X"][:1], X_m=fd["X_m"][:1]))
    for tied in (False, True):
        with pytest.raises(NotImplementedError, match="context"):
            m.conditional_probs(_good(), tied=tied)
    with pytest.raises(NotImplementedError, match="one state only"):           # the item kernel's unit of one carries no weight
        fd = _good(); fd["state_mask"][0, 5] = 0                               # residue 5 is left to state 1, whose weight is -0.5
        m.score_tied(fd, method="items")


# ---- parse_states(contexts=True) -------------------------------------------------------------------------------------------------

def _pieces():
    """28 residues of the 1AM9 crop: 8 + 8 nucleotides of the two DNA strands E and H, 12 residues of the protein chain A."""
    cx = real_structures.variant("1am9_crop")
    letters = [real_structures.chain_letters("1am9")[i] for i in real_structures.rows_of_chains("1am9", real_structures.CROP_CHAINS)]
    names = [spec.RESTYPES[int(t)] for t in cx["S"]]
    rows = np.r_[0:8, 21:29, 38:50]
    return cx, names, letters, rows


def _parse_both(path):
    with pytest.raises(ValueError, match="model 2"):                           # without contexts the models must list the same residues
        pdbio.parse_states(path)
    return pdbio.parse_states(path, contexts=True)


def test_parse_states_contexts_equal_models_change_nothing(tmp_path):
    cx, names, letters, rows = _pieces()
    path = os.path.join(str(tmp_path), "same.pdb")
    write_models(path, [model_of(cx, names, letters, rows)] * 2)
    A, B = pdbio.parse_states(path), pdbio.parse_states(path, contexts=True)
    for k in ("X", "X_m", "S", "mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type",
              "rna_mask_for_token_conversion"):
        assert np.array_equal(A[k], B[k]) and A[k].dtype == B[k].dtype, k
    assert A["chain_letters"] == B["chain_letters"] and A["icodes"] == B["icodes"] and A["na_chain_letters"] == B["na_chain_letters"]
    assert np.array_equal(B["state_S"], np.tile(A["S"], (2, 1))) and np.array_equal(B["state_mask"], np.tile(A["mask"], (2, 1)))
    assert "state_S" not in A and "state_mask" not in A


def test_parse_states_contexts_renamed_base(tmp_path):
    cx, names, letters, rows = _pieces()
    i = 3                                                                       # a nucleotide of strand E
    other = "DG" if names[rows[i]] != "DG" else "DA"
    path = os.path.join(str(tmp_path), "renamed.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(cx, names, letters, rows, rename={int(rows[i]): other})])
    P = _parse_both(path)
    rti = spec.restype_to_int(True)
    assert P["X"].shape == (2, len(rows), 16, 3) and P["state_S"].shape == (2, len(rows)) and P["state_S"].dtype == np.int32
    assert P["state_S"][0, i] == rti[names[rows[i]]] and P["state_S"][1, i] == rti[other] and P["S"][i] == rti[names[rows[i]]]
    differ = P["state_S"][0] != P["state_S"][1]
    assert differ.sum() == 1 and differ[i]
    assert np.array_equal(P["state_mask"][0], P["state_mask"][1]) and np.array_equal(P["mask"], P["state_mask"][0])
    assert np.array_equal(P["X"][0], P["X"][1])


def test_parse_states_contexts_dropped_chain(tmp_path):
    """Bound against unbound: model 2 holds the protein alone.  And the other way round — the partner appears in model 2 first."""
    cx, names, letters, rows = _pieces()
    prot = rows[16:]
    path = os.path.join(str(tmp_path), "unbound.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(cx, names, letters, prot)])
    P = _parse_both(path)
    one = pdbio.parse_pdb(path)
    assert P["chain_letters"] == one["chain_letters"] and np.array_equal(P["S"], one["S"]) and np.array_equal(P["mask"], one["mask"])
    assert np.array_equal(P["state_mask"][0], one["mask"])
    assert not P["state_mask"][1, :16].any() and np.array_equal(P["state_mask"][1, 16:], one["mask"][16:])
    assert not P["X"][1, :16].any() and not P["X_m"][1, :16].any() and np.array_equal(P["X"][1, 16:], one["X"][16:])
    assert np.array_equal(P["state_S"][1], one["S"])                            # an absent residue: the token of the first model that has it
    path2 = os.path.join(str(tmp_path), "unbound_first.pdb")
    write_models(path2, [model_of(cx, names, letters, prot), model_of(cx, names, letters, rows)])
    Q = pdbio.parse_states(path2, contexts=True)
    assert Q["chain_letters"] == ["A"] * 12 + ["E"] * 8 + ["H"] * 8             # chains in order of first appearance
    assert len(set(Q["chain_labels"][[0, 12, 20]].tolist())) == 3               # three chains, three labels
    assert not Q["state_mask"][0, 12:].any() and Q["state_mask"][1, 13:].all()
    perm = np.r_[16:28, 0:16]
    assert np.array_equal(Q["S"], one["S"][perm]) and np.array_equal(Q["X"][1], one["X"][perm])


def test_parse_states_contexts_dropped_loop(tmp_path):
    cx, names, letters, rows = _pieces()
    keep = np.r_[rows[:16], rows[16:19], rows[23:]]                            # the protein lacks four residues in model 2
    path = os.path.join(str(tmp_path), "loop.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(cx, names, letters, keep)])
    P = _parse_both(path)
    assert P["X"].shape[1] == len(rows)
    assert not P["state_mask"][1, 19:23].any() and P["state_mask"][1, 16:19].all() and P["state_mask"][1, 23:].all()
    assert np.array_equal(P["X"][1, 23:], P["X"][0, 23:]) and np.array_equal(P["R_idx"], cx["R_idx"][rows])
    # the longer model need not be the first one
    path2 = os.path.join(str(tmp_path), "loop2.pdb")
    write_models(path2, [model_of(cx, names, letters, keep), model_of(cx, names, letters, rows)])
    Q = pdbio.parse_states(path2, contexts=True)
    assert np.array_equal(Q["R_idx"], P["R_idx"]) and np.array_equal(Q["state_mask"], P["state_mask"][::-1])


def test_parse_states_contexts_refuses_a_non_subsequence(tmp_path):
    cx, names, letters, rows = _pieces()
    swapped = rows.copy()
    swapped[[17, 18]] = swapped[[18, 17]]                                      # two protein residues in the other order
    path = os.path.join(str(tmp_path), "order.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(cx, names, letters, swapped[:-1])])
    with pytest.raises(ValueError, match="model 2"):
        pdbio.parse_states(path, contexts=True)
    with pytest.raises(ValueError, match="model 2"):
        pdbio.parse_states(path)


def test_parse_states_contexts_refuses_a_polymer_clash(tmp_path):
    """Residue E4 is a deoxynucleotide in model 1 and carries an O2' — a ribonucleotide — in model 2."""
    cx, names, letters, rows = _pieces()
    i = int(rows[3])
    rna = {k: v.copy() for k, v in cx.items()}
    o2 = spec.ATOM_TYPES.index("O2'")
    rna["X_m"][i, o2] = 1
    rna["X"][i, o2] = rna["X"][i, spec.ATOM_TYPES.index("C1'")] + 1.0
    path = os.path.join(str(tmp_path), "clash.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(rna, names, letters, rows)])
    with pytest.raises(ValueError, match="polymer type"):
        pdbio.parse_states(path, contexts=True)


def test_cli_state_contexts_needs_multi_state(tmp_path):
    cx, names, letters, rows = _pieces()
    path = os.path.join(str(tmp_path), "one.pdb")
    write_models(path, [model_of(cx, names, letters, rows)] * 2)
    with pytest.raises(ValueError, match="multi_state"):
        cli.main(["--pdb_path", path, "--out_folder", os.path.join(str(tmp_path), "out"), "--random_init_seed", "0", "--batch_size", "1",
                  "--temperature", "0.5", "--state_contexts", "1"])


# ---- the oracle's own premises -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_case(weights_np):
    """L = 24 (8 fixed), K = 12, three states: everything present; the fixed residues absent; other fixed tokens and one designable
    residue absent — with the oracle's result for one random sequence."""
    L, K, M = 24, 12, 3
    cx = synth.make_complex(seed=77, n=L)
    cx["mask"][:] = 1
    cx["chain_mask"][:] = 1
    cx["chain_mask"][16:] = 0
    rng = np.random.default_rng(5)
    sS = np.tile(cx["S"], (M, 1))
    sS[2, 16:] = (sS[2, 16:] + 1 + rng.integers(0, 18, 8)) % 20
    sm = np.ones((M, L), np.int32)
    sm[1, 16:] = 0
    sm[2, 5] = 0
    fd = contexts_fd(cx, make_states(cx, M, seed=9), (1.0, -0.5, 0.3), 2, 0.5, rng.standard_normal((2, L)).astype(np.float32),
                     state_S=sS, state_mask=sm)
    S = torch.from_numpy(rng.integers(0, 20, (2, L)))
    w = cpu_ref.to_torch(weights_np)
    return w, fd, K, S, oracle_contexts(w, fd, K, S)


def test_oracle_is_symmetric_in_the_states(small_case):
    """Swapping two states together with their weights leaves the drawn distribution unchanged (the sum over the states commutes; the
    per-state rows swap)."""
    w, fd, K, S, (lp, p, order) = small_case
    perm = [2, 1, 0]
    fd2 = dict(fd, X=fd["X"][perm], X_m=fd["X_m"][perm], state_S=fd["state_S"][perm], state_mask=fd["state_mask"][perm],
               state_weights=[fd["state_weights"][m] for m in perm])
    lp2, p2, order2 = oracle_contexts(w, fd2, K, S)
    assert torch.equal(order, order2)
    assert torch.equal(lp2, lp[:, perm])
    assert float((p2 - p).abs().max()) < 1e-12
    cm = (fd["mask"] * fd["chain_mask"])[0].bool()
    assert (p[:, ~cm] == 0).all() and float((p[:, cm].sum(-1) - 1).abs().max()) < 1e-12
    assert (p[:, :, list(cpu_ref.SPECIAL_TOKENS)] == 0).all()


def test_oracle_feels_a_fixed_token_of_one_state(small_case):
    """Changing ONE fixed token in ONE state changes the distribution of designable residues — through that state's rows alone.
    Without this the GPU cases could not tell per-state tokens from shared ones."""
    w, fd, K, S, (lp, p, _) = small_case
    sS = fd["state_S"].clone()
    sS[2, 20] = (sS[2, 20] + 7) % 20
    lp2, p2, _ = oracle_contexts(w, dict(fd, state_S=sS), K, S)
    assert torch.equal(lp2[:, :2], lp[:, :2])
    cm = (fd["mask"] * fd["chain_mask"])[0].bool()
    # (the oracle is deterministic: the unchanged states' rows are equal bit for bit, so any difference is the token's doing; one token
    #  of 24 residues through a state of weight 0.3 moves a probability by some 1e-5 .. 1e-4, the fp64 recombination rounds at 1e-16)
    assert float((lp2[:, 2][:, cm] - lp[:, 2][:, cm]).abs().max()) > 1e-3
    assert float((p2 - p).abs().max()) > 1e-5
    sS[2, 16:] = (fd["state_S"][2, 16:] + 3) % 20                              # ... and all eight of them by a visible amount
    _, p3, _ = oracle_contexts(w, dict(fd, state_S=sS), K, S)
    assert float((p3 - p).abs().max()) > 2e-4


def test_oracle_absent_copies_contribute_nothing(small_case):
    """The rows of absent copies do not enter the sum: any values there leave the distribution unchanged, and a residue present in one
    state only draws from that state's weighted row alone."""
    w, fd, K, S, (lp, p, _) = small_case
    junk = lp.clone()
    absent = fd["state_mask"] == 0
    junk[:, absent] = 123.0
    assert torch.equal(context_probs(junk, fd), p)
    only0 = dict(fd, state_mask=torch.cat((fd["state_mask"][:1], torch.zeros_like(fd["state_mask"][1:]))))
    lp0, _ = oracle_state_log_probs(w, only0, K, S)
    p0 = context_probs(lp0, only0)
    want = torch.softmax(lp0[:, 0] * fd["state_weights"][0] / fd["temperature"], -1)
    want[..., list(cpu_ref.SPECIAL_TOKENS)] = 0
    want = want / want.sum(-1, keepdim=True)
    cm = (fd["mask"] * fd["chain_mask"])[0].bool()
    assert float((p0[:, cm] - want[:, cm]).abs().max()) < 1e-12


def test_oracle_score_is_the_log_of_the_draw_at_T1(small_case):
    """oracle_score_tied's token_log_probs at designable positions are the log of the distribution at T = 1 with no bias and the special
    tokens kept; state_log_likelihood sums the own entries of the designed positions present in the state."""
    w, fd, K, S, (lp, _, _) = small_case
    sc = oracle_score_tied(w, fd, K, S)
    p1 = context_probs(lp, fd, T=1.0, bias=torch.zeros(1, 1, 33), special=())
    cm = (fd["mask"] * fd["chain_mask"])[0].bool()
    want = torch.log(p1.gather(2, S[:, :, None])[:, :, 0])
    assert float((sc["token_log_probs"][:, cm] - want[:, cm]).abs().max()) < 1e-9
    assert float((sc["log_likelihood"] - want[:, cm].sum(-1)).abs().max()) < 1e-9
    own = lp.gather(3, S[:, None, :, None].expand(-1, 3, -1, -1))[..., 0]
    counted = cm[None, :] & (fd["state_mask"] != 0)
    assert float((sc["state_log_likelihood"] - (own * counted[None]).sum(-1)).abs().max()) < 1e-9
