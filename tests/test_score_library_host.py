"""CPU tests of library scoring (ProteinMPNN.score_sequences): the numpy restatement of the active-row sets against the oracle's
decoder states, the premises of the GPU cases, the argument checks and the CLI's FASTA parsing.  No device needed."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import cli, pdbio, spec
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import library_ref as LR

torch.set_grad_enabled(False)


def cpu_fd(cx):
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd["batch_size"] = 1
    return fd


_sets = {}


def case_sets(name, weights_np):
    """(complex, feature_dict, positions, var, [act_1..3], torch weights) of a case on the oracle's graph and order, computed once."""
    if name not in _sets:
        k, cx, pos, tok = LR.make_case(name)
        fd, w = cpu_fd(cx), cpu_ref.to_torch(weights_np)
        E_idx = LR.encoded(w, fd, k, name)[2][0].numpy()
        order = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"])[0].numpy()
        var, acts = LR.active_sets(E_idx, LR.ranks_of(order), cx["mask"], pos)
        _sets[name] = (k, cx, fd, pos, var, acts, w)
    return _sets[name]


@pytest.mark.parametrize("name", ["n97", "crossing", "LltK", "all"])
def test_rows_whose_decoder_states_differ_are_the_active_rows(weights_np, name):
    """Two random libraries that differ only at `positions`: the rows whose oracle decoder states differ between two sequences at
    layer l are a subset of act_l; over a 12-sequence random library their union EQUALS act_l."""
    k, cx, fd, pos, var, acts, w = case_sets(name, weights_np)
    rng = np.random.default_rng(77)
    tok = LR.random_library(rng, cx["S"], pos, 12, cx["protein_mask"], cx["dna_mask"], cx["rna_mask"])
    S_full = LR.full_sequences(cx["S"], pos, tok)
    states = [LR.oracle_decoder_states(w, fd, k, S_k, key=name) for S_k in S_full]
    union = [np.zeros(len(cx["S"]), bool) for _ in range(3)]
    for a in range(len(S_full)):
        for b in range(a + 1, len(S_full)):
            for l in range(3):
                differ = ((states[a][l] - states[b][l]).abs().amax(-1) != 0).numpy()
                assert not (differ & ~acts[l]).any(), (name, a, b, l, np.nonzero(differ & ~acts[l])[0])
                union[l] |= differ
    for l in range(3):
        assert np.array_equal(union[l], acts[l]), (name, l, np.nonzero(union[l] != acts[l])[0])
    assert not (acts[0] & ~acts[1]).any() and not (acts[1] & ~acts[2]).any()          # act_1 in act_2 in act_3
    assert not (acts[2] & (cx["mask"] == 0)).any()


def test_premises_of_the_gpu_cases(weights_np):
    """In the "designed nucleic acid" case |act_3| <= L / 2; in the crossing case act_3 contains fixed residues; with every residue
    designed act_3 is nearly every row; n = 13 is no multiple of the 16-row tile; L < K in the LltK case."""
    k, cx, fd, pos, var, acts, w = case_sets("n97", weights_np)
    L = len(cx["S"])
    assert 0 < acts[2].sum() <= L / 2 and sum(int(a.sum()) for a in acts) < 3 * L / 2
    assert len(LR.make_case("n97")[3]) == 13
    k, cx, fd, pos, var, acts, w = case_sets("crossing", weights_np)
    assert (acts[2] & ~var).sum() > 0 and (cx["chain_mask"][acts[2] & ~var] == 0).all()
    k, cx, fd, pos, var, acts, w = case_sets("all", weights_np)
    assert acts[2].sum() >= 0.9 * len(cx["S"])
    k, cx, fd, pos, var, acts, w = case_sets("LltK", weights_np)
    assert len(cx["S"]) < k


def host_model():
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int())


def test_argument_checks():
    """positions out of range / unsorted / repeated raise ValueError, B = 2 raises ValueError, token 33 raises IndexError,
    state_weights NotImplementedError, an unknown method ValueError; both S_lib forms give the same full S; the default positions are
    the residues with mask * chain_mask != 0; everything outside `positions` is taken from feature_dict["S"]."""
    k, cx, pos, tok = LR.make_case("n97")
    fd, m = cpu_fd(cx), host_model()
    L = len(cx["S"])
    lib = torch.from_numpy(tok)
    p, t, S_a = m._library_arguments(fd, lib, torch.from_numpy(pos))
    assert p == pos.tolist() and torch.equal(t, lib)
    full = torch.from_numpy(np.random.default_rng(3).integers(0, 33, (len(tok), L)))
    full[:, torch.from_numpy(pos)] = lib
    p2, t2, S_b = m._library_arguments(fd, full, torch.from_numpy(pos))
    assert torch.equal(S_a, S_b) and torch.equal(t2, lib)
    assert np.array_equal(S_a.numpy(), LR.full_sequences(cx["S"], pos, tok))
    p3, _, S_c = m._library_arguments(fd, lib, None)                                    # the default positions
    assert p3 == np.nonzero(cx["mask"] * cx["chain_mask"])[0].tolist() and torch.equal(S_c, S_a)
    for bad in ([0, L], [-1, 3], [5, 3], [3, 3]):
        with pytest.raises(ValueError):
            m._library_arguments(fd, lib[:, :2], torch.tensor(bad))
    with pytest.raises(ValueError):
        m._library_arguments(fd, lib[:, :5], torch.from_numpy(pos))                     # neither [n, L] nor [n, n_var]
    fd2 = {k_: (torch.cat((v, v)) if isinstance(v, torch.Tensor) else v) for k_, v in fd.items()}
    with pytest.raises(ValueError):
        m._library_arguments(fd2, lib, torch.from_numpy(pos))
    with pytest.raises(ValueError):
        m.score_sequences(fd2, lib, torch.from_numpy(pos))
    bad_tok = lib.clone(); bad_tok[2, 1] = 33
    with pytest.raises(IndexError):
        m._library_arguments(fd, bad_tok, torch.from_numpy(pos))
    with pytest.raises(IndexError):
        m.score_sequences(fd, bad_tok, torch.from_numpy(pos))
    special = lib.clone(); special[0, 0], special[1, 1] = 31, 32                        # MAS / PAD are legal
    m._library_arguments(fd, special, torch.from_numpy(pos))
    with pytest.raises(NotImplementedError):
        m._library_arguments(dict(fd, state_weights=[0.5, 0.5]), lib, torch.from_numpy(pos))
    with pytest.raises(ValueError):
        m.score_sequences(fd, lib, torch.from_numpy(pos), method="sparse")


def fasta_setup(golden_dir):
    gd = os.path.join(golden_dir, "cli")
    P = pdbio.parse_pdb(os.path.join(gd, "input.pdb"))
    rti = spec.restype_to_int(True)
    int_to_str = {}
    for k, v in rti.items():
        int_to_str.setdefault(v, spec.RESTYPE_3TO1[k])
    dna_to_rna = {spec.RESTYPE_3TO1[d]: spec.RESTYPE_3TO1[r] for d, r in (("DA", "A"), ("DC", "C"), ("DG", "G"), ("DT", "U"), ("DX", "RX"))}
    str_to_int = {}
    for t, ch in int_to_str.items():
        str_to_int[ch] = t
        str_to_int[dna_to_rna.get(ch, ch)] = t
    encoded = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    return gd, P, int_to_str, dna_to_rna, str_to_int, encoded


def test_fasta_round_trip_with_the_cli_fixture(golden_dir):
    """The seqs/*.fa the CLI fixture wrote parses back: the native line IS the structure's S, and every sequence, written out again
    with the CLI's seq_string, is its own line."""
    gd, P, int_to_str, dna_to_rna, str_to_int, encoded = fasta_setup(golden_dir)
    names, seqs = cli.read_fasta(os.path.join(gd, "expected.fa"))
    assert len(seqs) == len(names) == 3 and names[0].startswith("input, T=") and names[2].startswith("input, id=2")
    L = len(P["S"])
    lib = cli.fasta_tokens(names, seqs, P["S"], list(P["chain_letters"]), np.ones(L, bool), str_to_int, encoded)
    assert lib.shape == (3, L) and lib.dtype == np.int64
    assert np.array_equal(lib[0], P["S"])
    for row, seq in zip(lib, seqs):
        assert cli.seq_string(row, P["rna_mask_for_token_conversion"], int_to_str, dna_to_rna, P["chain_letters"]) == seq


def test_fasta_errors_name_the_sequence(golden_dir):
    gd, P, int_to_str, dna_to_rna, str_to_int, encoded = fasta_setup(golden_dir)
    names, seqs = cli.read_fasta(os.path.join(gd, "expected.fa"))
    L = len(P["S"])
    chains = list(P["chain_letters"])
    with pytest.raises(ValueError, match="id=1.*residues"):
        cli.fasta_tokens(names, [seqs[0], seqs[1][:-1], seqs[2]], P["S"], chains, np.ones(L, bool), str_to_int, encoded)
    designable = np.ones(L, bool)
    first = int(np.nonzero(lib_differs(seqs, P, chains, str_to_int, encoded)[2])[0][0])
    designable[first] = False
    with pytest.raises(ValueError, match=f"id=2.*{encoded[first]}"):
        cli.fasta_tokens(names[2:], seqs[2:], P["S"], chains, designable, str_to_int, encoded)
    # the native line differs nowhere: it passes with nothing designable
    cli.fasta_tokens(names[:1], seqs[:1], P["S"], chains, np.zeros(L, bool), str_to_int, encoded)


def lib_differs(seqs, P, chains, str_to_int, encoded):
    lib = cli.fasta_tokens([str(i) for i in range(len(seqs))], seqs, P["S"], chains, np.ones(len(P["S"]), bool), str_to_int, encoded)
    return lib != np.asarray(P["S"])[None]
