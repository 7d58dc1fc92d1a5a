"""CPU tests of the compact pair terms (feature_dict["pair_terms"]): the CLI's builder against the dense one, the reference combine
(pair_terms_ref) against the CPU oracle on the densified tensor, the slot sort, the refusals of the model, and the three integer-only
entry points of the library (argument validation and workspace arithmetic need no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from na_mpnn_amd import cli, hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN, pair_terms_arguments, pair_terms_dense, sort_pair_slots
from oracle import cpu_ref
import pair_terms_ref
import paired_ref

torch.set_grad_enabled(False)
V = 33


def test_compact_builder_densifies_to_the_dense_builder():
    """make_pair_terms -> pair_terms_dense is make_pair_bias exactly, on an input with chain breaks and numbering gaps."""
    chain = torch.tensor([0] * 7 + [1] * 5 + [2] * 1 + [3] * 6)
    R_idx = torch.tensor([1, 2, 3, 5, 6, 7, 8, 1, 2, 3, 4, 6, 9, 10, 11, 12, 20, 21, 22])       # gaps inside chains 0, 1 and 3
    L = len(chain)
    AA = torch.from_numpy(np.random.default_rng(4).standard_normal((V, V)).astype(np.float32))
    dense = cli.make_pair_bias(chain, R_idx, AA)
    pt = cli.make_pair_terms(chain, R_idx, AA)
    assert pt["members"] == "closing" and tuple(pt["partner"].shape) == (1, L, 2) and tuple(pt["tables"].shape) == (2, V, V)
    assert torch.equal(pair_terms_dense(pt, L), dense)
    assert int((pt["partner"] >= 0).sum()) == 2 * 12                                           # 12 adjacent pairs of residues
    assert cli.make_pair_terms(chain, R_idx, AA, "all")["members"] == "all"


def test_slot_sort():
    """Stable by partner; absent slots (negative, >= L, the residue itself) last and -1; the table index travels with its partner."""
    partner = torch.tensor([[[5, -1, 2, 5, 0], [1, 9, 3, 3, -7], [4, 4, 4, 4, 4]]])[:, :, :].repeat(1, 2, 1)      # L = 6
    table = torch.arange(30).view(1, 6, 5)
    p, t = sort_pair_slots(partner, table)
    assert p[0, 0].tolist() == [2, 5, 5, -1, -1] and t[0, 0].tolist() == [2, 0, 3, 1, 4]      # (0 is residue 0 itself: absent)
    assert p[0, 1].tolist() == [3, 3, -1, -1, -1] and t[0, 1].tolist() == [7, 8, 5, 6, 9]     # (1 is itself, 9 >= L, -7 < 0)
    assert p[0, 2].tolist() == [4] * 5 and t[0, 2].tolist() == [10, 11, 12, 13, 14]           # duplicates keep their order
    assert p[0, 4].tolist() == [1, 3, 3, -1, -1] and t[0, 4].tolist() == [20, 22, 23, 21, 24]     # (on residue 4 partner 1 is a partner)
    # the reference's own sort agrees
    pt = {"partner": partner, "table": table, "tables": torch.zeros(40, V, V)}
    for i in range(6):
        ref = pair_terms_ref.slots_of(pt, 0, i, 6)
        n = len(ref)
        assert [s[0] for s in ref] == p[0, i, :n].tolist() and [s[1] for s in ref] == t[0, i, :n].tolist() and (p[0, i, n:] == -1).all()


def _case(L, bs, seed, sym=False):
    cx = synth.make_complex(seed=seed, n=L, n_chains=2)
    cx["chain_mask"][[3, 11]] = 0
    fd = {k: torch.from_numpy(np.ascontiguousarray(cx[k]))[None] for k in paired_ref.PER_RESIDUE}
    rng = np.random.default_rng(seed)
    fd.update({"batch_size": bs, "temperature": 0.7, "bias": torch.from_numpy(0.3 * rng.standard_normal((1, L, V)).astype(np.float32)),
               "symmetry_residues": [[]], "symmetry_weights": [[]],
               "randn": torch.from_numpy(rng.standard_normal((bs, L)).astype(np.float32))})
    if sym:
        fd["symmetry_residues"], fd["symmetry_weights"] = [[1, 2], [5, 20, 9], [14, 15]], [[1.0, 1.0], [0.5, 1.0, -0.5], [1.0, 2.0]]
        fd["randn"] = fd["randn"][:1].repeat(bs, 1)
    AA = torch.from_numpy(rng.standard_normal((V, V)).astype(np.float32))
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA)
    # and a far, one-sided partner with a table of its own, and a duplicate partner
    pt["partner"] = torch.cat((pt["partner"], torch.full((1, L, 2), -1, dtype=torch.int32)), 2)
    pt["table"] = torch.cat((pt["table"], torch.zeros(1, L, 2, dtype=torch.int32)), 2)
    for i in range(0, L - 9, 3):
        pt["partner"][0, i, 2], pt["table"][0, i, 2] = i + 9, 2
    pt["partner"][0, 6, 3], pt["table"][0, 6, 3] = 7, 2
    pt["tables"] = torch.cat((pt["tables"], torch.from_numpy(rng.standard_normal((1, V, V)).astype(np.float32))))
    return cx, fd, pt


@pytest.mark.parametrize("sym", [False, True])
def test_reference_combine_equals_the_oracle_on_the_dense_tensor(weights_np, sym):
    """"closing" and no maps is the reference's own rule: the combine on the oracle's log_probs equals cpu_ref.sample /
    sample_symmetric run with the densified tensor, teacher-forced with a sequence the oracle itself drew."""
    L, K, bs = 24, 12, 2
    cx, fd, pt = _case(L, bs, 77, sym)
    w = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    run = cpu_ref.sample_symmetric if sym else cpu_ref.sample
    fdd = dict(fd, pair_bias=pair_terms_dense(pt, L))
    torch.manual_seed(3)
    S = run(w, fdd, K)["S"]
    ref = run(w, fdd, K, S_forced=S)
    assert torch.equal(ref["S"], S)
    groups, gw = (fd["symmetry_residues"], fd["symmetry_weights"]) if sym else (None, None)
    p = pair_terms_ref.plain_probs(ref["log_probs"], fd, pt, S, ref["decoding_order"], groups, gw)
    assert float((p - ref["sampling_probs"]).abs().max()) < 2e-6
    # and the terms matter: without them the combine is off
    p0 = pair_terms_ref.plain_probs(ref["log_probs"], fd, dict(pt, tables=torch.zeros_like(pt["tables"])), S, ref["decoding_order"], groups, gw)
    assert float((p0 - ref["sampling_probs"]).abs().max()) > 1e-2


def test_model_refuses_bad_pair_terms(weights_np):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=12, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    L = 24
    _, fd, pt = _case(L, 2, 5)
    bad = lambda **kw: dict(fd, pair_terms=dict(pt, **kw))
    with pytest.raises(ValueError, match="one of them"):
        m.sample(dict(fd, pair_terms=pt, pair_bias=torch.zeros(1, L, V, L, V)))
    with pytest.raises(ValueError, match="slots"):
        m.sample(bad(partner=torch.full((1, L, 65), -1), table=torch.zeros(1, L, 65, dtype=torch.int64)))
    with pytest.raises(ValueError, match="slots"):
        m.sample(bad(partner=torch.full((1, L, 0), -1), table=torch.zeros(1, L, 0, dtype=torch.int64)))
    with pytest.raises(ValueError, match="tables"):
        m.sample(bad(tables=torch.zeros(257, V, V)))
    with pytest.raises(ValueError, match="tables"):
        m.sample(bad(tables=torch.zeros(2, V, V + 1)))
    with pytest.raises(ValueError, match="partner"):
        m.sample(bad(partner=pt["partner"][:, :-1]))
    with pytest.raises(ValueError, match="partner"):
        m.sample(bad(table=pt["table"][:, :, :-1]))
    with pytest.raises(ValueError, match="integer"):
        m.sample(bad(partner=pt["partner"].float()))
    with pytest.raises(ValueError, match="members"):
        m.sample(bad(members="both"))
    with pytest.raises(ValueError, match="dict"):
        m.sample(dict(fd, pair_terms=pt["partner"]))
    # the tied-states path checks the same before any device work
    fds = dict(fd, state_weights=[0.5, 0.5], X=fd["X"].repeat(2, 1, 1, 1), X_m=fd["X_m"].repeat(2, 1, 1), randn=fd["randn"])
    with pytest.raises(ValueError, match="members"):
        m.sample(dict(fds, pair_terms=dict(pt, members="both")))
    # the dense key keeps its refusals
    with pytest.raises(ValueError, match="pair_bias is not supported"):
        m.sample(dict(fd, pair_bias=torch.zeros(1, L, V, L, V), paired_residues=[(20, 23)]))
    assert pair_terms_arguments(pt, 1, L, V)[3] == 0 and pair_terms_arguments(dict(pt, members="all"), 1, L, V)[3] == 1


def test_pair_terms_entry_points_validate_without_a_gpu():
    Lb = hip.lib()
    for bad in ((0, 1, 0), (65, 1, 0), (-1, 1, 0)):
        assert Lb.namp_sample_pair_terms(*bad) == -1 and b"D=" in Lb.namp_last_error()
    for bad in ((2, 0, 0), (2, 257, 1)):
        assert Lb.namp_sample_pair_terms(*bad) == -1 and b"n_tables" in Lb.namp_last_error()
    for bad in ((2, 2, 2), (2, 2, -1)):
        assert Lb.namp_sample_pair_terms(*bad) == -1 and b"members" in Lb.namp_last_error()
    assert Lb.namp_sample_pair_terms(1, 1, 0) == 0 and Lb.namp_sample_pair_terms(64, 256, 1) == 0
    # the sampler call takes the attachment and clears it whether it succeeds or not: together with a dense pair_bias pointer it is
    # refused; the same call again no longer sees an attachment
    dummy = (C.c_float * 4)()
    pb = C.cast(dummy, C.POINTER(C.c_float))
    nul = [None] * 16
    call = lambda pair_bias: Lb.namp_decoder_sample(*nul, pair_bias, 1.0, 0, None, None, None, None, 0, 1, 1, 10, 4, None)
    assert call(pb) == -1 and b"pair terms and the dense pair_bias" in Lb.namp_last_error()
    assert call(pb) == -1 and b"pair terms" not in Lb.namp_last_error()
    assert Lb.namp_sample_pair_terms(2, 2, 1) == 0 and Lb.namp_sample_pair_terms(65, 2, 1) == -1      # a bad attach leaves nothing attached
    assert call(pb) == -1 and b"pair terms" not in Lb.namp_last_error()
    assert Lb.namp_sample_pair_terms(2, 2, 1) == 0
    assert call(None) == -1 and b"null weights" in Lb.namp_last_error()
    assert call(pb) == -1 and b"pair terms" not in Lb.namp_last_error()


def test_pair_terms_workspace_arithmetic():
    Lb = hip.lib()
    for dims in ((1, 1, 1000, 48, 3), (1, 3, 97, 32, 3), (2, 4, 80, 24, 3), (1, 1, 1, 1, 1), (1, 8, 16000, 48, 8)):
        base = Lb.namp_sample_workspace_bytes_n(*dims)
        off = Lb.namp_sample_pair_terms_offset(*dims)
        assert base > 0 and off % 256 == 0 and base <= off < base + 256                    # behind the carve, barrier words included
        G = dims[0] * dims[2]
        last = off
        for D in (1, 2, 7, 64):
            need = Lb.namp_sample_pair_terms_workspace_bytes(*dims, D, 1)
            assert need >= off + 4 * (2 * G * D + V * V) and need > last                   # monotone in D
            last = need
        last = Lb.namp_sample_pair_terms_workspace_bytes(*dims, 2, 1)
        for n_tab in (2, 17, 256):
            need = Lb.namp_sample_pair_terms_workspace_bytes(*dims, 2, n_tab)
            assert need >= off + 4 * (4 * G + n_tab * V * V) and need > last               # monotone in n_tables
            last = need
        assert last - off <= 4 * (4 * G + 256 * 64 * 64)                                   # slot- and table-sized: never O(N^2)
    for args in ((1, 1, 100, 24, 3, 0, 1), (1, 1, 100, 24, 3, 65, 1), (1, 1, 100, 24, 3, 2, 0), (1, 1, 100, 24, 3, 2, 257),
                 (0, 1, 100, 24, 3, 2, 2), (1, 1, 100, 24, 9, 2, 2), (1, 1, 0, 24, 3, 2, 2)):
        assert Lb.namp_sample_pair_terms_workspace_bytes(*args) == 0, args
    assert Lb.namp_sample_pair_terms_offset(1, 1, 100, 24, 9) == 0 and Lb.namp_sample_pair_terms_offset(1, 0, 100, 24, 3) == 0
