"""CPU tests of the pair conditionals (ProteinMPNN.conditional_probs with paired_residues): the definition on the CPU
oracle (the pair stream with the hidden token against the tied branch of the sampler), that hiding the token matters exactly where
the first member is a neighbour of the second, the numpy restatement of the grids against a brute force on the oracle's layer
outputs, and the library's sizing / attach entry points."""
import functools

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec
from oracle import cpu_ref
import paired_ref
from pair_loo_numpy import brute_force_cone, pair_loo_grids, pair_tables
from pair_loo_ref import combine, neighbour_kinds, pair_specs, pair_stream_logits

torch.set_grad_enabled(False)
K = 16


@functools.lru_cache(maxsize=None)
def premise_case():
    """paired_ref.make_case(L=48, ..., n_pairs=5, seed=11) at K = 16: pairs (43, 37), (19, 40), (44, 28), (42, 38), (21, 29) — two
    mutual neighbours, two that are not neighbours, one where only j is a neighbour of i."""
    from na_mpnn_amd import synth
    w = cpu_ref.to_torch(synth.make_weights(0))
    cx, fd, pairs = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    enc = cpu_ref.encode(w, fd, K)
    order0 = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"])[0]
    return w, cx, fd, pairs, enc, order0


def test_the_case_has_the_pairs_the_issue_names():
    _, _, _, pairs, enc, _ = premise_case()
    assert pairs == [(43, 37), (19, 40), (44, 28), (42, 38), (21, 29)]
    kinds = neighbour_kinds(enc[2][0].numpy(), pairs)               # (i in N(j), j in N(i))
    assert sorted(kinds) == sorted([(True, True)] * 2 + [(False, False)] * 2 + [(False, True)])


def test_pair_stream_equals_the_tied_branch_decoded_last():
    """The premise: the stream's member rows equal cpu_ref.sample_symmetric teacher-forced with the group [i, j] visited last, within
    1e-5 (measured: 1.9e-6 over the five pairs)."""
    w, cx, fd, pairs, enc, order0 = premise_case()
    L = fd["S"].shape[1]
    z = pair_stream_logits(w, enc, fd["S"], fd["mask"], order0, pairs)
    worst = 0.0
    for (i, j), zz in zip(pairs, z):
        order = torch.cat((order0[(order0 != i) & (order0 != j)], order0.new_tensor([i, j])))
        randn = torch.empty(L); randn[order] = torch.arange(1, L + 1, dtype=torch.float32)
        fdo = {k: v for k, v in fd.items() if k != "paired_residues"}
        fdo.update(symmetry_residues=[[i, j]], symmetry_weights=[[1.0, 1.0]], randn=randn[None], chain_mask=torch.ones_like(fd["chain_mask"]),
                   bias=torch.zeros(1, L, 33))
        ref = cpu_ref.sample_symmetric(w, fdo, K, S_forced=fd["S"].long())
        assert torch.equal(ref["decoding_order"][0], order)
        d = float((torch.log_softmax(zz, -1) - ref["log_probs"][0, [i, j]]).abs().max())
        worst = max(worst, d)
    print(f"pair stream vs tied branch: max|dlogp| = {worst:.3e}")
    assert worst < 1e-5, worst


def test_hiding_the_token_matters_where_i_is_a_neighbour_of_j():
    """Un-hiding i's token moves row j by more than 2e-3 on the two mutual-neighbour pairs (measured 2.8e-3 and 5.5e-3) and by exactly
    0 on the three pairs where i is not in N(j); row i never moves."""
    w, cx, fd, pairs, enc, order0 = premise_case()
    hid = torch.log_softmax(pair_stream_logits(w, enc, fd["S"], fd["mask"], order0, pairs), -1)
    vis = torch.log_softmax(pair_stream_logits(w, enc, fd["S"], fd["mask"], order0, pairs, hide=False), -1)
    kinds = neighbour_kinds(enc[2][0].numpy(), pairs)
    for n, (i_in_Nj, _) in enumerate(kinds):
        d = float((hid[n, 1] - vis[n, 1]).abs().max())
        print(f"pair {pairs[n]}: i in N(j) = {i_in_Nj}, un-hiding moves row j by {d:.3e}")
        assert torch.equal(hid[n, 0], vis[n, 0])
        assert (d > 2e-3) if i_in_Nj else (d == 0.0), (pairs[n], d)
    assert sum(k[0] for k in kinds) == 2


def test_pair_grids_equal_a_brute_force_on_the_layer_outputs():
    """The numpy grids against the oracle's layer outputs (fp64): per stream — every pair, and every unpaired residue — the residues
    of the active layer-1 slots are exactly those whose layer-1 output differs from the base stream's, the residues of the active
    layer-2 slots exactly the stream members' neighbours whose layer-2 output differs; a residue that used to see both members as
    decoded holds two layer-1 slots."""
    w, cx, fd, pairs, enc, order0 = premise_case()
    w64 = cpu_ref.to_dtype(w, torch.float64)
    enc64 = (enc[0].double(), enc[1].double(), enc[2])
    E = enc[2][0].numpy()
    L = E.shape[0]
    rank = np.empty(L, np.int64); rank[order0.numpy()] = np.arange(L)
    mask = cx["mask"]
    partner, lead = pair_tables(L, pairs, mask)
    act1, act2 = pair_loo_grids(E, rank, mask, partner, lead)
    streams = [tuple(p) for p in pairs] + [(g,) for g in range(L) if partner[g] < 0][:12]
    doubles = 0
    for members in streams:
        s1, s2 = brute_force_cone(w64, enc64, fd["S"], fd["mask"].double(), order0, members)
        slots1 = [(int(m), int(k)) for m, k in zip(*np.nonzero(act1)) if int(E[m, k]) in members]
        assert {m for m, _ in slots1} == s1, members
        doubles += len(slots1) - len(s1)
        assert len(slots1) - len(s1) == sum(1 for m in s1 if all(g in E[m] and rank[g] < rank[m] for g in members)) * (len(members) - 1)
        for g in members:
            got = {int(E[g, kq]) for kq in np.nonzero(act2[g])[0]}
            assert got == (s2 & set(E[g].tolist())) - set(members), (members, g)
    assert doubles > 0
    # without pairs: the grids of the leave-one-out cone
    from loo_numpy import loo_grids
    none = np.full(L, -1, np.int64)
    a1, a2 = pair_loo_grids(E, rank, mask, none, np.zeros(L, bool))
    _, b1, b2 = loo_grids(E, rank, mask)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)


def test_combine_is_a_permutation_and_a_distribution():
    rti = spec.restype_to_int()
    _, _, fd, pairs, _, _ = premise_case()
    g = torch.Generator().manual_seed(3)
    for i, j, wi, wj, Pi, Pj in pair_specs(dict(fd, paired_weights=(1.0, 0.5)), rti):
        assert (wi, wj) == (1.0, 0.5)
        ri, rj = combine(torch.randn(33, generator=g), torch.randn(33, generator=g), wi, wj, Pi, Pj)
        assert torch.equal(ri[torch.tensor(Pi)], rj[torch.tensor(Pj)])
        assert abs(float(ri.exp().sum()) - 1) < 1e-12 and abs(float(rj.exp().sum()) - 1) < 1e-12


def test_pair_entry_points_validate_without_a_gpu():
    L = hip.lib()
    base = L.namp_loo_workspace_bytes(1, 1000, 48, 3)
    need = L.namp_loo_pairs_workspace_bytes(1, 1000, 48, 3, 3)
    off = L.namp_loo_pairs_offset(1, 1000, 48, 3)
    assert off == base and off % 256 == 0 and L.namp_loo_pairs_offset(1, 97, 32, 3) % 256 == 0
    assert need >= off + 4 * (4 * 1000 + 3 * 64) + 2 * 1000 * 128 * 4                       # the section and the two row buffers
    assert need - base < (1 << 21) + 4 * 48000 + 256                                         # residue-sized additions and one [G*K] int32 table (the group carve)
    assert L.namp_loo_pairs_workspace_bytes(1, 3000, 48, 3, 3) < 3 * need + (1 << 20)        # linear in N
    for args in ((1, 100, 24, 4, 2), (0, 100, 24, 3, 2), (1, 100, 24, 3, 0), (1, 100, 24, 3, 65)):
        assert L.namp_loo_pairs_workspace_bytes(*args) == 0, args
    assert L.namp_loo_pairs_offset(1, 100, 24, 4) == 0
    for bad in (0, 65, -1):
        assert L.namp_loo_pairs(bad) == -1 and b"n_maps" in L.namp_last_error()
    # a failed namp_decoder_loo clears the attachment: the next call no longer reports one
    null_call = lambda: L.namp_decoder_loo(None, None, None, None, None, None, None, None, None, None, 0, 1, 10, 4, None)
    assert L.namp_loo_pairs(3) == 0
    assert null_call() == -1 and b"pair tables were attached" in L.namp_last_error()
    assert null_call() == -1 and b"null pointer" in L.namp_last_error() and b"attached" not in L.namp_last_error()
    assert L.namp_loo_pairs(3) == 0 and L.namp_loo_pairs(65) == -1                           # an invalid attach leaves nothing attached
    assert null_call() == -1 and b"attached" not in L.namp_last_error()


def test_pair_arguments_are_refused_before_any_device_work(weights_np):
    from na_mpnn_amd.model import ProteinMPNN
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=K, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    _, _, fd, pairs, _, _ = premise_case()
    with pytest.raises(NotImplementedError, match="pair classes"):
        m.conditional_probs(dict(fd, paired_wobble=True))
    with pytest.raises(NotImplementedError):
        m.conditional_probs(dict(fd, symmetry_residues=[[1, 2]], symmetry_weights=[[1.0, 1.0]]))
    with pytest.raises(NotImplementedError):
        m.conditional_probs(dict(fd, state_weights=[0.5, 0.5]))
    fd2 = {k: (torch.cat((v, v)) if torch.is_tensor(v) and k != "randn" else v) for k, v in fd.items()}
    with pytest.raises(ValueError, match="one input complex"):
        m.conditional_probs(fd2)
    with pytest.raises(ValueError, match="two pairs"):
        m.conditional_probs(dict(fd, paired_residues=pairs + [(pairs[0][0], 20)]))


def test_a_pair_only_call_builds_one_section_through_either_route():
    """A feature_dict with base pairs alone gives the builder the same input section, number of tables and index of the ties with
    tied=False and tied=True (a pair's partner table IS its successor cycle), in token maps and in class tables; in token maps it is
    the section that section_of of the GPU pair tests lays out independently from the same pairs, weights and maps."""
    from na_mpnn_amd.model import ProteinMPNN
    import class_loo_ref
    from test_gpu_pair_conditional import section_of
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=K, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    _, fd, pairs = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    fd = dict(fd, paired_weights=(1.0, 0.5))
    for classes, fdc in ((False, fd), (True, class_loo_ref.case_inputs("l48_k16"))):
        a, b = m._conditional_arguments(fdc, 1, 48, None, False, classes), m._conditional_arguments(fdc, 1, 48, None, True, classes)
        assert a is not b and a["n_tables"] == b["n_tables"]
        assert a["section"].dtype == torch.int32 and torch.equal(a["section"], b["section"])
        assert a["index"].dtype == torch.int64 and torch.equal(a["index"], b["index"])
        assert a["index"].tolist() == [list(p) for p in fdc["paired_residues"]]
    # the first member reads through the identity, the second through the Watson-Crick map of the pair's kind (RNA with RNA, DNA with
    # DNA: "same"; DNA with RNA: "cross"), the maps numbered as the pairs first need them
    a = m._conditional_arguments(fd, 1, 48)
    dna = fd["dna_mask"][0].tolist()
    kinds = ["same" if dna[i] == dna[j] else "cross" for i, j in pairs]
    assert kinds == ["same", "cross", "cross", "same", "same"]
    maps = [list(range(64))] + [spec.token_map(spec.restype_to_int(), kind) + list(range(33, 64)) for kind in ("same", "cross")]
    want = section_of(48, pairs, [(1.0, 0.5)] * 5, maps, 3, second=[1 + ("same", "cross").index(kind) for kind in kinds])
    assert a["n_tables"] == 3 and torch.equal(a["section"], want)
