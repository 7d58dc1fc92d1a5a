"""CPU tests of the leave-one-out conditionals (ProteinMPNN.conditional_probs): the stream ranks of the dense form, the index grids
of the cone (numpy restatement of loo_prepare_kernel / loo_edges_kernel against brute-force set definitions, with the counted work
of DESIGN.md 5.5), the library's argument checks, and the definition itself on the CPU oracle."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN, leave_one_out_ranks
from loo_numpy import cone_sets, loo_grids


def explicit_ranks(order):
    """rank of every stream from the explicitly built order_i = order with i taken out and appended."""
    L = len(order)
    out = np.empty((L, L), np.int64)
    for i in range(L):
        oi = [j for j in order if j != i] + [i]
        out[i, oi] = np.arange(L)
    return out


@pytest.mark.parametrize("L,seed", [(1, 0), (2, 1), (7, 2), (40, 3), (97, 4)])
def test_leave_one_out_ranks_equal_the_explicit_orders(L, seed):
    rng = np.random.default_rng(seed)
    B = 2
    mask = (rng.random((B, L)) > 0.2).astype(np.float32)
    chain = (rng.random((B, L)) > 0.3).astype(np.float32)
    randn = rng.standard_normal((B, L)).astype(np.float32)
    if L > 4:
        randn[:, 3] = randn[:, 1]; randn[0, 4] = -randn[0, 1]            # ties in |randn|
    order = ProteinMPNN.decoding_order(torch.from_numpy(mask * chain), torch.from_numpy(randn))
    rank = ProteinMPNN.ranks_of(order)
    for dt in (torch.int64, torch.int32):
        got = leave_one_out_ranks(rank.to(dt))
        assert got.dtype == dt and tuple(got.shape) == (B, L, L)
        for b in range(B):
            assert np.array_equal(got[b].numpy(), explicit_ranks(order[b].tolist()))
    if L > 4:                                                             # a slice of the streams (the dense form's chunks)
        assert torch.equal(leave_one_out_ranks(rank, 2, 5), leave_one_out_ranks(rank)[:, 2:5])


def graph_case(n, k, masked_frac=0.0, seed=5):
    g = synth.make_graph(seed, 1, n, k, masked_frac=masked_frac)
    E_idx, mask = g["E_idx"][0], g["mask"][0]
    order = np.argsort((mask * g["chain_mask"][0] + 1e-4) * np.abs(g["randn"][0]), kind="stable")
    rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    return E_idx, rank, mask


@pytest.mark.parametrize("n,k,mf,per_stream", [(97, 32, 0.0, (14.4, 13.9)), (300, 48, 0.0, (21.8, 21.7)), (80, 16, 0.05, None),
                                                (20, 48, 0.1, None)])
def test_cone_grids_equal_the_set_definitions(n, k, mf, per_stream):
    """rev and the two active grids against sets built straight from the definition (L < K and masked residues included), and the
    counted work of the table in DESIGN.md 5.5: layer-1 / layer-2 evaluations per stream that residue i's own layers read."""
    E_idx, rank, mask = graph_case(n, k, mf)
    rev, act1, act2 = loo_grids(E_idx, rank, mask)
    K = E_idx.shape[1]
    for a in range(n):
        for kk in range(K):
            b = E_idx[a, kk]
            pos = np.nonzero(E_idx[b] == a)[0]
            assert rev[a, kk] == (pos[0] if len(pos) else -1)
    A1, need1, need2 = cone_sets(E_idx, rank, mask)
    for i in range(n):
        assert {int(m) for m, kk in zip(*np.nonzero(act1)) if E_idx[m, kk] == i} == A1[i]
        assert {int(E_idx[i, kq]) for kq in np.nonzero(act2[i])[0]} == need2[i]
        assert need1[i] <= A1[i]
    assert act1.sum() == sum(map(len, A1)) <= n * K and act2.sum() == sum(map(len, need2))     # every directed edge is one item at most
    if per_stream:
        assert round(sum(map(len, need1)) / n, 1) == per_stream[0]
        assert round(act2.sum() / n, 1) == per_stream[1]


def test_loo_entry_points_validate_without_a_gpu():
    L = hip.lib()
    assert L.namp_loo_workspace_bytes(1, 1000, 48, 3) > 5 * 1000 * 48 * 128 * 4
    assert L.namp_loo_workspace_bytes(1, 3000, 48, 3) < 3 * L.namp_loo_workspace_bytes(1, 1000, 48, 3) + (1 << 20)   # linear in N
    assert L.namp_loo_workspace_bytes(1, 100, 24, 4) == 0 and L.namp_loo_workspace_bytes(0, 100, 24, 3) == 0
    rc = L.namp_decoder_loo(None, None, None, None, None, None, None, None, None, None, 0, 1, 10, 4, None)
    assert rc == -1 and b"null pointer" in L.namp_last_error()


def test_conditional_probs_needs_a_device_and_a_known_method(weights_np):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=16, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    cx = synth.make_complex(seed=3, n=24)
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd["batch_size"] = 1
    with pytest.raises(ValueError):
        m.conditional_probs(fd, method="nope")
    with pytest.raises(RuntimeError, match="HIP device"):
        m.conditional_probs(fd)


def test_conditionals_are_not_score_on_the_oracle(weights_np):
    """The definition on the CPU oracle (n = 40): row i of the stream that decodes i last; most rows differ from score()'s."""
    from oracle import cpu_ref
    from loo_numpy import oracle_conditional
    torch.set_grad_enabled(False)
    w = cpu_ref.to_torch(weights_np)
    cx = synth.make_complex(seed=11, n=40)
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    lp, order, _ = oracle_conditional(w, fd, 16)
    sc = cpu_ref.score(w, dict(fd, batch_size=1), 16)
    assert torch.equal(order[0], sc["decoding_order"])
    assert float((lp.exp().sum(-1) - 1).abs().max()) < 1e-5
    last = int(order[0][-1])                       # the residue score() decodes last already sees everything: the same row
    assert float((lp[0, last] - sc["log_probs"][0, last]).abs().max()) < 1e-5
    assert int(((lp - sc["log_probs"]).abs().amax(-1) > 1e-3).sum()) > 20
