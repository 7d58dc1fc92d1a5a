"""CPU tests of the mutational scan (ProteinMPNN.score_mutations): the per-site sets against the oracle's decoder states, the
argument checks, the expansion of pairs=True and the chunk cutter.  No device needed."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN, mutation_chunks, variant_row_order
from oracle import cpu_ref
import library_ref as LR
import mutation_ref as MR

torch.set_grad_enabled(False)


def cpu_fd(cx):
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd["batch_size"] = 1
    return fd


def host_model():
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int())


@pytest.mark.parametrize("name", ["n97", "crossing", "LltK", "all"])
def test_rows_that_differ_from_the_wild_type_are_the_cone_of_the_site(weights_np, name):
    """Per site of the GPU cases (mutation_ref.case_sites): the rows whose oracle decoder states differ between the wild type and a
    mutant at layer l lie inside act_l(site), and over three mutants that change every residue of the site their union EQUALS
    act_l(site); the last-decoded residue reaches nothing (U_l is the site alone); the cones of the "disjoint" site's two residues
    do not meet; some cone size is no multiple of the 16-row item tile."""
    k, cx, pos, tok = LR.make_case(name)
    fd, w = cpu_fd(cx), cpu_ref.to_torch(weights_np)
    E_idx = LR.encoded(w, fd, k, name)[2][0].numpy()
    order = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"])[0].numpy()
    rank = LR.ranks_of(order)
    sites, site_tokens, names = MR.case_sites(cx, E_idx, order)
    assert "eight" in names and (sites[names.index("eight")] >= 0).sum() == 8
    assert ("disjoint" in names) == (name != "LltK")             # (L < K: every residue reaches all that decode later)
    assert ("masked" in names) == (name in ("n97", "crossing"))
    wild = LR.oracle_decoder_states(w, fd, k, cx["S"], key=name)
    sizes, _ = MR.site_rows(E_idx, rank, cx["mask"], sites)
    assert (sizes % 16 != 0).any()
    for s, site in enumerate(sites):
        res = [int(r) for r in site if r >= 0]
        lists, acts = MR.site_lists(E_idx, rank, cx["mask"], res)
        union = [np.zeros(len(cx["S"]), bool) for _ in range(3)]
        for shift in (1, 2, 3):
            S_k = cx["S"].copy()
            for r in res:
                al = list(MR.alphabet(cx, r))
                S_k[r] = al[(al.index(int(cx["S"][r])) + shift) % len(al)]
            states = LR.oracle_decoder_states(w, fd, k, S_k, key=name)
            for l in range(3):
                differ = ((states[l] - wild[l]).abs().amax(-1) != 0).numpy()
                assert not (differ & ~acts[l]).any(), (name, names[s], l)
                union[l] |= differ
        for l in range(3):
            assert np.array_equal(union[l], acts[l]), (name, names[s], l)
            assert set(res) <= set(lists[l].tolist()) and len(lists[l]) == sizes[s, l]
        if names[s] == "last":
            assert sizes[s].tolist() == [1, 1, 1]
        if names[s] == "disjoint":
            a, b = (set(MR.site_lists(E_idx, rank, cx["mask"], [r])[0][2].tolist()) for r in res)
            assert not (a & b) and len(a) > 1
        if names[s] == "masked":
            assert cx["mask"][res[0]] == 0
        if names[s] == "neighbours":
            assert res[1] in E_idx[res[0]]


def test_argument_checks():
    """B != 1, positions out of range / not ascending, M > 8, a repeated residue, both forms at once: ValueError; a token outside
    [0, vocab): IndexError; state_weights and pairs=True with paired_wobble: NotImplementedError; an unknown method: ValueError.  The
    default scan walks the residues with mask * chain_mask != 0 over their own alphabets."""
    k, cx, pos, tok = LR.make_case("n97")
    fd, m = cpu_fd(cx), host_model()
    L = len(cx["S"])
    st, tk, scan = m._mutation_arguments(fd, None, None, None, None, False)
    assert scan["positions"] == pos.tolist() and st.shape == (len(pos), 1) and st[:, 0].tolist() == pos.tolist()
    assert len(tk) == 4 * len(pos)                                                      # nucleotides: four letters each
    for s, p in enumerate(pos):
        assert sorted(tk[tk[:, 0] == s, 1].tolist()) == list(MR.alphabet(cx, p))
    assert scan["valid"].sum() == len(tk) and scan["valid"].shape == (len(pos), len(scan["tokens"]))
    st2, tk2, scan2 = m._mutation_arguments(fd, torch.tensor([3, 90]), torch.tensor([1, 31]), None, None, False)
    assert st2.tolist() == [[3], [90]] and tk2.tolist() == [[0, 1], [0, 31], [1, 1], [1, 31]] and scan2["valid"].all()
    for bad in ([0, L], [-1, 3], [5, 3], [3, 3]):
        with pytest.raises(ValueError):
            m._mutation_arguments(fd, torch.tensor(bad), None, None, None, False)
    with pytest.raises(IndexError):
        m._mutation_arguments(fd, torch.tensor([3]), torch.tensor([33]), None, None, False)
    sites = torch.tensor([[3, 5, -1], [7, -1, -1]])
    toks = torch.tensor([[0, 1, 2, 32], [1, 4, 9, 9]])
    st3, tk3, scan3 = m._mutation_arguments(fd, None, None, sites, toks, False)
    assert scan3 is None and st3.tolist() == sites.tolist() and tk3.tolist() == [[0, 1, 2, 0], [1, 4, 0, 0]]
    with pytest.raises(ValueError):
        m._mutation_arguments(fd, torch.tensor([3]), None, sites, toks, False)         # both forms
    with pytest.raises(ValueError):
        m._mutation_arguments(fd, None, None, torch.zeros(1, 9, dtype=torch.long) + torch.arange(9), torch.zeros(1, 10, dtype=torch.long), False)
    with pytest.raises(ValueError):
        m._mutation_arguments(fd, None, None, torch.tensor([[3, 3]]), torch.tensor([[0, 1, 1]]), False)      # a repeated residue
    with pytest.raises(ValueError):
        m._mutation_arguments(fd, None, None, torch.tensor([[3, L]]), torch.tensor([[0, 1, 1]]), False)
    with pytest.raises(ValueError):
        m._mutation_arguments(fd, None, None, sites, torch.tensor([[2, 1, 1, 1]]), False)                    # a site index out of range
    with pytest.raises(IndexError):
        m._mutation_arguments(fd, None, None, sites, torch.tensor([[0, 1, 33, 0]]), False)
    fd2 = {k_: (torch.cat((v, v)) if isinstance(v, torch.Tensor) else v) for k_, v in fd.items()}
    with pytest.raises(ValueError):
        m.score_mutations(fd2)
    with pytest.raises(NotImplementedError):
        m.score_mutations(dict(fd, state_weights=[0.5, 0.5]))
    with pytest.raises(ValueError):
        m.score_mutations(fd, method="sparse")
    with pytest.raises(RuntimeError):
        m.score_mutations(fd)                                                           # a CPU feature_dict, as for the other calls


def test_pairs_expand_to_canonical_duplexes():
    """pairs=True on a 2 x 6 RNA duplex: scanning any member edits the pair — the site is (first listed, second listed), scanned
    once from its first member, the partner's token is the Watson-Crick complement (spec.WC_SAME) —, an unpaired residue stays a
    site of one; paired_wobble raises NotImplementedError."""
    cx = synth.make_complex(seed=12, n=12, n_chains=2, frac_protein=0.0, frac_dna=0.0)
    assert int(cx["rna_mask"].sum()) == 12
    fd, m = cpu_fd(cx), host_model()
    fd["paired_residues"] = [(i, 11 - i) for i in range(5)]                             # residues 5 and 6 stay unpaired
    st, tk, scan = m._mutation_arguments(fd, None, None, None, None, True)
    assert st.tolist() == [[0, 11], [1, 10], [2, 9], [3, 8], [4, 7], [5, -1], [6, -1]]
    assert scan["positions"] == [0, 1, 2, 3, 4, 5, 6] and scan["tokens"] == [26, 27, 28, 29] and scan["valid"].all()
    P = spec.token_map(spec.restype_to_int(), "same")
    rti = spec.restype_to_int()
    assert P[rti["A"]] == rti["U"] and P[rti["G"]] == rti["C"]
    for s, t, u in tk.tolist():
        assert u == (P[t] if s < 5 else 0)
    assert len(tk) == 7 * 4
    st2, tk2, scan2 = m._mutation_arguments(fd, torch.tensor([9, 10]), None, None, None, True)      # second members: the pairs, from the first
    assert st2.tolist() == [[2, 9], [1, 10]] and scan2["positions"] == [2, 1]
    st3, _, _ = m._mutation_arguments(fd, torch.tensor([1, 10]), None, None, None, True)            # both members: scanned once
    assert st3.tolist() == [[1, 10]]
    st4, tk4, _ = m._mutation_arguments(fd, torch.tensor([1, 10]), None, None, None, False)         # pairs=False: the ties are not read
    assert st4.tolist() == [[1], [10]] and tk4.shape == (8, 2)
    with pytest.raises(NotImplementedError):
        m._mutation_arguments(dict(fd, paired_wobble=True), None, None, None, None, True)
    with pytest.raises(ValueError):
        m._mutation_arguments({k: v for k, v in fd.items() if k != "paired_residues"}, None, None, None, None, True)


def test_chunk_cutter():
    """No chunk exceeds the budget unless a single variant does alone; every variant is in exactly one chunk; the chunks are grouped
    by site (a site's variants are neighbours in the cut order, which is stable)."""
    rng = np.random.default_rng(3)
    for trial in range(20):
        n_sites = int(rng.integers(1, 9))
        site_rows = rng.integers(1, 40, (n_sites, 3)).tolist()
        site_index = rng.integers(0, n_sites, int(rng.integers(0, 60))).tolist()
        budget = int(rng.integers(20, 400))
        perm, cuts = mutation_chunks(site_index, site_rows, budget)
        assert sorted(perm) == list(range(len(site_index)))
        assert [site_index[v] for v in perm] == sorted(site_index)
        for s in range(n_sites):
            mine = [v for v in perm if site_index[v] == s]
            assert mine == sorted(mine)
        covered = [q for q0, q1 in cuts for q in range(q0, q1)]
        assert covered == list(range(len(perm))) and all(q1 > q0 for q0, q1 in cuts)
        for q0, q1 in cuts:
            total = sum(sum(site_rows[site_index[v]]) for v in perm[q0:q1])
            assert total <= budget or q1 - q0 == 1
        for (a0, a1), (b0, b1) in zip(cuts, cuts[1:]):                                   # (greedy: the next variant did not fit)
            total = sum(sum(site_rows[site_index[v]]) for v in perm[a0:a1])
            assert total + sum(site_rows[site_index[perm[b0]]]) > budget
    assert mutation_chunks([], [[1, 1, 1]], 10) == ([], [])
    assert mutation_chunks([0, 0, 0], [[50, 50, 50]], 10)[1] == [(0, 1), (1, 2), (2, 3)]


@pytest.mark.parametrize("name,site_index,rows3", [
    ("three sites interleaved", [2, 0, 1, 0, 2, 1, 1, 0], [3, 1, 5]),
    ("a site without rows", [1, 0, 2, 1, 0, 2], [4, 0, 2]),
    ("one variant", [0], [3]),
    ("the identity", [0, 0, 1, 2, 2], [2, 3, 1])])
def test_rows_return_to_the_order_the_variants_were_given_in(name, site_index, rows3):
    """variant_row_order against a loop: the variants run grouped by site (mutation_chunks' perm), each leaving rows3[site] rows; the
    restored rows are every variant's own, in the order given, and row_offsets are their prefix sums.  The identity order takes the
    fast path: the rows stay untouched."""
    n = len(site_index)
    perm = mutation_chunks(site_index, [[0, 0, r] for r in rows3], 10 ** 6)[0]
    counts = [rows3[s] for s in site_index]
    ran = [(v, k) for v in perm for k in range(counts[v])]                              # what the calls leave: (variant, its k-th row)
    offs, idx = variant_row_order(np.asarray(perm, np.int64), torch.tensor(counts, dtype=torch.int64))
    assert offs.dtype == torch.int64 and offs.tolist() == [sum(counts[:v]) for v in range(n + 1)]
    want = [(v, k) for v in range(n) for k in range(counts[v])]
    if name == "the identity":
        assert perm == list(range(n)) and idx is None and ran == want
    else:
        assert perm != list(range(n)) or n == 1
        got = ran if idx is None else [ran[q] for q in idx.tolist()]
        assert got == want and (idx is None or (idx.dtype == torch.int64 and sorted(idx.tolist()) == list(range(len(ran)))))
    if name == "a site without rows":
        assert 0 in counts
