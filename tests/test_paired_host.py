"""CPU tests of base-paired design: the token maps of spec, the host-side plan (mapped_groups, the CLI's pair flags) and the
recombination helper of the reference (paired_ref) on the CPU oracle."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import cli, spec
from na_mpnn_amd.model import mapped_groups, symmetry_visits
from oracle import cpu_ref
import paired_ref
import tied_states_ref

torch.set_grad_enabled(False)
AMINO = spec.RESTYPES[:20]


@pytest.mark.parametrize("shared", [False, True])
def test_token_maps(shared):
    rti = spec.restype_to_int(shared)
    same, cross = spec.token_map(rti, "same"), spec.token_map(rti, "cross")
    for m in (same, cross):
        assert sorted(m) == list(range(33)) and all(m[m[t]] == t for t in range(33))
        assert all(m[rti[n]] == rti[n] for n in AMINO + list(spec.SPECIAL_RESTYPES))
        assert spec.check_token_map(rti, m) == m
    dna, rna = {"DA", "DC", "DG", "DT"}, {"A", "C", "G", "U"}
    for a, b in spec.NA_CANONICAL_BASE_PAIRS:                       # pair for pair: the map of the pair's kind sends a to b
        m = same if ({a, b} <= dna or {a, b} <= rna) else cross
        assert m[rti[a]] == rti[b], (a, b)
    for name, m in (("same", spec.WC_SAME), ("cross", spec.WC_CROSS)):
        assert all((a, b) in spec.NA_CANONICAL_BASE_PAIRS for a, b in m.items()), name
    assert (same == cross) == shared
    if not shared:
        assert cross[rti["DA"]] == rti["U"] and cross[rti["A"]] == rti["DT"] and same[rti["A"]] == rti["U"]


def test_check_token_map_refuses():
    rti = spec.restype_to_int()
    m = list(range(33)); m[0], m[1], m[2] = 1, 2, 0
    with pytest.raises(ValueError, match="not an involution"):
        spec.check_token_map(rti, m)
    m = list(range(33)); m[rti["UNK"]], m[0] = 0, rti["UNK"]
    with pytest.raises(ValueError, match="special token UNK"):
        spec.check_token_map(rti, m)
    with pytest.raises(ValueError, match="expected 33"):
        spec.check_token_map(rti, list(range(32)))


def test_mapped_groups_plan():
    rti = spec.restype_to_int()
    L = 12
    polymer = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    fixed = [False] * L
    fixed[9] = True
    g, w, m, pl = mapped_groups(L, rti, [(4, 7), (5, 9), (8, 11)], None, polymer, fixed)
    same, cross, ident = spec.token_map(rti, "same"), spec.token_map(rti, "cross"), list(range(33))
    assert g == [[4, 7], [9, 5], [8, 11]]                                   # the fixed member is listed first
    assert w == [[1.0, 1.0]] * 3 and m == [[ident, same], [ident, cross], [ident, same]]
    assert pl == [(4, 7, 1.0, 1.0, "same"), (9, 5, 1.0, 1.0, "cross"), (8, 11, 1.0, 1.0, "same")]
    fixed[5] = True                                                         # both fixed: allowed, the listed order stays
    assert mapped_groups(L, rti, [(5, 9)], (0.5, 2.0), polymer, fixed)[:2] == ([[5, 9]], [[0.5, 2.0]])
    # per-pair weights follow a swapped pair
    fixed[5] = False
    assert mapped_groups(L, rti, [(4, 7), (5, 9)], [(1.0, 1.0), (0.5, 2.0)], polymer, fixed)[1] == [[1.0, 1.0], [2.0, 0.5]]
    # with symmetry_residues: the union, i's side first, weights multiplied, maps composed
    g, w, m, pl = mapped_groups(L, rti, [(5, 10)], (2.0, 3.0), polymer, [False] * L, [[4, 5], [10, 11]], [[0.5, 0.25], [1.0, 0.5]])
    assert pl is None and g == [[4, 5, 10, 11]] and w == [[1.0, 0.5, 3.0, 1.5]] and m == [[ident, ident, cross, cross]]
    # explicit maps pass through; identity for None
    g, w, m, _ = mapped_groups(L, rti, groups=[[4, 6], [8, 9]], weights=[[1.0, 1.0], [1.0, 1.0]], maps=[[None, torch.tensor(same)], None])
    assert g == [[4, 6], [8, 9]] and m == [[ident, same], [ident, ident]]
    # the visits of the plan: a pair is emitted in listed order by whichever member the order reaches first
    g, w, _, _ = mapped_groups(L, rti, [(4, 7)], None, polymer, [False] * L)
    assert symmetry_visits(g, w, [7, 0, 4] + [1, 2, 3, 5, 6, 8, 9, 10, 11], L)[0][:3] == [4, 7, 0]


def test_mapped_groups_errors():
    rti = spec.restype_to_int()
    L = 8
    polymer = [0, 0, 1, 1, 1, 2, 2, 2]
    mg = lambda pairs, **kw: mapped_groups(L, rti, pairs, None, polymer, [False] * L, **kw)
    with pytest.raises(ValueError, match="residue 3 is in two pairs"):
        mg([(2, 3), (3, 5)])
    with pytest.raises(ValueError, match="residue 4 is paired with itself"):
        mg([(4, 4)])
    with pytest.raises(ValueError, match="residue 1 is not a nucleic acid"):
        mg([(1, 5)])
    with pytest.raises(ValueError, match=r"residue 8 is outside \[0, 8\)"):
        mg([(2, 8)])
    with pytest.raises(ValueError, match=r"residue -1 is outside"):
        mg([(-1, 2)])
    with pytest.raises(ValueError, match="already tied"):
        mg([(2, 5)], groups=[[2, 5]], weights=[[1.0, 1.0]])
    bad = list(range(33)); bad[21], bad[22], bad[23] = 22, 23, 21
    with pytest.raises(ValueError, match="not an involution"):
        mapped_groups(L, rti, groups=[[2, 3]], weights=[[1.0, 1.0]], maps=[[None, bad]])
    moved = list(range(33)); moved[rti["MAS"]], moved[21] = 21, rti["MAS"]
    with pytest.raises(ValueError, match="special token MAS"):
        mapped_groups(L, rti, groups=[[2, 3]], weights=[[1.0, 1.0]], maps=[[None, moved]])
    with pytest.raises(ValueError, match="parallel to symmetry_residues"):
        mapped_groups(L, rti, groups=[[2, 3]], weights=[[1.0, 1.0]], maps=[None, None])
    # maps that are involutions one by one, but whose composition through a pair is not
    swap_ac = list(range(33)); swap_ac[21], swap_ac[22] = 22, 21
    with pytest.raises(ValueError, match="token map of residue 3"):
        mg([(2, 4)], groups=[[4, 3]], weights=[[1.0, 1.0]], maps=[[swap_ac, None]])


def test_cli_pair_flags():
    chains = list("AAAABBBBC")
    enc = [f"{c}{i}" for i, c in enumerate(chains)]
    assert cli.parse_pairs("A0:B7, A1:B6", "", enc, chains) == [(0, 7), (1, 6)]
    assert cli.parse_pairs("", "A:B", enc, chains) == [(0, 7), (1, 6), (2, 5), (3, 4)]         # antiparallel
    assert cli.parse_pairs("", "", enc, chains) == []
    with pytest.raises(ValueError, match="equal lengths"):
        cli.parse_pairs("", "A:C", enc, chains)
    with pytest.raises(ValueError, match="not in the structure"):
        cli.parse_pairs("", "A:D", enc, chains)
    with pytest.raises(ValueError, match="no residue 'B9'"):
        cli.parse_pairs("A0:B9", "", enc, chains)
    with pytest.raises(ValueError, match="RES:RES"):
        cli.parse_pairs("A0", "", enc, chains)
    args = cli.build_parser().parse_args(["--out_folder", "x", "--paired_strands", "A:B", "--paired_residues", "A1:B2", "--multi_state", "1"])
    assert (args.paired_strands, args.paired_residues, args.multi_state) == ("A:B", "A1:B2", 1)


def test_recombination_with_identity_maps_is_the_tied_distribution(weights_np):
    """On the CPU oracle (L = 30 <= K = 48): paired_probs with identity maps equals tied_states_ref.tied_probs with one state for the
    same groups; with the Watson-Crick maps the second member's row is the first's, permuted."""
    L, K, bs, T = 30, 48, 2, 0.5
    rti = spec.restype_to_int()
    cx, fd, pairs = paired_ref.make_case(L, bs, T, 3, seed=4100, fixed_every=0)
    w = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    groups, weights, maps = paired_ref.groups_of(fd, rti)
    assert [tuple(g) for g in groups] == pairs
    S = torch.from_numpy(cx["S"].astype(np.int64))[None].repeat(bs, 1)
    fdo = dict(fd, symmetry_residues=groups, symmetry_weights=weights)
    lp = cpu_ref.sample_symmetric(w, fdo, K, S_forced=S)["log_probs"]
    ident = [[list(range(33))] * len(g) for g in groups]
    mine = paired_ref.paired_probs(lp, fd, groups, weights, ident)
    theirs = tied_states_ref.tied_probs(lp[:, None], dict(fdo, state_weights=[1.0]), groups, weights)
    assert torch.allclose(mine, theirs, rtol=0, atol=1e-7) and float(mine.sum(-1).min()) > 0.999
    p = paired_ref.paired_probs(lp, fd, groups, weights, maps)
    for (i, j), gm in zip(pairs, maps):
        assert torch.equal(p[:, j][:, gm[1]], p[:, i]) and not torch.equal(p[:, j], p[:, i])
    assert float((p - mine).abs().max()) > 1e-3                                 # the maps matter
