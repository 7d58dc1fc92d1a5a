"""CPU tests of base-paired design with G-U wobble: the class tables of spec, the host-side plan (mapped_groups with wobble, the
model's deduplicated tables, the CLI's flags) and the identities of the reference helper (wobble_ref) on the CPU oracle."""
import argparse

import numpy as np
import pytest
import torch

from na_mpnn_amd import cli, spec
from na_mpnn_amd.model import ProteinMPNN, mapped_groups
import paired_ref
import wobble_ref

torch.set_grad_enabled(False)
GU, UG, V = spec.CLASS_GU, spec.CLASS_UG, len(spec.RESTYPES)


@pytest.mark.parametrize("shared", [False, True])
def test_class_tables(shared):
    rti = spec.restype_to_int(shared)
    ident = list(range(V))
    own = {"dna": ("DG", "DT"), "rna": ("G", "U")}
    for kind in spec.PAIR_KINDS:
        wc = spec.token_map(rti, "same" if kind in ("dna-dna", "rna-rna") else "cross")
        pa, pb = kind.split("-")
        for wobble in (False, True):
            first, second = (spec.class_table(rti, kind, wobble, f) for f in (True, False))
            for t in (first, second):
                assert len(t) == 64 and spec.check_class_table(rti, t) == t
                assert t[GU + 2:] == [-1] * (64 - GU - 2)                       # lanes 35..63 are never a class
            assert first[:V] == ident and second[:V] == wc                      # lanes 0..32: the parent's maps
            if wobble and kind != "dna-dna":                                    # a pair with an RNA member, and only if asked
                assert (first[GU], second[GU]) == (rti[own[pa][0]], rti[own[pb][1]])     # first holds its G, second its U / T
                assert (first[UG], second[UG]) == (rti[own[pa][1]], rti[own[pb][0]])     # first holds its U / T, second its G
            else:
                assert first[GU] == first[UG] == second[GU] == second[UG] == -1
    # without wobble the kinds of the token maps are accepted; with wobble they do not say which member is RNA
    assert spec.class_table(rti, "cross", False, False)[:V] == spec.token_map(rti, "cross")
    with pytest.raises(ValueError, match="which member is RNA"):
        spec.class_table(rti, "cross", True, True)
    rna = spec.class_table(rti, "rna-rna", True, True)
    assert (rna[GU], rna[UG]) == ((rti["DG"], rti["DT"]) if shared else (rti["G"], rti["U"]))


def test_check_class_table_refuses():
    rti = spec.restype_to_int()
    good = spec.class_table(rti, "rna-rna", True, False)
    t = list(good); t[GU] = rti["MAS"]
    with pytest.raises(ValueError, match="special token MAS"):
        spec.check_class_table(rti, t)
    t = list(good); t[rti["UNK"]], t[0] = 0, rti["UNK"]
    with pytest.raises(ValueError, match="special token UNK"):
        spec.check_class_table(rti, t)
    for bad in (V, -2):
        t = list(good); t[UG] = bad
        with pytest.raises(ValueError, match=r"entries in \[-1, 33\)"):
            spec.check_class_table(rti, t)
    t = list(good); t[0], t[1], t[2] = 1, 2, 0
    with pytest.raises(ValueError, match="not an involution"):
        spec.check_class_table(rti, t)
    t = list(good); t[40] = rti["G"]
    with pytest.raises(ValueError, match="beyond the 35 pair classes"):
        spec.check_class_table(rti, t)
    with pytest.raises(ValueError, match="expected 64"):
        spec.check_class_table(rti, good[:V])


def test_mapped_groups_with_wobble():
    rti = spec.restype_to_int()
    L = 12
    polymer = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    fixed = [False] * L
    fixed[9] = True
    pairs = [(4, 7), (5, 9), (8, 11)]
    g, w, t, pl, cb = mapped_groups(L, rti, pairs, None, polymer, fixed, wobble=True, wobble_bias=0.5)
    assert g == [[4, 7], [9, 5], [8, 11]]                                   # the fixed member is listed first
    assert pl == [(4, 7, 1.0, 1.0, "same"), (9, 5, 1.0, 1.0, "cross"), (8, 11, 1.0, 1.0, "same")]
    ct = spec.class_table
    assert t[0] == [ct(rti, "dna-dna", False, True), ct(rti, "dna-dna", False, False)]           # a DNA-DNA pair never wobbles
    assert t[1] == [ct(rti, "rna-dna", True, True), ct(rti, "rna-dna", True, False)]             # (listed RNA first: 9 is fixed)
    assert t[2] == [ct(rti, "rna-rna", True, True), ct(rti, "rna-rna", True, False)]
    assert t[1][0][GU] == rti["G"] and t[1][1][GU] == rti["DT"] and t[1][0][UG] == rti["U"] and t[1][1][UG] == rti["DG"]
    zero = [0.0] * 64
    half = list(zero); half[GU] = half[UG] = 0.5
    assert cb == [zero, half, half]
    # the groups, weights and pair list are those of the call without wobble; wobble=False gives the maps as tables
    g0, w0, m0, pl0 = mapped_groups(L, rti, pairs, None, polymer, fixed)
    assert (g0, w0, pl0) == (g, w, pl)
    g1, w1, t1, pl1, cb1 = mapped_groups(L, rti, pairs, None, polymer, fixed, wobble=False)
    assert (g1, w1, pl1) == (g, w, pl) and cb1 == [zero] * 3
    assert t1 == [[list(m) + [-1] * 31 for m in ms] for ms in m0]
    # per-pair flags and biases
    g, w, t, pl, cb = mapped_groups(L, rti, pairs, None, polymer, fixed, wobble=[True, False, True], wobble_bias=[1.0, 2.0, -3.0])
    assert t[1] == t1[1] and cb[1] == zero and t[2][0][GU] == rti["G"] and cb[2][GU] == cb[2][UG] == -3.0 and cb[0] == zero
    # a wobble pair does not join a symmetry group; a pair without wobble beside it may
    with pytest.raises(ValueError, match="residue 10 of the wobble pair .* sits in a symmetry_residues group"):
        mapped_groups(L, rti, [(5, 10)], None, polymer, [False] * L, [[10, 11]], [[1.0, 0.5]], wobble=True)
    g, w, t, pl, cb = mapped_groups(L, rti, [(5, 10), (8, 9)], None, polymer, [False] * L, [[10, 11]], [[1.0, 0.5]], wobble=[False, True])
    cross = spec.token_map(rti, "cross")
    assert g == [[5, 10, 11], [8, 9]] and pl is None and t[0] == [list(range(V)) + [-1] * 31] + [cross + [-1] * 31] * 2
    assert t[1][1][GU] == rti["U"] and cb[0] == zero
    with pytest.raises(ValueError, match="needs the polymer type"):
        mapped_groups(L, rti, [(5, 10)], wobble=True)


def test_model_tables_are_deduplicated_on_table_and_bias():
    rti = spec.restype_to_int()
    L = 12
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=8, atom_dict=spec.atom_dict(), restype_to_int=rti,
                    polytype_to_int=spec.polytype_to_int())
    polymer = torch.tensor([[0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]])
    fd = {"dna_mask": (polymer == 1).int(), "rna_mask": (polymer == 2).int(), "mask": torch.ones(1, L), "chain_mask": torch.ones(1, L),
          "paired_residues": [(8, 9), (10, 11), (4, 5), (6, 7)]}
    assert m._mapped_arguments(dict(fd), 1, L)[5] is None                     # no wobble key: the token maps
    assert m._mapped_arguments(dict(fd, paired_wobble=False, paired_wobble_bias=1.0), 1, L)[2][0] == list(range(64))
    groups, weights, table, idx, pl, bias = m._mapped_arguments(dict(fd, paired_wobble=True, paired_wobble_bias=[0.5, 0.5, 0.5, 0.5]), 1, L)
    # table 0: untied residues; both RNA pairs share two tables, both DNA pairs share one new one (their first members are table 0)
    assert len(table) == len(bias) == 4 and idx == [0, 0, 0, 0, 0, 3, 0, 3, 1, 2, 1, 2]
    assert table[0] == list(range(V)) + [-1] * 31 and bias[0] == [0.0] * 64 and bias[1][GU] == bias[2][UG] == 0.5 and bias[3] == [0.0] * 64
    # distinct biases (and distinct flags) make distinct tables
    _, _, table, idx, _, bias = m._mapped_arguments(dict(fd, paired_wobble=[True, True, False, False], paired_wobble_bias=[0.5, -2.0, 0.0, 0.0]), 1, L)
    assert len(table) == 6 and idx[8:] == [1, 2, 3, 4] and table[1] == table[3] and bias[1][GU] == 0.5 and bias[3][GU] == -2.0
    arr = ProteinMPNN._token_map_array(table, idx, "cpu", bias)
    assert arr.dtype == torch.int32 and arr.numel() == 6 * 64 + L + 6 * 64
    assert arr[:6 * 64].view(6, 64).tolist() == table and arr[6 * 64:6 * 64 + L].tolist() == idx
    assert arr[6 * 64 + L:].view(torch.float32).view(6, 64).tolist() == bias
    with pytest.raises(ValueError, match="paired_wobble has 2 entries for 4 pairs"):
        m._mapped_arguments(dict(fd, paired_wobble=[True, False]), 1, L)
    with pytest.raises(ValueError, match="paired_wobble needs paired_residues"):
        m._mapped_arguments({"paired_wobble": True}, 1, L)
    with pytest.raises(ValueError, match="pair_bias is not supported"):
        m._mapped_arguments(dict(fd, paired_wobble=True, pair_bias=None), 1, L)


@pytest.fixture(scope="module")
def case40(weights_np):
    """make_case(40, ...) with its teacher-forced oracle rows, computed once: (cx, fd, pairs, w, S, lp_groups)."""
    L, K, bs, T = 40, 48, 2, 0.5
    cx, fd, pairs = paired_ref.make_case(L, bs, T, 6, seed=3100 + L)
    w = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    S = torch.from_numpy(cx["S"].astype(np.int64))[None].repeat(bs, 1)
    rti = spec.restype_to_int()
    _, p_canonical, _, (groups, weights, maps), lp_groups = paired_ref.oracle_paired(w, fd, K, S, rti)
    return cx, fd, pairs, p_canonical, (groups, weights, maps), lp_groups


def test_oracle_rows_and_reduction(case40):
    """Rows of designable members sum to 1 and hold wobble mass where a pair may wobble; with paired_wobble_bias = -1e9 the marginals
    are paired_ref.paired_probs to 1e-12."""
    cx, fd, pairs, p_canonical, (groups, weights, maps), lp_groups = case40
    rti = spec.restype_to_int()
    fdw = dict(fd, paired_wobble=True)
    g, w_, tables, cb = wobble_ref.groups_of(fdw, rti)
    assert g == groups and w_ == weights
    rows, draws = wobble_ref.class_probs(lp_groups, fdw, g, w_, tables, cb)
    cm = (fd["mask"] * fd["chain_mask"])[0].bool()
    assert float((rows[:, cm].sum(-1) - 1).abs().max()) < 1e-12 and float(rows[:, ~cm].abs().max()) == 0
    eligible = [k for k, gt in enumerate(tables) if gt[0][GU] >= 0]
    assert eligible and len(eligible) < len(groups)                          # (the case holds DNA-DNA pairs too)
    for k in eligible:
        if all(bool(cm[j]) for j in groups[k]):
            mass = draws[k][1][:, [GU, UG]].sum(-1)
            assert float(mass.min()) > 0 and float(mass.max()) < 1
    off = dict(fdw, paired_wobble_bias=-1e9)
    g, w_, tables, cb = wobble_ref.groups_of(off, rti)
    rows_off, _ = wobble_ref.class_probs(lp_groups, off, g, w_, tables, cb)
    p_ref = paired_ref.paired_probs(lp_groups.double(), fd, groups, weights, maps)     # (float32 rows of float64 arithmetic)
    assert float((rows_off.float() - p_ref).abs().max()) == 0
    exact = wobble_ref.class_probs(lp_groups, dict(fd, paired_wobble=False), *wobble_ref.groups_of(dict(fd, paired_wobble=False), rti))[0]
    assert float((rows_off - exact).abs().max()) < 1e-12 and float((rows - exact).abs().max()) > 1e-3


def test_oracle_pinned_members(case40):
    """A fixed G restricts its partner to {C, U}; an inconsistent fixed pair leaves both tokens as they are; a forced G-U pair is the
    one class GU."""
    cx, fd, pairs, _, _, lp_groups = case40
    rti = spec.restype_to_int()
    rna = [(i, j) for i, j in pairs if cx["rna_mask"][i] or cx["rna_mask"][j]]
    assert rna
    i, j = rna[0]
    own = lambda r, n: rti[{"G": "DG", "C": "DC", "U": "DT", "A": "DA"}[n] if cx["dna_mask"][r] else n]      # residue r's base n
    G_i, C_j, U_j, A_j = own(i, "G"), own(j, "C"), own(j, "U"), own(j, "A")
    S = fd["S"].clone(); S[0, i] = G_i
    cmask = fd["chain_mask"].clone(); cmask[0, i] = 0; cmask[0, j] = 1
    fdw = dict(fd, S=S, chain_mask=cmask, paired_wobble=True, mask=torch.ones_like(fd["mask"]))
    g, w_, tables, cb = wobble_ref.groups_of(fdw, rti)
    k = g.index([i, j])                                                       # the fixed member is listed first
    rows, draws = wobble_ref.class_probs(lp_groups, fdw, g, w_, tables, cb)
    pr = draws[k][1]
    assert set(pr[0].nonzero().flatten().tolist()) == {G_i, GU}
    assert {wobble_ref.tokens_of(c, g[k], tables[k], fdw)[1] for c in (G_i, GU)} == {C_j, U_j}
    assert float((pr.sum(-1) - 1).abs().max()) < 1e-12 and float(rows[:, i].abs().max()) == 0
    # the partner's row is the UNRESTRICTED marginal: it has mass on A and G as well
    assert float(rows[:, j, A_j].min()) > 0 and abs(float(rows[0, j].sum()) - 1) < 1e-12
    # both fixed and inconsistent (G with A): the second restriction would leave no class and is skipped; both keep their tokens
    S2 = S.clone(); S2[0, j] = A_j
    cm2 = cmask.clone(); cm2[0, j] = 0
    fd2 = dict(fdw, S=S2, chain_mask=cm2)
    g2, w2, t2, cb2 = wobble_ref.groups_of(fd2, rti)
    k2 = [sorted(x) for x in g2].index(sorted([i, j]))
    _, draws2 = wobble_ref.class_probs(lp_groups, fd2, g2, w2, t2, cb2)
    first = g2[k2][0]
    kept = G_i if first == i else A_j
    assert set(draws2[k2][1][0].nonzero().flatten().tolist()) <= {c for c in range(35) if t2[k2][0][c] == kept}
    for c in draws2[k2][1][0].nonzero().flatten().tolist():
        assert wobble_ref.tokens_of(c, g2[k2], t2[k2], fd2) == [int(S2[0, r]) for r in g2[k2]]
    # forced: G on the first member, U on the second -> the class GU alone
    fd3 = dict(fd, paired_wobble=True, mask=torch.ones_like(fd["mask"]), chain_mask=torch.ones_like(fd["chain_mask"]))
    g3, w3, t3, cb3 = wobble_ref.groups_of(fd3, rti)
    k3 = g3.index([i, j])
    forced = fd["S"].repeat(2, 1).clone(); forced[:, i], forced[:, j] = G_i, U_j
    _, draws3 = wobble_ref.class_probs(lp_groups, fd3, g3, w3, t3, cb3, S_forced=forced)
    assert draws3[k3][1][0].nonzero().flatten().tolist() == [GU]
    assert wobble_ref.drawn_class(draws3[k3][1][0], draws3[k3][2][0], 0.3)[0] == GU


def test_cli_wobble_flags():
    p = cli.build_parser()
    args = p.parse_args(["--out_folder", "x", "--paired_strands", "A:B", "--paired_wobble", "1", "--paired_wobble_bias", "-0.5"])
    assert (args.paired_wobble, args.paired_wobble_bias) == (1, -0.5)
    assert cli.wobble_arguments(args, True) == {"paired_wobble": True, "paired_wobble_bias": -0.5}
    args = p.parse_args(["--out_folder", "x", "--paired_strands", "A:B", "--paired_wobble", "1"])
    assert cli.wobble_arguments(args, True) == {"paired_wobble": True, "paired_wobble_bias": 0.0}
    args = p.parse_args(["--out_folder", "x", "--paired_strands", "A:B"])
    assert (args.paired_wobble, args.paired_wobble_bias) == (0, None) and cli.wobble_arguments(args, True) == {}
    ns = lambda **kw: argparse.Namespace(**dict(dict(paired_wobble=0, paired_wobble_bias=None), **kw))
    with pytest.raises(ValueError, match="need --paired_residues or --paired_strands"):
        cli.wobble_arguments(ns(paired_wobble=1), False)
    with pytest.raises(ValueError, match="need --paired_residues or --paired_strands"):
        cli.wobble_arguments(ns(paired_wobble_bias=1.0), False)
    with pytest.raises(ValueError, match="needs --paired_wobble 1"):
        cli.wobble_arguments(ns(paired_wobble_bias=1.0), True)
    with pytest.raises(ValueError, match="is 0 or 1"):
        cli.wobble_arguments(ns(paired_wobble=2), True)
