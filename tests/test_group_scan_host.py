"""CPU tests of the symmetric scan (ProteinMPNN.score_mutations(tied=True)): the reference tests/group_scan_ref.py and
its premises, the per-site sets on the keys against the reference's decoder states, the leader rule against a brute force, the
expansion of sites and every refusal, and the size functions and attach state machine of namp_group_mutations without a device.

Bars.  The GPU tests hold units to 1e-3 and a delta to 1e-3 x the variant's leader rows.  Premise (a): on every grouped case the plain
scan with all members edited (score()'s own stream, the sum of the members' own entries) differs from the tied delta by more than 100
x 1e-3 on some variant.  Premise (b): a reference that reads hidden-backward edges as backward ones moves some variant's unit by at
least 5 x 1e-3 on at least one case.  Premise (c): symmetry_weights dropped (all 1) move some unit of trimer_l24, whose weights are (1,
0.5, 0.25), by at least 5 x 1e-3.  The figures are printed."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec
from na_mpnn_amd.model import MUT_MAX_EDITS, ProteinMPNN, _section_bytes, expand_group_sites, output_section_layout
import group_scan_ref as GR
import tied_score_ref as TR

torch.set_grad_enabled(False)
EINVAL = -1
BAR = 1e-3


def host_model(k=16):
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int())


# ---- the reference and the sets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GR.CASES)
def test_rows_that_differ_lie_inside_the_sets_and_the_wild_type_has_delta_zero(name):
    """parallel_states is tied_score_ref.parallel_logits; per variant and layer the rows whose decoder state differs from the base
    stream's lie inside U_l(expanded site) planned on the keys; the wild-type variant of every site has delta exactly 0."""
    c, ref = GR.case(name), GR.reference(name)
    assert torch.equal(ref["S"][0], c["fd"]["S"][0].long())
    for g in c["groups"]:
        assert len({int(ref["S"][0][r]) for r in g}) == 1
    n = len(c["tk"])
    seen = [0, 0, 0]
    for v, row in enumerate(c["tk"]):
        for l in range(3):
            differ = np.nonzero((ref["states"][l][v + 1] != ref["states"][l][0]).any(-1).numpy())[0]
            inside = set(c["lists"][row[0]][l].tolist())
            assert set(differ.tolist()) <= inside, (name, v, l)
            seen[l] = max(seen[l], len(differ))
        if all(int(t) == int(ref["S"][0][r]) for r, t in zip(c["st"][row[0]], row[1:]) if r >= 0):
            assert float(ref["delta"][v]) == 0.0
    assert len(ref["delta"]) == n and (name == "plain_l1" or seen[2] > 1)


def test_the_cases_reach_what_they_are_for():
    what = {name: GR.case(name)["what"] for name in GR.CASES}
    for name in GR.GROUPED:
        assert "hidden-backward edge between two members" in what[name] and "first-visited unit" in what[name]
    assert any("a foreign group led by a later-listed member" in w for w in what.values())
    assert "an ungrouped residue beside groups" in what["mixed_l12"] and "an ungrouped residue beside groups" in what["trimer_l24"]
    d = GR.case("dimer_l48")
    assert sorted((d["sites8"] >= 0).sum(1).tolist())[-2:] == [4, 8]
    assert 6 in (GR.case("mixed_l12")["sites8"] >= 0).sum(1).tolist()
    for name in GR.CASES:                                         # the last-visited unit: U_l is the site alone
        c = GR.case(name)
        if "last-visited unit" in c["what"]:
            q = c["what"].index("last-visited unit")
            assert c["site_rows"][q].tolist() == [int((c["sites8"][q] >= 0).sum())] * 3


@pytest.mark.parametrize("name", GR.CASES)
def test_leader_rule_against_the_brute_force(name):
    c = GR.case(name)
    for u3 in c["u3"]:
        lead = GR.lead_rows(u3, c["leader"], c["gpos"], c["mask"])
        assert np.array_equal(np.sort(c["leader"][u3[lead]]), GR.unit_list(u3, c["leader"], c["mask"]))
        assert len(set(c["leader"][u3[lead]].tolist())) == int(lead.sum())
    if "a foreign group led by a later-listed member" in c["what"]:
        u3 = c["u3"][c["what"].index("a foreign group led by a later-listed member")]
        lead = GR.lead_rows(u3, c["leader"], c["gpos"], c["mask"])
        assert (c["leader"][u3[lead]] != u3[lead]).any()


# ---- the premises ------------------------------------------------------------------------------------------------------------------
def test_premises_untied_scan_hidden_edges_and_weights():
    worst_hidden, worst_untied = 0.0, {}
    for name in GR.GROUPED:
        ref, untied = GR.reference(name), GR.reference(name, "untied")
        a = float((ref["delta"] - untied["delta"]).abs().max())
        print(f"premise (a) {name}: tied delta against the plain scan with all members edited, max {a:.3g} nats")
        worst_untied[name] = a
        hid = GR.reference(name, "unhidden")
        b = float((ref["units"][1:] - hid["units"][1:]).abs().max())
        b_delta = float((ref["delta"] - hid["delta"]).abs().max())
        print(f"premise (b) {name}: hidden-backward edges read as backward, units {b:.3g} delta {b_delta:.3g}")
        worst_hidden = max(worst_hidden, b)
    assert all(a > 100 * BAR for a in worst_untied.values()), worst_untied
    assert worst_hidden >= 5 * BAR
    ref, flat = GR.reference("trimer_l24"), GR.reference("trimer_l24", "weights")
    cdiff = float((ref["units"][1:] - flat["units"][1:]).abs().max())
    print(f"premise (c) trimer_l24: symmetry_weights dropped, units {cdiff:.3g}")
    assert cdiff >= 5 * BAR


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_expand_group_sites():
    groups = [[1, 7], [2, 5, 8, 11]]
    st = np.array([[5, 1], [4, -1], [7, -1]], np.int64)
    tk = np.array([[0, 3, 9], [1, 6, 0], [2, 4, 0], [0, 10, 11]], np.int64)
    st_x, tk_x = expand_group_sites(st, tk, groups, 12)
    assert st_x.tolist() == [[2, 5, 8, 11, 1, 7], [4, -1, -1, -1, -1, -1], [1, 7, -1, -1, -1, -1]]
    assert tk_x.tolist() == [[0, 3, 3, 3, 3, 9, 9], [1, 6, 0, 0, 0, 0, 0], [2, 4, 4, 0, 0, 0, 0], [0, 10, 10, 10, 10, 11, 11]]
    with pytest.raises(ValueError, match="two residues of one tied unit"):
        expand_group_sites(np.array([[2, 8]]), np.array([[0, 1, 1]]), groups, 12)
    with pytest.raises(ValueError, match=f"expands to 9 flat residues.*{MUT_MAX_EDITS}"):
        expand_group_sites(np.array([[2, 1, 0, 3, 4]]), np.zeros((0, 6), np.int64), groups, 12)
    empty = expand_group_sites(np.zeros((0, 1), np.int64), np.zeros((0, 2), np.int64), groups, 12)
    assert empty[0].shape == (0, 1) and empty[1].shape == (0, 2)


def test_refusals_and_defaults():
    c = GR.case("mixed_l12")
    fd, m = c["fd"], host_model()
    for extra in (dict(symmetry_token_maps=[[None, None], [None] * 4, [None]]), dict(paired_residues=[[0, 3]]), dict(paired_wobble=True),
                  dict(pair_terms={})):
        with pytest.raises(NotImplementedError, match="identity token maps"):
            m.score_mutations(dict(fd, **extra), positions=[1], tied=True)
    with pytest.raises(NotImplementedError, match="identity token maps"):
        m.score_mutations(fd, pairs=True, tied=True)
    with pytest.raises(NotImplementedError, match="joined with state_weights"):
        m.score_mutations(dict(fd, state_weights=[0.5, 0.5]), positions=[1], tied=True)
    with pytest.raises(ValueError, match="two residues of one tied unit"):
        m.score_mutations(fd, sites=[[2, 8]], site_tokens=[[0, 1, 1]], tied=True)
    with pytest.raises(ValueError, match="expands to 9"):
        m.score_mutations(fd, sites=[[2, 1, 0, 3, 4]], site_tokens=[[0, 1, 1, 1, 1, 1]], tied=True)
    masked = dict(fd, chain_mask=fd["chain_mask"].clone())
    masked["chain_mask"][0, 0] = 0
    with pytest.raises(ValueError, match="mask \\* chain_mask == 0"):
        m.score_mutations(masked, positions=[0], tied=True)
    broken = dict(fd, S=fd["S"].clone())
    broken["S"][0, 7] = (int(fd["S"][0, 7]) + 1) % 20
    with pytest.raises(ValueError, match="not tie-consistent on the group of residue 1"):
        m.score_mutations(broken, positions=[0], tied=True)
    with pytest.raises(RuntimeError):
        m.score_mutations(fd, positions=[1], tied=True)          # a CPU feature_dict, as for the other calls
    # the default positions: the listed-first members of the units whose leader counts
    ties, groups, leader, st, tk, scan, st_x, tk_x, sites8, tok9 = m._group_scan_arguments(fd, None, None, None, None, False)
    assert groups == c["groups"] and leader == c["leader"].tolist()
    assert scan["positions"] == [i for i in range(12) if leader[i] == i and c["mask"][i] != 0]
    assert (sites8[scan["positions"].index(2)] == [2, 5, 8, 11, -1, -1, -1, -1]).all()
    q = int(np.nonzero(tk[:, 0] == scan["positions"].index(2))[0][0])
    assert tok9[q, 1:5].tolist() == [int(tk[q, 1])] * 4 and tok9[q, 5:].tolist() == [0] * 4
    # a member named in the place of the first one stands for the same unit
    got = m._group_scan_arguments(fd, torch.tensor([8]), torch.tensor([3]), None, None, False)
    assert got[8][0].tolist() == [2, 5, 8, 11, -1, -1, -1, -1] and got[9][0].tolist() == [0, 3, 3, 3, 3, 0, 0, 0, 0]
    # no tie at all is legal: units of one
    plain = GR.case("plain_l17")["fd"]
    got = m._group_scan_arguments(plain, None, None, None, None, False)
    assert got[0] is None and got[1] == [] and got[2] == list(range(17))


# ---- the size functions and the attach state machine ---------------------------------------------------------------------------------
def test_size_functions_layout_and_attach():
    Lb = hip.lib()
    dims = (24, 16, 3, 5, 15, 20, 40, 60, 60, 120, 180)
    size, i_off, o_off = (int(getattr(Lb, "namp_group_mutations" + f)(*dims)) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
    plain = int(Lb.namp_mutations_workspace_bytes(*dims))
    assert 0 < i_off < o_off < size and size > plain and i_off % 256 == 0 and o_off % 256 == 0
    layout = output_section_layout("group_mutations", dims)
    assert [(e, str(t)) for _, e, t in layout] == [(15, "torch.int32"), (15, "torch.float32"), (180, "torch.int32"), (180, "torch.float32"),
                                                   (180, "torch.int32"), (180, "torch.float32"), (24, "torch.float32"), (63, "torch.int32")]
    assert sum(_section_bytes(e) for _, e, _ in layout) == size - o_off
    assert int(Lb.namp_group_mutations_workspace_bytes(24, 16, 4, *dims[3:])) == 0             # n_dec != 3
    assert int(Lb.namp_group_mutations_workspace_bytes(1 << 27, 16, 3, 0, 0, 0, 0, 0, 0, 0, 0)) == 0
    assert int(Lb.namp_group_mutations_workspace_bytes(24, 16, 3, 1, 1, 1, 1, 1, 1 << 27, 1, 1)) == 0
    # the sizes of the other scans are what they were
    assert int(Lb.namp_state_mutations_workspace_bytes(24, 16, 3, 1, *dims[3:])) > plain
    assert Lb.namp_group_mutations(-1, 0, 0, 0, 0, 0, 0, 0) == EINVAL and b"namp_group_mutations" in Lb.namp_last_error()
    # attached, the next carrier call takes it (and refuses its null pointers by the kind's noun); the call after is plain
    assert Lb.namp_group_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0
    carried = lambda: (Lb.namp_decoder_fwd(None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 24, 16, None),
                       Lb.namp_last_error())[1]
    assert b"a group scan was attached" in carried()
    assert b"attached" not in carried()
    # it shares the attach kind of namp_mutations: the later of the two holds, a refused one leaves neither
    assert Lb.namp_group_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0 and Lb.namp_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0
    assert b"a mutational scan was attached" in carried() and b"attached" not in carried()
    assert Lb.namp_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0 and Lb.namp_group_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0
    assert b"a group scan was attached" in carried() and b"attached" not in carried()
    assert Lb.namp_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0 and Lb.namp_group_mutations(-1, 0, 0, 0, 0, 0, 0, 0) == EINVAL
    assert b"attached" not in carried()
    # together with another kind neither runs
    assert Lb.namp_group_mutations(1, 0, 0, 0, 0, 0, 0, 0) == 0 and Lb.namp_tied_score(1, 33, 0) == 0
    assert b"were attached together; none is run" in carried()
    assert b"attached" not in carried()
