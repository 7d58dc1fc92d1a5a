"""CPU tests of the paired scan (ProteinMPNN.score_mutations(tied=True, classes=True)): the lowest-lane rule and the
expansion against the numpy restatement of tests/class_scan_ref.py, every refusal, the unchanged refusals of classes=False, the
reference and its premises, the per-site sets on the keys against the reference's decoder states, and — without a device — the size
functions of namp_class_mutations against tests/golden/class_scan_layout.json (with the group and state layouts as the parent commit's
build gave them) and the attach record's re-routing.

Bars.  The GPU tests hold every entry, leader term and delta to 1e-3.  Premises: for every mistake the helper can make — "untied",
"unhidden", "canonical" (wobble lanes dropped), "nobias" (class bias dropped), "weights" (member weights all 1) — the reference's
deltas on the scan's OWN variants move by at least 3 x 1e-3 on the case meant to catch it (class_scan_ref.CATCHES; "canonical" turns
the delta of a wobble variant into -inf and moves the canonical variants of the same pairs by 1e-4 at most: the wobble classes hold
little of the mass).  The figures are printed for every case."""
import json
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec
from na_mpnn_amd.model import ProteinMPNN, _section_bytes, class_lane, expand_class_sites, output_section_layout
import class_scan_ref as CR
import group_scan_ref as GR

torch.set_grad_enabled(False)
EINVAL = -1
BAR = 1e-3
RTI = spec.restype_to_int()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_scan_layout.json")


def host_model(k=16):
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=RTI,
                       polytype_to_int=spec.polytype_to_int())


# ---- the rule and the expansion --------------------------------------------------------------------------------------------------------
def test_the_lowest_lane_rule():
    first, second = spec.class_table(RTI, "rna-rna", True, True), spec.class_table(RTI, "rna-rna", True, False)
    G, C, A, U = RTI["G"], RTI["C"], RTI["A"], RTI["U"]
    tabs = [first, second]
    assert class_lane(tabs, {0: G}) == G                          # G alone: G-C, the canonical class lies below the wobble lanes
    assert class_lane(tabs, {0: G, 1: C}) == G and class_lane(tabs, {0: G, 1: U}) == spec.CLASS_GU
    assert class_lane(tabs, {0: U, 1: G}) == spec.CLASS_UG and class_lane(tabs, {1: G}) == C and class_lane(tabs, {1: U}) == A
    assert class_lane(tabs, {0: A, 1: A}) == -1 and class_lane(tabs, {0: G, 1: A}) == -1
    canon = [spec.class_table(RTI, "dna-dna", True, True), spec.class_table(RTI, "dna-dna", True, False)]
    assert class_lane(canon, {0: RTI["DG"], 1: RTI["DT"]}) == -1                               # DNA:DNA never wobbles
    assert class_lane([first, [-1] * 64], {0: G}) == -1                                         # no class every member has
    for tables, named in ((tabs, {0: G}), (tabs, {0: U, 1: G}), (tabs, {0: A, 1: A}), (canon, {1: RTI["DA"]})):
        assert class_lane(tables, named) == CR.lowest_lane(tables, named)


@pytest.mark.parametrize("name", CR.CASES)
def test_expansion_against_the_numpy_restatement(name):
    """expand_class_sites and the model's checked arguments give the helper's expanded sites and tokens; every member of every named
    unit gets the token of the unit's class; the leaders are the listed-first members."""
    c = CR.case(name)
    st_x, tk_x = expand_class_sites(c["st"], c["tk"], c["units"], len(c["key"]))
    width = st_x.shape[1]
    assert np.array_equal(st_x, c["sites8"][:, :width]) and np.array_equal(tk_x, c["tok"][:, :1 + width])
    got = host_model(c["K"])._class_scan_arguments(c["fd"], None, None, torch.from_numpy(c["st"]), torch.from_numpy(c["tk"]), False)
    ties, groups, leader, st, tk, scan, st_x2, tk_x2, sites8, tok9, extra = got
    assert groups == [m for m, _ in c["units"]] and leader == c["leader"].tolist() and scan is None and extra == {}
    assert np.array_equal(sites8, c["sites8"]) and np.array_equal(tok9, c["tok"]) and sites8.dtype == np.int32
    for members, tables in c["units"]:
        for v, row in enumerate(c["tok"]):
            site = c["sites8"][row[0]].tolist()
            if members[0] in site:
                toks = [int(row[1 + site.index(r)]) for r in members]
                assert CR.lowest_lane(tables, dict(enumerate(toks))) >= 0, (name, v)


def test_the_cases_reach_what_they_are_for():
    what = {name: CR.case(name)["what"] for name in CR.CASES}
    for name in CR.CASES:
        for w in ("first-visited unit", "last-visited unit", "hidden-backward edge between two members", "two units"):
            assert w in what[name], (name, w)
        c = CR.case(name)
        q = c["what"].index("last-visited unit")
        assert c["site_rows"][q].tolist() == [int((c["sites8"][q] >= 0).sum())] * 3
    assert any("a foreign unit led by a later-listed member" in w for w in what.values())
    for name in ("paired_l40", "l48_k16", "hybrid", "4oqu", "joined_l32"):
        assert "four pairs, 8 edits: the cap" in what[name] and 8 in (CR.case(name)["sites8"] >= 0).sum(1).tolist()
    for name in ("l48_k16", "l12_lt_k", "hybrid", "4oqu", "joined_l32"):
        assert "a wobble class named by both members" in what[name] and "G named alone" in what[name]
        c = CR.case(name)
        q = c["what"].index("G named alone")
        v = int(np.nonzero(c["tk"][:, 0] == q)[0][0])
        first = int(c["sites8"][q, 0])
        kind_g = RTI["G"] if int(c["fd"]["S"][0, first]) >= 26 else RTI["DG"]
        assert c["tk"][v, 1] == kind_g and c["tok"][v, 1] == kind_g and c["tok"][v, 2] in (RTI["C"], RTI["DC"])      # G alone is G-C
        qw = c["what"].index("a wobble class named by both members")
        vw = int(np.nonzero(c["tk"][:, 0] == qw)[0][0])
        assert c["tok"][vw, 1] in (RTI["G"], RTI["DG"]) and c["tok"][vw, 2] in (RTI["U"], RTI["DT"])
    hyb = CR.case("hybrid")                                        # a pair with a masked member is not tied; DNA:DNA has no wobble lane
    assert all(50 not in m for m, _ in hyb["units"]) and hyb["leader"][50] == 50
    dd = [t for m, t in hyb["units"] if m == [28, 43]][0]
    assert dd[0][spec.CLASS_GU] == -1


def test_refusals_and_allowances():
    c = CR.case("l12_lt_k")
    fd, m = c["fd"], host_model()
    G, C, A, U = RTI["G"], RTI["C"], RTI["A"], RTI["U"]
    with pytest.raises(ValueError, match="needs tied=True"):
        m.score_mutations(fd, positions=[1], classes=True)
    with pytest.raises(NotImplementedError, match="state_weights"):
        m.score_mutations(dict(fd, state_weights=[0.5, 0.5]), positions=[1], tied=True, classes=True)
    with pytest.raises(NotImplementedError, match="state_weights"):
        m.score_mutations(dict(fd, state_weights=[0.5, 0.5], paired_residues=[], symmetry_residues=[[]]), positions=[1], tied=True, classes=True)
    with pytest.raises(NotImplementedError, match="pair_terms"):
        m.score_mutations(dict(fd, pair_terms={}), positions=[1], tied=True, classes=True)
    with pytest.raises(ValueError, match="the unit of residue 4 has no class with token .* at residue 4, token .* at residue 11"):
        m.score_mutations(fd, sites=[[4, 11]], site_tokens=[[0, A, A]], tied=True, classes=True)
    with pytest.raises(ValueError, match="has no class"):          # wobble is on for the first pair only
        m.score_mutations(fd, sites=[[5, 10]], site_tokens=[[0, G, U]], tied=True, classes=True)
    with pytest.raises(ValueError, match="expands to 9 flat residues.*8"):
        expand_class_sites(np.array([[0, 2, 4, 6, 8]]), np.zeros((0, 6), np.int64), [([0, 1], [[0] * 64] * 2), ([2, 3], [[0] * 64] * 2),
                                                                                     ([4, 5], [[0] * 64] * 2), ([6, 7], [[0] * 64] * 2)], 12)
    masked = dict(fd, chain_mask=fd["chain_mask"].clone())
    masked["chain_mask"][0, 0] = 0
    with pytest.raises(ValueError, match="mask \\* chain_mask == 0"):
        m.score_mutations(masked, positions=[0], tied=True, classes=True)
    broken = dict(fd, S=fd["S"].clone())
    broken["S"][0, 11] = A
    broken["S"][0, 4] = A
    with pytest.raises(ValueError, match="matches no class of the unit of residue 4"):
        m.score_mutations(broken, positions=[0], tied=True, classes=True)
    with pytest.raises(ValueError, match="pairs=True belongs to the scan form"):
        m.score_mutations(fd, sites=[[4]], site_tokens=[[0, G]], pairs=True, tied=True, classes=True)
    with pytest.raises(ValueError, match="takes no tokens"):
        m.score_mutations(fd, tokens=[G], pairs=True, tied=True, classes=True)
    with pytest.raises(RuntimeError):
        m.score_mutations(fd, positions=[1], tied=True, classes=True)          # a CPU feature_dict, as for the other calls
    # naming two members of one unit is allowed here
    got = m._class_scan_arguments(fd, None, None, torch.tensor([[4, 11]]), torch.tensor([[0, G, U], [0, G, C]]), False)
    assert got[9].tolist() == [[0, G, U, 0, 0, 0, 0, 0, 0], [0, G, C, 0, 0, 0, 0, 0, 0]]
    # the scan form: the default positions are the listed-first members of the counted units; G alone is G-C
    got = m._class_scan_arguments(fd, None, torch.tensor([G]), None, None, False)
    lead = c["leader"]
    assert got[5]["positions"] == [i for i in range(12) if lead[i] == i and c["mask"][i] != 0]
    q = got[5]["positions"].index(4)
    assert got[8][q].tolist() == [4, 11, -1, -1, -1, -1, -1, -1] and got[9][q].tolist() == [q, G, C, 0, 0, 0, 0, 0, 0]
    # pairs=True: the class axis — 6 classes with wobble, 4 without, a protein residue over its 20 letters
    *_, sites8, tok9, extra = m._class_scan_arguments(fd, None, None, None, None, True)
    lanes = extra["classes"].tolist()
    valid = (extra["class_tokens"][:, :, 0] >= 0).numpy()
    pos = m._class_scan_arguments(fd, None, None, None, None, True)[5]["positions"]
    per = dict(zip(pos, valid.sum(1).tolist()))
    assert per[4] == 6 and per[5] == 4 and per[0] == 20 and spec.CLASS_GU in lanes and lanes == sorted(lanes)
    assert extra["class_tokens"][pos.index(4), lanes.index(spec.CLASS_UG)].tolist() == [U, G]
    assert extra["class_tokens"][pos.index(0), lanes.index(3)].tolist() == [3, -1]
    assert len(tok9) == int(valid.sum())


def test_classes_false_refusals_are_unchanged():
    c = GR.case("mixed_l12")
    fd, m = c["fd"], host_model()
    for extra in (dict(symmetry_token_maps=[[None, None], [None] * 4, [None]]), dict(paired_residues=[[0, 3]]), dict(paired_wobble=True),
                  dict(pair_terms={})):
        with pytest.raises(NotImplementedError, match="identity token maps"):
            m.score_mutations(dict(fd, **extra), positions=[1], tied=True, classes=False)
    with pytest.raises(NotImplementedError, match="identity token maps"):
        m.score_mutations(fd, pairs=True, tied=True)
    with pytest.raises(ValueError, match="two residues of one tied unit"):
        m.score_mutations(fd, sites=[[2, 8]], site_tokens=[[0, 1, 1]], tied=True)
    # with classes=True the same groups are legal, and a member named beside the first one names the same class
    got = m._class_scan_arguments(fd, None, None, torch.tensor([[2, 8]]), torch.tensor([[0, 1, 1]]), False)
    assert got[8][0].tolist() == [2, 5, 8, 11, -1, -1, -1, -1] and got[9][0].tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 0]


# ---- the reference, the sets and the premises --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.CASES)
def test_rows_that_differ_lie_inside_the_sets_and_the_wild_type_has_delta_zero(name):
    c, ref = CR.case(name), CR.reference(name)
    assert torch.equal(ref["S"][0], c["fd"]["S"][0].long()) and bool(torch.isfinite(ref["delta"]).all())
    seen = 0
    for v, row in enumerate(c["tok"]):
        for l in range(3):
            differ = np.nonzero((ref["states"][l][v + 1] != ref["states"][l][0]).any(-1).numpy())[0]
            assert set(differ.tolist()) <= set(c["lists"][row[0]][l].tolist()), (name, v, l)
            seen = max(seen, len(differ))
        if all(int(t) == int(ref["S"][0][r]) for r, t in zip(c["sites8"][row[0]], row[1:]) if r >= 0):
            assert float(ref["delta"][v]) == 0.0
    assert seen > 1


def test_premises_on_the_scans_own_variants():
    moved = {}
    for name in CR.CASES:
        ref = CR.reference(name)
        for mistake in CR.MISTAKES:
            d = (ref["delta"] - CR.reference(name, mistake)["delta"]).abs()
            d = torch.nan_to_num(d, nan=float("inf"))              # ("canonical": a wobble variant has no class there: its delta is -inf)
            moved[(mistake, name)] = float(d.max())
        print(f"premises {name}: " + ", ".join(f"{mk} {moved[(mk, name)]:.3g}" for mk in CR.MISTAKES))
    for mistake, name in CR.CATCHES.items():
        assert moved[(mistake, name)] >= 3 * BAR, (mistake, name, moved[(mistake, name)])


# ---- the size functions and the attach record ----------------------------------------------------------------------------------------------
def test_every_size_and_offset_is_the_recorded_one():
    Lb, want = hip.lib(), json.load(open(GOLDEN))
    assert sorted(want) == sorted(f"namp_{fam}_mutations{f}" for fam in ("class", "group", "state") for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
    for name, rows in want.items():
        for row in rows:
            assert int(getattr(Lb, name)(*row[:-1])) == row[-1], (name, row)
    # a class layout is the group layout with N + 128 n_tables more words in the input section; refused where the group layout is, or
    # where n_tables / n_classes lies outside [1, 64]
    size, i_off, o_off = (want["namp_class_mutations" + f] for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
    group = {tuple(r[:-1]): r[-1] for r in want["namp_group_mutations_workspace_bytes"]}
    legal = 0
    for s, i, o in zip(size, i_off, o_off):
        dims = tuple(s[:-1])
        ok = group[dims[:3] + dims[5:]] > 0 and 1 <= dims[3] <= 64 and 1 <= dims[4] <= 64
        assert (0 < i[-1] < o[-1] < s[-1] and s[-1] > group[dims[:3] + dims[5:]]) if ok else (s[-1] == i[-1] == o[-1] == 0), dims
        legal += ok
    assert legal == 24
    dims = (24, 16, 3, 3, 35, 5, 15, 20, 40, 60, 60, 120, 180)
    size, o_off = int(Lb.namp_class_mutations_workspace_bytes(*dims)), int(Lb.namp_class_mutations_out_offset(*dims))
    layout = output_section_layout("class_mutations", dims)
    assert layout == output_section_layout("group_mutations", dims[:3] + dims[5:])
    assert sum(_section_bytes(e) for _, e, _ in layout) == size - o_off


def test_the_attach_record_reroutes_the_later_of_the_three_holds():
    Lb = hip.lib()
    carried = lambda: (Lb.namp_decoder_fwd(None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 24, 16, None),
                       Lb.namp_last_error())[1]
    tail = (1, 0, 0, 0, 0, 0, 0, 0)
    attach = {b"a class scan": lambda: Lb.namp_class_mutations(2, 35, *tail), b"a group scan": lambda: Lb.namp_group_mutations(*tail),
              b"a mutational scan": lambda: Lb.namp_mutations(*tail)}
    assert attach[b"a class scan"]() == 0
    assert b"a class scan was attached" in carried() and b"attached" not in carried()
    for first in attach:
        for second in attach:
            assert attach[first]() == 0 and attach[second]() == 0
            assert second + b" was attached" in carried() and b"attached" not in carried()
    # a refused one leaves none
    for bad in ((0, 35) + tail, (65, 35) + tail, (2, 0) + tail, (2, 65) + tail, (2, 35, -1, 0, 0, 0, 0, 0, 0, 0)):
        for other in attach.values():
            assert other() == 0 and Lb.namp_class_mutations(*bad) == EINVAL and b"namp_class_mutations" in Lb.namp_last_error()
            assert b"attached" not in carried()
    assert attach[b"a class scan"]() == 0 and Lb.namp_group_mutations(-1, 0, 0, 0, 0, 0, 0, 0) == EINVAL
    assert b"attached" not in carried()
    # together with another kind none runs
    assert attach[b"a class scan"]() == 0 and Lb.namp_tied_score(1, 33, 0) == 0
    assert b"were attached together; none is run" in carried() and b"attached" not in carried()
    assert attach[b"a class scan"]() == 0 and Lb.namp_state_mutations(2, 12, *tail) == 0
    assert b"were attached together; none is run" in carried() and b"attached" not in carried()
