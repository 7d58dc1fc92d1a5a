"""score_tied on the CPU: the plan (keys, leaders, edge kinds) against a brute force over the sampler's visit plan, the
parallel form of the tied stream against the sequential oracles teacher-forced on the same sequences, the sensitivity of a paired
case to hidden-backward edges, the combine's consistency rule and the argument checks (none of which needs a device)."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import ProteinMPNN, tied_stream_keys
import class_loo_ref
import group_loo_ref
import tied_score_ref as tr

PLAN_CASES = tr.GROUP_CASES + tr.CLASS_CASES + ("paired_l40", "trimer_l24_k48")
ORACLE_CASES = ("trimer_l24", "mixed_l12", "states_pairs_m2_l32", "trimer_maps_l24", "l12_lt_k", "l48_k16", "hybrid", "4oqu",
                "trimer_l24_k48", "paired_l40", "plain_l17")


@pytest.mark.parametrize("name", PLAN_CASES)
def test_keys_reduce_the_visit_plan(name):
    """key(i) = (min of rank0 over the group) << 4 | listed position orders the residues as symmetry_visits visits them: the edge kinds
    from the keys equal the brute force over dense visit ranks and group membership — with the ranks of the flattened order and with
    the one order's ranks repeated per state, which is what the device reads.  model.tied_stream_keys, which orders the sampler
    route's check of the design call, gives the same keys and leaders."""
    c = tr.oracle_case(name)
    groups = [s[0] for s in c["specs"]]
    brute = tr.edge_kinds_brute(c["E_idx"], c["order0"].tolist(), groups)
    assert np.array_equal(c["kinds"], brute)
    mkey, mleader = tied_stream_keys(tr.rank_of(c["order0"].numpy()), groups)
    assert mkey == c["key"].tolist() and mleader == c["leader"].tolist()
    assert np.array_equal(tr.edge_kinds(c["E_idx"], np.asarray(mkey), np.asarray(mleader)), brute)
    L = c["fd"]["S"].shape[1]
    M = len(c["mask"]) // L
    base = tr.rank_of(c["order0"].numpy()[::M] % L) if M > 1 else tr.rank_of(c["order0"].numpy())
    key, leader = tr.keys_and_leaders(group_loo_ref.flat_rank(base, M), groups)
    assert np.array_equal(tr.edge_kinds(c["E_idx"], key, leader), brute)
    assert all(l < L for l in leader[:L]) and all(len(g) <= group_loo_ref.GROUP_MAX for g in groups)


def test_the_cases_hold_what_they_are_chosen_for():
    """An L < K complex where every pair of members is a pair of neighbours, a group of 16, a group with a masked member."""
    c = tr.oracle_case("mixed_l12")
    sizes = sorted(len(s[0]) for s in c["specs"])
    assert sizes == [2, 4] and int((c["kinds"] == tr.HID).sum()) == 1 + 6            # every ordered member pair (t < u) is an edge
    assert max(len(s[0]) for s in tr.oracle_case("cap_m8_l16")["specs"]) == 16
    assert max(len(s[0]) for s in tr.oracle_case("cap16")["specs"]) == 16
    c = tr.oracle_case("trimer_l24")
    assert c["fd"]["mask"][0, 11] == 0 and all(3 not in s[0] for s in c["specs"]) and c["leader"][3] == 3 and c["leader"][19] == 19
    assert int((tr.oracle_case("states_m3_l20")["kinds"] == tr.HID).sum()) == 0      # pure states: members are never neighbours


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_parallel_form_reproduces_the_sequential_oracle(name):
    """The parallel form (cpu_ref.dec_layer with per-edge token hiding, fp32) against the sequential oracle teacher-forced on the
    same sequences, on the own log-softmax rows of every unmasked residue and on the unit log-probs: within 2e-4 (measured maximum
    over the cases: 2.9e-6 on the rows, 2.6e-6 on the units)."""
    c = tr.oracle_case(name)
    rows = tr.sequential_rows(c["w"], c["fd"], tr.K_OF[name], c["S_lib"], c["specs"])
    on = c["mask"] != 0
    par = torch.log_softmax(c["logits"], -1)
    d_rows = float((par[:, on] - rows[:, on]).abs().max())
    unit, own = tr.unit_values(rows, c["S_flat"], c["specs"])
    fin = torch.isfinite(c["unit"][:, on])
    assert torch.equal(fin, torch.isfinite(unit[:, on]))
    d_unit = float((c["unit"][:, on][fin] - unit[:, on][fin]).abs().max())
    print(f"{name}: rows {d_rows:.2e} units {d_unit:.2e}")
    assert d_rows < 2e-4 and d_unit < 2e-4


def test_hidden_backward_edges_matter():
    """Treating hidden-backward edges as ordinary backward edges moves a unit of a paired case by more than 1e-3 (measured on the
    oracle: 5.0e-3 on this case, two hidden-backward edges)."""
    a, b = tr.oracle_case(tr.SENSITIVE), tr.oracle_case(tr.SENSITIVE, hide=False)
    assert int((a["kinds"] == tr.HID).sum()) > 0
    on = (a["mask"] != 0)[None, :] & torch.isfinite(a["unit"])
    d = float((a["unit"][on] - b["unit"][on]).abs().max())
    print(f"hide=False moves a unit by {d:.2e}")
    assert d > 1e-3


def test_the_combine_asks_for_a_consistent_sequence():
    """An inconsistent pair is -inf; a G-U pair is consistent only with paired_wobble."""
    rti = spec.restype_to_int()
    c = tr.oracle_case("l48_k16")                        # wobble on for every pair
    assert torch.isfinite(c["unit"][:2]).all() and not torch.isfinite(c["unit"][2]).all()
    g = c["specs"][0][0]
    assert c["unit"][2, g[0]] == tr.NEG and c["unit"][2, g[1]] == tr.NEG
    fd = c["fd"]
    i, j = fd["paired_residues"][1]
    S = c["S_lib"][:1].clone()
    S[0, i], S[0, j] = rti["G"], rti["U"]
    with_w = tr.unit_values(c["logits"][:1], S, c["specs"])[0]
    no_wobble = tr.specs_of(dict(fd, paired_wobble=False), rti)
    without = tr.unit_values(c["logits"][:1], S, no_wobble)[0]
    assert torch.isfinite(with_w[0, i]) and without[0, i] == tr.NEG and without[0, j] == tr.NEG


def test_the_reference_combine_against_the_conditionals_references():
    """tied_score_ref.unit_values against the combines of the group and class conditionals' references, which this pull request
    did not write.  Token maps: the unit of a consistent sequence is the listed-first member's entry of group_loo_ref.combine's row.
    Classes: over ALL 33 x 33 token pairs of a wobble pair exp(unit) sums to 1, and summed over the second member's token it is the
    first member's marginal row of class_loo_ref.class_combine."""
    c = tr.oracle_case("trimer_maps_l24")
    for g, gw, maps, _ in c["specs"]:
        rows = group_loo_ref.combine(c["logits"][0, g], gw, maps)
        assert abs(float(rows[0][int(c["S_flat"][0, g[0]])]) - float(c["unit"][0, g[0]])) < 1e-12
    c = tr.oracle_case("l48_k16")
    g, gw, tabs, gb = c["specs"][0]
    V = c["logits"].shape[-1]
    pairs = torch.cartesian_prod(torch.arange(V), torch.arange(V))
    S = c["S_flat"][:1].repeat(len(pairs), 1)
    S[:, g[0]], S[:, g[1]] = pairs[:, 0], pairs[:, 1]
    unit = tr.unit_values(c["logits"][:1].expand(len(pairs), -1, -1), S, [c["specs"][0]])[0][:, g[0]].view(V, V)
    assert abs(float(unit.exp().sum()) - 1.0) < 1e-12
    rows, clp = class_loo_ref.class_combine(c["logits"][0, g], gw, tabs, gb)
    marg = torch.logsumexp(unit, 1)
    fin = torch.isfinite(rows[0])
    assert torch.equal(fin, torch.isfinite(marg)) and int(fin.sum()) >= 4 and float((marg[fin] - rows[0][fin]).abs().max()) < 1e-12
    assert int(torch.isfinite(unit).sum()) == int(torch.isfinite(clp).sum())     # one class per consistent token pair


def _model(k=16):
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int())


@pytest.mark.parametrize("name", ["trimer_maps_l24", "states_pairs_m2_l32", "l48_k16", "states_pairs", "plain_l17"])
def test_the_torch_combine_of_the_slow_routes(name):
    """ProteinMPNN._tied_combine (the combine of the sampler route, fp32, groups of one size batched) on the oracle's logits against
    the reference combine in fp64: within 1e-5, the same sequences -inf."""
    c = tr.oracle_case(name)
    m = _model(tr.K_OF[name])
    fd = c["fd"]
    L = fd["S"].shape[1]
    state_w = None if fd.get("state_weights") is None else [float(v) for v in fd["state_weights"]]
    classes = tr.wobble_asked(fd)
    ties = m._conditional_arguments(fd, 1, L, state_w, True, classes)
    assert (ties is None) == (not c["specs"]) and (ties is None or [t[0] for t in ties["tied"]] == [s[0] for s in c["specs"]])
    unit, own = m._tied_combine(c["logits"], c["S_flat"], m._tied_combine_plan(ties, classes, "cpu"))
    assert torch.equal(torch.isfinite(unit), torch.isfinite(c["unit"]))
    fin = torch.isfinite(unit)
    assert float((unit[fin] - c["unit"][fin]).abs().max()) < 1e-5 and float((own - c["own"]).abs().max()) < 1e-5


def test_argument_checks():
    m = _model()
    fd = tr.case_inputs("trimer_l24")
    L = fd["S"].shape[1]
    with pytest.raises(ValueError, match="method"):
        m.score_tied(fd, method="cone")
    with pytest.raises(ValueError, match="B == 1"):
        m.score_tied(dict(fd, S=fd["S"].repeat(2, 1)))
    with pytest.raises(ValueError, match="S_lib"):
        m.score_tied(fd, S_lib=torch.zeros(2, L + 1, dtype=torch.long))
    with pytest.raises(ValueError, match="S_lib"):
        m.score_tied(fd, S_lib=torch.zeros(2, L))
    with pytest.raises(IndexError):
        m.score_tied(fd, S_lib=torch.full((1, L), 33, dtype=torch.long))
    with pytest.raises(ValueError, match="stream"):
        m.score_tied(fd, method="stream")
    with pytest.raises(ValueError, match="disjoint"):
        m.score_tied(dict(fd, symmetry_residues=[[0, 1], [1, 2]], symmetry_weights=[[1.0, 1.0], [1.0, 1.0]]))
    with pytest.raises(ValueError, match="at most"):
        m.score_tied(dict(fd, symmetry_residues=[list(range(17))], symmetry_weights=[[1.0] * 17]))
    m.message_precision = "bf16"
    with pytest.raises(NotImplementedError, match="items"):
        m.score_tied(fd, method="items")
    # score_sequences / score_mutations keep their refusal of state_weights
    with pytest.raises(NotImplementedError, match="state_weights"):
        m.score_sequences(tr.case_inputs("states_m3_l20"), torch.zeros(1, 20, dtype=torch.long))
