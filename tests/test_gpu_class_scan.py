"""GPU tests of the paired scan — ProteinMPNN.score_mutations(tied=True, classes=True) (namp_class_mutations): the
cone route against the CPU reference (class_scan_ref: tied_score_ref.parallel_logits + unit_values on the explicit sequences), against
the dense route and score_tied, its own invariants (the sparse layouts against the numpy restatement, the fp32 sum of delta, chunks,
determinism), the identity invariant against the group scan, the class axis of pairs=True against the general form, and the CLI.

Bars: 1e-3 against the CPU oracle (the project's bar on log-probs) on every entry, leader term and delta; 2e-4 per entry between two
GPU routes and 2e-4 x the variant's leader rows on their deltas (DESIGN.md 5.20's)."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import ProteinMPNN
import class_scan_ref as CR
import group_scan_ref as GR
from tied_states_ref import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
TOL, TOL_GPU = 1e-3, 2e-4
_models = {}


def model(weights_np, k, prec):
    if (k, prec) not in _models:
        m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                        polytype_to_int=spec.polytype_to_int())
        m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
        m = m.to(DEV).eval()
        m.message_precision = prec
        _models[(k, prec)] = m
    return _models[(k, prec)]


def setup(name, weights_np, prec):
    c = CR.case(name)
    return c, model(weights_np, c["K"], prec), to_dev(c["fd"], DEV), torch.from_numpy(c["st"]), torch.from_numpy(c["tk"])


def scan(m, fd, st, tk, method="cone"):
    return m.score_mutations(fd, sites=st, site_tokens=tk, method=method, tied=True, classes=True)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", CR.CASES)
def test_class_scan_matches_the_reference_the_dense_route_and_score_tied(weights_np, name, prec):
    """Per case: the sizes, lists, sparse units and the tokens every member received equal the numpy restatement exactly; own entries,
    units, base units, base rows, leader terms and delta against the CPU reference within 1e-3; the cone against the dense route and the base units against score_tied within 2e-4;
    delta against the fp64 sum of its own fp32 leader terms; the wild type within 2e-4 x leader rows.
    Measured, max over the seven cases (MI355X, x3 / fp32): against the reference own entries 1.7e-5 / 3.0e-6, units 2.5e-5 / 3.7e-6,
    base units 1.7e-5 / 3.7e-6, base rows 2.2e-5 / 3.9e-6, leader terms 2.4e-5 / 3.8e-6, delta 5.6e-5 / 1.7e-5; cone against dense
    units 1.4e-6, delta / leader rows 9.5e-6 / 2.1e-5; base units against score_tied 9.5e-7; delta error / bound at most 0.033."""
    c, m, fd, st, tk = setup(name, weights_np, prec)
    ref = CR.reference(name)
    L, n = len(c["key"]), len(c["tk"])
    out = scan(m, fd, st, tk)
    assert out["method"] == "cone" and out["chunks"] == 1
    # ---- the layouts
    assert out["site_rows"].dtype == torch.int32 and np.array_equal(out["site_rows"].cpu().numpy(), c["site_rows"])
    assert out["leader"].cpu().tolist() == c["leader"].tolist()
    width = out["sites_flat"].shape[1]
    assert np.array_equal(out["sites_flat"].cpu().numpy(), c["sites8"][:, :width]) and (c["sites8"][:, width:] < 0).all()
    assert np.array_equal(out["site_tokens_flat"].cpu().numpy(), c["tok"][:, :1 + width])
    site_of = c["tk"][:, 0]
    rows = c["site_rows"][site_of, 2]
    want_res = np.concatenate([c["u3"][q] for q in site_of])
    assert np.array_equal(out["row_offsets"].cpu().numpy(), np.concatenate(([0], np.cumsum(rows))))
    assert out["row_residue"].dtype == torch.int32 and np.array_equal(out["row_residue"].cpu().numpy(), want_res)
    want_units = [GR.unit_list(c["u3"][q], c["leader"], c["mask"]) for q in site_of]
    n_units = np.array([len(u) for u in want_units])
    assert out["unit_offsets"].dtype == torch.int64 and out["unit_residue"].dtype == torch.int32
    assert np.array_equal(out["unit_offsets"].cpu().numpy(), np.concatenate(([0], np.cumsum(n_units))))
    assert np.array_equal(out["unit_residue"].cpu().numpy(), np.concatenate(want_units))
    assert out["base_log_probs"].shape == (1, L, 33) and out["base_token_log_probs"].shape == (L,)
    assert torch.equal(out["sites"].cpu(), st) and torch.equal(out["site_tokens"].cpu(), tk)
    # ---- against the CPU reference
    assert bool(torch.isfinite(ref["delta"]).all())
    vid_r, vid_u, ures = np.repeat(np.arange(n), rows), np.repeat(np.arange(n), n_units), np.concatenate(want_units)
    unmasked = c["mask"] != 0
    d_own = np.abs(out["row_token_log_prob"].cpu().numpy() - ref["own"][1:].numpy()[vid_r, want_res])[unmasked[want_res]].max()
    d_unit = np.abs(out["unit_log_prob"].cpu().numpy() - ref["units"][1:].numpy()[vid_u, ures]).max()
    d_bunit = float((out["base_token_log_probs"].cpu().double() - ref["units"][0])[torch.from_numpy(unmasked)].abs().max())
    d_base = float((out["base_log_probs"][0].cpu().double() - ref["log_probs"][0])[torch.from_numpy(unmasked)].abs().max())
    d_delta = np.abs(out["delta_log_likelihood"].cpu().numpy() - ref["delta"].numpy())
    w = (c["mask"] != 0).astype(np.float32)                      # mask * chain_mask (all ones) at the unit's listed-first member
    base = out["base_token_log_probs"].cpu().numpy()
    terms = w[ures] * (out["unit_log_prob"].cpu().numpy() - base[ures])
    ref_terms = w[ures] * (ref["units"][1:].numpy()[vid_u, ures] - ref["units"][0].numpy()[ures])
    d_term = np.abs(terms - ref_terms).max()
    print(f"class scan {name} {prec} vs the reference: own {d_own:.2e} unit {d_unit:.2e} base units {d_bunit:.2e} base rows {d_base:.2e} "
          f"leader terms {d_term:.2e} delta {d_delta.max():.2e}; rows {sorted(set(rows.tolist()))}")
    assert max(d_own, d_unit, d_bunit, d_base) < TOL and d_delta.max() < TOL and d_term < TOL
    # ---- the cone against the dense route
    dense = scan(m, fd, st, tk, "dense")
    assert dense["method"] == "dense" and dense["site_rows"] is None and dense["row_residue"].numel() == n * L
    assert torch.equal(dense["leader"], out["leader"]) and torch.equal(dense["site_tokens_flat"], out["site_tokens_flat"])
    g_own = np.abs(out["row_token_log_prob"].cpu().numpy() - dense["row_token_log_prob"].view(n, L).cpu().numpy()[vid_r, want_res])[unmasked[want_res]].max()
    du = dense["unit_residue"].view(n, -1)[0].cpu().numpy()
    col = {int(u): q for q, u in enumerate(du)}
    g_unit = np.abs(out["unit_log_prob"].cpu().numpy() - dense["unit_log_prob"].view(n, len(du)).cpu().numpy()[vid_u, [col[int(u)] for u in ures]]).max()
    g_bunit = float((out["base_token_log_probs"] - dense["base_token_log_probs"])[torch.from_numpy(unmasked).to(DEV)].abs().max())
    g_delta = (out["delta_log_likelihood"] - dense["delta_log_likelihood"]).abs().cpu().numpy() / n_units
    print(f"class scan {name} {prec} cone vs dense: own {g_own:.2e} unit {g_unit:.2e} base units {g_bunit:.2e} delta / leader rows {g_delta.max():.2e}")
    assert max(g_own, g_unit, g_bunit) < TOL_GPU and g_delta.max() < TOL_GPU
    # ---- base units are score_tied's
    tied = m.score_tied(fd)
    d = float((tied["token_log_probs"][0] - out["base_token_log_probs"])[torch.from_numpy(unmasked).to(DEV)].abs().max())
    print(f"class scan {name} {prec}: base units vs score_tied {d:.2e}")
    assert d < TOL_GPU and torch.equal(tied["leader"], out["leader"])
    # ---- delta is the fp32 recursive sum of the call's own leader terms
    assert terms.dtype == np.float32
    delta = out["delta_log_likelihood"].cpu().numpy()
    worst = 0.0
    for v in range(n):
        t = terms[vid_u == v].astype(np.float64)
        err, bound = abs(float(delta[v]) - t.sum()), (int(rows[v]) - 1) * 2.0 ** -24 * np.abs(t).sum()
        assert err <= bound, (v, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    print(f"class scan {name} {prec}: delta error / bound of the fp32 recursive sum at most {worst:.3f}")
    # ---- the wild type, the losses
    S0, wild = c["fd"]["S"][0].numpy(), 0
    for v, row in enumerate(c["tok"]):
        if all(int(t) == int(S0[r]) for r, t in zip(c["sites8"][row[0]], row[1:]) if r >= 0):
            assert abs(float(delta[v])) < TOL_GPU * n_units[v]
            wild += 1
    assert wild >= len(c["st"]) - 1                               # (every site but "G named alone" lists its wild type)
    cnt = CR.counted(c)
    loss = -(ref["units"][0] * cnt.double()).sum() / (cnt.double().sum() + 1e-8)
    assert abs(float(out["base_loss"]) - float(loss)) < TOL
    assert torch.allclose(out["loss"], out["base_loss"] - out["delta_log_likelihood"] / (cnt.sum() + 1e-8).to(DEV))


BITS = ("delta_log_likelihood", "base_token_log_probs", "base_log_probs", "row_token_log_prob", "unit_log_prob", "row_residue", "unit_residue",
        "row_offsets", "unit_offsets", "site_rows")


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_identity_maps_give_the_bits_of_the_group_scan(weights_np, prec):
    """Identity symmetry_token_maps on trimer_l24 with classes=True: every output has the bits of tied=True, classes=False, which still
    reports the group route's keys alone."""
    g = GR.case("trimer_l24")
    m, fd = model(weights_np, g["K"], prec), to_dev(g["fd"], DEV)
    st, tk = torch.from_numpy(g["st"]), torch.from_numpy(g["tk"])
    group = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    assert group["method"] == "cone" and "site_tokens_flat" not in group and "classes" not in group
    ident = list(range(33))
    maps = dict(fd, symmetry_token_maps=[[ident] * len(grp) for grp in fd["symmetry_residues"]])
    for fdc in (fd, maps):
        cls = m.score_mutations(fdc, sites=st, site_tokens=tk, method="cone", tied=True, classes=True)
        assert cls["method"] == "cone"
        for k in BITS + ("leader",):
            assert torch.equal(cls[k], group[k]), k
    with pytest.raises(NotImplementedError, match="identity token maps"):
        m.score_mutations(maps, sites=st, site_tokens=tk, method="cone", tied=True)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_equal_bits_across_calls_and_chunks(weights_np, prec):
    """Two calls give equal bits; a small score_library_tokens that forces several chunks gives the one-chunk bits per variant."""
    c, m, fd, st, tk = setup("l48_k16", weights_np, prec)
    n = len(tk)
    one, two = scan(m, fd, st, tk), scan(m, fd, st, tk)
    for k in BITS:
        assert torch.equal(one[k], two[k]), k
    budget = m.score_library_tokens
    try:
        m.score_library_tokens = max(1, int(c["site_rows"][c["tk"][:, 0]].sum()) // 9)      # 3 x that many item rows per call
        cut = scan(m, fd, st, tk)
    finally:
        m.score_library_tokens = budget
    assert cut["chunks"] >= 3
    for k in BITS:
        assert torch.equal(one[k], cut[k]), k
    assert n == one["delta_log_likelihood"].numel()


def test_the_class_axis_is_the_general_form(weights_np):
    """pairs=True: every pair once from its first listed member over its classes (4 canonical, 6 with wobble on an RNA-containing pair),
    an unpaired position over its alphabet; classes / class_tokens / delta [P, T] against the general form on the first two listed
    members, bit for bit; "auto" and the scan form without pairs."""
    c, m, fd, st, tk = setup("l12_lt_k", weights_np, "x3")
    out = m.score_mutations(fd, pairs=True, method="cone", tied=True, classes=True)
    P, T = out["delta"].shape
    lead = c["leader"]
    assert out["positions"].tolist() == [i for i in range(12) if lead[i] == i and c["mask"][i] != 0]
    assert out["classes"].tolist() == out["tokens"].tolist() and out["class_tokens"].shape == (P, T, 2)
    lanes = out["classes"].tolist()
    assert spec.CLASS_GU in lanes and spec.CLASS_UG in lanes
    valid = ~torch.isnan(out["delta"])
    ct = out["class_tokens"]
    assert torch.equal(valid, ct[:, :, 0] >= 0)
    per_pos = dict(zip(out["positions"].tolist(), valid.sum(1).tolist()))
    assert per_pos[4] == 6 and per_pos[5] == 4 and per_pos[0] == 20       # wobble on the first pair only; a protein residue
    units = {m_[0]: m_ for m_, _ in c["units"]}
    sites = torch.tensor([[p, units[p][1] if p in units else -1] for p in out["positions"].tolist()])
    rows = [[q, int(ct[q, k, 0]), max(int(ct[q, k, 1]), 0)] for q in range(P) for k in range(T) if bool(valid[q, k])]
    general = m.score_mutations(fd, sites=sites, site_tokens=torch.tensor(rows), method="cone", tied=True, classes=True)
    assert torch.equal(general["delta_log_likelihood"], out["delta"][valid])
    for k in BITS:
        assert torch.equal(general[k], out[k]), k
    assert torch.equal(general["site_tokens_flat"], out["site_tokens_flat"])
    # the wobble lane gives the first member its G and the second its U
    rti = spec.restype_to_int()
    q, k = out["positions"].tolist().index(4), lanes.index(spec.CLASS_GU)
    assert ct[q, k].tolist() == [rti["G"], rti["U"]]
    # the scan form without pairs: positions x tokens by the lowest-lane rule (G alone: G-C); "auto" on a case whose cones are small
    a = m.score_mutations(fd, positions=torch.tensor([4]), tokens=torch.tensor([rti["G"]]), method="cone", tied=True, classes=True)
    assert a["site_tokens_flat"][0].tolist() == [0, rti["G"], rti["C"]]
    c2, m2, fd2, st2, tk2 = setup("4oqu", weights_np, "x3")
    auto = m2.score_mutations(fd2, sites=st2, site_tokens=tk2, tied=True, classes=True)
    assert auto["method"] == "cone"
    heavy = m.score_mutations(fd, sites=st[:1], site_tokens=tk[tk[:, 0] == 0], tied=True, classes=True)
    assert c["site_rows"][0].sum() > 2 * 12 and heavy["method"] == "dense"
    ref = CR.reference("l12_lt_k")
    assert float((heavy["delta_log_likelihood"].cpu().double() - ref["delta"][torch.from_numpy(c["tk"][:, 0] == 0)]).abs().max()) < TOL * 12


def test_refusals_are_followed_by_a_valid_call(weights_np):
    c, m, fd, st, tk = setup("l12_lt_k", weights_np, "x3")
    want = scan(m, fd, st, tk)

    def then_good():
        got = scan(m, fd, st, tk)
        for k in BITS:
            assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError, match="needs tied=True"):
        m.score_mutations(fd, sites=st, site_tokens=tk, classes=True)
    then_good()
    with pytest.raises(NotImplementedError, match="state_weights"):
        m.score_mutations(dict(fd, state_weights=[0.5, 0.5]), positions=[1], tied=True, classes=True)
    with pytest.raises(NotImplementedError, match="pair_terms"):
        m.score_mutations(dict(fd, pair_terms={}), positions=[1], tied=True, classes=True)
    rti = spec.restype_to_int()
    with pytest.raises(ValueError, match="has no class with token"):
        m.score_mutations(fd, sites=[[4, 11]], site_tokens=[[0, rti["A"], rti["A"]]], tied=True, classes=True)
    then_good()
    with pytest.raises(NotImplementedError, match="identity token maps"):
        m.score_mutations(fd, positions=[1], tied=True)
    then_good()


def test_cli_mutation_classes(tmp_path, golden_dir):
    """--mutation_scan 1 --mutation_tied 1 --mutation_classes 1 on 1AM9: the protein dimer tied at two positions, the DNA duplex E / F
    paired at two; mutations/<name>.npz equals the Python call; without the flag the pinned errors hold."""
    import lzma
    import os
    from na_mpnn_amd import cli, pdbio, synth
    pdb = os.path.join(str(tmp_path), "1am9.pdb")
    with lzma.open(os.path.join(golden_dir, "pdb", "1am9.pdb.xz"), "rb") as fh, open(pdb, "wb") as out:
        out.write(fh.read())
    base = os.path.join(str(tmp_path), "out")
    P = pdbio.parse_pdb(pdb)
    L = len(P["S"])
    enc = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    at = {e: i for i, e in enumerate(enc)}
    prs = [("E5", "F34"), ("E6", "F33")]                           # (E_k pairs with F_(39 - k): A-T and G-C)
    red, sym = " ".join(["A330", "B330", "A340", "B340", "A335"] + [r for p in prs for r in p]), "A330,B330|A340,B340"
    argv = ["--mode", "design", "--pdb_path", pdb, "--out_folder", base, "--random_init_seed", "0", "--seed", "7", "--redesigned_residues", red,
            "--symmetry_residues", sym, "--paired_residues", ",".join(f"{a}:{b}" for a, b in prs), "--mutation_scan", "1", "--mutation_tied", "1"]
    with pytest.raises(ValueError, match="--mutation_tied"):       # pinned: pair flags beside --mutation_tied without the new flag
        cli.main(argv)
    with pytest.raises(ValueError, match="--mutation_classes 1 needs"):
        cli.main(argv[:-2] + ["--mutation_classes", "1"])
    cli.main(argv + ["--mutation_classes", "1"])
    z = np.load(os.path.join(base, "mutations", "1am9.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["residues", "tokens", "delta", "base_loss", "wild_type_token", "site_rows", "leader", "unit_offsets",
                                      "unit_residue", "unit_log_prob", "classes", "class_tokens"])
    chain_mask = np.array([int(e in red.split()) for e in enc], np.int32)
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(True),
                    polytype_to_int=spec.polytype_to_int())      # (the command line's model: --na_shared_tokens is 1 by default)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    m = m.to(DEV).eval()
    fd = pdbio.to_feature_dict(P, chain_mask, torch.device(DEV))
    fd.update(batch_size=1, symmetry_residues=[[at[t] for t in g.split(",")] for g in sym.split("|")], symmetry_weights=[[1.0, 1.0]] * 2,
              paired_residues=[(at[a], at[b]) for a, b in prs])
    torch.manual_seed(7)
    fd["randn"] = torch.randn(1, L, device=DEV)
    out = m.score_mutations(fd, pairs=True, tied=True, classes=True)
    want = sorted([at["A330"], at["A335"], at["A340"]] + [at[a] for a, _ in prs])
    assert out["positions"].tolist() == want and z["residues"].tolist() == [enc[i] for i in want]
    assert np.array_equal(z["delta"], out["delta"].cpu().numpy(), equal_nan=True) and z["delta"].shape == (5, 24)
    for k in ("leader", "unit_offsets", "unit_residue", "unit_log_prob", "site_rows", "classes", "class_tokens"):
        assert np.array_equal(z[k], out[k].cpu().numpy()), k
    assert int(z["leader"][at[prs[0][1]]]) == at[prs[0][0]] and int(z["leader"][at["B330"]]) == at["A330"]
    assert (~np.isnan(z["delta"])).sum(1).tolist() == [4 if enc[i].startswith("E") else 20 for i in want]
