"""GPU tests of the symmetric scan — ProteinMPNN.score_mutations(tied=True) (namp_group_mutations): the cone route
against the CPU reference (group_scan_ref: tied_score_ref.parallel_logits + unit_values on the explicit sequences), against the dense
route and score_tied, its own invariants (the sparse layouts against the numpy restatement, the fp32 sum of delta, chunks, orders,
determinism), the unchanged paths, "auto" and the refusals.

Bars: 1e-3 per entry against the CPU oracle (the project's bar on log-probs) and 1e-3 x the variant's leader rows on the deltas (a
delta sums that many unit differences); 2e-4 per entry between two GPU routes."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import ProteinMPNN
import group_scan_ref as GR
import state_scan_ref as SR
from tied_states_ref import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
TOL, TOL_GPU = 1e-3, 2e-4
_models = {}


def new_model(weights_np, k, prec):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    m = m.to(DEV).eval()
    m.message_precision = prec
    return m


def model(weights_np, k, prec):
    if (k, prec) not in _models:
        _models[(k, prec)] = new_model(weights_np, k, prec)
    return _models[(k, prec)]


def setup(name, weights_np, prec):
    c = GR.case(name)
    return c, model(weights_np, c["K"], prec), to_dev(c["fd"], DEV), torch.from_numpy(c["st"]), torch.from_numpy(c["tk"])


def per_variant(out, key_off, keys, v):
    a, b = int(out[key_off][v]), int(out[key_off][v + 1])
    return tuple(out[k][a:b] for k in keys)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", GR.CASES)
def test_group_scan_matches_the_reference_the_dense_route_and_score_tied(weights_np, name, prec):
    """Per case: the sizes, lists and sparse units equal the numpy restatement exactly; own entries, units, base units and base rows
    against the CPU reference within 1e-3, delta within 1e-3 x the variant's leader rows; the cone against the dense route and the base
    units against score_tied within 2e-4; delta against the fp64 sum of its own fp32 leader terms.
    Measured, max over the six cases (MI355X, x3 / fp32): against the reference own entries 1.0e-5 / 3.0e-6, units 1.1e-5 / 3.4e-6, base
    units 8.6e-6 / 3.4e-6, base rows 1.6e-5 / 3.7e-6, delta / leader rows 8.6e-6 / 3.2e-6; cone against dense per entry 7.6e-6 / 1.9e-6,
    delta / leader rows 2.5e-5 / 1.1e-5; base units against score_tied at most 5.3e-6; delta error / bound at most 0.15."""
    c, m, fd, st, tk = setup(name, weights_np, prec)
    ref = GR.reference(name)
    L, n = len(c["key"]), len(c["tk"])
    out = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    assert out["method"] == "cone" and out["chunks"] == 1
    # ---- the layouts
    assert out["site_rows"].dtype == torch.int32 and np.array_equal(out["site_rows"].cpu().numpy(), c["site_rows"])
    assert out["leader"].cpu().tolist() == c["leader"].tolist()
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
    vid_r, vid_u, ures = np.repeat(np.arange(n), rows), np.repeat(np.arange(n), n_units), np.concatenate(want_units)
    unmasked = c["mask"] != 0
    d_own = np.abs(out["row_token_log_prob"].cpu().numpy() - ref["own"][1:].numpy()[vid_r, want_res])[unmasked[want_res]].max()
    d_unit = np.abs(out["unit_log_prob"].cpu().numpy() - ref["units"][1:].numpy()[vid_u, ures]).max()
    d_bunit = float((out["base_token_log_probs"].cpu().double() - ref["units"][0])[torch.from_numpy(unmasked)].abs().max())
    d_base = float((out["base_log_probs"][0].cpu().double() - ref["log_probs"][0])[torch.from_numpy(unmasked)].abs().max())
    d_delta = np.abs(out["delta_log_likelihood"].cpu().numpy() - ref["delta"].numpy()) / n_units
    print(f"group scan {name} {prec} vs the reference: own {d_own:.2e} unit {d_unit:.2e} base units {d_bunit:.2e} base rows {d_base:.2e} "
          f"delta / leader rows {d_delta.max():.2e}; rows {sorted(set(rows.tolist()))}")
    assert max(d_own, d_unit, d_bunit, d_base) < TOL and d_delta.max() < TOL
    # ---- the cone against the dense route
    dense = m.score_mutations(fd, sites=st, site_tokens=tk, method="dense", tied=True)
    assert dense["method"] == "dense" and dense["site_rows"] is None and dense["row_residue"].numel() == n * L
    assert torch.equal(dense["leader"], out["leader"])
    g_own = np.abs(out["row_token_log_prob"].cpu().numpy() - dense["row_token_log_prob"].view(n, L).cpu().numpy()[vid_r, want_res])[unmasked[want_res]].max()
    du = dense["unit_residue"].view(n, -1)[0].cpu().numpy()
    col = {int(u): q for q, u in enumerate(du)}
    g_unit = np.abs(out["unit_log_prob"].cpu().numpy() - dense["unit_log_prob"].view(n, len(du)).cpu().numpy()[vid_u, [col[int(u)] for u in ures]]).max()
    g_bunit = float((out["base_token_log_probs"] - dense["base_token_log_probs"])[torch.from_numpy(unmasked).to(DEV)].abs().max())
    g_delta = (out["delta_log_likelihood"] - dense["delta_log_likelihood"]).abs().cpu().numpy() / n_units
    print(f"group scan {name} {prec} cone vs dense: own {g_own:.2e} unit {g_unit:.2e} base units {g_bunit:.2e} delta / leader rows {g_delta.max():.2e}")
    assert max(g_own, g_unit, g_bunit) < TOL_GPU and g_delta.max() < TOL_GPU
    # ---- base units are score_tied's
    tied = m.score_tied(fd)
    d = float((tied["token_log_probs"][0] - out["base_token_log_probs"])[torch.from_numpy(unmasked).to(DEV)].abs().max())
    print(f"group scan {name} {prec}: base units vs score_tied {d:.2e}")
    assert d < TOL_GPU and torch.equal(tied["leader"], out["leader"])
    # ---- delta is the fp32 recursive sum of the call's own leader terms
    w = (c["mask"] != 0).astype(np.float32)                      # mask * chain_mask (all ones) at the unit's listed-first member
    base = out["base_token_log_probs"].cpu().numpy()
    terms = w[ures] * (out["unit_log_prob"].cpu().numpy() - base[ures])
    assert terms.dtype == np.float32
    delta = out["delta_log_likelihood"].cpu().numpy()
    worst = 0.0
    for v in range(n):
        t = terms[vid_u == v].astype(np.float64)
        err, bound = abs(float(delta[v]) - t.sum()), (int(rows[v]) - 1) * 2.0 ** -24 * np.abs(t).sum()
        assert err <= bound, (v, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    print(f"group scan {name} {prec}: delta error / bound of the fp32 recursive sum at most {worst:.3f}")
    # ---- the wild type, the losses
    for v, row in enumerate(c["tk"]):
        if all(int(t) == int(c["fd"]["S"][0, r]) for r, t in zip(c["st"][row[0]], row[1:]) if r >= 0):
            assert abs(float(delta[v])) < TOL_GPU * n_units[v]
    cnt = GR.counted(c)
    loss = -(ref["units"][0] * cnt.double()).sum() / (cnt.double().sum() + 1e-8)
    assert abs(float(out["base_loss"]) - float(loss)) < TOL
    assert torch.allclose(out["loss"], out["base_loss"] - out["delta_log_likelihood"] / (cnt.sum() + 1e-8).to(DEV))


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_no_tie_is_the_plain_scan(weights_np, prec):
    """tied=True on a complex without ties against the plain scan: the same lists, the deltas within 2e-4 x rows (the base stream is an
    item pass there, the ordinary decoder here: not bits)."""
    c, m, fd, st, tk = setup("plain_l17", weights_np, prec)
    out = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    plain = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone")
    assert torch.equal(plain["row_residue"], out["row_residue"]) and torch.equal(plain["site_rows"], out["site_rows"])
    assert torch.equal(out["unit_residue"], out["row_residue"]) and torch.equal(out["unit_log_prob"], out["row_token_log_prob"])
    rows = c["site_rows"][c["tk"][:, 0], 2]
    d = (plain["delta_log_likelihood"] - out["delta_log_likelihood"]).abs().cpu().numpy() / rows
    e = float((plain["row_token_log_prob"] - out["row_token_log_prob"]).abs().max())
    b = float((plain["base_log_probs"] - out["base_log_probs"]).abs().max())
    print(f"group scan plain_l17 {prec} vs the plain scan: delta / rows {d.max():.2e} own {e:.2e} base rows {b:.2e}")
    assert d.max() < TOL_GPU and e < TOL_GPU and b < TOL_GPU


BITS = ("delta_log_likelihood", "base_token_log_probs", "base_log_probs")


def assert_same_variant(a, va, b, vb):
    assert torch.equal(a["delta_log_likelihood"][va], b["delta_log_likelihood"][vb])
    for off, keys in (("row_offsets", ("row_residue", "row_token_log_prob")), ("unit_offsets", ("unit_residue", "unit_log_prob"))):
        for x, y in zip(per_variant(a, off, keys, va), per_variant(b, off, keys, vb)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_equal_bits_across_calls_chunks_orders_and_company(weights_np, prec):
    """Two calls, three or more chunks, a shuffled variant list and a variant alone give the one-chunk bits."""
    c, m, fd, st, tk = setup("dimer_l48", weights_np, prec)
    n = len(tk)
    one = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    two = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    for k in BITS + ("row_token_log_prob", "unit_log_prob", "row_residue", "unit_residue", "row_offsets", "unit_offsets"):
        assert torch.equal(one[k], two[k]), k
    budget = m.score_library_tokens
    try:
        m.score_library_tokens = max(1, int(c["site_rows"][c["tk"][:, 0]].sum()) // 9)      # 3 x that many item rows per call
        cut = m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    finally:
        m.score_library_tokens = budget
    assert cut["chunks"] >= 3
    for v in range(n):
        assert_same_variant(one, v, cut, v)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    shuffled = m.score_mutations(fd, sites=st, site_tokens=tk[perm], method="cone", tied=True)
    for q, v in enumerate(perm.tolist()):
        assert_same_variant(one, v, shuffled, q)
    for v in (0, n // 2, n - 1):
        alone = m.score_mutations(fd, sites=st[c["tk"][v, 0]:c["tk"][v, 0] + 1], site_tokens=torch.tensor([[0] + c["tk"][v, 1:].tolist()]),
                                  method="cone", tied=True)
        assert_same_variant(one, v, alone, 0)
        for k in BITS[1:]:
            assert torch.equal(one[k], alone[k]), k


def test_auto_the_scan_form_and_the_unchanged_untied_call(weights_np):
    c, m, fd, st, tk = setup("dimer_l48", weights_np, "x3")
    L = 48
    assert c["site_rows"][c["tk"][:, 0]].sum() <= 2 * L * len(c["tk"])
    out = m.score_mutations(fd, sites=st, site_tokens=tk, tied=True)
    assert out["method"] == "cone" and np.array_equal(out["site_rows"].cpu().numpy(), c["site_rows"])
    # the cones of the first-visited units of mixed_l12 cover the complex: "auto" reads the sizes back and takes the dense route
    c2, m2, fd2, st2, tk2 = setup("mixed_l12", weights_np, "x3")
    q = c2["what"].index("first-visited unit")
    assert c2["site_rows"][q].sum() > 2 * 12
    first = torch.from_numpy(c2["tk"][c2["tk"][:, 0] == q])
    heavy = m2.score_mutations(fd2, sites=st2, site_tokens=first, tied=True)
    assert heavy["method"] == "dense" and heavy["site_rows"].cpu().tolist() == c2["site_rows"].tolist()
    ref2 = GR.reference("mixed_l12")
    assert float((heavy["delta_log_likelihood"].cpu().double() - ref2["delta"][torch.from_numpy(c2["tk"][:, 0] == q)]).abs().max()) < TOL * 12
    # the scan form: the default positions are the listed-first members of the counted units; a member stands for its unit
    scan = m.score_mutations(fd, tokens=torch.tensor([0, 5]), tied=True, method="cone")
    assert scan["positions"].tolist() == [i for i in range(L) if c["leader"][i] == i and c["mask"][i] != 0]
    assert scan["delta"].shape == (len(scan["positions"]), 2) and torch.equal(scan["delta"].reshape(-1), scan["delta_log_likelihood"])
    a = m.score_mutations(fd, positions=torch.tensor([5]), tokens=torch.tensor([0, 5]), tied=True, method="cone")
    b = m.score_mutations(fd, positions=torch.tensor([29]), tokens=torch.tensor([0, 5]), tied=True, method="cone")
    assert torch.equal(a["delta_log_likelihood"], b["delta_log_likelihood"]) and torch.equal(a["unit_log_prob"], b["unit_log_prob"])
    empty = m.score_mutations(fd, positions=torch.zeros(0, dtype=torch.long), tied=True)
    assert empty["delta_log_likelihood"].shape == (0,) and empty["unit_offsets"].tolist() == [0] and empty["row_offsets"].tolist() == [0]
    assert empty["base_token_log_probs"].shape == (L,) and empty["method"] == "dense"
    # tied=False reads no symmetry group: the bits of the call without the key
    bare = {k: v for k, v in fd.items() if k not in ("symmetry_residues", "symmetry_weights")}
    x = m.score_mutations(fd, sites=st[:2, :1], site_tokens=torch.tensor([[0, 3], [1, 7]]), method="cone")
    y = m.score_mutations(bare, sites=st[:2, :1], site_tokens=torch.tensor([[0, 3], [1, 7]]), method="cone")
    for k in ("delta_log_likelihood", "row_token_log_prob", "row_residue", "base_log_probs", "site_rows"):
        assert torch.equal(x[k], y[k]), k
    assert "leader" not in x and "unit_offsets" not in x


def test_cli_mutation_tied(tmp_path, golden_dir):
    """--mutation_scan 1 --mutation_tied 1 --symmetry_residues on the dimer 1AM9 (chains A and B): mutations/<name>.npz equals the Python
    call and holds leader and the sparse units; the flag without its companions is refused."""
    import lzma
    import os
    from na_mpnn_amd import cli, pdbio, synth
    pdb = os.path.join(str(tmp_path), "1am9.pdb")
    with lzma.open(os.path.join(golden_dir, "pdb", "1am9.pdb.xz"), "rb") as fh, open(pdb, "wb") as out:
        out.write(fh.read())
    base = os.path.join(str(tmp_path), "out")
    red, sym = "A330 B330 A340 B340 A335", "A330,B330|A340,B340"
    cli.main(["--mode", "design", "--pdb_path", pdb, "--out_folder", base, "--random_init_seed", "0", "--seed", "7", "--redesigned_residues", red,
              "--symmetry_residues", sym, "--mutation_scan", "1", "--mutation_tied", "1"])
    z = np.load(os.path.join(base, "mutations", "1am9.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["residues", "tokens", "delta", "base_loss", "wild_type_token", "site_rows", "leader", "unit_offsets",
                                      "unit_residue", "unit_log_prob"])
    P = pdbio.parse_pdb(pdb)
    L = len(P["S"])
    enc = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    at = {e: i for i, e in enumerate(enc)}
    chain_mask = np.array([int(e in red.split()) for e in enc], np.int32)
    m = model(synth.make_weights(0), 32, "x3")
    fd = pdbio.to_feature_dict(P, chain_mask, torch.device(DEV))
    fd.update(batch_size=1, symmetry_residues=[[at[t] for t in g.split(",")] for g in sym.split("|")], symmetry_weights=[[1.0, 1.0]] * 2)
    torch.manual_seed(7)
    fd["randn"] = torch.randn(1, L, device=DEV)
    out = m.score_mutations(fd, tied=True)
    assert z["residues"].tolist() == ["A330", "A335", "A340"] and out["positions"].tolist() == [at["A330"], at["A335"], at["A340"]]
    assert np.array_equal(z["delta"], out["delta"].cpu().numpy(), equal_nan=True) and z["delta"].shape == (3, 20)
    for k in ("leader", "unit_offsets", "unit_residue", "unit_log_prob", "site_rows"):
        assert np.array_equal(z[k], out[k].cpu().numpy()), k
    assert int(z["leader"][at["B330"]]) == at["A330"] and int(z["leader"][at["B340"]]) == at["A340"] and float(z["base_loss"]) == float(out["base_loss"])
    wt = z["delta"][np.arange(3), [out["tokens"].tolist().index(int(t)) for t in z["wild_type_token"]]]
    assert np.abs(wt).max() < TOL_GPU * L
    untied = m.score_mutations(fd, sites=torch.tensor([[at["A330"], at["B330"]]]), site_tokens=torch.tensor([[0, 5, 5]]))
    assert "leader" not in untied
    for bad in (["--mutation_tied", "1"], ["--mutation_tied", "1", "--mutation_scan", "1"],
                ["--mutation_tied", "1", "--mutation_scan", "1", "--symmetry_residues", sym, "--paired_residues", "E1,F21"]):
        with pytest.raises(ValueError, match="--mutation_tied"):
            cli.main(["--mode", "design", "--pdb_path", pdb, "--out_folder", base] + bad)


def test_every_refusal_is_followed_by_a_valid_call(weights_np):
    c, m, fd, st, tk = setup("mixed_l12", weights_np, "x3")
    good = lambda: m.score_mutations(fd, sites=st, site_tokens=tk, method="cone", tied=True)
    want = good()

    def then_good():
        got = good()
        for k in BITS + ("unit_log_prob", "row_token_log_prob"):
            assert torch.equal(got[k], want[k]), k
    for extra in (dict(symmetry_token_maps=[[None, None], [None] * 4, [None]]), dict(paired_residues=[[0, 3]]), dict(paired_wobble=True),
                  dict(pair_terms={})):
        with pytest.raises(NotImplementedError):
            m.score_mutations(dict(fd, **extra), positions=[1], tied=True)
        then_good()
    with pytest.raises(NotImplementedError):
        m.score_mutations(fd, pairs=True, tied=True)
    then_good()
    with pytest.raises(NotImplementedError):
        m.score_mutations(dict(fd, state_weights=[0.5, 0.5]), positions=[1], tied=True)
    then_good()
    with pytest.raises(ValueError, match="two residues of one tied unit"):
        m.score_mutations(fd, sites=[[2, 8]], site_tokens=[[0, 1, 1]], tied=True)
    then_good()
    with pytest.raises(ValueError, match="expands to 9 flat residues.*8"):
        m.score_mutations(fd, sites=[[2, 1, 0, 3, 4]], site_tokens=[[0, 1, 1, 1, 1, 1]], tied=True)
    then_good()
    masked = dict(fd, chain_mask=fd["chain_mask"].clone())
    masked["chain_mask"][0, 0] = 0
    with pytest.raises(ValueError, match="mask \\* chain_mask == 0"):
        m.score_mutations(masked, positions=[0], tied=True)
    then_good()
    broken = dict(fd, S=fd["S"].clone())
    broken["S"][0, 7] = (int(fd["S"][0, 7]) + 1) % 20
    with pytest.raises(ValueError, match="not tie-consistent"):
        m.score_mutations(broken, positions=[0], tied=True)
    then_good()
    # state_weights with tied=True and no listed group: the specificity scan as it stands
    cx, fd_s, K, sites, tks = SR.case("LltK")
    ms, fds = model(weights_np, K, "x3"), to_dev(fd_s, DEV)
    a = ms.score_mutations(fds, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tks), method="cone", tied=True)
    b = ms.score_mutations(fds, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tks), method="cone")
    for k in ("delta_log_likelihood", "state_delta", "unit_log_prob", "base_log_probs"):
        assert torch.equal(a[k], b[k]), k
    then_good()
