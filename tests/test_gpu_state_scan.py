"""GPU tests of the specificity scan — ProteinMPNN.score_mutations with feature_dict["state_weights"] (namp_state_mutations, DESIGN.md
5.19): the cone route against the CPU reference (state_scan_ref: context_states_ref.oracle_score_tied on the explicit sequences), against
the dense route, its own invariants (the sparse layouts, the fp32 sum of delta, chunks, determinism), the unchanged paths and "auto".

Bars (the project's own): 1e-3 per entry against the CPU oracle and 1e-3 x the variant's layer-3 rows on the deltas (a delta sums at
most that many entries); 2e-4 per entry and 2e-4 x rows between two GPU routes.  Entries are compared where they are defined: own
entries and base rows at PRESENT copies, units where the present copies of the residue hold one token (everywhere but at fixed residues
whose state_S rows differ; there score_tied reports -inf and so does base_token_log_probs)."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import ProteinMPNN
import context_states_ref as CR
import state_scan_ref as SR
from tied_states_ref import state_fd, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
TOL, TOL_GPU = 1e-3, 2e-4
_models, _refs = {}, {}


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
    """The case, its reference (computed once, shared, never modified) and its numpy restatement of the flat lists."""
    cx, fd, K, sites, tk = SR.case(name)
    if name not in _refs:
        ref = SR.reference(fd, K, sites, tk)
        rows, u3 = SR.flat_rows(fd, K, sites)
        _refs[name] = (ref, rows, u3)
    return cx, fd, K, sites, tk, _refs[name], model(weights_np, K, prec), to_dev(fd, DEV)


def presence(fd):
    """present [M, L] bool, counted [L] bool, same [L] bool: the present copies of the residue hold one token."""
    sS, sm = CR.contexts_of(fd)
    present = sm != 0
    counted = (fd["mask"] * fd["chain_mask"])[0] != 0
    rows = CR.token_rows(fd, fd["S"])[0]                                                 # [M, L]
    seat = present.float().argmax(0)
    same = ((rows == rows.gather(0, seat[None])) | ~present).all(0)
    return present, counted, same


def per_variant(out, key_off, keys, v):
    a, b = int(out[key_off][v]), int(out[key_off][v + 1])
    return tuple(out[k][a:b] for k in keys)


def delta_bound(out, counted, rows):
    """delta[v] against the fp64 sum of the call's own fp32 leader terms w_i * (unit_v - unit) within (rows - 1) * 2^-24 * sum |terms|."""
    uo = out["unit_offsets"].cpu().numpy()
    res = out["unit_residue"].cpu().numpy().astype(np.int64)
    base = out["base_token_log_probs"].cpu().numpy()
    w = counted.numpy().astype(np.float32)
    diff = out["unit_log_prob"].cpu().numpy() - np.where(w[res] != 0, base[res], np.float32(0))
    terms = w[res] * diff
    assert terms.dtype == np.float32
    delta = out["delta_log_likelihood"].cpu().numpy()
    worst = 0.0
    for v in range(len(delta)):
        t = terms[uo[v]:uo[v + 1]].astype(np.float64)
        err, bound = abs(float(delta[v]) - t.sum()), (int(rows[v]) - 1) * 2.0 ** -24 * np.abs(t).sum()
        assert err <= bound, (v, err, bound, len(t))
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", SR.CASES)
def test_state_scan_matches_the_reference_and_the_dense_route(weights_np, name, prec):
    """The cone route per case: the flat layouts equal the numpy restatement on the oracle's graphs exactly; every entry and both deltas
    against the CPU reference; the cone against the dense route; delta against the fp64 sum of its own fp32 leader terms; the wild
    type; the base units against score_tied; one state of weight 1 against the plain scan.
    Measured, max over the seven cases (MI355X, x3 / fp32): against the reference own entries 1.6e-5 / 3.4e-6, units 1.3e-5 / 3.8e-6,
    base rows 2.1e-5 / 3.9e-6, delta / rows 4.8e-6 / 2.4e-6, state_delta / rows 4.5e-6 / 2.4e-6; cone against dense per entry 1.3e-5 /
    1.9e-6, delta / rows 7.4e-6 / 8.1e-6, state_delta / rows 8.1e-6 / 1.1e-5; delta error / bound at most 0.07; base units against
    score_tied at most 9.5e-7; one state against the plain scan 4.3e-8 x rows."""
    cx, fd_cpu, K, sites, tk, (ref, site_rows, u3), m, fd = setup(name, weights_np, prec)
    M, L = fd_cpu["X"].shape[:2]
    N, n = M * L, len(tk)
    present, counted, same = presence(fd_cpu)
    out = m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tk), method="cone")
    assert out["method"] == "cone" and out["chunks"] == 1
    # ---- the layouts: flat rows, sparse units
    assert out["site_rows"].dtype == torch.int32 and np.array_equal(out["site_rows"].cpu().numpy(), site_rows)
    rows = site_rows[tk[:, 0], 2]
    assert np.array_equal(out["row_offsets"].cpu().numpy(), np.concatenate(([0], np.cumsum(rows))))
    want_res = np.concatenate([u3[int(q)] for q in tk[:, 0]])
    assert out["row_residue"].dtype == torch.int32 and np.array_equal(out["row_residue"].cpu().numpy(), want_res)
    pres_flat = present.reshape(N).numpy()
    want_units = [np.unique(u3[int(q)][pres_flat[u3[int(q)]]] % L) for q in tk[:, 0]]
    assert out["unit_offsets"].dtype == torch.int64 and out["unit_residue"].dtype == torch.int32
    assert np.array_equal(out["unit_offsets"].cpu().numpy(), np.concatenate(([0], np.cumsum([len(u) for u in want_units]))))
    assert np.array_equal(out["unit_residue"].cpu().numpy(), np.concatenate(want_units))
    assert out["base_log_probs"].shape == (1, N, 33) and out["state_delta"].shape == (n, M) and out["base_token_log_probs"].shape == (L,)
    assert out["base_state_log_likelihood"].shape == (M,) and out["state_weights"].cpu().tolist() == [float(np.float32(v)) for v in fd_cpu["state_weights"]]
    assert (rows % 16 != 0).any() and out["delta_log_likelihood"].dtype == torch.float32
    # ---- against the CPU reference: every entry, then the deltas
    vid_r = np.repeat(np.arange(n), rows)
    keep = pres_flat[want_res]
    own_ref = ref["own"][:-1].reshape(n, N).numpy()[vid_r, want_res]
    d_own = np.abs(out["row_token_log_prob"].cpu().numpy() - own_ref)[keep].max()
    ures = np.concatenate(want_units)
    vid_u = np.repeat(np.arange(n), [len(u) for u in want_units])
    ok = same.numpy()[ures]
    d_unit = np.abs(out["unit_log_prob"].cpu().numpy() - ref["units"][:-1].numpy()[vid_u, ures])[ok].max()
    d_base = float((out["base_log_probs"][0].cpu().double() - ref["log_probs"][-1].reshape(N, 33))[present.reshape(N)].abs().max())
    btlp = out["base_token_log_probs"].cpu()
    assert torch.equal(torch.isfinite(btlp), same)
    d_bunit = float((btlp.double() - ref["units"][-1])[same].abs().max())
    d_delta = np.abs(out["delta_log_likelihood"].cpu().numpy() - ref["delta"].numpy()) / rows
    d_state = np.abs(out["state_delta"].cpu().numpy() - ref["state_delta"].numpy()) / rows[:, None]
    own_base = ref["own"][-1] * (counted[None] & present).double()
    d_bstate = float((out["base_state_log_likelihood"].cpu().double() - own_base.sum(-1)).abs().max())
    print(f"state scan {name} {prec} vs the reference: own {d_own:.2e} unit {d_unit:.2e} base rows {d_base:.2e} base units {d_bunit:.2e} "
          f"delta / rows {d_delta.max():.2e} state_delta / rows {d_state.max():.2e} base state ll {d_bstate:.2e}; rows {sorted(set(rows.tolist()))}")
    assert max(d_own, d_unit, d_base, d_bunit) < TOL and d_delta.max() < TOL and d_state.max() < TOL and d_bstate < TOL * L
    # ---- the cone against the dense route
    dense = m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tk), method="dense")
    assert dense["method"] == "dense" and dense["site_rows"] is None and dense["row_residue"].numel() == n * N
    g_own = np.abs(out["row_token_log_prob"].cpu().numpy() - dense["row_token_log_prob"].view(n, N).cpu().numpy()[vid_r, want_res])[keep].max()
    g_unit = np.abs(out["unit_log_prob"].cpu().numpy() - dense["unit_log_prob"].view(n, L).cpu().numpy()[vid_u, ures])[ok].max()
    g_base = float((out["base_log_probs"] - dense["base_log_probs"])[0][present.reshape(N).to(DEV)].abs().max())
    g_delta = (out["delta_log_likelihood"] - dense["delta_log_likelihood"]).abs().cpu().numpy() / rows
    g_state = (out["state_delta"] - dense["state_delta"]).abs().cpu().numpy() / rows[:, None]
    print(f"state scan {name} {prec} cone vs dense: own {g_own:.2e} unit {g_unit:.2e} base rows {g_base:.2e} delta / rows {g_delta.max():.2e} "
          f"state_delta / rows {g_state.max():.2e}")
    assert max(g_own, g_unit, g_base) < TOL_GPU and g_delta.max() < TOL_GPU and g_state.max() < TOL_GPU
    assert float((dense["base_state_log_likelihood"] - out["base_state_log_likelihood"]).abs().max()) < TOL_GPU * L
    # ---- delta is the fp32 sum of the call's own leader terms
    worst = delta_bound(out, counted, rows)
    print(f"state scan {name} {prec}: delta error / bound of the fp32 recursive sum at most {worst:.3f}")
    # ---- the wild type
    S = cx["S"]
    wild = [v for v, row in enumerate(tk) if all(int(S[r]) == int(t) for r, t in zip(sites[row[0]], row[1:]) if r >= 0)]
    assert len(wild) >= 2
    for v in wild:
        assert abs(float(out["delta_log_likelihood"][v])) < TOL_GPU * rows[v]
        assert float(out["state_delta"][v].abs().max()) < TOL_GPU * rows[v]
    # ---- base units are score_tied's
    tied = m.score_tied(fd)["token_log_probs"][0].cpu()
    assert torch.equal(torch.isfinite(tied), torch.isfinite(btlp))
    d = float((tied - btlp)[same].abs().max())
    print(f"state scan {name} {prec}: base units vs score_tied {d:.2e}")
    assert d < TOL_GPU
    loss = -(ref["units"][-1] * counted.double()).sum() / (counted.double().sum() + 1e-8)
    assert abs(float(out["base_loss"]) - float(loss)) < TOL
    assert torch.allclose(out["loss"], out["base_loss"] - out["delta_log_likelihood"] / (counted.sum() + 1e-8).to(DEV))
    if M == 1:                                                   # one state of weight 1 is the plain scan
        plain = m.score_mutations(to_dev(state_fd(fd_cpu, 0), DEV), sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tk), method="cone")
        assert torch.equal(plain["row_residue"], out["row_residue"])
        d = (plain["delta_log_likelihood"] - out["delta_log_likelihood"]).abs().cpu().numpy() / rows
        print(f"state scan {name} {prec}: one state of weight 1 vs the plain scan, delta / rows {d.max():.2e}")
        assert d.max() < TOL_GPU
        assert float((plain["delta_log_likelihood"][:, None] - out["state_delta"]).abs().max()) < TOL_GPU * rows.max()


BITS = ("delta_log_likelihood", "state_delta", "base_token_log_probs", "base_log_probs", "base_state_log_likelihood")


def assert_same_variant(a, va, b, vb):
    assert torch.equal(a["delta_log_likelihood"][va], b["delta_log_likelihood"][vb]) and torch.equal(a["state_delta"][va], b["state_delta"][vb])
    for off, keys in (("row_offsets", ("row_residue", "row_token_log_prob")), ("unit_offsets", ("unit_residue", "unit_log_prob"))):
        for x, y in zip(per_variant(a, off, keys, va), per_variant(b, off, keys, vb)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_equal_bits_across_calls_chunks_orders_and_company(weights_np, prec):
    """Two calls, three or more chunks, a shuffled variant list and a variant alone give the one-chunk bits."""
    cx, fd_cpu, K, sites, tk, _, m, fd = setup("LltK", weights_np, prec)
    n = len(tk)
    st, tt = torch.from_numpy(sites), torch.from_numpy(tk)
    one = m.score_mutations(fd, sites=st, site_tokens=tt, method="cone")
    two = m.score_mutations(fd, sites=st, site_tokens=tt, method="cone")
    for k in BITS + ("row_token_log_prob", "unit_log_prob", "row_residue", "unit_residue", "row_offsets", "unit_offsets"):
        assert torch.equal(one[k], two[k]), k
    budget = m.score_library_tokens
    try:
        m.score_library_tokens = 150                              # 3 * 150 item rows per call: a site of 59 rows per layer fills a call with three variants
        cut = m.score_mutations(fd, sites=st, site_tokens=tt, method="cone")
    finally:
        m.score_library_tokens = budget
    assert cut["chunks"] >= 3
    for v in range(n):
        assert_same_variant(one, v, cut, v)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    shuffled = m.score_mutations(fd, sites=st, site_tokens=tt[perm], method="cone")
    for q, v in enumerate(perm.tolist()):
        assert_same_variant(one, v, shuffled, q)
    for v in (0, n // 2, n - 1):
        alone = m.score_mutations(fd, sites=st[tk[v, 0]:tk[v, 0] + 1], site_tokens=torch.tensor([[0] + tk[v, 1:].tolist()]), method="cone")
        assert_same_variant(one, v, alone, 0)
        for k in BITS[2:]:
            assert torch.equal(one[k], alone[k]), k


def test_the_unchanged_paths_keep_the_bits_of_a_fresh_model(weights_np):
    """Plain score_mutations and score_tied before and after a state scan on one model give the bits of a fresh model."""
    cx, fd_cpu, K, sites, tk = SR.case("LltK")
    fd, fd0 = to_dev(fd_cpu, DEV), to_dev(state_fd(fd_cpu, 0), DEV)
    lib = torch.from_numpy(SR.sequences(fd_cpu, sites, tk).numpy()[:4]).to(DEV)

    def unchanged(m):
        a = m.score_mutations(fd0, positions=torch.tensor([0, 4, 9]), method="cone")
        b = m.score_tied(fd, lib)
        return [a[k] for k in ("delta_log_likelihood", "row_token_log_prob", "base_log_probs", "row_residue")] + \
               [b[k] for k in ("token_log_probs", "log_likelihood", "member_log_probs", "state_log_likelihood")]
    fresh = unchanged(new_model(weights_np, K, "x3"))
    m = new_model(weights_np, K, "x3")
    before = unchanged(m)
    m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tk), method="cone")
    m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(tk), method="dense")
    after = unchanged(m)
    for x, y, z in zip(fresh, before, after):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_auto_takes_the_route_the_read_back_decides_and_the_empty_scan_has_its_shapes(weights_np):
    cx, fd_cpu, K, sites, tk, (ref, site_rows, u3), m, fd = setup("LltK", weights_np, "x3")
    M, L = fd_cpu["X"].shape[:2]
    st, tt = torch.from_numpy(sites), torch.from_numpy(tk)
    out = m.score_mutations(fd, sites=st, site_tokens=tt)
    assert np.array_equal(out["site_rows"].cpu().numpy(), site_rows)
    assert out["method"] == ("cone" if site_rows[tk[:, 0]].sum() <= 2 * M * L * len(tk) else "dense") == "cone"
    # two first-decoded residues in four states of 20: every layer is three quarters of the flat graph, more than two thirds of the
    # dense price — "auto" reads the sizes back, reports them and takes the dense route
    cx2, fd2_cpu, K2, sites2, tk2, (ref2, rows2, _), m2, fd2 = setup("two_residue_sites", weights_np, "x3")
    M2, L2 = fd2_cpu["X"].shape[:2]
    assert rows2[0].sum() > 2 * M2 * L2 and rows2[1].sum() <= 2 * M2 * L2
    first = torch.from_numpy(tk2[tk2[:, 0] == 0])
    heavy = m2.score_mutations(fd2, sites=torch.from_numpy(sites2), site_tokens=first)
    assert heavy["method"] == "dense" and heavy["site_rows"].cpu().tolist() == rows2.tolist()
    assert float((heavy["delta_log_likelihood"].cpu().double() - ref2["delta"][torch.from_numpy(tk2[:, 0] == 0)]).abs().max()) < TOL * rows2[0, 2]
    light = m2.score_mutations(fd2, sites=torch.from_numpy(sites2), site_tokens=torch.from_numpy(tk2[tk2[:, 0] == 1]))
    assert light["method"] == "cone"
    # the scan form over shared residues, here the two that are absent in a state
    scan =m.score_mutations(fd, positions=torch.tensor([3, 11]), tokens=torch.tensor([0, 5, 7]))
    assert scan["delta"].shape == (2, 3) and scan["positions"].tolist() == [3, 11] and scan["state_delta"].shape == (6, M)
    assert torch.equal(scan["delta"].reshape(-1), scan["delta_log_likelihood"])
    empty = m.score_mutations(fd, positions=torch.zeros(0, dtype=torch.long))
    assert empty["delta_log_likelihood"].shape == (0,) and empty["state_delta"].shape == (0, M) and empty["delta"].shape == (0, 0)
    assert empty["row_offsets"].tolist() == [0] and empty["unit_offsets"].tolist() == [0] and empty["chunks"] == 0
    assert empty["row_residue"].dtype == torch.int32 and empty["unit_residue"].dtype == torch.int32 and empty["unit_log_prob"].numel() == 0
    assert empty["base_log_probs"].shape == (1, M * L, 33) and empty["base_token_log_probs"].shape == (L,)
    assert empty["base_state_log_likelihood"].shape == (M,) and empty["method"] == "dense"
    assert float((empty["base_log_probs"] - out["base_log_probs"]).abs().max()) < TOL_GPU
