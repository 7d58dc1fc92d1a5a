"""CPU tests of the group conditionals (ProteinMPNN.conditional_probs(tied=True)): the definition on the CPU oracle
(the group stream with every member's token hidden against the tied branch of the sampler), that hiding an earlier member's token
matters exactly where it is a neighbour of a later one, the premises of the GPU cases (near-tie rows, neighbour kinds, sensitivity
to a forgotten hide), the numpy restatement of the grids against a brute force on the oracle's layer outputs, the library's sizing /
attach entry points, and the argument handling that needs no device."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec, synth
from oracle import cpu_ref
import group_loo_ref as G
import paired_ref
from loo_numpy import loo_grids
from pair_loo_numpy import brute_force_cone, pair_loo_grids, pair_tables

torch.set_grad_enabled(False)
K = G.K_CASE


def weights():
    return cpu_ref.to_torch(synth.make_weights(0))


def test_group_stream_equals_the_tied_branch_decoded_last():
    """The premise: on trimer_l24 the stream's member rows equal cpu_ref.sample_symmetric teacher-forced with the group visited last,
    within 1e-5, the bound of test_pair_conditional_host.py (measured: 1.9e-6 over the seven tied groups)."""
    fd, _, _, order0, _, specs = G.oracle_case("trimer_l24")
    w = weights()
    L = fd["S"].shape[1]
    enc = cpu_ref.encode(w, fd, K)
    groups = [s[0] for s in specs]
    zs = G.group_stream_logits(w, enc, fd["S"], fd["mask"], order0, groups)
    worst = 0.0
    for g, z in zip(groups, zs):
        keep = torch.ones_like(order0, dtype=torch.bool)
        for r in g:
            keep &= order0 != r
        order = torch.cat((order0[keep], order0.new_tensor(g)))
        randn = torch.empty(L); randn[order] = torch.arange(1, L + 1, dtype=torch.float32)
        randn = torch.where(fd["mask"][0] != 0, randn, randn * 1e4)          # (a masked residue's sort key is 1e-4 |randn|: its place again)
        fdo = dict(fd, symmetry_residues=[g], symmetry_weights=[[1.0] * len(g)], randn=randn[None], chain_mask=torch.ones_like(fd["chain_mask"]),
                   bias=torch.zeros(1, L, 33))
        ref = cpu_ref.sample_symmetric(w, fdo, K, S_forced=fd["S"].long())
        assert torch.equal(ref["decoding_order"][0], order)
        worst = max(worst, float((torch.log_softmax(z, -1) - ref["log_probs"][0, g]).abs().max()))
    print(f"group stream vs tied branch: max|dlogp| = {worst:.3e}")
    assert worst < 1e-5, worst


def test_hiding_an_earlier_token_matters_exactly_where_it_is_a_neighbour():
    """trimer_l24, per group and per ordered member pair (t < u): un-hiding m_t's token alone moves row m_u by more than 1e-4 where
    m_t is in N(m_u), by more than 0 where only a member between them passes it on, and by exactly 0 otherwise; row m_t itself and
    the rows of earlier members never move."""
    fd, _, _, order0, E, specs = G.oracle_case("trimer_l24")
    w = weights()
    enc = cpu_ref.encode(w, fd, K)
    groups = [s[0] for s in specs]
    hid = G.group_stream_logits(w, enc, fd["S"], fd["mask"], order0, groups)
    En = E.numpy()
    seen = {True: 0, False: 0}
    for t in range(2):
        vis = G.group_stream_logits(w, enc, fd["S"], fd["mask"], order0, groups, visible=tuple(g[t] for g in groups))
        for g, a, b in zip(groups, hid, vis):
            for u in range(t + 1):
                assert torch.equal(a[u], b[u]), (g, t, u)
            reach = {g[t]}                                                    # members that read m_t's token, directly or through a member
            for u in range(t + 1, len(g)):
                direct, reached = bool((En[g[u]] == g[t]).any()), bool(set(En[g[u]].tolist()) & reach)
                d = float((a[u] - b[u]).abs().max())
                print(f"group {g}: un-hiding member {t} moves row {u} by {d:.3e} (neighbour: {direct}, reached: {reached})")
                assert (d > 1e-4) if direct else (d > 0.0) if reached else (d == 0.0), (g, t, u, d)
                seen[reached] += 1
                if reached:
                    reach.add(g[u])
    assert seen[True] >= 8 and seen[False] >= 2, seen


EXPECTED_KINDS = {      # ordered member pairs (t < u) of the tied groups by (m_t in N(m_u), m_u in N(m_t))
    "trimer_l24": {(True, True): 14, (True, False): 1, (False, True): 3, (False, False): 3},
    "mixed_l12": {(True, True): 7},
    "dimer_l48": {(True, True): 2, (True, False): 1, (False, True): 3, (False, False): 18},
    "states_m3_l20": {(False, False): 60},
    "states_pairs_m2_l32": {(True, True): 7, (True, False): 1, (False, True): 2, (False, False): 46},
    "cap_m8_l16": {(True, True): 8, (False, False): 504},
    "trimer_maps_l24": {(True, True): 14, (True, False): 1, (False, True): 3, (False, False): 3},
}
GROUP_SIZES = {"trimer_l24": [3] * 7, "mixed_l12": [2, 4], "dimer_l48": [2] * 24, "states_m3_l20": [3] * 20,
               "states_pairs_m2_l32": [4] * 6 + [2] * 20, "cap_m8_l16": [16] + [8] * 14, "trimer_maps_l24": [3] * 7}
UNHIDDEN_MOVES = {"trimer_l24": 3.0e-3, "dimer_l48": 8.3e-3, "states_pairs_m2_l32": 4.0e-3}


@pytest.mark.parametrize("name", G.CASES)
def test_the_premises_of_the_gpu_cases(name):
    """Every GPU case on the oracle alone: no unmasked row is a near tie (top-two gap < 2e-3), so the arg-max comparison leaves
    nothing out (0 in all seven cases); the groups have the sizes and the neighbour kinds the case is there for; every grouped row is
    more than 1e-2 from the leave-one-out row (at least 5.6e-2); and on trimer_l24, dimer_l48 and states_pairs_m2_l32 a stream
    that does not hide the members' tokens is more than 1e-3 away on some row (3.1e-3 / 8.4e-3 / 4.1e-3): the condition for
    keeping those cases."""
    fd, ref, loo, order0, E, specs = G.oracle_case(name)
    L = fd["S"].shape[1]
    assert G.left_out(name) == 0
    assert sorted(len(s[0]) for s in specs) == sorted(GROUP_SIZES[name])
    assert max(len(s[0]) for s in specs) <= hip.loo_group_max()
    kinds = [k for s in specs for k in G.neighbour_kinds(E.numpy(), s[0])]
    assert {k: kinds.count(k) for k in set(kinds)} == EXPECTED_KINDS[name]
    rows = sorted({r for s in specs for r in s[0] if r < L})
    assert float((ref - loo)[0, rows].abs().amax(-1).min()) > 1e-2
    assert float((ref.double().exp().sum(-1) - 1).abs().max()) < 1e-5
    if name in UNHIDDEN_MOVES:
        d = float((G.oracle_case_unhidden(name) - ref).abs().max())
        print(f"{name}: a stream that does not hide the tokens is off by {d:.3e}")
        assert d > 1e-3 and d > UNHIDDEN_MOVES[name], d
    if name == "mixed_l12":                                  # the listed group of one is not tied: its row is the leave-one-out row
        assert [4] in fd["symmetry_residues"] and all(4 not in s[0] for s in specs) and torch.equal(ref[0, 4], loo[0, 4])
    if name == "trimer_maps_l24":                            # the maps change the group rows (the second member's logits enter permuted)
        plain = G.oracle_case("trimer_l24")[1]
        assert all(s[2][1] != s[2][0] and s[2][2] == s[2][0] for s in specs)
        assert float((ref - plain)[0, rows].abs().amax(-1).min()) > 1e-2
    if name in ("trimer_l24", "trimer_maps_l24"):
        assert int(fd["mask"][0, 11]) == 0 and all(3 not in s[0] for s in specs)
        assert torch.equal(ref[0, [3, 11, 19]], loo[0, [3, 11, 19]])


@pytest.mark.parametrize("name", ["trimer_l24", "states_pairs_m2_l32"])
def test_group_grids_equal_a_brute_force_on_the_layer_outputs(name):
    """The numpy grids against the oracle's layer outputs (fp64) on the call's flattened graph: per stream — every group, and some
    ungrouped residues — the residues of the active layer-1 slots are exactly those whose layer-1 output differs from the base
    stream's, the residues of the active layer-2 slots exactly the members' neighbours whose layer-2 output differs."""
    fd, _, _, order0, E, specs = G.oracle_case(name)
    w = weights()
    enc, S, mask, _ = G.flat_encoding(w, fd, K)
    w64 = cpu_ref.to_dtype(w, torch.float64)
    enc64 = (enc[0].double(), enc[1].double(), enc[2])
    En = E.numpy()
    N = En.shape[0]
    rank = np.empty(N, np.int64); rank[order0.numpy()] = np.arange(N)
    mk = mask[0].numpy()
    groups = [s[0] for s in specs]
    sid, pos = G.group_tables(N, groups, mk)
    act1, act2 = G.group_loo_grids(En, rank, mk, sid)
    tied = {r for g in groups for r in g}
    streams = [tuple(g) for g in groups][:10] + [(r,) for r in range(N) if r not in tied][:3]
    doubles = 0
    for members in streams:
        s1, s2 = brute_force_cone(w64, enc64, S, mask.double(), order0, members)
        slots1 = [(int(m), int(k)) for m, k in zip(*np.nonzero(act1)) if int(En[m, k]) in members]
        assert {m for m, _ in slots1} == s1, members
        doubles += len(slots1) - len(s1)
        for g in members:
            got = {int(En[g, kq]) for kq in np.nonzero(act2[g])[0]}
            assert got == (s2 & set(En[g].tolist())) - set(members), (members, g)
    assert doubles > 0


def test_group_grids_restate_the_pair_grids_and_the_plain_grids():
    _, fd, pairs = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    E = cpu_ref.encode(weights(), fd, K)[2][0].numpy()
    order0 = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"])[0].numpy()
    rank = np.empty(48, np.int64); rank[order0] = np.arange(48)
    mask = fd["mask"][0].numpy()
    sid, pos = G.group_tables(48, [list(p) for p in pairs], mask)
    a1, a2 = G.group_loo_grids(E, rank, mask, sid)
    b1, b2 = pair_loo_grids(E, rank, mask, *pair_tables(48, pairs, mask))
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    a1, a2 = G.group_loo_grids(E, rank, mask, np.arange(48))
    _, b1, b2 = loo_grids(E, rank, mask)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)


def test_combine_is_a_permutation_and_a_distribution():
    fd = G.case_inputs("states_pairs_m2_l32")
    g = torch.Generator().manual_seed(3)
    for members, ws, maps in G.group_specs(fd, spec.restype_to_int()):
        rows = G.combine([torch.randn(33, generator=g) for _ in members], ws, maps)
        for row, P in zip(rows, maps):
            assert torch.equal(row[torch.tensor(P)], rows[0][torch.tensor(maps[0])])
            assert abs(float(row.exp().sum()) - 1) < 1e-12


def test_group_entry_points_validate_without_a_gpu():
    L = hip.lib()
    import os, re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "namp.h")).read()
    cap = int(re.search(r"#define\s+NAMP_LOO_GROUP_MAX\s+(\d+)", header).group(1))
    assert hip.loo_group_max() == L.namp_loo_group_max() == cap == G.GROUP_MAX       # the header's value, as the library was built with it
    base = L.namp_loo_workspace_bytes(1, 1000, 48, 3)
    need = L.namp_loo_groups_workspace_bytes(1, 1000, 48, 3, 3)
    off = L.namp_loo_groups_offset(1, 1000, 48, 3)
    assert off == base == L.namp_loo_pairs_offset(1, 1000, 48, 3) and off % 256 == 0
    pair_need = L.namp_loo_pairs_workspace_bytes(1, 1000, 48, 3, 3)
    assert pair_need == need                                                                 # a pair is a group of two: one carve
    assert need - base >= 4 * 48000 + 4 * (4 * 1000 + 3 * 64) + 2 * 1000 + 2 * 2 * 1000 * 128 * 4     # ... with one [R] table, one row per residue whatever the group size
    assert need >= off + 4 * (4 * 1000 + 3 * 64) + 2 * 1000 * 128 * 4
    for args in ((1, 100, 24, 4, 2), (0, 100, 24, 3, 2), (1, 100, 24, 3, 0), (1, 100, 24, 3, 65)):
        assert L.namp_loo_groups_workspace_bytes(*args) == 0, args
    assert L.namp_loo_groups_offset(1, 100, 24, 4) == 0
    for bad in (0, 65, -1):
        assert L.namp_loo_groups(bad) == -1 and b"n_maps" in L.namp_last_error()
    # a failed namp_decoder_loo clears the attachment; the later of a pair and a group attachment holds
    null_call = lambda: L.namp_decoder_loo(None, None, None, None, None, None, None, None, None, None, 0, 1, 10, 4, None)
    assert L.namp_loo_groups(3) == 0
    assert null_call() == -1 and b"group tables were attached" in L.namp_last_error()
    assert null_call() == -1 and b"null pointer" in L.namp_last_error() and b"attached" not in L.namp_last_error()
    assert L.namp_loo_groups(3) == 0 and L.namp_loo_pairs(2) == 0
    assert null_call() == -1 and b"pair tables were attached" in L.namp_last_error()
    assert L.namp_loo_pairs(2) == 0 and L.namp_loo_groups(3) == 0
    assert null_call() == -1 and b"group tables were attached" in L.namp_last_error()
    assert L.namp_loo_groups(3) == 0 and L.namp_loo_groups(65) == -1                         # an invalid attach leaves nothing attached
    assert null_call() == -1 and b"attached" not in L.namp_last_error()


def test_tied_arguments_are_handled_before_any_device_work(weights_np):
    """tied=False keeps the refusals of the pair conditionals; tied=True refuses pair classes, a group above the cap, overlapping
    groups and several complexes, and builds the tables of every supported tie — all on the host."""
    from na_mpnn_amd.model import ProteinMPNN
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=K, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    _, fd, pairs = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    sym = dict(symmetry_residues=[[1, 2]], symmetry_weights=[[1.0, 1.0]])
    for kw in ({}, {"tied": False}):
        with pytest.raises(NotImplementedError, match="symmetry_residues"):
            m.conditional_probs(dict(fd, **sym), **kw)
        with pytest.raises(NotImplementedError, match="state_weights"):
            m.conditional_probs(dict(fd, state_weights=[0.5, 0.5]), **kw)
        with pytest.raises(NotImplementedError, match="pair classes"):
            m.conditional_probs(dict(fd, paired_wobble=True), **kw)
    with pytest.raises(NotImplementedError, match="pair classes"):
        m.conditional_probs(dict(fd, paired_wobble=True), tied=True)
    with pytest.raises(ValueError, match="at most 16"):
        m.conditional_probs(dict(fd, symmetry_residues=[list(range(1, 18))], symmetry_weights=[[1.0] * 17]), tied=True)
    with pytest.raises(ValueError, match="disjoint"):
        m.conditional_probs(dict(fd, symmetry_residues=[[1, 2], [2, 3]], symmetry_weights=[[1.0, 1.0]] * 2), tied=True)
    fd2 = {k: (torch.cat((v, v)) if torch.is_tensor(v) and k != "randn" else v) for k, v in fd.items()}
    with pytest.raises(ValueError, match="one input complex"):
        m.conditional_probs(fd2, tied=True)
    with pytest.raises(ValueError, match="method"):
        m.conditional_probs(fd, method="fast", tied=True)
    with pytest.raises(ValueError, match="symmetry_token_maps"):                             # pairs with maps but no groups: as the pair path
        m.conditional_probs(dict(fd, symmetry_token_maps=[[None, None]]), tied=True)
    # a call with maps leaves nothing behind that a call without maps on the same resident feature_dict could pick up
    fdm = G.case_inputs("trimer_maps_l24")
    fdn = {k: v for k, v in fdm.items() if k != "symmetry_token_maps"}
    with_maps = m._conditional_arguments(fdm, 1, 24, None, True)
    without = m._conditional_arguments(fdn, 1, 24, None, True)
    assert with_maps["n_tables"] == 2 and without["n_tables"] == 1 and not torch.equal(with_maps["section"], without["section"])
    assert m._conditional_arguments(fdn, 1, 24, None, True) is without                      # (and the entry without maps is kept)
    assert m._conditional_arguments(fdm, 1, 24, None, True) is not with_maps
    # nine states of a pair are 18 members
    fd9 = G.case_inputs("cap_m8_l16")
    fd9 = dict(fd9, X=torch.cat((fd9["X"], fd9["X"][:1])), X_m=torch.cat((fd9["X_m"], fd9["X_m"][:1])), state_weights=[1 / 9] * 9)
    with pytest.raises(ValueError, match="at most 16"):
        m.conditional_probs(fd9, tied=True)
    # the tables of a supported call: the successor cycles in listed order, one `first` per group, the state-major flat indices
    for name in G.CASES:
        fdc = G.case_inputs(name)
        M = 1 if fdc.get("state_weights") is None else fdc["X"].shape[0]
        L = fdc["S"].shape[1]
        grp = m._conditional_arguments(fdc, 1, L, fdc.get("state_weights"), True)
        specs = G.group_specs(fdc, spec.restype_to_int())
        assert [t[0] for t in grp["tied"]] == [s[0] for s in specs]
        for t, s in zip(grp["tied"], specs):
            assert np.allclose(t[1], s[1]) and t[2] == s[2]
        N = M * L
        sec = grp["section"]
        assert sec.numel() == 4 * N + 64 * grp["n_tables"]
        nxt, first, midx, wts = sec[:N].tolist(), sec[N:2 * N].tolist(), sec[2 * N:3 * N].tolist(), sec[3 * N:4 * N].view(torch.float32).tolist()
        maps = sec[4 * N:].view(-1, 64).tolist()
        for g, gw, gm in specs:
            assert [nxt[r] for r in g] == g[1:] + g[:1] and [first[r] for r in g] == [1] + [0] * (len(g) - 1)
            assert np.allclose([wts[r] for r in g], gw) and [maps[midx[r]][:33] for r in g] == gm
        assert grp["index"].shape == (len(specs), max(len(s[0]) for s in specs))
