"""GPU tests of the group conditionals — ProteinMPNN.conditional_probs(tied=True): the cone kernels with groups
(namp_loo_groups + namp_decoder_loo) against the CPU oracle's group stream, against per-state calls, against the slow route and
against the pair path, their invariants, malformed tables under guarded buffers, the command line and a call history."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec
from na_mpnn_amd.model import ProteinMPNN
import call_history as ch
import group_loo_ref as G
import paired_ref
import tied_states_ref as ts
from loo_numpy import near_tie_rows

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MAX_LEFT_OUT = 0.05          # near-tie rows (oracle top-two gap < 2e-3) whose arg-max is not compared: at most 5 % of a case's rows
DEV = "cuda:0"


def make_model(weights_np, k, prec="x3"):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    m = m.to(DEV).eval()
    m.message_precision = prec
    return m


def to_dev(fd):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


UNTIED = ("paired_residues", "paired_weights", "symmetry_residues", "symmetry_weights", "symmetry_token_maps")


def untied_call(m, fd, **kw):
    """The same build's leave-one-out rows of the call's residues: tied=False without the tie keys — state 0's with states."""
    one = fd if fd.get("state_weights") is None else ts.state_fd(fd, 0)
    return m.conditional_probs({k: v for k, v in one.items() if k not in UNTIED}, **kw)


def device_graph(m, fd):
    """The call's own flattened graph from the device: E_idx [N, K], rank [N], mask [N] as numpy."""
    M = 1 if fd.get("state_weights") is None else fd["X"].shape[0]
    one = dict(fd)
    if M > 1:
        for k in ts.SHARED:
            one[k] = fd[k].expand(M, -1)
    E = m.featurize(one)[2].cpu().numpy()
    L = E.shape[1]
    E = np.concatenate([E[s] + s * L for s in range(M)])
    rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"][:1])[1][0].cpu().numpy()
    return E, G.flat_rank(rank, M), np.tile(fd["mask"][0].cpu().numpy(), M)


def check_argmax(got, ref, mask):
    compared, left_out = near_tie_rows(ref, mask)
    assert left_out <= MAX_LEFT_OUT * mask.numel(), (left_out, mask.numel())
    assert torch.equal(got.argmax(-1)[compared], ref.argmax(-1)[compared])
    return left_out


def check_group_rows(out, specs, L):
    """`groups` / `group_log_probs` name the tied groups; the rows of a group's members are exact permutations of each other."""
    lp = out["log_probs"][0].cpu()
    width = max(len(s[0]) for s in specs)
    assert out["groups"].dtype == torch.int64
    assert out["groups"].cpu().tolist() == [s[0] + [-1] * (width - len(s[0])) for s in specs]
    assert torch.equal(out["group_log_probs"].cpu(), lp[[s[0][0] for s in specs]])
    for g, _, maps in specs:
        first = lp[g[0]][torch.tensor(maps[0])]
        for r, P in zip(g, maps):
            if r < L:
                assert torch.equal(lp[r][torch.tensor(P)], first), (g, r)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", G.CASES)
def test_group_conditionals_match_the_oracle(weights_np, name, prec):
    """Parity of the cone with groups with the oracle's group stream (every member's token hidden) from coordinates, on the seven cases of
    group_loo_ref.case_inputs (the issue's six, and the trimer with explicit symmetry_token_maps): max |dlogp| < 1e-3 on EVERY row, arg-max identical on every unmasked row whose oracle top-two gap is
    at least 2e-3 (the oracle leaves no row out in any case: 0 in all seven, counted in test_group_conditional_host.py), every
    row sums to 1 within 1e-5, every grouped row differs from the same build's tied=False call by more than 1e-2, every other row is
    that call's bit for bit, and cone_items equals the numpy restatement of the grids on the call's own graph.  trimer_l24,
    dimer_l48 and states_pairs_m2_l32 hold earlier-listed members that are neighbours of later ones: a build that does not hide their
    tokens is off by 3.1e-3 / 8.4e-3 / 4.1e-3 there (asserted on the oracle in test_group_conditional_host.py).
    Measured max |dlogp| (MI355X), x3 / fp32: 9.1e-6 / 3.6e-6 (trimer_l24), 1.6e-5 / 5.5e-6 (mixed_l12), 1.2e-5 / 4.3e-6 (dimer_l48),
    6.2e-6 / 1.9e-6 (states_m3_l20), 8.6e-6 / 2.9e-6 (states_pairs_m2_l32), 8.6e-6 / 2.4e-6 (cap_m8_l16), 9.1e-6 / 3.6e-6
    (trimer_maps_l24); the grouped rows differ from the tied=False call's by at least 1.56 / 3.05 / 2.77 / 0.056 / 0.075 / 0.061 (1.64 with maps)."""
    fd_cpu, ref, ref_loo, order0, E_ref, specs = G.oracle_case(name)
    L = fd_cpu["S"].shape[1]
    m = make_model(weights_np, G.K_CASE, prec)
    fd = to_dev(fd_cpu)
    out = m.conditional_probs(fd, method="cone", tied=True)
    got = out["log_probs"].cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(out["S"].cpu(), fd_cpu["S"])
    rows = sorted({r for s in specs for r in s[0] if r < L})
    d = float((got - ref).abs().max())
    print(f"group conditional parity {name} {prec}: max|dlogp| = {d:.3e} (grouped rows {float((got - ref)[0, rows].abs().max()):.3e}), "
          f"near-tie rows left out {near_tie_rows(ref, fd_cpu['mask'])[1]}, {len(specs)} groups of sizes {sorted({len(s[0]) for s in specs})}")
    assert d < 1e-3, d
    check_argmax(got, ref, fd_cpu["mask"])
    check_group_rows(out, specs, L)
    assert float((got.exp().sum(-1) - 1).abs().max()) < 1e-5
    plain = untied_call(m, fd, method="cone")
    assert "groups" not in plain
    moved = (got - plain["log_probs"].cpu())[0].abs().amax(-1)
    print(f"   grouped rows differ from the tied=False call by at least {float(moved[rows].min()):.3f}")
    assert float(moved[rows].min()) > 1e-2
    rest = [r for r in range(L) if r not in rows]
    assert torch.equal(got[0, rest], plain["log_probs"].cpu()[0, rest])
    E_dev, rank, mask = device_graph(m, fd)
    sid, _ = G.group_tables(len(mask), [s[0] for s in specs], mask)
    act1, act2 = G.group_loo_grids(E_dev, rank, mask, sid)
    assert out["cone_items"].cpu().tolist() == [int(act1.sum()), int(act2.sum())]


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_unpaired_states_equal_the_combine_of_per_state_calls(weights_np, prec):
    """states_m3_l20: the members of a group sit in different blocks of the flattened graph and are never neighbours, so every row
    is the combine of the three states' own conditional_probs() rows, within 2e-4 (measured on an MI355X: x3 7.5e-7, fp32 8.6e-7)."""
    fd_cpu = G.oracle_case("states_m3_l20")[0]
    m = make_model(weights_np, G.K_CASE, prec)
    fd = to_dev(fd_cpu)
    got = m.conditional_probs(fd, tied=True)["log_probs"][0].cpu().double()
    w = fd_cpu["state_weights"]
    per = [m.conditional_probs({k: v for k, v in ts.state_fd(fd, s).items() if k not in UNTIED})["log_probs"][0].cpu().double() for s in range(3)]
    want = torch.log_softmax(sum(ws * lp for ws, lp in zip(w, per)), -1)
    valid = fd_cpu["mask"][0].bool()
    d = float((got - want)[valid].abs().max())
    print(f"states vs per-state calls {prec}: max|dlogp| = {d:.3e}")
    assert d < 2e-4, d
    assert torch.equal(got[~valid], per[0][~valid])


@pytest.mark.parametrize("name,prec", [("trimer_l24", "x3"), ("trimer_l24", "fp32"), ("mixed_l12", "x3"), ("states_pairs_m2_l32", "x3"),
                                       ("states_pairs_m2_l32", "fp32"), ("cap_m8_l16", "x3"), ("trimer_maps_l24", "x3"),
                                       ("trimer_maps_l24", "fp32")])
def test_cone_equals_the_slow_route(weights_np, name, prec):
    """The cone with groups against the slow route — the L streams for the other rows, ONE teacher-forced design call of the sampler per
    group (the group decoded last) — two implementations that share no decoder kernel on the grouped rows: max |dlogp| < 2e-4, the bound
    of test_gpu_pair_conditional's test_cone_equals_the_sampler_route.  Measured (MI355X): trimer_l24 x3 3.6e-5, fp32 1.9e-6; mixed_l12
    x3 4.6e-5; states_pairs_m2_l32 x3 3.6e-5, fp32 2.9e-6; cap_m8_l16 x3 2.1e-5; trimer_maps_l24 x3 3.7e-5, fp32 2.4e-6."""
    fd_cpu, _, _, _, _, specs = G.oracle_case(name)
    m = make_model(weights_np, G.K_CASE, prec)
    fd = to_dev(fd_cpu)
    cone, slow = m.conditional_probs(fd, tied=True), m.conditional_probs(fd, method="dense", tied=True)
    assert "cone_items" in cone and "cone_items" not in slow
    assert torch.equal(cone["groups"], slow["groups"])
    a, b = cone["log_probs"].cpu(), slow["log_probs"].cpu()
    d = float((a - b).abs().max())
    print(f"cone vs slow route {name} {prec}: max|dlogp| = {d:.3e} over {len(specs)} groups")
    assert d < 2e-4, d
    check_argmax(a, b, fd_cpu["mask"])
    assert torch.equal(slow["group_log_probs"].cpu(), b[0, [s[0][0] for s in specs]])


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_a_group_of_two_is_the_pair_path_bit_for_bit(weights_np, prec):
    """The pairs of test_gpu_pair_conditional's l48_k16 case with weights (1.0, 0.5): through namp_loo_groups every row and both counts
    are the bits of namp_loo_pairs.  The two entry points attach the same tables: what differs is the host route, encode() with
    tied=False and the featurise-as-states path with tied=True, and the test pins the two against each other."""
    _, fd_cpu, pairs = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    fd_cpu["paired_weights"] = (1.0, 0.5)
    m = make_model(weights_np, 16, prec)
    fd = to_dev(fd_cpu)
    as_pairs, as_groups = m.conditional_probs(fd, method="cone"), m.conditional_probs(fd, method="cone", tied=True)
    assert torch.equal(as_groups["log_probs"], as_pairs["log_probs"]) and torch.equal(as_groups["cone_items"], as_pairs["cone_items"])
    assert torch.equal(as_groups["groups"], as_pairs["pairs"]) and torch.equal(as_groups["group_log_probs"], as_pairs["pair_log_probs"])
    assert "pairs" not in as_groups and "groups" not in as_pairs


def test_group_conditional_invariants(weights_np):
    """Two identical calls are bit-identical; tied=False does not read symmetry_residues; tied=True without anything to tie is the
    plain call; the refusals."""
    fd_cpu = G.oracle_case("trimer_l24")[0]
    m = make_model(weights_np, G.K_CASE)
    fd = to_dev(fd_cpu)
    a, b = m.conditional_probs(fd, tied=True), m.conditional_probs(fd, tied=True)
    assert torch.equal(a["log_probs"], b["log_probs"]) and torch.equal(a["cone_items"], b["cone_items"])
    plain = untied_call(m, fd)
    for other in (m.conditional_probs(fd), m.conditional_probs(fd, tied=False), untied_call(m, fd, tied=True),
                  m.conditional_probs(dict(fd, symmetry_residues=[[]], symmetry_weights=[[]]), tied=True)):
        assert sorted(other) == sorted(plain)
        assert torch.equal(other["log_probs"], plain["log_probs"]) and torch.equal(other["cone_items"], plain["cone_items"])
    assert not torch.equal(a["log_probs"], plain["log_probs"])
    with pytest.raises(ValueError, match="at most 16"):
        m.conditional_probs(dict(fd, symmetry_residues=[list(range(17))], symmetry_weights=[[1.0] * 17]), tied=True)
    with pytest.raises(ValueError, match="disjoint"):
        m.conditional_probs(dict(fd, symmetry_residues=[[0, 1], [1, 2]], symmetry_weights=[[1.0, 1.0]] * 2), tied=True)
    _, fd_p, _ = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    fd_p = to_dev(fd_p)
    with pytest.raises(NotImplementedError, match="pair classes"):
        m.conditional_probs(dict(fd_p, paired_wobble=True), tied=True)
    with pytest.raises(NotImplementedError):
        m.conditional_probs(dict(fd_p, symmetry_residues=[[1, 2]], symmetry_weights=[[1.0, 1.0]]))
    got = m.conditional_probs(dict(fd_p, symmetry_residues=[[1, 2]], symmetry_weights=[[1.0, 1.0]]), tied=True)
    assert got["groups"].shape == (6, 2)


# ---- malformed tables under guarded buffers ---------------------------------------------------------------------------------------
def section_of(N, groups, maps, n_maps, weights=(1.0, 0.5, 0.25, 0.125)):
    """The input section of include/namp.h for one complex: next, first, map_idx, weight bits, maps[n_maps][64] as int32 words."""
    nxt, first, midx, w = [-1] * N, [0] * N, [0] * N, [1.0] * N
    for g in groups:
        for t, r in enumerate(g):
            nxt[r], midx[r], w[r] = g[(t + 1) % len(g)], t % n_maps, weights[t % len(weights)]
        first[g[0]] = 1
    return torch.cat((torch.tensor(nxt + first + midx, dtype=torch.int32), torch.tensor(w).view(torch.int32),
                      torch.tensor(maps, dtype=torch.int32).reshape(-1)))


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_malformed_group_tables_give_leave_one_out_rows(weights_np, shape, prec):
    """namp_decoder_loo with groups attached, under the guarded buffers of the contract table's row: a valid table (a group of three
    and a group of two) moves exactly its rows; tables with a successor out of range, a self-loop, two `first` flags and a tail
    that leads into a cycle give the rows of the call that ties only what stays valid (the cycle behind the tail; nothing else), and
    a cycle through all 17 residues — longer than the cap — the rows of the call without an attachment.  The input section is found
    unchanged and nothing is written outside the declared buffers.  These are valid inputs with a defined result."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t = mc.graph_case(B, N, K)
    K = t["K"]
    maps = [list(range(64)), spec.token_map(spec.restype_to_int(), "same") + list(range(33, 64))]
    free = [r for r in range(N) if t["mask"][0].tolist()[r]]
    big = N >= 17
    groups = [[free[1], free[6], free[4]], [free[9], free[2]]] if big else []
    good = section_of(N, groups, maps, 2)
    bad = good.clone()
    expect = None
    if big:
        bad[free[6]] = N + 5                                  # a successor out of range: the whole group of three is untied
        bad[N + free[2]] = 1                                  # two `first` flags in the group of two
        bad[free[11]] = free[11]                              # a self-loop
        c1, c2, tail = free[3], free[7], free[8]
        for sec in (bad,):
            sec[c1], sec[c2], sec[tail], sec[N + c1] = c2, c1, c1, 1      # a tail that leads into the (valid) cycle c1 <-> c2
        expect = section_of(N, [[c1, c2]], maps, 2)
        for r, wr in ((c1, bad[3 * N + c1]), (c2, bad[3 * N + c2])):
            expect[3 * N + r] = wr
        expect[2 * N + c1], expect[2 * N + c2] = bad[2 * N + c1], bad[2 * N + c2]
    else:
        bad[0] = 0                                            # N = 1: a self-loop with a `first` flag
        bad[N] = 1
    long_cycle = section_of(N, [list(range(N))], maps, 2) if big else section_of(N, [], maps, 2)
    if not big:
        long_cycle[0] = 5                                     # N = 1: a successor out of range
    off = env.L.namp_loo_groups_offset(B, N, K, 3)
    assert off == env.L.namp_loo_pairs_offset(B, N, K, 3)

    def run(section, mask=None):
        ar = Arena(env.dev)
        hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
        S, msk, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"] if mask is None else mask), ar.inp("rank", t["rank"])
        lp, counts = ar.out("log_probs", mc.f32, (B, N, mc.V33)), ar.out("counts", mc.i32, (2,))
        nbytes = env.L.namp_loo_groups_workspace_bytes(B, N, K, 3, 2) if section is not None else env.L.namp_loo_workspace_bytes(B, N, K, 3)
        ws = ar.ws("ws", nbytes)
        sec_dev = section.to(env.dev) if section is not None else None

        def call():
            if section is not None:
                ws.t[off:off + 4 * section.numel()].view(torch.int32).copy_(sec_dev)
                assert env.L.namp_loo_groups(2) == 0
            rc = env.L.namp_decoder_loo(env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, msk.ptr, rank.ptr, lp.ptr, counts.ptr, ws.ptr,
                                        ws.nbytes, B, N, K, env.s())
            if section is not None:
                torch.cuda.synchronize()
                assert torch.equal(ws.t[off:off + 4 * section.numel()].view(torch.int32), sec_dev), "the call wrote into its input section"
            return rc
        outs, reproducible = run_contract(lambda a: mc.with_precision(env, prec, call)(), ar)
        assert reproducible
        assert torch.equal(env.packed.flat, env.snapshot)
        return outs["log_probs"].cpu(), outs["counts"].cpu()

    lp_good, c_good = run(good)
    lp_bad, c_bad = run(bad)
    lp_none, c_none = run(None)
    ones = torch.ones_like(t["mask"])
    lp_long, c_long = run(long_cycle, ones)
    lp_ones, c_ones = run(None, ones)
    assert torch.equal(lp_long, lp_ones) and torch.equal(c_long, c_ones)
    if big:
        lp_exp, c_exp = run(expect)
        assert torch.equal(lp_bad, lp_exp) and torch.equal(c_bad, c_exp)
        moved = (lp_exp - lp_none)[0].abs().amax(-1)
        assert float(moved[[c1, c2]].min()) > 1e-2 and float(moved[[r for r in range(N) if r not in (c1, c2)]].max()) == 0.0
        rows = [r for g in groups for r in g]
        rest = [r for r in range(N) if r not in rows]
        assert torch.equal(lp_good[0, rest], lp_none[0, rest])
        assert float((lp_good - lp_none)[0, rows].abs().amax(-1).min()) > 1e-2
        P = torch.tensor(maps[1][:33])
        for g in groups:                                      # (members at odd listed positions speak through the Watson-Crick map)
            for tpos, r in enumerate(g):
                assert torch.equal(lp_good[0, r][P] if tpos % 2 else lp_good[0, r], lp_good[0, g[0]]), (g, r)
    else:
        assert torch.equal(lp_good, lp_none) and torch.equal(lp_bad, lp_none) and torch.equal(c_bad, c_none)


def test_cli_conditional_probs_tied(tmp_path, golden_dir):
    """--conditional_probs_only 1 --conditional_tied 1 on the tests/golden/cli input with --symmetry_residues (three residues of
    chain A tied, weights 1 / 0.5 / 0.25) and a base pair: the keys of the file, `groups` / `group_log_probs`, equal rows inside
    the symmetry group; without --conditional_tied the present error stands."""
    from na_mpnn_amd import cli, pdbio
    gd = os.path.join(golden_dir, "cli")
    out = os.path.join(str(tmp_path), "out")
    P = pdbio.parse_pdb(os.path.join(gd, "input.pdb"))
    enc = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    a = [i for i, c in enumerate(P["chain_letters"]) if c == "A"][2:5]
    b = [i for i, c in enumerate(P["chain_letters"]) if c == "B"][-1]
    c = [i for i, c in enumerate(P["chain_letters"]) if c == "C"][0]
    base = ["--mode", "design", "--pdb_path", os.path.join(gd, "input.pdb"), "--out_folder", out, "--random_init_seed", "0", "--seed", "7",
            "--conditional_probs_only", "1", "--symmetry_residues", ",".join(enc[i] for i in a), "--symmetry_weights", "1.0,0.5,0.25"]
    cli.main(base + ["--conditional_tied", "1", "--paired_residues", f"{enc[b]}:{enc[c]}"])
    z = dict(np.load(os.path.join(out, "conditional_probs", "input.npz"), allow_pickle=True))      # (read now: the file is written again below)
    assert sorted(z) == sorted(["log_probs", "S", "mask", "chain_mask", "chain_labels", "decoding_order", "encoded_residues", "groups",
                                      "group_log_probs"])
    L = z["S"].shape[0]
    assert z["log_probs"].shape == (L, 33) and z["groups"].tolist() == [a, [b, c, -1]]
    assert np.array_equal(z["group_log_probs"], z["log_probs"][[a[0], b]])
    assert np.allclose(np.exp(z["log_probs"].astype(np.float64)).sum(-1), 1.0, atol=1e-5)
    assert np.array_equal(z["log_probs"][a[1]], z["log_probs"][a[0]]) and np.array_equal(z["log_probs"][a[2]], z["log_probs"][a[0]])
    Pm = np.array(spec.token_map(spec.restype_to_int(True), "same"))
    assert np.array_equal(z["log_probs"][c], z["log_probs"][b][Pm]) and not np.array_equal(z["log_probs"][c], z["log_probs"][b])
    cli.main(base)                                                           # (tied off: symmetry_residues are not read, as before)
    z0 = dict(np.load(os.path.join(out, "conditional_probs", "input.npz"), allow_pickle=True))
    assert "groups" not in z0 and not np.array_equal(z0["log_probs"][a[1]], z0["log_probs"][a[0]])
    rest = [r for r in range(L) if r not in a + [b, c]]
    assert np.array_equal(z0["log_probs"][rest], z["log_probs"][rest])


def test_cli_conditional_probs_tied_multi_state(tmp_path, golden_dir):
    """--multi_state 1 --conditional_probs_only 1 --conditional_tied 1 on a two-model file made from the tests/golden/cli input
    (weights 0.6 / 0.4): every unmasked residue is the group (i, L + i) in flat indices, `group_log_probs` are the rows of state 0,
    the rows equal the Python call on the parsed states, and they differ from the single-structure profile of model 1.  Without
    --conditional_tied the present error stands; --conditional_tied without --conditional_probs_only is refused."""
    from na_mpnn_amd import cli
    gd = os.path.join(golden_dir, "cli")
    out = os.path.join(str(tmp_path), "out")
    two = os.path.join(str(tmp_path), "two_models.pdb")
    ts.write_multimodel(two, os.path.join(gd, "input.pdb"), 2, seed=5)
    base = ["--mode", "design", "--out_folder", out, "--random_init_seed", "0", "--seed", "7", "--conditional_probs_only", "1"]
    states = ["--pdb_path", two, "--multi_state", "1", "--state_weights", "0.6,0.4"]
    cli.main(base + states + ["--conditional_tied", "1"])
    z = dict(np.load(os.path.join(out, "conditional_probs", "two_models.npz"), allow_pickle=True))
    assert sorted(z) == sorted(["log_probs", "S", "mask", "chain_mask", "chain_labels", "decoding_order", "encoded_residues", "groups",
                                "group_log_probs"])
    L = z["S"].shape[0]
    tied = [i for i in range(L) if z["mask"][i]]
    assert z["log_probs"].shape == (L, 33) and z["groups"].tolist() == [[i, L + i] for i in tied] and len(tied) > L // 2
    assert np.array_equal(z["group_log_probs"], z["log_probs"][tied])
    assert np.allclose(np.exp(z["log_probs"].astype(np.float64)).sum(-1), 1.0, atol=1e-5)
    cli.main(base + ["--pdb_path", os.path.join(gd, "input.pdb")])                     # model 1 alone (the same seed: the same order)
    z1 = dict(np.load(os.path.join(out, "conditional_probs", "input.npz"), allow_pickle=True))
    assert np.array_equal(z1["decoding_order"], z["decoding_order"])
    assert float(np.abs(z1["log_probs"] - z["log_probs"])[tied].max(-1).min()) > 1e-4
    with pytest.raises(ValueError, match="multi_state"):
        cli.main(base + states)
    with pytest.raises(ValueError, match="conditional_probs_only"):
        cli.main(["--mode", "design", "--pdb_path", two, "--out_folder", out, "--random_init_seed", "0", "--conditional_tied", "1"])


def test_call_history_group_pair_plain(weights_np):
    """One long-lived model: a group call, a pair call, a plain call, a states call and the group call again, each bit-identical to a
    fresh model's on cloned inputs (the cached group tables, the cached pair tables and the thread's attachment do not leak); then
    a call with explicit symmetry_token_maps, the SAME resident feature_dict without them, and the maps again: the tables cached for one
    never serve the other."""
    m = ch.make_model(weights_np, G.K_CASE)
    fd_g = to_dev(G.case_inputs("trimer_l24"))
    _, fd_p, _ = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
    fd_p = to_dev(fd_p)
    fd_s = to_dev(G.case_inputs("states_pairs_m2_l32"))
    tied = lambda mo, f: mo.conditional_probs(f, tied=True)
    plain = lambda mo, f: mo.conditional_probs({k: v for k, v in f.items() if k not in UNTIED})
    first = ch.step(m, tied, fd_g, "group call")
    ch.step(m, lambda mo, f: mo.conditional_probs(f), fd_p, "pair call")
    ch.step(m, plain, fd_g, "plain call")
    ch.step(m, tied, fd_s, "states call")
    ch.step(m, tied, fd_p, "pairs as groups")
    again = ch.step(m, tied, fd_g, "group call again")
    ch.assert_same(again, first, "group call, first and last")
    # explicit token maps, then the SAME resident feature_dict without them (the cached tables of the first must not serve the second), and back
    fd_m = to_dev(G.case_inputs("trimer_maps_l24"))
    fd_n = {k: v for k, v in fd_m.items() if k != "symmetry_token_maps"}
    with_maps = ch.step(m, tied, fd_m, "maps")
    without = ch.step(m, tied, fd_n, "the same feature_dict without maps")
    ch.assert_same(without, first, "without maps: the group call")
    assert not torch.equal(with_maps["log_probs"], without["log_probs"])
    ch.assert_same(ch.step(m, tied, fd_m, "maps again"), with_maps, "maps, first and last")
