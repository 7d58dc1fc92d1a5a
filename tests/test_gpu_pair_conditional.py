"""GPU tests of the pair conditionals — ProteinMPNN.conditional_probs with feature_dict["paired_residues"]: the cone
kernels with pairs (namp_loo_pairs + namp_decoder_loo) against the CPU oracle's pair stream, against the sampler route at a size the
oracle cannot reach, their invariants, the memory contract of a call with pairs attached, and the command line."""
import functools
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import paired_ref
import real_structures as rs
from loo_numpy import near_tie_rows
from pair_loo_numpy import pair_loo_grids, pair_tables
from pair_loo_ref import neighbour_kinds, oracle_pair_conditional

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MAX_LEFT_OUT = 0.05          # near-tie rows (oracle top-two gap < 2e-3) whose arg-max is not compared: at most 5 % of a case's rows


def make_model(weights_np, k, dev, n_dec=3, shared=False):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, num_decoder_layers=n_dec, atom_dict=spec.atom_dict(),
                    restype_to_int=spec.restype_to_int(shared), polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def to_dev(fd, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def case_inputs(name):
    """name -> (k_neighbors, CPU feature_dict with paired_residues, shared tokens).
    l48_k16: pairs (43, 37), (19, 40), (44, 28), (42, 38), (21, 29) — two mutual neighbours, two that are not neighbours, one where only
    j is a neighbour of i; l64_k24_cross: a DNA:RNA pair, three masked residues, one mutual-neighbour pair; 1am9_crop_k32: the E-H
    duplex of 1AM9 with its protein (118 residues), 17 pairs listed, 16 tied (one has a masked member), every tied pair a mutual graph
    neighbour.  Rows the oracle leaves out of the arg-max comparison (mask == 1, top-two gap < 2e-3), counted on the CPU: 0 / 0 / 0."""
    if name == "l48_k16":
        _, fd, _ = paired_ref.make_case(L=48, bs=1, T=1.0, n_pairs=5, seed=11, fixed_every=0)
        return 16, fd, False
    if name == "l64_k24_cross":
        _, fd, _ = paired_ref.make_case(L=64, bs=1, T=1.0, n_pairs=6, seed=23, want_cross=True, masked_frac=0.04, fixed_every=0)
        return 24, fd, False
    rows = rs.rows_of_chains("1am9", rs.CROP_CHAINS).tolist()
    pairs = [(rows.index(i), rows.index(j)) for i, j in rs.pairs_1am9() if i in rows and j in rows]
    return 32, rs.fd_cpu(rs.variant("1am9_crop"), paired_residues=pairs), True


CASES = ("l48_k16", "l64_k24_cross", "1am9_crop_k32")


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle's rows, computed once and shared: (k, fd, rows with pairs, leave-one-out rows, base order, E_idx, tied specs)."""
    k, fd, shared = case_inputs(name)
    w = cpu_ref.to_torch(synth.make_weights(0))
    out, loo, order, E_idx, specs = oracle_pair_conditional(w, fd, k, spec.restype_to_int(shared))
    return k, fd, shared, out, loo, order, E_idx, specs


def check_argmax(got, ref, mask):
    compared, left_out = near_tie_rows(ref, mask)
    assert left_out <= MAX_LEFT_OUT * mask.numel(), (left_out, mask.numel())
    assert torch.equal(got.argmax(-1)[compared], ref.argmax(-1)[compared])
    return left_out


def check_pair_rows(out, specs):
    """The two rows of a pair are exact permutations of each other through the maps; `pairs` / `pair_log_probs` name them."""
    lp = out["log_probs"][0].cpu()
    assert out["pairs"].dtype == torch.int64 and out["pairs"].cpu().tolist() == [[s[0], s[1]] for s in specs]
    assert torch.equal(out["pair_log_probs"].cpu(), lp[[s[0] for s in specs]])
    for i, j, _, _, Pi, Pj in specs:
        assert torch.equal(lp[i][torch.tensor(Pi)], lp[j][torch.tensor(Pj)]), (i, j)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", CASES)
def test_pair_conditionals_match_the_oracle(weights_np, name, prec):
    """Parity of the cone with pairs with the oracle's pair stream (hidden token) from coordinates: max |dlogp| < 1e-3 on EVERY row,
    arg-max identical on every unmasked row whose oracle top-two gap is at least 2e-3 (no row left out in any case); the cases hold
    pairs where i is a neighbour of j, so a build that does not hide i's token fails (2.8e-3 to 5.6e-3 on those rows).
    Discrimination: every paired row differs from the same build's unpaired call by more than 1e-2 (3.0 or more on the oracle).
    Counts: cone_items equals the numpy restatement of the grids on the call's own E_idx and rank.
    Measured max |dlogp| (MI355X), x3 / fp32: 9.1e-6 / 4.8e-6 (l48_k16), 2.2e-5 / 3.3e-6 (l64_k24_cross), 3.1e-5 / 4.8e-6 (1am9_crop_k32);
    near-tie rows left out: 0 / 0 / 0; the paired rows differ from the unpaired call's by at least 3.19 / 2.99 / 3.59."""
    dev = torch.device("cuda:0")
    k, fd_cpu, shared, ref, ref_loo, order, E_idx, specs = oracle_case(name)
    m = make_model(weights_np, k, dev, shared=shared)
    m.message_precision = prec
    fd = to_dev(fd_cpu, dev)
    out = m.conditional_probs(fd, method="cone")
    got = out["log_probs"].cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(out["decoding_order"].cpu(), order[0]) and torch.equal(out["S"].cpu(), fd_cpu["S"])
    paired_rows = [r for s in specs for r in s[:2]]
    d = float((got - ref).abs().max())
    dp = float((got - ref)[0, paired_rows].abs().max())
    print(f"pair conditional parity {name} {prec}: max|dlogp| = {d:.3e} (paired rows {dp:.3e}), near-tie rows left out "
          f"{near_tie_rows(ref, fd_cpu['mask'])[1]}, tied {len(specs)} of {len(fd_cpu['paired_residues'])} pairs, "
          f"(i in N(j), j in N(i)): {neighbour_kinds(E_idx[0].numpy(), [s[:2] for s in specs])}")
    assert d < 1e-3, d
    check_argmax(got, ref, fd_cpu["mask"])
    check_pair_rows(out, specs)
    assert float((got.exp().sum(-1) - 1).abs().max()) < 1e-5
    # discrimination, and the unpaired rows of the same build
    plain = m.conditional_probs({k_: v for k_, v in fd.items() if k_ != "paired_residues"}, method="cone")
    assert "pairs" not in plain
    moved = (got - plain["log_probs"].cpu())[0].abs().amax(-1)
    print(f"   paired rows differ from the unpaired call by at least {float(moved[paired_rows].min()):.3f}")
    assert float(moved[paired_rows].min()) > 1e-2
    rest = [r for r in range(got.shape[1]) if r not in paired_rows]
    assert torch.equal(got[0, rest], plain["log_probs"].cpu()[0, rest])          # every unpaired row: bit-identical
    # counts
    E_dev = m.featurize(fd)[2][0].cpu().numpy()
    rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])[1][0].cpu().numpy()
    mask = fd_cpu["mask"][0].numpy()
    partner, lead = pair_tables(len(mask), fd_cpu["paired_residues"], mask)
    act1, act2 = pair_loo_grids(E_dev, rank, mask, partner, lead)
    assert out["cone_items"].cpu().tolist() == [int(act1.sum()), int(act2.sum())]
    assert out["cone_items"].cpu().tolist() != plain["cone_items"].cpu().tolist()


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_cone_equals_the_sampler_route(weights_np, prec):
    """The cone with pairs against the slow route — the L streams for the unpaired rows, one teacher-forced design call of the sampler
    per pair — at L = 300, K = 48 with 20 pairs and weights (1.0, 0.5): two implementations that share no decoder kernel on the paired
    rows; max |dlogp| < 2e-4 there and on every other row, arg-max identical outside near ties, counts as the numpy restatement.
    Measured max |dlogp| (MI355X): x3 2.8e-5 (paired rows 2.4e-5), fp32 2.1e-6 (1.9e-6)."""
    dev = torch.device("cuda:0")
    _, fd_cpu, pairs = paired_ref.make_case(L=300, bs=1, T=1.0, n_pairs=20, seed=31, masked_frac=0.02, fixed_every=0)
    fd_cpu["paired_weights"] = (1.0, 0.5)
    fd = to_dev(fd_cpu, dev)
    m = make_model(weights_np, 48, dev)
    m.message_precision = prec
    cone = m.conditional_probs(fd)
    slow = m.conditional_probs(fd, method="dense")
    assert "cone_items" in cone and "cone_items" not in slow
    assert cone["pairs"].cpu().tolist() == [list(p) for p in pairs] == slow["pairs"].cpu().tolist()
    a, b = cone["log_probs"].cpu(), slow["log_probs"].cpu()
    paired_rows = [r for p in pairs for r in p]
    d, dp = float((a - b).abs().max()), float((a - b)[0, paired_rows].abs().max())
    print(f"cone vs sampler route {prec}: max|dlogp| = {d:.3e} (paired rows {dp:.3e})")
    assert dp < 2e-4 and d < 2e-4, (dp, d)
    check_argmax(a, b, fd_cpu["mask"])
    assert torch.equal(slow["pair_log_probs"].cpu(), b[0, [p[0] for p in pairs]])
    plain = m.conditional_probs({k_: v for k_, v in fd.items() if k_ not in ("paired_residues", "paired_weights")})["log_probs"].cpu()
    assert float((a - plain)[0, paired_rows].abs().amax(-1).min()) > 1e-2
    E_dev = m.featurize(fd)[2][0].cpu().numpy()
    rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])[1][0].cpu().numpy()
    mask = fd_cpu["mask"][0].numpy()
    act1, act2 = pair_loo_grids(E_dev, rank, mask, *pair_tables(300, pairs, mask))
    assert cone["cone_items"].cpu().tolist() == [int(act1.sum()), int(act2.sum())]


def test_four_layers_take_the_sampler_route(weights_np):
    """One 4-layer model at (120, 24): "auto" takes the sampler route (the cone kernels walk three layers), "cone" is refused."""
    dev = torch.device("cuda:0")
    _, fd_cpu, pairs = paired_ref.make_case(L=120, bs=1, T=1.0, n_pairs=3, seed=41, fixed_every=0)
    fd = to_dev(fd_cpu, dev)
    m = make_model(synth.make_weights(0, 3, 4), 24, dev, n_dec=4)
    with pytest.raises(NotImplementedError):
        m.conditional_probs(fd, method="cone")
    out = m.conditional_probs(fd)
    assert "cone_items" not in out and out["pairs"].cpu().tolist() == [list(p) for p in pairs]
    lp = out["log_probs"][0].cpu()
    assert float((lp.exp().sum(-1) - 1).abs().max()) < 1e-5
    plain = m.conditional_probs({k_: v for k_, v in fd.items() if k_ != "paired_residues"})["log_probs"][0].cpu()
    paired_rows = [r for p in pairs for r in p]
    assert float((lp - plain)[paired_rows].abs().amax(-1).min()) > 1e-2
    rest = [r for r in range(120) if r not in paired_rows]
    assert torch.equal(lp[rest], plain[rest])


def test_pair_conditional_invariants(weights_np):
    """Two calls are bit-identical; an empty pair list is the call without pairs, bit for bit; a pair with a masked member gives both
    members their unpaired rows and is absent from `pairs`."""
    dev = torch.device("cuda:0")
    k, fd_cpu, shared, *_ = oracle_case("l48_k16")
    m = make_model(weights_np, k, dev)
    fd = to_dev(fd_cpu, dev)
    a, b = m.conditional_probs(fd), m.conditional_probs(fd)
    assert torch.equal(a["log_probs"], b["log_probs"]) and torch.equal(a["cone_items"], b["cone_items"])
    base = {k_: v for k_, v in fd.items() if k_ != "paired_residues"}
    plain = m.conditional_probs(base)
    empty = m.conditional_probs(dict(base, paired_residues=[]))
    assert torch.equal(empty["log_probs"], plain["log_probs"]) and "pairs" not in empty
    # mask the second member of the first pair: that pair is dropped, the others stay
    pairs = fd_cpu["paired_residues"]
    fd_m = dict(fd_cpu, mask=fd_cpu["mask"].clone())
    fd_m["mask"][0, pairs[0][1]] = 0
    fd_m = to_dev(fd_m, dev)
    got = m.conditional_probs(fd_m)
    plain_m = m.conditional_probs({k_: v for k_, v in fd_m.items() if k_ != "paired_residues"})
    assert got["pairs"].cpu().tolist() == [list(p) for p in pairs[1:]]
    for r in pairs[0]:
        assert torch.equal(got["log_probs"][0, r], plain_m["log_probs"][0, r])
    for p in pairs[1:]:
        assert float((got["log_probs"][0, list(p)] - plain_m["log_probs"][0, list(p)]).abs().amax(-1).min()) > 1e-2


def test_pair_conditional_arguments(weights_np):
    dev = torch.device("cuda:0")
    k, fd_cpu, *_ = oracle_case("l48_k16")
    m = make_model(weights_np, k, dev)
    fd = to_dev(fd_cpu, dev)
    with pytest.raises(NotImplementedError, match="pair classes"):
        m.conditional_probs(dict(fd, paired_wobble=True))
    with pytest.raises(NotImplementedError):
        m.conditional_probs(dict(fd, symmetry_residues=[[1, 2]], symmetry_weights=[[1.0, 1.0]]))
    with pytest.raises(NotImplementedError):
        m.conditional_probs(dict(fd, state_weights=[0.5, 0.5]))
    fd2 = {k_: (torch.cat((v, v)) if torch.is_tensor(v) else v) for k_, v in fd.items()}
    with pytest.raises(ValueError, match="one input complex"):
        m.conditional_probs(fd2)


# ---- memory contract of a call with pairs attached ---------------------------------------------------------------------------
def section_of(N, pairs, weights, maps, n_maps, second=None):
    """The input section of include/namp.h for one complex: partner, first, map_idx, weight bits, maps[n_maps][64] as int32 words.
    second: the map index of every pair's second member (default: map 1 where there is one)."""
    partner, first, midx, w = [-1] * N, [0] * N, [0] * N, [1.0] * N
    for n, ((i, j), (wi, wj)) in enumerate(zip(pairs, weights)):
        partner[i], partner[j], first[i], midx[i], midx[j], w[i], w[j] = j, i, 1, 0, (1 % n_maps if second is None else second[n]), wi, wj
    return torch.cat((torch.tensor(partner + first + midx, dtype=torch.int32), torch.tensor(w).view(torch.int32),
                      torch.tensor(maps, dtype=torch.int32).reshape(-1)))


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_memory_contract_with_pairs_attached(weights_np, shape, prec):
    """namp_decoder_loo with pairs attached, under guarded buffers as the contract table's row runs it without: the smallest shape of
    that row (one residue: the tables hold no pair) and the smallest at which a pair exists.  ws is sized by
    namp_loo_pairs_workspace_bytes and pre-filled by the arena; the test writes the input section and finds it unchanged afterwards.
    A second call with a corrupt partner table (out of range, self, not mutual) returns NAMP_OK and the rows of the unpaired call.
    A pair is a group of two, tied where exactly one member carries `first`: a section whose first pair has the flag on neither
    member, and one with it on both, each return NAMP_OK and give the rows and counts of the call that ties only the second pair."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t = mc.graph_case(B, N, K)
    K = t["K"]
    rti = spec.restype_to_int()
    maps = [list(range(64)), spec.token_map(rti, "same") + list(range(33, 64))]
    mask = t["mask"][0].tolist()
    free = [r for r in range(N) if mask[r]]
    pairs = [(free[1], free[6]), (free[9], free[2])] if N >= 17 else []
    good = section_of(N, pairs, [(1.0, 0.5)] * len(pairs), maps, 2)
    bad = good.clone()
    if pairs:
        bad[pairs[0][0]] = N + 5                              # out of range (its partner is no longer named back either)
        bad[pairs[1][0]] = pairs[1][0]                        # itself
        bad[free[12]] = free[3]                               # not mutual
    off = env.L.namp_loo_pairs_offset(B, N, K, 3)

    def run(section):
        ar = Arena(env.dev)
        hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
        S, msk, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
        lp, counts = ar.out("log_probs", mc.f32, (B, N, mc.V33)), ar.out("counts", mc.i32, (2,))
        nbytes = env.L.namp_loo_pairs_workspace_bytes(B, N, K, 3, 2) if section is not None else env.L.namp_loo_workspace_bytes(B, N, K, 3)
        ws = ar.ws("ws", nbytes)
        sec_dev = section.to(env.dev) if section is not None else None

        def call():
            if section is not None:
                ws.t[off:off + 4 * section.numel()].view(torch.int32).copy_(sec_dev)
                assert env.L.namp_loo_pairs(2) == 0
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

    lp_pairs, c_pairs = run(good)
    lp_bad, c_bad = run(bad)
    lp_none, c_none = run(None)
    assert torch.equal(lp_bad, lp_none) and torch.equal(c_bad, c_none)
    if pairs:
        rows = [r for p in pairs for r in p]
        rest = [r for r in range(N) if r not in rows]
        assert torch.equal(lp_pairs[0, rest], lp_none[0, rest])
        assert float((lp_pairs - lp_none)[0, rows].abs().amax(-1).min()) > 1e-2
        P = torch.tensor(maps[1][:33])
        for i, j in pairs:
            assert torch.equal(lp_pairs[0, i][P], lp_pairs[0, j]) and not torch.equal(lp_pairs[0, i], lp_pairs[0, j])
        lp_other, c_other = run(section_of(N, pairs[1:], [(1.0, 0.5)], maps, 2))
        assert not torch.equal(lp_other, lp_pairs) and not torch.equal(lp_other, lp_none)
        neither, both = good.clone(), good.clone()
        neither[N + pairs[0][0]] = 0
        both[N + pairs[0][1]] = 1
        assert [int(neither[N + r]) for r in pairs[0]] == [0, 0] and [int(both[N + r]) for r in pairs[0]] == [1, 1]
        for section in (neither, both):
            lp_flags, c_flags = run(section)
            assert torch.equal(lp_flags, lp_other) and torch.equal(c_flags, c_other)
    else:
        assert torch.equal(lp_pairs, lp_none) and torch.equal(c_pairs, c_none)


def test_cli_conditional_probs_with_pairs(tmp_path, golden_dir):
    """--conditional_probs_only 1 with pair flags on the tests/golden/cli input: the keys of the file, the shape of `pairs`, and the
    permutation property of the two rows of every pair.  The input's chains have 27 / 10 / 11 residues, so --paired_strands (equal
    lengths) cannot name two of them: the three DNA residues that end chain B are paired with chain C's through --paired_residues,
    which shares parse_pairs and everything behind it with --paired_strands."""
    from na_mpnn_amd import cli, pdbio
    gd = os.path.join(golden_dir, "cli")
    out = os.path.join(str(tmp_path), "out")
    P = pdbio.parse_pdb(os.path.join(gd, "input.pdb"))
    enc = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    b = [i for i, c in enumerate(P["chain_letters"]) if c == "B"][-3:]
    c = [i for i, c in enumerate(P["chain_letters"]) if c == "C"][:3]
    want = list(zip(b, reversed(c)))
    cli.main(["--mode", "design", "--pdb_path", os.path.join(gd, "input.pdb"), "--out_folder", out, "--random_init_seed", "0",
              "--seed", "7", "--conditional_probs_only", "1", "--paired_residues", ",".join(f"{enc[i]}:{enc[j]}" for i, j in want)])
    z = np.load(os.path.join(out, "conditional_probs", "input.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["log_probs", "S", "mask", "chain_mask", "chain_labels", "decoding_order", "encoded_residues", "pairs"])
    L = z["S"].shape[0]
    assert z["log_probs"].shape == (L, 33) and z["pairs"].shape == (3, 2) and z["pairs"].tolist() == [list(p) for p in want]
    assert np.allclose(np.exp(z["log_probs"].astype(np.float64)).sum(-1), 1.0, atol=1e-5)
    Pm = np.array(spec.token_map(spec.restype_to_int(True), "same"))          # (DNA with DNA)
    for i, j in z["pairs"]:
        assert np.array_equal(z["log_probs"][j], z["log_probs"][i][Pm]), (i, j)
        assert not np.array_equal(z["log_probs"][j], z["log_probs"][i])
    with pytest.raises(ValueError, match="paired_wobble"):
        cli.main(["--mode", "design", "--pdb_path", os.path.join(gd, "input.pdb"), "--out_folder", out, "--random_init_seed", "0",
                  "--conditional_probs_only", "1", "--paired_wobble", "1", "--paired_residues", f"{enc[want[0][0]]}:{enc[want[0][1]]}"])
