"""GPU tests of base-paired design — ProteinMPNN.sample with feature_dict["paired_residues"] / "symmetry_token_maps": the partner of a
residue receives the Watson-Crick complement — against the CPU oracle (paired_ref), across the sampler's forms and the routes of the
plan (namp_pairs_plan + namp_pairs_work_lists on the device, the host route), with fixed strands, states and symmetry groups beside the
pairs, and through the CLI's --paired_strands."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import metrics, spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import paired_ref
import tied_states_ref
from paired_ref import make_case, oracle_paired, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def make_model(weights_np, k, dev, n_dec=3, shared=False):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, num_decoder_layers=n_dec, atom_dict=spec.atom_dict(),
                    restype_to_int=spec.restype_to_int(shared), polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def maxdiff(a, b):
    return float((torch.as_tensor(a).cpu().float() - torch.as_tensor(b).cpu().float()).abs().max())


def check_complement(S, fd_cpu, groups, maps, rti):
    """Every mapped group holds ONE group token: member j's token is P_j[a]; on the paired positions the canonical-pair accuracy is 1."""
    S = S.cpu()
    for g, gm in zip(groups, maps):
        a = torch.tensor(gm[0])[S[:, g[0]]]                                  # (P^-1 = P)
        for j, P_j in zip(g, gm):
            assert torch.equal(S[:, j], torch.tensor(P_j)[a]), (g, j)
    pairs = fd_cpu.get("paired_residues") or []
    if pairs:
        L = S.shape[1]
        idx, msk = torch.zeros(S.shape, dtype=torch.int64), torch.zeros(S.shape, dtype=torch.int64)
        for i, j in pairs:
            idx[:, i], idx[:, j], msk[:, i], msk[:, j] = j, i, 1, 1
        acc = metrics.compute_canonical_base_pair_accuracy(torch.nn.functional.one_hot(S, 33).float(), msk, idx,
                                                           spec.na_canonical_base_pair_ints(rti))
        assert int(acc.sum()) == int(msk.sum()) == 2 * len(pairs) * S.shape[0] and L > 0


def check_against_oracle(m, weights_np, cx, fd_cpu, K, out, shared=False):
    """The complement holds; fixed residues keep S and have zero sampling_probs; no special token; the oracle teacher-forced with the
    sampled S agrees within 1e-3 on log_probs and on sampling_probs (both members of a pair: the second row is the first, permuted);
    every draw is the inverse CDF of the ORACLE's distribution at the call's uniform — a draw may differ only where u lies within 1e-5
    of a boundary of that CDF, at most once per case, and the case's seeds keep every u at least 1e-4 away from the boundaries, so the
    reference alone uses none of that allowance."""
    rti = spec.restype_to_int(shared)
    special = paired_ref.special_tokens(rti)
    L, bs = fd_cpu["S"].shape[1], fd_cpu["batch_size"]
    S, P, U, order, LP = (out[k].cpu() for k in ("S", "sampling_probs", "uniform", "decoding_order", "log_probs"))
    assert S.shape == (bs, L) and P.shape == (bs, L, 33) and LP.shape == (bs, L, 33) and U.shape == (bs, L) and order.shape == (bs, L)
    assert torch.isfinite(LP).all() and m.sample_walk_status() == 0
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    assert torch.equal(S[:, ~cm], torch.from_numpy(cx["S"].astype(np.int64))[~cm].expand(bs, -1))
    for tok in special:
        assert not (S[:, cm] == tok).any()
    assert (LP[:, ~cm] == 0).all() and (P[:, ~cm] == 0).all()
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lp_ref, p_ref, order_ref, (groups, weights, maps), _ = oracle_paired(w, fd_cpu, K, S, rti, special)
    check_complement(S, fd_cpu, groups, maps, rti)
    assert torch.equal(order_ref, order)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(LP[:, valid], lp_ref[:, valid]), maxdiff(P[:, valid], p_ref[:, valid])
    # the draws: per group, in the group's alphabet, from the oracle's distribution
    rank = torch.empty(L, dtype=torch.int64); rank[order[0]] = torch.arange(L)
    in_group = {i: (g, gm) for g, gm in zip(groups, maps) for i in g}
    margin, off = 1.0, 0
    for i in range(L):
        g, gm = in_group.get(i, ([i], [list(range(33))]))
        if i != g[-1] or not all(bool(cm[j]) for j in g):
            continue                                                          # (a fixed member decides the group's token, not the draw)
        t = int(rank[i])                                                      # the closing visit reads the uniform
        Pc = torch.tensor(gm[-1])
        for b in range(bs):
            cdf = torch.cumsum(p_ref[b, i][Pc].double(), 0)                   # p[a] = probs_c[P_c[a]]
            u = float(U[b, t])
            pos = p_ref[b, i][Pc] > 0
            a = int((pos & (cdf > u)).nonzero()[0]) if (pos & (cdf > u)).any() else int(pos.nonzero()[-1])
            dist = float((cdf[pos] - u).abs().min())
            margin = min(margin, dist)
            if int(Pc[a]) != int(S[b, i]):
                off += 1
                assert dist < 1e-5, (b, i, dist)
    print(f"paired L={L} K={K} bs={bs} groups={len(groups)}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; "
          f"min |cdf - u| = {margin:.3e}, draws off the oracle's: {off}; levels {int(out['levels'])}, work items {out['work_items']}")
    assert margin >= 1e-4, f"seed precondition: a uniform lies {margin:.2e} from a boundary of the oracle's CDF — choose another seed"
    assert off <= 1
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)
    return groups, maps


CASES = [(60, 24, 2, 0.5, 0.0, 8, False, True), (60, 24, 2, 0.5, 0.0, 8, True, True), (97, 32, 1, 1.0, 0.03, 10, False, False),
         (40, 48, 3, 0.5, 0.0, 6, False, False)]


@pytest.mark.parametrize("L,K,bs,T,mf,n_pairs,shared,cross", CASES)
def test_paired_free_running(weights_np, L, K, bs, T, mf, n_pairs, shared, cross):
    """Free-running paired sampling (device plan) against the oracle; the (60, 24) case holds a DNA-RNA pair and runs under both
    token variants.  sum_j |w_j| / T <= 4 (what keeps the sampler's 1e-3 bar valid for a group's sum)."""
    dev = torch.device("cuda:0")
    assert 2.0 / T <= 4.0
    cx, fd_cpu, pairs = make_case(L, bs, T, n_pairs, seed=3100 + L, masked_frac=mf, shared=shared, want_cross=cross)
    if cross:
        assert cx["dna_mask"][pairs[0][0]] != cx["dna_mask"][pairs[0][1]]
    m = make_model(weights_np, K, dev, shared=shared)
    torch.manual_seed(5)
    out = m.sample(to_dev(fd_cpu, dev))
    assert out["work_items"] == bs * (L - n_pairs)
    check_against_oracle(m, weights_np, cx, fd_cpu, K, out, shared)


def test_paired_routes_are_bit_identical(weights_np):
    """The sequential walk, per-level launches, the persistent walk with split groups on and off (host route) and the device plan give
    bit-identical S, sampling_probs and log_probs under the same uniforms; at least one pair's members are not graph neighbours (the
    split route decodes them as separate work items and draws deferred); the device plan's arrays equal the host route's."""
    dev = torch.device("cuda:0")
    L, K, bs, T, n_pairs = 60, 24, 2, 0.5, 8
    cx, fd_cpu, pairs = make_case(L, bs, T, n_pairs, seed=3100 + L, want_cross=True)
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    E_idx = cpu_ref.encode(w, fd_cpu, K)[2][0]
    apart = [(i, j) for i, j in pairs if j not in E_idx[i].tolist() and i not in E_idx[j].tolist()]
    assert apart
    fd = to_dev(fd_cpu, dev)
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(3)).to(dev)
    outs, plans = {}, {}
    routes = {"sequential": (False, True, True, False), "per_level": (True, False, True, False), "host_split": (True, True, True, False),
              "host_whole": (True, True, False, False), "device": (True, True, True, True)}
    for name, (par, walk, split, plan) in routes.items():
        m.sample_level_parallel, m.sample_split_groups, m.sample_pairs_device_plan = par, split, plan
        plans[name] = {}
        outs[name] = m._sample(fd, walk, uniform=u, plan_out=plans[name])
        if par and walk:
            assert m.sample_walk_status() == 0
    ref = outs["sequential"]
    assert torch.isfinite(ref["log_probs"]).all()
    for name, o in outs.items():
        assert torch.equal(o["decoding_order"], ref["decoding_order"]), name
        assert torch.equal(o["S"], ref["S"]), name
        assert torch.equal(o["sampling_probs"], ref["sampling_probs"]), name
        assert torch.equal(o["log_probs"], ref["log_probs"]), name
    assert outs["device"]["work_items"] == outs["host_whole"]["work_items"] == bs * (L - n_pairs)
    assert outs["host_split"]["work_items"] == bs * (L - n_pairs + len(apart))
    assert int(outs["device"]["levels"]) == int(outs["host_whole"]["levels"]) == int(outs["per_level"]["levels"])
    for k, v in plans["host_whole"].items():
        assert torch.equal(torch.as_tensor(v).cpu().to(torch.float64), torch.as_tensor(plans["device"][k]).cpu().to(torch.float64)), k
    check_complement(ref["S"], fd_cpu, *paired_ref.groups_of(fd_cpu, spec.restype_to_int())[::2], spec.restype_to_int())


def test_identity_maps_change_nothing(weights_np):
    """symmetry_token_maps that are all the identity give the bits of the same call without maps (the mapped path of the kernel
    against the plain one), on the persistent walk with deferred draws and on the sequential walk."""
    dev = torch.device("cuda:0")
    L, K, bs = 60, 24, 2
    cx, fd_cpu, _ = make_case(L, bs, 0.5, 0, seed=3160)
    ok = [i for i in range(L) if cx["mask"][i] and cx["chain_mask"][i]]
    fd_cpu["symmetry_residues"], fd_cpu["symmetry_weights"] = [ok[0:3], ok[10:12]], [[0.4, 0.3, 0.3], [0.5, 0.5]]
    fd_cpu.pop("paired_residues")
    ident = list(range(33))
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(4)).to(dev)
    for par in (True, False):
        m.sample_level_parallel = par
        plain = m._sample(to_dev(fd_cpu, dev), True, uniform=u)
        mapped = m._sample(to_dev(dict(fd_cpu, symmetry_token_maps=[[ident, None, torch.tensor(ident)], None]), dev), True, uniform=u)
        for k in ("S", "sampling_probs", "log_probs", "decoding_order"):
            assert torch.equal(plain[k], mapped[k]), (par, k)


def test_fixed_strand_forces_the_complement(weights_np):
    """chain_mask 0 on one strand (listed SECOND in every pair): every partner holds the complement of S_true in all streams, the fixed
    residues keep S_true and have zero sampling_probs."""
    dev = torch.device("cuda:0")
    L, K, bs, T = 60, 24, 3, 0.5
    cx, fd_cpu, pairs = make_case(L, bs, T, 8, seed=3100 + L, fixed_every=0)
    rti = spec.restype_to_int()
    for i, j in pairs:
        cx["chain_mask"][j] = 0
    fd_cpu["chain_mask"] = torch.from_numpy(cx["chain_mask"])[None]
    m = make_model(weights_np, K, dev)
    torch.manual_seed(8)
    out = m.sample(to_dev(fd_cpu, dev))
    S, P = out["S"].cpu(), out["sampling_probs"].cpu()
    S_true = torch.from_numpy(cx["S"].astype(np.int64))
    for i, j in pairs:
        kind = "same" if cx["dna_mask"][i] == cx["dna_mask"][j] else "cross"
        comp = spec.token_map(rti, kind)[int(S_true[j])]
        assert (S[:, j] == S_true[j]).all() and (S[:, i] == comp).all() and comp != int(S_true[j])
        assert (P[:, j] == 0).all() and float(P[:, i].sum(-1).min()) > 0.999
    check_against_oracle(m, weights_np, cx, fd_cpu, K, out)


def test_paired_exact_fp32(weights_np):
    dev = torch.device("cuda:0")
    L, K, bs, T = 60, 24, 2, 0.5
    cx, fd_cpu, _ = make_case(L, bs, T, 8, seed=3100 + L, want_cross=True)
    m = make_model(weights_np, K, dev)
    m.message_precision = "fp32"
    torch.manual_seed(5)
    check_against_oracle(m, weights_np, cx, fd_cpu, K, m.sample(to_dev(fd_cpu, dev)))


def test_paired_with_four_decoder_layers():
    dev = torch.device("cuda:0")
    L, K, bs, T = 60, 24, 2, 0.5
    w4 = synth.make_weights(0, 3, 4)
    cx, fd_cpu, _ = make_case(L, bs, T, 8, seed=3100 + L, want_cross=True)
    m = make_model(w4, K, dev, n_dec=4)
    torch.manual_seed(5)
    check_against_oracle(m, w4, cx, fd_cpu, K, m.sample(to_dev(fd_cpu, dev)))


def test_pairs_beside_symmetry_residues(weights_np):
    """symmetry_residues beside the pairs: a pair whose member sits in a symmetry group joins it (weights multiplied, the far side
    through the pair's map); the host route."""
    dev = torch.device("cuda:0")
    L, K, bs, T = 60, 24, 2, 1.0
    cx, fd_cpu, pairs = make_case(L, bs, T, 4, seed=3100 + L, fixed_every=0)
    used = {r for p in pairs for r in p}
    i0, j0 = pairs[0]
    free = [i for i in range(L) if i not in used and cx["dna_mask"][i] == cx["dna_mask"][i0] and cx["rna_mask"][i] == cx["rna_mask"][i0]]
    free += [i for i in range(L) if i not in used and i not in free]
    fd_cpu["symmetry_residues"], fd_cpu["symmetry_weights"] = [[i0, free[0]], [free[5], free[9], free[20]]], [[0.5, 0.5], [0.4, 0.3, 0.3]]
    fd_cpu["paired_weights"] = (1.0, 1.0)                                     # sum |w| of the joined group: 0.5 + 0.5 + 1 = 2 <= 4 T
    m = make_model(weights_np, K, dev)
    torch.manual_seed(6)
    out = m.sample(to_dev(fd_cpu, dev))
    groups, maps = check_against_oracle(m, weights_np, cx, fd_cpu, K, out)
    assert [i0, free[0], j0] in groups
    S = out["S"].cpu()
    assert torch.equal(S[:, i0], S[:, free[0]])


def test_pairs_beside_states(weights_np):
    """state_weights (M = 2, L = 40) beside the pairs: one sequence over the states whose paired positions are complementary; the
    recombined per-state oracle agrees within 1e-3."""
    dev = torch.device("cuda:0")
    L, K, M, bs, T = 40, 48, 2, 2, 1.0
    sw = (0.6, 0.4)
    cx, fd1, pairs = make_case(L, bs, T, 6, seed=3100 + L)
    rti = spec.restype_to_int()
    fd_cpu = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, M, seed=L + 7 * M), sw, bs, T, fd1["randn"].numpy(),
                                      bias=fd1["bias"])
    fd_cpu["paired_residues"] = pairs
    m = make_model(weights_np, K, dev)
    torch.manual_seed(7)
    out = m.sample(to_dev(fd_cpu, dev))
    S, P, LP = out["S"].cpu(), out["sampling_probs"].cpu(), out["log_probs"].cpu()
    assert LP.shape == (bs, M, L, 33) and m.sample_walk_status() == 0
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lps, lps_g = [], []
    for mi in range(M):
        fdm = dict(tied_states_ref.state_fd(fd_cpu, mi), paired_residues=pairs)
        lp_m, _, _, (groups, weights, maps), lp_g = oracle_paired(w, fdm, K, S, rti)
        lps.append(lp_m); lps_g.append(lp_g)                                 # (lp_g keeps the rows of fixed pair members)
    check_complement(S, fd_cpu, groups, maps, rti)
    lp_ref = torch.stack(lps, 1)
    p_ref = paired_ref.paired_probs(torch.stack(lps_g, 1), fd1, groups, weights, maps, state_weights=sw)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(LP[:, :, valid], lp_ref[:, :, valid]), maxdiff(P[:, valid], p_ref[:, valid])
    print(f"pairs beside states: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}")
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)


def test_pair_bias_with_maps_is_refused(weights_np):
    dev = torch.device("cuda:0")
    cx, fd_cpu, _ = make_case(40, 1, 0.5, 2, seed=3140)
    m = make_model(weights_np, 24, dev)
    fd = to_dev(fd_cpu, dev)
    fd["pair_bias"] = torch.zeros(1, 40, 33, 40, 33, device=dev)
    with pytest.raises(ValueError, match="pair_bias is not supported together with paired_residues"):
        m.sample(fd)


@pytest.mark.parametrize("L,K,bs,n_pairs", [(150, 32, 3, 20), (33, 48, 1, 16), (70, 24, 2, 0), (300, 48, 2, 1)])
def test_pairs_plan_equals_the_host_route(L, K, bs, n_pairs):
    """namp_pairs_plan + namp_sample_levels_dep + namp_pairs_work_lists against the host route's building blocks (symmetry_visits,
    level_work_lists without split groups) on random neighbour lists, array for array: visits, rank, group_first / group_last, work,
    work_n, level_off, n_levels.  One pair holds the first and the last residue of the order, listed last-first (the member the order
    reaches first is the second listed one); about half of the other pairs are listed that way too."""
    from na_mpnn_amd import hip
    from na_mpnn_amd.model import level_work_lists, symmetry_visits
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(L + n_pairs)
    Kk = min(K, L)
    E = np.stack([rng.permutation(L)[:Kk] for _ in range(L)]).astype(np.int32)
    order0 = rng.permutation(L).astype(np.int32)
    rank0 = np.empty(L, np.int32); rank0[order0] = np.arange(L, dtype=np.int32)
    pairs = [(int(order0[-1]), int(order0[0]))] if n_pairs else []
    rest = [int(v) for v in rng.permutation(order0[1:-1])]
    while len(pairs) < n_pairs:
        pairs.append((rest.pop(), rest.pop()))
    partner, first = np.full(L, -1, np.int32), np.zeros(L, np.int32)
    for i, j in pairs:
        partner[i], partner[j], first[i] = j, i, 1
    if n_pairs > 1:
        assert any(rank0[i] > rank0[j] for i, j in pairs[1:]) and any(rank0[i] < rank0[j] for i, j in pairs[1:])
    t = lambda a: torch.from_numpy(a).to(dev)
    E_d, o_d, r_d, p_d, f_d = t(E), t(order0), t(rank0), t(partner), t(first)
    i32e = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    order, rank, gf, gl, level = (i32e(bs, L) for _ in range(5))
    work, work_n, level_off, n_levels = i32e(bs * L, 2), i32e(bs * L), i32e(L + 2), i32e(1)
    Lb, st = hip.lib(), hip.current_stream()
    hip.check(Lb.namp_pairs_plan(p_d.data_ptr(), f_d.data_ptr(), o_d.data_ptr(), r_d.data_ptr(), order.data_ptr(), rank.data_ptr(),
                                 gf.data_ptr(), gl.data_ptr(), bs, L, st), "pairs_plan")
    hip.check(Lb.namp_sample_levels_dep(E_d.data_ptr(), order.data_ptr(), rank.data_ptr(), None, 0, gf.data_ptr(), gl.data_ptr(),
                                        level.data_ptr(), bs, 1, L, Kk, st), "sample_levels")
    hip.check(Lb.namp_pairs_work_lists(level.data_ptr(), gf.data_ptr(), work.data_ptr(), work_n.data_ptr(), level_off.data_ptr(),
                                       n_levels.data_ptr(), bs, L, st), "pairs_work_lists")
    visits, gf_h, gl_h, _ = symmetry_visits([list(p) for p in pairs], [[1.0, 1.0]] * len(pairs), order0.tolist(), L)
    order_h = torch.tensor(visits, dtype=torch.int32, device=dev).repeat(bs, 1)
    gf_t = torch.tensor(gf_h, dtype=torch.int32, device=dev).repeat(bs, 1).contiguous()
    gl_t = torch.tensor(gl_h, dtype=torch.int32, device=dev).repeat(bs, 1).contiguous()
    rank_h = ProteinMPNN.ranks_of(order_h.long()).to(torch.int32).contiguous()
    assert torch.equal(order, order_h) and torch.equal(rank, rank_h) and torch.equal(gf, gf_t) and torch.equal(gl, gl_t)
    lvl_h = torch.empty(bs, L, dtype=torch.int32, device=dev)
    hip.check(Lb.namp_sample_levels_dep(E_d.data_ptr(), order_h.data_ptr(), rank_h.data_ptr(), None, 0, gf_t.data_ptr(), gl_t.data_ptr(),
                                        lvl_h.data_ptr(), bs, 1, L, Kk, st), "sample_levels")
    sel, flat, wn_h, close_h, _ = level_work_lists(lvl_h, gf_t, gl_t, order_h[0], E_d.long(), split=False)
    n = bs * (L - n_pairs)
    assert close_h is None and sel.numel() == n
    assert torch.equal(work[:n], torch.stack((sel // L, sel % L), 1).to(torch.int32)) and torch.equal(work_n[:n], wn_h.to(torch.int32))
    assert (work[n:] == -7).all() and (work_n[n:] == -7).all()                 # nothing written past the items
    hist = torch.zeros(L + 1, dtype=torch.int64, device=dev).scatter_add_(0, flat, torch.ones_like(flat))
    assert torch.equal(level_off, torch.cat((hist.new_zeros(1), hist.cumsum(0))).to(torch.int32))
    assert int(n_levels) == int((hist > 0).sum())


def test_cli_paired_strands(tmp_path):
    """--paired_strands on a synthetic two-strand DNA file: in every sample the two chains' FASTA sequences are reverse complements;
    with --fixed_residues covering chain A, chain B is the exact complement of the input's chain A."""
    from na_mpnn_amd import cli, pdbio
    n = 12
    cx = synth.make_complex(seed=77, n=2 * n, n_chains=1, frac_protein=0.0, frac_dna=1.0)
    chains = ["A"] * n + ["B"] * n
    R_idx = list(range(1, n + 1)) * 2
    path = os.path.join(str(tmp_path), "duplex.pdb")
    pdbio.write_pdb(path, cx["X"], cx["X_m"], [spec.RESTYPES[t] for t in cx["S"]], chains, R_idx)
    comp = {"a": "t", "t": "a", "c": "g", "g": "c"}
    # (synthetic weights know no chemistry: the amino-acid letters are omitted, as the RNA letters are under the shared tokens)
    common = ["--pdb_path", path, "--random_init_seed", "0", "--seed", "11", "--batch_size", "3", "--temperature", "0.5", "--output_pdbs", "0",
              "--paired_strands", "A:B", "--omit_AA", "ARNDCQEGHILKMFPSTWYVX"]

    def seqs(folder):
        lines = open(os.path.join(folder, "seqs", "duplex.fa")).read().splitlines()
        assert len(lines) == 2 * (1 + 3)
        return [ln.split("/") for ln in lines[1::2]]

    out = os.path.join(str(tmp_path), "out")
    cli.main(common + ["--out_folder", out])
    native, *samples = seqs(out)
    for a, b in samples:
        assert len(a) == len(b) == n and set(a) <= set("acgt") and b == "".join(comp[c] for c in reversed(a))
    assert len({a for a, _ in samples} | {native[0]}) > 1                     # (designed, not copied)
    out_f = os.path.join(str(tmp_path), "out_fixed")
    cli.main(common + ["--out_folder", out_f, "--fixed_residues", " ".join(f"A{r}" for r in range(1, n + 1))])
    native, *samples = seqs(out_f)
    for a, b in samples:
        assert a == native[0] and b == "".join(comp[c] for c in reversed(native[0]))
