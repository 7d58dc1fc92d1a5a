"""GPU tests of the compact pair terms (ProteinMPNN.sample with feature_dict["pair_terms"]): bit identity with the dense pair_bias on
every route of the sampler, the ties the dense key refuses (base pairs, wobble classes, states) against the CPU oracle recombined by
pair_terms_ref, neutral inputs, the property the key is used for (no homopolymer step on any strand), a length the dense tensor cannot
reach, and the CLI."""
import lzma
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import cli, spec, synth
from na_mpnn_amd.model import ProteinMPNN, pair_terms_dense
import pair_terms_ref
import paired_ref
import tied_states_ref
import wobble_ref
from paired_ref import make_case, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
V = 33
ROUTES = {"walk": (True, True), "per_level": (True, False), "sequential": (False, False)}
KEYS = ("S", "sampling_probs", "log_probs")


def make_model(weights_np, k, dev):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def maxdiff(a, b):
    return float((torch.as_tensor(a).cpu().double() - torch.as_tensor(b).cpu().double()).abs().max())


def fd_of(cx, bs, T, seed):
    L = cx["S"].shape[0]
    fd = {k: torch.from_numpy(np.ascontiguousarray(cx[k]))[None] for k in paired_ref.PER_RESIDUE}
    fd.update({"batch_size": bs, "temperature": T, "bias": torch.zeros(1, L, V), "symmetry_residues": [[]], "symmetry_weights": [[]],
               "randn": torch.from_numpy(np.random.default_rng(seed).standard_normal((bs, L)).astype(np.float32))})
    return fd


def run_routes(m, fd, u, split=(True,)):
    """The call on every route of the sampler under the same uniforms -> {route: out}; S, probabilities and log-probs must agree bit for bit."""
    outs = {}
    for name, (par, walk) in ROUTES.items():
        for sp in (split if par and walk else (True,)):
            m.sample_level_parallel, m.sample_split_groups = par, sp
            outs[name + ("" if sp else "_whole")] = m._sample(fd, walk, uniform=u)
            if par and walk:
                assert m.sample_walk_status() == 0
    m.sample_level_parallel, m.sample_split_groups = True, True
    ref = outs["sequential"]
    assert torch.isfinite(ref["log_probs"]).all()
    for name, o in outs.items():
        for k in KEYS:
            assert torch.equal(o[k], ref[k]), (name, k)
    return outs


def asymmetric_terms(n, AA):
    """The asymmetric pattern of test_pair_bias_sampling_by_level_equals_the_sequential_walk: i reads i + 9 through AA (i + 9 does not
    read i) and i + 2 reads (7 i) % n through AA.t(); a residue that would read itself has no such slot."""
    partner, table = torch.full((1, n, 1), -1, dtype=torch.int32), torch.zeros(1, n, 1, dtype=torch.int32)
    for i in range(0, n - 9, 3):
        partner[0, i, 0] = i + 9
        partner[0, i + 2, 0], table[0, i + 2, 0] = (i * 7) % n, 1
    return {"partner": partner, "table": table, "tables": torch.stack((AA, AA.t())).contiguous()}


@pytest.mark.parametrize("kind", ["sequence_neighbours", "asymmetric"])
def test_compact_is_the_dense_route_bit_for_bit(weights_np, kind):
    """n = 80, K = 24, bs = 3, T = 0.7, two fixed residues: the compact key and the dense tensor it stands for give identical bits
    on the persistent walk, per-level launches and the sequential walk."""
    dev = torch.device("cuda:0")
    n, k, bs = 80, 24, 3
    cx = synth.make_complex(seed=812, n=n, n_chains=2)
    cx["chain_mask"][[5, 33]] = 0
    fd = fd_of(cx, bs, 0.7, 12)
    AA = torch.from_numpy(2.0 * np.random.default_rng(13).standard_normal((V, V)).astype(np.float32))
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA) if kind == "sequence_neighbours" else asymmetric_terms(n, AA)
    dense = pair_terms_dense(pt, n)
    if kind == "sequence_neighbours":
        assert torch.equal(dense, cli.make_pair_bias(fd["chain_labels"][0], fd["R_idx"][0], AA))
    m = make_model(weights_np, k, dev)
    u = torch.rand(bs, n, generator=torch.Generator().manual_seed(8)).to(dev)
    fdd = to_dev(fd, dev)
    compact = run_routes(m, dict(fdd, pair_terms=pt), u)
    dense_out = run_routes(m, dict(fdd, pair_bias=dense.to(dev)), u)
    plain = m._sample(fdd, True, uniform=u)
    assert not torch.equal(plain["sampling_probs"], compact["walk"]["sampling_probs"])      # (the key reaches the kernel)
    for route in ROUTES:
        for key in KEYS:
            assert torch.equal(compact[route][key], dense_out[route][key]), (route, key)
    assert int(compact["walk"]["levels"]) == compact["per_level"]["levels"] == dense_out["per_level"]["levels"] < n


def test_compact_is_the_dense_route_with_symmetry_groups(weights_np):
    """The same with symmetry_residues — the mixed groups of test_symmetric_sampling_by_level_equals_the_sequential_walk, "closing" (the
    reference's rule, what the dense tensor means) —, the split of the groups on and off."""
    dev = torch.device("cuda:0")
    n, k, bs = 96, 24, 3
    cx = synth.make_complex(seed=902, n=n, n_chains=2, masked_frac=0.03)
    cx["chain_mask"][[2, 40, 71]] = 0
    fd = fd_of(cx, bs, 0.6, 21)
    fd["randn"] = fd["randn"][:1].repeat(bs, 1)
    fd.update({"symmetry_residues": [[1, 2, 3], [10, 50], [40, 41], [20, 21, 22, 23, 24], [60, 7, 90, 33], [70, 71]],
               "symmetry_weights": [[1., 1., 1.], [0.5, 1.5], [1., 2.], [1., -.5, 1., 1., 1.], [.25, .25, .25, .25], [1., 1.]]})
    AA = torch.from_numpy(2.0 * np.random.default_rng(22).standard_normal((V, V)).astype(np.float32))
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA)
    m = make_model(weights_np, k, dev)
    u = torch.rand(bs, n, generator=torch.Generator().manual_seed(11)).to(dev)
    fdd = to_dev(fd, dev)
    compact = run_routes(m, dict(fdd, pair_terms=pt), u, split=(True, False))
    dense_out = run_routes(m, dict(fdd, pair_bias=pair_terms_dense(pt, n).to(dev)), u, split=(True, False))
    assert compact["walk"]["work_items"] > compact["walk_whole"]["work_items"]               # (some group was split: the deferred close ran)
    for route in compact:
        for key in KEYS:
            assert torch.equal(compact[route][key], dense_out[route][key]), (route, key)


def test_compact_is_the_dense_route_for_two_complexes(weights_np):
    """B = 2 encoded complexes with bs = 2 streams each: a residue's slots are those of its own complex."""
    dev = torch.device("cuda:0")
    n, k, bs = 60, 24, 2
    cxs = [synth.make_complex(seed=s, n=n, n_chains=2) for s in (31, 32)]
    fds = [fd_of(cx, bs, 0.7, 5) for cx in cxs]
    fd = {key: (torch.cat((fds[0][key], fds[1][key])) if torch.is_tensor(v) and key not in ("randn", "bias") else v) for key, v in fds[0].items()}
    fd["randn"] = torch.from_numpy(np.random.default_rng(6).standard_normal((2 * bs, n)).astype(np.float32))
    fd["bias"] = torch.zeros(2, n, V)
    rng = np.random.default_rng(7)
    AA = torch.from_numpy(2.0 * rng.standard_normal((V, V)).astype(np.float32))
    pts = [cli.make_pair_terms(f["chain_labels"][0], f["R_idx"][0], AA) for f in fds]
    pts[1]["partner"][0, ::4, 1] = -1                                                       # (the complexes differ in their slots)
    pt = {"partner": torch.cat([p["partner"] for p in pts]), "table": torch.cat([p["table"] for p in pts]), "tables": pts[0]["tables"]}
    m = make_model(weights_np, k, dev)
    u = torch.rand(2 * bs, n, generator=torch.Generator().manual_seed(9)).to(dev)
    fdd = to_dev(fd, dev)
    compact = run_routes(m, dict(fdd, pair_terms=pt), u)
    dense_out = run_routes(m, dict(fdd, pair_bias=pair_terms_dense(pt, n).to(dev)), u)
    for route in ROUTES:
        for key in KEYS:
            assert torch.equal(compact[route][key], dense_out[route][key]), (route, key)


# ---------------------------------------------------------------------------------------------------------------------------------
# the ties the dense key refuses, against the oracle (teacher-forced with the sampled S); 1e-3 is the project's bar (test_gpu_model.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def strand_terms(cx, seed, members, scale=1.0):
    AA = torch.from_numpy(scale * np.random.default_rng(seed).standard_normal((V, V)).astype(np.float32))
    return pair_terms_ref.neighbour_terms(len(cx["S"]), AA, members, chain_of=cx["chain_labels"].tolist())


@pytest.mark.parametrize("L,K,bs,n_pairs,members", [(60, 24, 2, 8, "closing"), (60, 24, 2, 8, "all"), (40, 48, 3, 6, "all")])
def test_pairs_with_pair_terms_against_the_oracle(weights_np, L, K, bs, n_pairs, members):
    """Base pairs (token maps) with pair terms under both member rules; (40, 48): L < K, with fixed pair members."""
    dev = torch.device("cuda:0")
    T = 0.5
    cx, fd_cpu, pairs = make_case(L, bs, T, n_pairs, seed=3100 + L, want_cross=(L == 60))
    pt = strand_terms(cx, L, members)
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(3)).to(dev)
    out = run_routes(m, to_dev(dict(fd_cpu, pair_terms=pt), dev), u, split=(True, False))["walk"]
    S, P, LP, order = (out[k].cpu() for k in ("S", "sampling_probs", "log_probs", "decoding_order"))
    rti = spec.restype_to_int()
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lp_ref, p0, order_ref, (groups, weights, maps), lp_g = paired_ref.oracle_paired(w, fd_cpu, K, S, rti, paired_ref.special_tokens(rti))
    assert torch.equal(order_ref, order)
    p_ref = pair_terms_ref.paired_probs(lp_g, fd_cpu, pt, S, order, groups, weights, maps)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p, d_0 = maxdiff(LP[:, valid], lp_ref[:, valid]), maxdiff(P[:, valid], p_ref[:, valid]), maxdiff(P[:, valid], p0[:, valid])
    print(f"pairs + pair terms ({members}) L={L} K={K}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; without the terms {d_0:.3e}")
    assert d_lp < 1e-3 and d_p < 1e-3 and d_0 > 1e-2, (d_lp, d_p, d_0)
    if members == "all" and L == 60:                                                      # the rules differ where a first-listed member has neighbours
        p_cl = pair_terms_ref.paired_probs(lp_g, fd_cpu, dict(pt, members="closing"), S, order, groups, weights, maps)
        assert maxdiff(p_cl, p_ref) > 1e-2


def test_wobble_classes_with_pair_terms_against_the_oracle(weights_np):
    """Class tables (G-U wobble) with "all": every member's term through its own class table; L = 40 holds pairs with a fixed member."""
    dev = torch.device("cuda:0")
    L, K, bs, T = 40, 48, 3, 0.5
    cx, fd_cpu, pairs = make_case(L, bs, T, 6, seed=3100 + L)
    cm = cx["mask"] * cx["chain_mask"]
    assert any(not (cm[i] and cm[j]) for i, j in pairs)
    fd_cpu.update(paired_wobble=True, paired_wobble_bias=1.0)
    pt = strand_terms(cx, 41, "all")
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(4)).to(dev)
    out = run_routes(m, to_dev(dict(fd_cpu, pair_terms=pt), dev), u, split=(True, False))["walk"]
    S, P, LP, order = (out[k].cpu() for k in ("S", "sampling_probs", "log_probs", "decoding_order"))
    rti = spec.restype_to_int()
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lp_ref, rows0, _, order_ref, (groups, weights, tables, cb), lp_g = wobble_ref.oracle_wobble(w, fd_cpu, K, S, rti, paired_ref.special_tokens(rti))
    assert torch.equal(order_ref, order)
    rows = pair_terms_ref.class_probs(lp_g, fd_cpu, pt, S, order, groups, weights, tables, cb)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p, d_0 = maxdiff(LP[:, valid], lp_ref[:, valid]), maxdiff(P[:, valid], rows[:, valid]), maxdiff(P[:, valid], rows0[:, valid])
    print(f"wobble + pair terms (all) L={L} K={K}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; without the terms {d_0:.3e}")
    assert d_lp < 1e-3 and d_p < 1e-3 and d_0 > 1e-2, (d_lp, d_p, d_0)


@pytest.mark.parametrize("with_pairs", [False, True])
def test_states_with_pair_terms_against_the_oracle(weights_np, with_pairs):
    """state_weights with M = 3, alone and joined with base pairs ("all"): the terms sit on state 0's copies — a residue counts once."""
    dev = torch.device("cuda:0")
    L, K, M, bs, T = 40, 24, 3, 2, 1.0
    sw = (0.5, 0.3, 0.2)
    cx, fd1, pairs = make_case(L, bs, T, 6, seed=3100 + L)
    fd_cpu = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, M, seed=L + 7 * M), sw, bs, T, fd1["randn"].numpy(), bias=fd1["bias"])
    pt = strand_terms(cx, 43, "all" if with_pairs else "closing")
    if with_pairs:
        fd_cpu["paired_residues"] = pairs
    else:
        fd1 = {k: v for k, v in fd1.items() if k != "paired_residues"}
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(5)).to(dev)
    outs = {}
    for name, (par, walk) in ROUTES.items():
        if not par:
            continue                                                                          # (states decode by level only)
        outs[name] = m._sample(to_dev(dict(fd_cpu, pair_terms=pt), dev), walk, uniform=u)
    for k in KEYS:
        assert torch.equal(outs["walk"][k], outs["per_level"][k]), k
    out = outs["walk"]
    S, P, LP, order = (out[k].cpu() for k in ("S", "sampling_probs", "log_probs", "decoding_order"))
    assert LP.shape == (bs, M, L, V) and m.sample_walk_status() == 0 and torch.isfinite(LP).all()
    rti = spec.restype_to_int()
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    valid = torch.from_numpy(cx["mask"].astype(bool))
    if with_pairs:
        lps, lps_g = [], []
        for mi in range(M):
            fdm = dict(tied_states_ref.state_fd(fd_cpu, mi), paired_residues=pairs)
            lp_m, _, _, _, lp_g = paired_ref.oracle_paired(w, fdm, K, S, rti)
            lps.append(lp_m); lps_g.append(lp_g)
        groups, weights, maps = paired_ref.groups_of(fd1, rti)
        lp_ref = torch.stack(lps, 1)
        p_ref = pair_terms_ref.paired_probs(torch.stack(lps_g, 1), fd1, pt, S, order, groups, weights, maps, state_weights=sw)
        p0 = paired_ref.paired_probs(torch.stack(lps_g, 1), fd1, groups, weights, maps, state_weights=sw)
    else:
        lp_ref, p0, order_ref = tied_states_ref.oracle_tied(w, fd_cpu, K, S)
        assert torch.equal(order_ref, order)
        p_ref = pair_terms_ref.plain_probs(lp_ref, fd_cpu, pt, S, order, state_weights=sw)
    d_lp, d_p, d_0 = maxdiff(LP[:, :, valid], lp_ref[:, :, valid]), maxdiff(P[:, valid], p_ref[:, valid]), maxdiff(P[:, valid], p0[:, valid])
    print(f"states M={M} pairs={with_pairs} + pair terms: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; without the terms {d_0:.3e}")
    assert d_lp < 1e-3 and d_p < 1e-3 and d_0 > 1e-2, (d_lp, d_p, d_0)


@pytest.mark.parametrize("tie", ["plain", "pairs", "states"])
def test_neutral_pair_terms_keep_the_bits(weights_np, tie):
    """All-zero tables, or every partner -1, give the bits of the call without the key (which takes other routes: the early levels, the
    device plans)."""
    dev = torch.device("cuda:0")
    L, K, bs, T = 40, 24, 2, 0.5
    cx, fd_cpu, pairs = make_case(L, bs, T, 6, seed=3140)
    if tie != "pairs":
        del fd_cpu["paired_residues"]
    if tie == "states":
        fd_cpu = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, 2, seed=9), (0.6, 0.4), bs, T, fd_cpu["randn"].numpy(),
                                          bias=fd_cpu["bias"])
    pt = strand_terms(cx, 44, "all")
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(6)).to(dev)
    fd = to_dev(fd_cpu, dev)
    base = m._sample(fd, True, uniform=u)
    zero = m._sample(dict(fd, pair_terms=dict(pt, tables=torch.zeros_like(pt["tables"]))), True, uniform=u)
    none = m._sample(dict(fd, pair_terms=dict(pt, partner=torch.full_like(pt["partner"], -1))), True, uniform=u)
    live = m._sample(dict(fd, pair_terms=pt), True, uniform=u)
    assert m.sample_walk_status() == 0
    for k in KEYS:
        assert torch.equal(zero[k], base[k]) and torch.equal(none[k], base[k]), k
    assert not torch.equal(live["sampling_probs"], base["sampling_probs"])


# ---------------------------------------------------------------------------------------------------------------------------------
# what the key is for
# ---------------------------------------------------------------------------------------------------------------------------------
def homopolymer_steps(S, cx, order0, groups, G, counted):
    """Adjacent residues of one chain that both hold a token of G where the later-drawn one is in `counted` (its group's draw felt the
    earlier one) -> their number over all samples."""
    L = S.shape[1]
    step = pair_terms_ref.steps_of(order0, groups, L)
    n = 0
    for i in range(L - 1):
        if cx["chain_labels"][i] != cx["chain_labels"][i + 1] or step[i] == step[i + 1]:
            continue
        later = i if step[i] > step[i + 1] else i + 1
        if later in counted:
            n += int((torch.isin(S[:, i], G) & torch.isin(S[:, i + 1], G)).sum())
    return n


@pytest.mark.parametrize("wobble", [False, True])
def test_no_adjacent_g_on_any_strand(weights_np, wobble):
    """GG: -1e9 on an all-designable complex with base pairs (no fixed, no masked residue), T = 0.5, bs = 8.  "all": no two adjacent
    residues of a chain both hold G, on either side of a pair; "closing": none where the later-drawn residue closes its group (or is
    untied) — the first-listed members are not covered, which is why base pairs want "all".  The unbiased design under the same
    uniforms does hold such steps on both sides (else the test shows nothing; the case's seed and its G / C bias see to that)."""
    dev = torch.device("cuda:0")
    L, K, bs, T = 60, 24, 8, 0.5
    cx, fd_cpu, pairs = make_case(L, bs, T, 10, seed=3162, fixed_every=0)
    assert (cx["mask"] * cx["chain_mask"]).all()
    if wobble:
        fd_cpu.update(paired_wobble=True, paired_wobble_bias=2.0)
    rti = spec.restype_to_int()
    # (synthetic weights know no chemistry: a bias towards G and C on the nucleic-acid residues makes G common on either side of a pair)
    na = torch.from_numpy(cx["protein_mask"] == 0)
    for name in ("DG", "DC", "G", "C"):
        fd_cpu["bias"][0, na, rti[name]] += 2.0
    G = torch.tensor([rti["DG"], rti["G"]])
    AA = torch.zeros(V, V)
    AA[G[:, None], G[None, :]] = -1e9
    groups = (wobble_ref.groups_of(fd_cpu, rti) if wobble else paired_ref.groups_of(fd_cpu, rti))[0]
    first, closing = {g[0] for g in groups}, {g[-1] for g in groups}
    everyone = set(range(L))
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(7)).to(dev)
    fd = to_dev(fd_cpu, dev)
    count = lambda out, counted: homopolymer_steps(out["S"].cpu(), cx, out["decoding_order"][0].tolist(), groups, G, counted)
    free = m._sample(fd, True, uniform=u)
    n_first, n_rest = count(free, first), count(free, everyone - first)
    print(f"GG steps of the unbiased design (wobble={wobble}): {n_first} felt by first-listed members, {n_rest} by the others")
    assert n_first >= 1 and n_rest >= 1, "seed precondition: the unbiased design holds no GG step on one side — choose another seed"
    out_all = m._sample(dict(fd, pair_terms=pair_terms_ref.neighbour_terms(L, AA, "all", cx["chain_labels"].tolist())), True, uniform=u)
    assert count(out_all, everyone) == 0
    out_cl = m._sample(dict(fd, pair_terms=pair_terms_ref.neighbour_terms(L, AA, "closing", cx["chain_labels"].tolist())), True, uniform=u)
    assert count(out_cl, everyone - first) == 0 and closing <= everyone - first
    assert m.sample_walk_status() == 0


def test_large_complex_stays_compact(weights_np):
    """L = 1500, K = 32: KK: -1e9 on a protein.  No two adjacent designable residues hold K K, and the call's peak allocation stays
    under 1 GiB — the dense tensor alone would be 1500^2 * 33^2 * 4 bytes = 9.8 GB."""
    dev = torch.device("cuda:0")
    L, K = 1500, 32
    cx = synth.make_complex(seed=1500, n=L, n_chains=3, frac_protein=1.0, frac_dna=0.0)
    cx["chain_mask"][::11] = 0
    fd = fd_of(cx, 1, 0.5, 15)
    rti = spec.restype_to_int()
    kk = rti["LYS"]
    fd["bias"][:, :, kk] = 3.0                                                                # (synthetic weights: make K common enough to repeat)
    fd = to_dev(fd, dev)
    AA = torch.zeros(V, V)
    AA[kk, kk] = -1e9
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA)
    m = make_model(weights_np, K, dev)
    u = torch.rand(1, L, generator=torch.Generator().manual_seed(2)).to(dev)
    free = m._sample(fd, True, uniform=u)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = m._sample(dict(fd, pair_terms=pt), True, uniform=u)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    assert m.sample_walk_status() == 0 and torch.isfinite(out["log_probs"]).all()
    des = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    adj = torch.from_numpy((cx["chain_labels"][1:] == cx["chain_labels"][:-1]) & (cx["R_idx"][1:] - cx["R_idx"][:-1] == 1))
    steps = lambda S: int(((S[0, :-1] == kk) & (S[0, 1:] == kk) & adj & des[:-1] & des[1:]).sum())
    print(f"L=1500: K K steps {steps(free['S'].cpu())} unbiased, {steps(out['S'].cpu())} with pair terms; peak allocation {peak / 2**20:.0f} MiB")
    assert steps(free["S"].cpu()) >= 1 and steps(out["S"].cpu()) == 0
    assert peak < (1 << 30), peak


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def _duplex(tmp_path):
    """The 17 + 17 nt DNA duplex of 1AM9 (chains E and G) from tests/golden/pdb."""
    path = os.path.join(str(tmp_path), "1am9.pdb")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdb", "1am9.pdb.xz")
    with lzma.open(src) as fh, open(path, "wb") as dst:
        dst.write(fh.read())
    return path


def _strands(folder):
    lines = open(os.path.join(folder, "seqs", "1am9.fa")).read().splitlines()
    return [s for ln in lines[3::2] for s in ln.split("/")]                                  # (the samples: the first record is the input)


def test_cli_pair_bias_with_paired_strands(tmp_path):
    """--pair_bias_AA with --paired_strands runs (the dense key refused the combination) and no designed strand holds g g; 'auto' is
    'all' with base pairs.  (DNA letters are lower case; synthetic weights know no chemistry: the amino-acid letters are omitted.)"""
    path = _duplex(tmp_path)
    common = ["--pdb_path", path, "--parse_these_chains_only", "EG", "--random_init_seed", "0", "--seed", "11", "--batch_size", "4",
              "--temperature", "0.5", "--output_pdbs", "0", "--paired_strands", "E:G", "--omit_AA", "ARNDCQEGHILKMFPSTWYVX"]
    plain, biased = os.path.join(str(tmp_path), "plain"), os.path.join(str(tmp_path), "biased")
    cli.main(common + ["--out_folder", plain])
    cli.main(common + ["--out_folder", biased, "--pair_bias_AA", "gg:-1e9"])
    got0, got = _strands(plain), _strands(biased)
    assert len(got) == 8 and all(len(s) == 17 for s in got)
    assert any("gg" in s for s in got0[0::2]) and any("gg" in s for s in got0[1::2]), got0  # (both strands of the unbiased run hold g g)
    assert not any("gg" in s for s in got), got


def test_cli_pair_bias_without_ties_is_the_dense_run(tmp_path, monkeypatch):
    """Without ties the compact form writes the files of a run through the dense key, byte for byte."""
    path = _duplex(tmp_path)
    common = ["--pdb_path", path, "--parse_these_chains_only", "EG", "--random_init_seed", "0", "--seed", "5", "--batch_size", "3",
              "--temperature", "0.5", "--output_pdbs", "1", "--pair_bias_AA", "gg:-3.0,ac:1.5,ca:-2.0"]
    compact, dense = os.path.join(str(tmp_path), "compact"), os.path.join(str(tmp_path), "dense")
    cli.main(common + ["--out_folder", compact])

    real = ProteinMPNN.sample

    def through_the_dense_key(self, fd):
        pt = fd["pair_terms"]
        fd = {k: v for k, v in fd.items() if k != "pair_terms"}
        fd["pair_bias"] = pair_terms_dense(pt, fd["S"].shape[1]).to(fd["S"].device)
        return real(self, fd)
    monkeypatch.setattr(ProteinMPNN, "sample", through_the_dense_key)
    cli.main(common + ["--out_folder", dense])
    n = 0
    for root, _, files in os.walk(compact):
        for f in files:
            a, b = os.path.join(root, f), os.path.join(dense, os.path.relpath(os.path.join(root, f), compact))
            assert open(a, "rb").read() == open(b, "rb").read(), f
            n += 1
    assert n >= 4                                                                              # the FASTA and three backbones
