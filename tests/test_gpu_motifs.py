"""GPU tests of the forbidden motifs (ProteinMPNN.sample with feature_dict["forbidden_motifs"]): motifs that cannot fire
keep the bits of the call without the key; length 2 agrees with pair terms; every tie against the brute-force reference (motifs_ref) on
the CPU oracle's log-probs; the property the key is for (motif_hits == 0); a skipped ban; and the CLI.  Every case runs on the three
routes of the sampler, bit for bit among them.  1e-3 is the project's bar (test_gpu_model.py, as test_gpu_pair_terms.py uses it)."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import cli, spec, synth
from oracle import cpu_ref
import context_states_ref
import motifs_cases
import motifs_ref
import paired_ref
import pair_terms_ref
import tied_states_ref
import wobble_ref
from motifs_cases import A_, R_, RTI, fd_of, two_chain_complex
from paired_ref import to_dev
from test_gpu_pair_terms import KEYS, ROUTES, _duplex, _strands, make_model, maxdiff, run_routes

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
V = 33
DEV = "cuda:0"
TOL, FAR = 1e-3, 1e-2


def weights_t(weights_np):
    return {k: torch.from_numpy(v) for k, v in weights_np.items()}


def run_state_routes(m, fd, u):
    """States decode by level only: the persistent walk and the per-level launches, bit for bit."""
    outs = {name: m._sample(fd, walk, uniform=u) for name, (par, walk) in ROUTES.items() if par}
    assert m.sample_walk_status() == 0
    for k in KEYS:
        assert torch.equal(outs["walk"][k], outs["per_level"][k]), k
    return outs


def check(what, out, fd_cpu, motifs, lp_ref, p_ref, p_without, valid, info, free=True):
    """sampling_probs and log_probs within 1e-3 of the reference, the reference without the key further than 1e-2 away; on free designs
    no ban was skipped and motif_hits == 0 in every stream, as the reference's own counter says."""
    S, P, LP = (out[k].cpu() for k in ("S", "sampling_probs", "log_probs"))
    d_lp = maxdiff(LP[..., valid, :], lp_ref[..., valid, :])
    d_p, d_0 = maxdiff(P[:, valid], p_ref[:, valid]), maxdiff(P[:, valid], p_without[:, valid])
    hits = out["motif_hits"].cpu()
    print(f"motifs {what}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; with the key dropped {d_0:.3e}; draws with a ban {info['bans']}, "
          f"skipped {info['skipped']}; motif_hits {hits.tolist()}; levels {int(out['levels'])}")
    assert hits.dtype == torch.int64 and torch.equal(hits, motifs_ref.hits(S, fd_cpu, motifs))
    assert d_lp < TOL and d_p < TOL and d_0 > FAR, (d_lp, d_p, d_0)
    if free:
        assert info["skipped"] == 0 and info["bans"] > 0 and int(hits.sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. motifs that cannot fire keep the bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", ["plain", "pairs", "states"])
def test_motifs_that_cannot_fire_keep_the_bits(weights_np, tie):
    """Motifs over a token whose bias is -1e9 ban nothing that has mass: S, probabilities and log-probs of the call without the key, on
    every route (the levels differ — the windows are dependencies —, the draws may not)."""
    L, K, bs, T = 40, 24, 2, 0.5
    cx, fd_cpu, pairs = paired_ref.make_case(L, bs, T, 6, seed=3140)
    W_ = RTI["TRP"]                                                                        # (a token the maps of the pairs fix)
    fd_cpu["bias"][:, :, W_] = -1e9
    fd_cpu["S"][fd_cpu["S"] == W_] = RTI["ALA"]                                              # (a fixed residue may hold it)
    if tie != "pairs":
        del fd_cpu["paired_residues"]
    if tie == "states":
        fd_cpu = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, 2, seed=9), (0.6, 0.4), bs, T, fd_cpu["randn"].numpy(),
                                          bias=fd_cpu["bias"])
    motifs = [(W_, RTI["ALA"]), (RTI["DA"], W_, RTI["DA"]), (W_,) * 8, (RTI["ALA"], W_, RTI["ALA"], RTI["ALA"]), (RTI["G"], RTI["C"], W_)]
    m = make_model(weights_np, K, DEV)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(6)).to(DEV)
    fd = to_dev(fd_cpu, DEV)
    routes = run_state_routes if tie == "states" else (lambda m_, f, u_: run_routes(m_, f, u_, split=(True, False)))
    base, got = routes(m, fd, u), routes(m, dict(fd, forbidden_motifs=motifs), u)
    for route in base:
        for k in KEYS:
            assert torch.equal(got[route][k], base[route][k]), (route, k)
        assert "motif_hits" not in base[route] and int(got[route]["motif_hits"].sum()) == 0
    assert int(got["walk"]["levels"]) >= int(base["walk"]["levels"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. length 2 agrees with pair terms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", ["plain", "pairs"])
def test_length_two_agrees_with_pair_terms(weights_np, tie):
    """["gg"] against pair_terms gg: -1e9 on both neighbours (members "all"): the same S, sampling_probs within 1e-6 (a candidate at -1e9
    has p = 0 exactly either way; what differs is the rounding of the addend 0.0 on the others)."""
    L, K, bs, T = 60, 24, 4, 0.5
    cx, fd_cpu, pairs = paired_ref.make_case(L, bs, T, 10, seed=3162, fixed_every=0)
    if tie == "plain":
        del fd_cpu["paired_residues"]
    na = torch.from_numpy(cx["protein_mask"] == 0)
    for name in ("DG", "DC", "G", "C"):
        fd_cpu["bias"][0, na, RTI[name]] += 2.0
    motifs = [(RTI["DG"], RTI["DG"]), (RTI["G"], RTI["G"])]
    AA = torch.zeros(V, V)
    for a, b in motifs:
        AA[a, b] = -1e9
    pt = pair_terms_ref.neighbour_terms(L, AA, "all", cx["chain_labels"].tolist())
    m = make_model(weights_np, K, DEV)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(7)).to(DEV)
    fd = to_dev(fd_cpu, DEV)
    with_motifs = run_routes(m, dict(fd, forbidden_motifs=motifs), u, split=(True, False))["walk"]
    with_terms = m._sample(dict(fd, pair_terms=pt), True, uniform=u)
    free = m._sample(fd, True, uniform=u)
    assert torch.equal(with_motifs["S"], with_terms["S"]) and not torch.equal(with_motifs["S"], free["S"])
    d = maxdiff(with_motifs["sampling_probs"], with_terms["sampling_probs"])
    print(f"length-2 motifs against pair terms ({tie}): max|dp| = {d:.3e}; motif_hits {with_motifs['motif_hits'].tolist()}")
    assert d < 1e-6 and int(with_motifs["motif_hits"].sum()) == 0
    assert int(motifs_ref.hits(free["S"].cpu(), fd_cpu, motifs).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. against the reference, and the property
# ---------------------------------------------------------------------------------------------------------------------------------
def plain_reference(weights_np, fd_cpu, K, motifs, out, groups=None, gw=None, S_forced=None):
    """The oracle teacher-forced with the sampled S and recombined by motifs_ref -> the arguments of check()."""
    S, order = out["S"].cpu(), out["decoding_order"].cpu()
    run = cpu_ref.sample_symmetric if groups else cpu_ref.sample
    ref = run(weights_t(weights_np), fd_cpu, K, S_forced=S)
    assert torch.equal(ref["S"], S) and torch.equal(ref["decoding_order"], order)
    info = {}
    p_ref = motifs_ref.plain_probs(ref["log_probs"], fd_cpu, motifs, S, order, groups, gw, S_forced=S_forced, info=info)
    return ref["log_probs"], p_ref, ref["sampling_probs"], info


@pytest.mark.parametrize("L,K", [(40, 24), (12, 32)])
def test_plain_against_the_reference(weights_np, L, K):
    """Two chains and one R_idx gap, motifs of length 3, 5 and 8 under a +6 bias on their tokens, bs = 3; L = 12 < K = 32.  Free design:
    motif_hits == 0 in every stream while the same call without the key holds the motifs (this fails without the feature)."""
    cx, fd_cpu, motifs = motifs_cases.plain_case(L=L)
    m = make_model(weights_np, K, DEV)
    u = torch.rand(3, L, generator=torch.Generator().manual_seed(L)).to(DEV)
    fd = to_dev(fd_cpu, DEV)
    out = run_routes(m, dict(fd, forbidden_motifs=motifs), u)["walk"]
    lp, p_ref, p0, info = plain_reference(weights_np, fd_cpu, min(K, L), motifs, out)
    check(f"plain L={L} K={K}", out, fd_cpu, motifs, lp, p_ref, p0, torch.ones(L, dtype=torch.bool), info)
    free = m._sample(fd, True, uniform=u)
    n_free = motifs_ref.hits(free["S"].cpu(), fd_cpu, motifs)
    print(f"  occurrences without the key: {n_free.tolist()}")
    assert int(n_free.sum()) > 0                                                             # (L = 40: the premise test_motifs_host.py holds)
    # the tensor form of the key is the list form
    rows = torch.full((len(motifs), 8), -1, dtype=torch.int64)
    for r, mo in enumerate(motifs):
        rows[r, :len(mo)] = torch.tensor(mo)
    again = m._sample(dict(fd, forbidden_motifs=rows.to(DEV)), True, uniform=u)
    assert all(torch.equal(again[k], out[k]) for k in KEYS)


def test_two_complexes_against_the_reference(weights_np):
    """B = 2 complexes with bs = 2 streams each: stream r samples complex r % 2 with that complex's windows."""
    L, K, bs = 30, 24, 2
    cxs = [two_chain_complex(4200 + b, L, 14 + b, gap_at=6 + 3 * b) for b in range(2)]
    fds = [fd_of(cx, bs, 1.0, 5) for cx in cxs]
    fd_cpu = {key: (torch.cat((fds[0][key], fds[1][key])) if torch.is_tensor(v) and key not in ("randn", "bias") else v) for key, v in fds[0].items()}
    fd_cpu["randn"] = torch.from_numpy(np.random.default_rng(6).standard_normal((2 * bs, L)).astype(np.float32))
    fd_cpu["bias"] = torch.zeros(2, L, V)
    fd_cpu["bias"][:, :, [A_, R_]] = 6.0
    motifs = motifs_cases.PLAIN_MOTIFS
    m = make_model(weights_np, K, DEV)
    u = torch.rand(2 * bs, L, generator=torch.Generator().manual_seed(9)).to(DEV)
    out = run_routes(m, to_dev(dict(fd_cpu, forbidden_motifs=motifs), DEV), u)["walk"]
    assert int(out["motif_hits"].sum()) == 0 and torch.equal(out["motif_hits"].cpu(), motifs_ref.hits(out["S"].cpu(), fd_cpu, motifs))
    for b in range(2):
        fd_b = dict(fds[b], bias=fd_cpu["bias"][b:b + 1], randn=fd_cpu["randn"][b::2])
        sub = {k: out[k][b::2] for k in ("S", "sampling_probs", "log_probs", "decoding_order")}
        sub.update(motif_hits=out["motif_hits"][b::2], levels=out["levels"])
        lp, p_ref, p0, info = plain_reference(weights_np, fd_b, K, motifs, sub)
        check(f"complex {b} of 2", sub, fd_b, motifs, lp, p_ref, p0, torch.ones(L, dtype=torch.bool), info)


def test_symmetry_groups_against_the_reference(weights_np):
    """Symmetry groups with two members inside one window ([4, 6], [20, 21, 23]), one across the chains and one with a fixed member."""
    cx, fd_cpu, motifs = motifs_cases.plain_case(L=40)
    fd_cpu["chain_mask"][0, 31] = 0
    fd_cpu["S"][0, 31] = A_
    fd_cpu["randn"] = fd_cpu["randn"][:1].repeat(3, 1)
    groups, gw = [[4, 6], [20, 21, 23], [2, 30], [31, 33]], [[1.0, 1.0], [0.5, 1.0, 0.5], [1.0, 1.0], [1.0, 1.0]]
    fd_cpu.update(symmetry_residues=groups, symmetry_weights=gw)
    m = make_model(weights_np, 24, DEV)
    u = torch.rand(3, 40, generator=torch.Generator().manual_seed(12)).to(DEV)
    out = run_routes(m, to_dev(dict(fd_cpu, forbidden_motifs=motifs), DEV), u, split=(True, False))["walk"]
    S, order = out["S"].cpu(), out["decoding_order"].cpu()
    # (oracle_paired keeps the log-prob rows of fixed group members, whose logits count in their group's sum; the maps are identities)
    lp, p0, order_ref, (groups_m, gw_m, maps), lp_g = paired_ref.oracle_paired(weights_t(weights_np), fd_cpu, 24, S, RTI,
                                                                               paired_ref.special_tokens(RTI))
    assert torch.equal(order_ref, order) and groups_m == groups
    info = {}
    p_ref = motifs_ref.paired_probs(lp_g, fd_cpu, motifs, S, order, groups_m, gw_m, maps, info=info)
    valid = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0].bool()
    check("symmetry groups", out, fd_cpu, motifs, lp, p_ref, p0, valid, info, free=False)
    assert info["skipped"] == 0 and info["bans"] > 0


def na_case(kind, bs=3, T=1.0):
    """A 2 x 10 RNA duplex (pairs i : 19 - i) or a 13-nt RNA hairpin (stem 5, loop 3: both members of a pair share a window), every
    residue designable on its four bases, G and C favoured; the motifs are the runs of three."""
    if kind == "duplex":
        cx = two_chain_complex(4300, 20, 10)
        pairs = [(i, 19 - i) for i in range(10)]
    else:
        cx = two_chain_complex(4301, 13, 13)
        pairs = [(i, 12 - i) for i in range(5)]
    L = len(cx["S"])
    cx["protein_mask"][:], cx["dna_mask"][:], cx["rna_mask"][:] = 0, 0, 1
    cx["R_polymer_type"][:] = spec.polytype_to_int()["RNA"]
    cx["S"][:] = RTI["A"]
    fd = fd_of(cx, bs, T, 4302)
    fd["randn"] = fd["randn"][:1].repeat(bs, 1)
    fd["bias"][:] = -1e8
    fd["bias"][:, :, [RTI[n] for n in "ACGU"]] = 0.0
    fd["bias"][:, :, [RTI["G"], RTI["C"]]] = 1.0
    fd["paired_residues"] = pairs
    return cx, fd, [(RTI[n],) * 3 for n in "ACGU"]


@pytest.mark.parametrize("kind", ["duplex", "hairpin"])
@pytest.mark.parametrize("wobble", [False, True])
def test_base_pairs_against_the_reference(weights_np, kind, wobble):
    """Token maps and wobble classes: a motif completed on either strand is a motif; in the hairpin both members of a pair sit in one
    window."""
    cx, fd_cpu, motifs = na_case(kind)
    if wobble:
        fd_cpu.update(paired_wobble=True, paired_wobble_bias=1.0)
    L, bs = len(cx["S"]), fd_cpu["batch_size"]
    K = min(24, L)
    m = make_model(weights_np, 24, DEV)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(13)).to(DEV)
    fd = to_dev(fd_cpu, DEV)
    out = run_routes(m, dict(fd, forbidden_motifs=motifs), u, split=(True, False))["walk"]
    S, order = out["S"].cpu(), out["decoding_order"].cpu()
    w, info = weights_t(weights_np), {}
    if wobble:
        lp, p0, _, order_ref, (groups, gw, tables, cb), lp_g = wobble_ref.oracle_wobble(w, fd_cpu, K, S, RTI, paired_ref.special_tokens(RTI))
        p_ref = motifs_ref.class_probs(lp_g, fd_cpu, motifs, S, order, groups, gw, tables, cb, info=info)
    else:
        lp, p0, order_ref, (groups, gw, maps), lp_g = paired_ref.oracle_paired(w, fd_cpu, K, S, RTI, paired_ref.special_tokens(RTI))
        p_ref = motifs_ref.paired_probs(lp_g, fd_cpu, motifs, S, order, groups, gw, maps, info=info)
    assert torch.equal(order_ref, order)
    check(f"{kind} wobble={wobble}", out, fd_cpu, motifs, lp, p_ref, p0, torch.ones(L, dtype=torch.bool), info)
    free = m._sample(fd, True, uniform=u)
    n_free = motifs_ref.hits(free["S"].cpu(), fd_cpu, motifs)
    print(f"  occurrences without the key: {n_free.tolist()}")
    assert int(n_free.sum()) > 0


@pytest.mark.parametrize("with_pairs", [False, True])
def test_states_against_the_reference(weights_np, with_pairs):
    """M = 2 states, alone (the plain case's complex) and with the base pairs of the duplex: the windows sit on state 0's copies."""
    M, sw = 2, (0.6, 0.4)
    if with_pairs:
        cx, fd1, motifs = na_case("duplex", bs=2)
    else:
        cx, fd1, motifs = motifs_cases.plain_case(L=40, bs=2)
    L, bs, T = len(cx["S"]), 2, fd1["temperature"]
    K = min(24, L)
    fd_cpu = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, M, seed=L + 7 * M), sw, bs, T, fd1["randn"].numpy(), bias=fd1["bias"])
    if with_pairs:
        fd_cpu["paired_residues"] = fd1["paired_residues"]
    m = make_model(weights_np, 24, DEV)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(14)).to(DEV)
    out = run_state_routes(m, to_dev(dict(fd_cpu, forbidden_motifs=motifs), DEV), u)["walk"]
    S, order = out["S"].cpu(), out["decoding_order"].cpu()
    w, info = weights_t(weights_np), {}
    if with_pairs:
        lps, lps_g = [], []
        for mi in range(M):
            fdm = dict(tied_states_ref.state_fd(fd_cpu, mi), paired_residues=fd1["paired_residues"])
            lp_m, _, _, _, lp_g = paired_ref.oracle_paired(w, fdm, K, S, RTI)
            lps.append(lp_m); lps_g.append(lp_g)
        groups, gw, maps = paired_ref.groups_of(fd1, RTI)
        lp = torch.stack(lps, 1)
        p_ref = motifs_ref.paired_probs(torch.stack(lps_g, 1), fd1, motifs, S, order, groups, gw, maps, state_weights=sw, info=info)
        p0 = paired_ref.paired_probs(torch.stack(lps_g, 1), fd1, groups, gw, maps, state_weights=sw)
    else:
        lp, p0, order_ref = tied_states_ref.oracle_tied(w, fd_cpu, K, S)
        assert torch.equal(order_ref, order)
        p_ref = motifs_ref.plain_probs(lp, fd_cpu, motifs, S, order, state_weights=sw, info=info)
    assert out["log_probs"].shape == (bs, M, L, V)
    check(f"states M={M} pairs={with_pairs}", out, fd_cpu, motifs, lp, p_ref, p0, torch.ones(L, dtype=torch.bool), info)


def test_context_states_against_the_reference(weights_np):
    """Context states ("tokens_deformed" of test_gpu_context_states.py: the fixed block holds other tokens in state 1): the windows read
    state 0's copies, so a fixed residue counts with state 0's token."""
    cx, fd_cpu, K = context_states_ref.case("tokens_deformed")
    fd_cpu = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in fd_cpu.items()}        # (the case is shared with other tests)
    L, bs = fd_cpu["S"].shape[1], fd_cpu["batch_size"]
    fd_cpu["bias"] = torch.zeros(1, L, V)
    fd_cpu["bias"][:, :, [A_, R_]] = 6.0
    head = torch.tensor([A_, A_, R_, A_])                                                      # a fixed block the motifs can run into
    fd_cpu["state_S"][0, 40:44] = head.to(fd_cpu["state_S"].dtype)
    fd_cpu["S"][0, 40:44] = head.to(fd_cpu["S"].dtype)
    motifs = motifs_cases.PLAIN_MOTIFS
    m = make_model(weights_np, K, DEV)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(15)).to(DEV)
    out = run_state_routes(m, to_dev(dict(fd_cpu, forbidden_motifs=motifs), DEV), u)["walk"]
    S = out["S"].cpu()
    order = out["decoding_order"].cpu()
    lp, p0, order_ref = context_states_ref.oracle_contexts(weights_t(weights_np), fd_cpu, K, S)
    assert torch.equal(order_ref, order[0])
    info = {}
    p_ref = motifs_ref.plain_probs(lp, fd_cpu, motifs, S, order, state_weights=fd_cpu["state_weights"], S_true=fd_cpu["state_S"][0].tolist(),
                                   info=info)
    valid = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0].bool()
    check("context states", out, fd_cpu, motifs, lp, p_ref, p0.float(), valid, info, free=False)
    assert info["skipped"] == 0 and info["bans"] > 0


def test_fixed_residues_and_forced_tokens_against_the_reference(weights_np):
    """Fixed residues inside windows (their tokens are part of occurrences from the first draw on), and S_forced: half the streams are
    forced with a design that holds the motifs, the other half with the constrained design itself.  A forced member holds its forced
    token under every candidate, so a draw's ban takes either every candidate or none and changes no row: the call gives the bits of
    the forced call without the key, the reference agrees, and motif_hits counts what the forced half holds."""
    cx, fd_cpu, motifs = motifs_cases.plain_case(L=40, bs=4)
    for i, tok in ((5, A_), (6, A_), (18, R_), (25, A_), (27, A_)):
        fd_cpu["chain_mask"][0, i] = 0
        fd_cpu["S"][0, i] = tok
    m = make_model(weights_np, 24, DEV)
    u = torch.rand(4, 40, generator=torch.Generator().manual_seed(16)).to(DEV)
    fd = to_dev(dict(fd_cpu, forbidden_motifs=motifs), DEV)
    out = run_routes(m, fd, u)["walk"]
    valid = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0].bool()
    lp, p_ref, p0, info = plain_reference(weights_np, fd_cpu, 24, motifs, out)
    check("fixed residues in windows", out, fd_cpu, motifs, lp, p_ref, p0, valid, info, free=False)
    assert info["skipped"] == 0 and info["bans"] > 0
    occ = [o for b in range(4) for o in motifs_ref.occurrences(out["S"][b].tolist(), motifs_ref.next_ok(fd_cpu), motifs)]
    assert all(all(not valid[j] for j in range(s, s + n)) for s, n in occ)                    # only occurrences wholly on fixed residues are left
    free = m._sample(to_dev(fd_cpu, DEV), True, uniform=u)
    forced = torch.cat((free["S"][:2], out["S"][2:]))
    assert int(motifs_ref.hits(forced[:2].cpu(), fd_cpu, motifs).sum()) > 0
    got = run_routes(m, dict(fd, S_forced=forced), u)["walk"]
    same = m._sample(dict(to_dev(fd_cpu, DEV), S_forced=forced), True, uniform=u)
    assert torch.equal(got["S"], forced) and all(torch.equal(got[k], same[k]) for k in KEYS)
    lp, p_ref, p0, info = plain_reference(weights_np, fd_cpu, 24, motifs, got, S_forced=forced.cpu())
    d_lp, d_p = maxdiff(got["log_probs"][:, valid], lp[:, valid]), maxdiff(got["sampling_probs"][:, valid], p_ref[:, valid])
    print(f"motifs S_forced: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; skipped {info['skipped']}, bans {info['bans']}; "
          f"motif_hits {got['motif_hits'].tolist()}")
    assert d_lp < TOL and d_p < TOL and info["bans"] == 0
    assert torch.equal(got["motif_hits"].cpu(), motifs_ref.hits(forced.cpu(), fd_cpu, motifs)) and int(got["motif_hits"][:2].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a skipped ban
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_ban_that_leaves_nothing_is_skipped(weights_np):
    """Fixed a a on both sides of a designable RNA residue and the motifs a a X for all four bases X: every candidate with mass is banned
    there, so the ban is skipped — the row is the unrestricted one, motif_hits counts the occurrence, and the reference agrees."""
    cx, fd_cpu, _ = na_case("duplex")
    del fd_cpu["paired_residues"]
    a = RTI["A"]
    for i in (3, 4):
        fd_cpu["chain_mask"][0, i] = 0
        fd_cpu["S"][0, i] = a
    motifs = [(a, a, RTI[n]) for n in "ACGU"]
    L, bs = 20, fd_cpu["batch_size"]
    m = make_model(weights_np, 24, DEV)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(17)).to(DEV)
    fd = to_dev(fd_cpu, DEV)
    out = run_routes(m, dict(fd, forbidden_motifs=motifs), u)["walk"]
    lp, p_ref, p0, info = plain_reference(weights_np, fd_cpu, 20, motifs, out)
    S, P = out["S"].cpu(), out["sampling_probs"].cpu()
    hits = out["motif_hits"].cpu()
    print(f"skipped ban: max|dp| = {maxdiff(P, p_ref):.3e}; skipped {info['skipped']}, bans {info['bans']}; motif_hits {hits.tolist()}")
    assert info["skipped"] >= bs and maxdiff(P, p_ref) < TOL and maxdiff(out["log_probs"], lp) < TOL
    assert maxdiff(P[:, 5], p0[:, 5]) < TOL and bool((P[:, 5, [RTI[n] for n in "ACGU"]] > 0).all())      # the unrestricted row at residue 5
    assert torch.equal(hits, motifs_ref.hits(S, fd_cpu, motifs)) and bool((hits >= 1).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def _headers(folder):
    return [ln for ln in open(os.path.join(folder, "seqs", "1am9.fa")).read().splitlines() if ln.startswith(">")][1:]


def test_cli_max_homopolymer(tmp_path):
    """--max_homopolymer 3 on the 17 + 17 nt duplex writes no run of four and reports motif_hits=0; the run without the flag holds one."""
    path = _duplex(tmp_path)
    common = ["--pdb_path", path, "--parse_these_chains_only", "EG", "--random_init_seed", "0", "--seed", "11", "--batch_size", "4",
              "--temperature", "1.0", "--output_pdbs", "0", "--omit_AA", "ARNDCQEGHILKMFPSTWYVX", "--bias_AA", "g:2.0"]
    plain, limited = os.path.join(str(tmp_path), "plain"), os.path.join(str(tmp_path), "limited")
    cli.main(common + ["--out_folder", plain])
    cli.main(common + ["--out_folder", limited, "--max_homopolymer", "3"])
    runs = [c * 4 for c in "acgt"]
    got0, got = _strands(plain), _strands(limited)
    assert len(got) == 8 and all(len(s) == 17 for s in got)
    assert any(r in s for s in got0 for r in runs), got0
    assert not any(r in s for s in got for r in runs), got
    assert all(h.endswith("motif_hits=0") for h in _headers(limited)) and not any("motif_hits" in h for h in _headers(plain))


def test_cli_forbidden_motifs_beside_pairs_and_pair_bias(tmp_path):
    """--forbidden_motifs beside --paired_strands and --pair_bias_AA runs; no strand holds the motifs."""
    path = _duplex(tmp_path)
    out = os.path.join(str(tmp_path), "out")
    cli.main(["--pdb_path", path, "--parse_these_chains_only", "EG", "--random_init_seed", "0", "--seed", "11", "--batch_size", "4",
              "--temperature", "0.5", "--output_pdbs", "0", "--paired_strands", "E:G", "--omit_AA", "ARNDCQEGHILKMFPSTWYVX",
              "--pair_bias_AA", "gg:-1e9", "--forbidden_motifs", "cc,dna:ATA,tat", "--out_folder", out])
    got = _strands(out)
    assert len(got) == 8 and all(len(s) == 17 for s in got)
    # (a pair's draw can lose all four candidates to its two strands, and then skips its ban: the header counts what is left)
    count = lambda s: sum(s[i:i + len(x)] == x for x in ("cc", "ata", "tat") for i in range(len(s)))
    heads = _headers(out)
    assert len(heads) == 4
    for ix, h in enumerate(heads):
        assert int(h.rsplit("motif_hits=", 1)[1]) == count(got[2 * ix]) + count(got[2 * ix + 1]), (h, got[2 * ix:2 * ix + 2])
    assert sum(count(s) for s in got) <= 1, got
