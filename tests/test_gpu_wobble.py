"""GPU tests of base-paired design with G-U wobble — ProteinMPNN.sample with feature_dict["paired_wobble"]: a pair draws a pair class
(the canonical pairs, G-U and U-G) and its members read their tokens from class tables — against the CPU oracle (wobble_ref), reduced
to the canonical call, across the sampler's forms and the routes of the plan, teacher-forced, with states beside the pairs and
through the CLI's --paired_wobble."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import paired_ref
import tied_states_ref
import wobble_ref
from paired_ref import make_case, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GU, UG = spec.CLASS_GU, spec.CLASS_UG


def make_model(weights_np, k, dev, shared=False):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, num_decoder_layers=3, atom_dict=spec.atom_dict(),
                    restype_to_int=spec.restype_to_int(shared), polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def maxdiff(a, b):
    return float((torch.as_tensor(a).cpu().double() - torch.as_tensor(b).cpu().double()).abs().max())


def check_pairs(S, cx, fd_cpu, rti):
    """Every pair that may wobble (asked for, an RNA member) holds a canonical or a wobble pair, every other pair a canonical one ->
    (wobble pairs drawn, canonical pairs drawn) among the pairs that may wobble, over all streams."""
    pairs = fd_cpu["paired_residues"]
    flags = fd_cpu.get("paired_wobble", False)
    n_w = n_c = 0
    for n, (i, j) in enumerate(pairs):
        may = bool(flags[n] if hasattr(flags, "__len__") else flags) and bool(cx["rna_mask"][i] or cx["rna_mask"][j])
        for b in range(S.shape[0]):
            kind = wobble_ref.pair_kind(int(S[b, i]), int(S[b, j]), rti)
            assert kind == "canonical" or (may and kind == "wobble"), (b, i, j, int(S[b, i]), int(S[b, j]), may)
            n_w, n_c = n_w + (may and kind == "wobble"), n_c + (may and kind == "canonical")
    return n_w, n_c


def check_draws(S, U, draws, tables_of, fd_cpu, u_index, what):
    """Every draw is the inverse CDF, in class order, of the ORACLE's restricted distribution at the call's uniform: the members hold
    the tokens of that class.  A draw may differ only where u lies within 1e-5 of a boundary of that CDF, at most once per case, and
    the case's seeds keep every u at least 1e-4 away from the boundaries (the reference alone uses none of that allowance)."""
    cm = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0].bool()
    margin, off, n = 1.0, 0, 0
    for k, (g, pr, cdf) in enumerate(draws):
        if not any(bool(cm[j]) for j in g):
            continue                                                          # (every member keeps its token: nothing is drawn)
        for b in range(S.shape[0]):
            c, dist = wobble_ref.drawn_class(pr[b], cdf[b], float(U[b, u_index(k, g)]))
            margin, n = min(margin, dist), n + 1
            if wobble_ref.tokens_of(c, g, tables_of(k), fd_cpu) != [int(S[b, j]) for j in g]:
                off += 1
                assert dist < 1e-5, (what, b, g, c, dist)
    print(f"{what}: {n} draws, min |cdf - u| = {margin:.3e}, draws off the oracle's: {off}")
    assert margin >= 1e-4, f"seed precondition: a uniform lies {margin:.2e} from a boundary of the oracle's CDF — choose another seed"
    assert off <= 1


def check_against_oracle(m, weights_np, cx, fd_cpu, K, out, shared=False):
    """Fixed residues keep S and have zero rows; no special token; the pairs hold what they may; the oracle teacher-forced with the
    sampled S agrees within 1e-3 on log_probs and on sampling_probs (the unrestricted marginals); the draws are the oracle's."""
    rti = spec.restype_to_int(shared)
    special = paired_ref.special_tokens(rti)
    L, bs = fd_cpu["S"].shape[1], fd_cpu["batch_size"]
    S, P, U, order, LP = (out[k].cpu() for k in ("S", "sampling_probs", "uniform", "decoding_order", "log_probs"))
    assert S.shape == (bs, L) and P.shape == (bs, L, 33) and LP.shape == (bs, L, 33) and U.shape == (bs, L) and order.shape == (bs, L)
    assert torch.isfinite(LP).all() and torch.isfinite(P).all() and m.sample_walk_status() == 0
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    assert torch.equal(S[:, ~cm], torch.from_numpy(cx["S"].astype(np.int64))[~cm].expand(bs, -1))
    for tok in special:
        assert not (S[:, cm] == tok).any()
    assert (LP[:, ~cm] == 0).all() and (P[:, ~cm] == 0).all()
    counts = check_pairs(S, cx, fd_cpu, rti)
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lp_ref, rows, draws, order_ref, (groups, weights, tables, cb), _ = wobble_ref.oracle_wobble(w, fd_cpu, K, S, rti, special)
    assert torch.equal(order_ref, order)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(LP[:, valid], lp_ref[:, valid]), maxdiff(P[:, valid], rows[:, valid])
    rank = torch.empty(L, dtype=torch.int64); rank[order[0]] = torch.arange(L)
    all_tables = wobble_ref.with_singletons(L, groups, weights, tables, cb)[2]
    what = f"wobble L={L} K={K} bs={bs} groups={len(groups)} shared={shared}"
    print(f"{what}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; wobble / canonical pairs drawn where wobble may be: {counts}; "
          f"levels {int(out['levels'])}, work items {out['work_items']}")
    check_draws(S, U, draws, lambda k: all_tables[k], fd_cpu, lambda k, g: int(rank[g[-1]]), what)      # the closing visit reads the uniform
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)
    return counts


#        L   K  bs  T    masked pairs shared cross wobble_bias
CASES = [(60, 24, 2, 0.5, 0.0, 8, False, True, 1.0), (60, 24, 2, 0.5, 0.0, 8, True, True, 0.0), (40, 48, 3, 0.5, 0.0, 6, False, False, 0.0),
         (97, 32, 1, 1.0, 0.03, 10, False, False, 0.0)]


@pytest.mark.parametrize("L,K,bs,T,mf,n_pairs,shared,cross,wbias", CASES)
def test_wobble_free_running(weights_np, L, K, bs, T, mf, n_pairs, shared, cross, wbias):
    """Free-running sampling with wobble (device plan) against the oracle, on the shapes and seeds of the canonical tests: the (60, 24)
    case holds a DNA-RNA pair and runs under both token variants, the (40, 48) case has fixed pair members.  (2 + |bias|) / T <= 6 keeps
    the sampler's 1e-3 bar on the rows.  The biased case must draw both kinds of pair where wobble may be (else the test shows nothing)."""
    dev = torch.device("cuda:0")
    cx, fd_cpu, pairs = make_case(L, bs, T, n_pairs, seed=3100 + L, masked_frac=mf, shared=shared, want_cross=cross)
    if cross:
        assert cx["dna_mask"][pairs[0][0]] != cx["dna_mask"][pairs[0][1]]
    fd_cpu.update(paired_wobble=True, paired_wobble_bias=wbias)
    m = make_model(weights_np, K, dev, shared=shared)
    torch.manual_seed(5)
    out = m.sample(to_dev(fd_cpu, dev))
    assert out["work_items"] == bs * (L - n_pairs)
    n_w, n_c = check_against_oracle(m, weights_np, cx, fd_cpu, K, out, shared)
    if wbias:
        assert n_w >= 1 and n_c >= 1, (n_w, n_c)


@pytest.mark.parametrize("L,K,bs,n_pairs,cross", [(40, 48, 3, 6, False), (60, 24, 2, 8, True)])
def test_wobble_without_mass_is_the_canonical_call(weights_np, L, K, bs, n_pairs, cross):
    """paired_wobble with paired_wobble_bias = -1e9 (no mass on the two wobble classes) gives the BITS of the same call without
    wobble under the same uniforms — S, sampling_probs and log_probs — with fixed pair members ((40, 48)) and without: the class path
    of the kernel against its token-map path."""
    dev = torch.device("cuda:0")
    cx, fd_cpu, pairs = make_case(L, bs, 0.5, n_pairs, seed=3100 + L, want_cross=cross)
    cm = cx["mask"] * cx["chain_mask"]
    if not cross:
        assert any(not (cm[i] and cm[j]) for i, j in pairs)
    m = make_model(weights_np, K, dev)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(3)).to(dev)
    plain = m._sample(to_dev(fd_cpu, dev), True, uniform=u)
    off = m._sample(to_dev(dict(fd_cpu, paired_wobble=True, paired_wobble_bias=-1e9), dev), True, uniform=u)
    assert m.sample_walk_status() == 0
    for k in ("S", "sampling_probs", "log_probs", "decoding_order"):
        assert torch.equal(plain[k], off[k]), k
    on = m._sample(to_dev(dict(fd_cpu, paired_wobble=True), dev), True, uniform=u)
    assert not torch.equal(on["sampling_probs"], plain["sampling_probs"])     # (the key does reach the kernel)


def test_wobble_routes_are_bit_identical(weights_np):
    """With wobble on: the sequential walk, per-level launches, the persistent walk with split groups on and off (host route) and the
    device plan give bit-identical S, sampling_probs and log_probs under the same uniforms; at least one pair's members are not graph
    neighbours (the split route draws them in the deferred closing pass); the device plan's arrays equal the host route's."""
    dev = torch.device("cuda:0")
    L, K, bs, T, n_pairs = 60, 24, 2, 0.5, 8
    cx, fd_cpu, pairs = make_case(L, bs, T, n_pairs, seed=3100 + L, want_cross=True)
    fd_cpu.update(paired_wobble=True, paired_wobble_bias=1.0)
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
        for k in ("decoding_order", "S", "sampling_probs", "log_probs"):
            assert torch.equal(o[k], ref[k]), (name, k)
    assert outs["device"]["work_items"] == outs["host_whole"]["work_items"] == bs * (L - n_pairs)
    assert outs["host_split"]["work_items"] == bs * (L - n_pairs + len(apart))
    for k, v in plans["host_whole"].items():
        assert torch.equal(torch.as_tensor(v).cpu().to(torch.float64), torch.as_tensor(plans["device"][k]).cpu().to(torch.float64)), k
    n_w, n_c = check_pairs(ref["S"].cpu(), cx, fd_cpu, spec.restype_to_int())
    assert n_w >= 1 and n_c >= 1, (n_w, n_c)                                  # (the routes agree on draws of both kinds)


def test_wobble_teacher_forcing(weights_np):
    """A consistent S_forced that holds a G-U pair is reproduced exactly (the forced members restrict the classes to the one they
    spell); the rows stay the unrestricted marginals, those of the oracle teacher-forced with the same sequence."""
    dev = torch.device("cuda:0")
    L, K, bs, T = 60, 24, 2, 0.5
    rti = spec.restype_to_int()
    cx, fd_cpu, pairs = make_case(L, bs, T, 8, seed=3100 + L, want_cross=True)
    fd_cpu["paired_wobble"] = True
    m = make_model(weights_np, K, dev)
    torch.manual_seed(5)
    free = m.sample(to_dev(fd_cpu, dev))
    forced = free["S"].cpu().clone()                                          # consistent: canonical or wobble pairs, fixed residues as given
    cm = cx["mask"] * cx["chain_mask"]
    own = lambda r, n: rti[{"G": "DG", "U": "DT"}[n] if cx["dna_mask"][r] else n]
    i, j = next((i, j) for i, j in pairs if cm[i] and cm[j] and (cx["rna_mask"][i] or cx["rna_mask"][j]))
    forced[:, i], forced[:, j] = own(i, "G"), own(j, "U")
    assert wobble_ref.pair_kind(int(forced[0, i]), int(forced[0, j]), rti) == "wobble"
    out = m._sample(to_dev(dict(fd_cpu, S_forced=forced), dev), True, uniform=free["uniform"])
    assert torch.equal(out["S"].cpu(), forced) and m.sample_walk_status() == 0
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lp_ref, rows, draws, _, (groups, _, tables, _), _ = wobble_ref.oracle_wobble(w, fd_cpu, K, forced, rti, S_forced=forced)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(out["log_probs"].cpu()[:, valid], lp_ref[:, valid]), maxdiff(out["sampling_probs"].cpu()[:, valid], rows[:, valid])
    print(f"wobble teacher-forced: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}")
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)
    k = [sorted(g) for g in groups].index(sorted([i, j]))
    first_is_i = groups[k][0] == i
    assert draws[k][1][0].nonzero().flatten().tolist() == [GU if first_is_i else UG]


def test_wobble_beside_states(weights_np):
    """state_weights (M = 2, L = 40) beside pairs with wobble (the host route: the flattened groups with per-residue tables): the
    recombined per-state oracle agrees within 1e-3 and the draws are its inverse-CDF classes."""
    dev = torch.device("cuda:0")
    L, K, M, bs, T = 40, 48, 2, 2, 1.0
    sw = (0.6, 0.4)
    cx, fd1, pairs = make_case(L, bs, T, 6, seed=3100 + L)
    rti = spec.restype_to_int()
    fd_cpu = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, M, seed=L + 7 * M), sw, bs, T, fd1["randn"].numpy(),
                                      bias=fd1["bias"])
    fd_cpu.update(paired_residues=pairs, paired_wobble=True)
    fd1.update(paired_wobble=True)
    m = make_model(weights_np, K, dev)
    torch.manual_seed(7)
    out = m.sample(to_dev(fd_cpu, dev))
    S, P, LP, U = (out[k].cpu() for k in ("S", "sampling_probs", "log_probs", "uniform"))
    assert LP.shape == (bs, M, L, 33) and m.sample_walk_status() == 0
    n_w, n_c = check_pairs(S, cx, fd1, rti)
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lps, lps_g = [], []
    for mi in range(M):
        fdm = dict(tied_states_ref.state_fd(fd_cpu, mi), paired_residues=pairs)
        lp_m, _, _, _, lp_g = paired_ref.oracle_paired(w, {k: v for k, v in fdm.items() if k not in wobble_ref.WOBBLE_KEYS}, K, S, rti)
        lps.append(lp_m); lps_g.append(lp_g)                                 # (lp_g keeps the rows of fixed pair members)
    groups, weights, tables, cb = wobble_ref.groups_of(fd1, rti)
    rows, draws = wobble_ref.class_probs(torch.stack(lps_g, 1), fd1, groups, weights, tables, cb, state_weights=sw)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(LP[:, :, valid], torch.stack(lps, 1)[:, :, valid]), maxdiff(P[:, valid], rows[:, valid])
    print(f"wobble beside states: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; wobble / canonical pairs: {(n_w, n_c)}")
    # `uniform` is by STEP with states: the groups take their steps as the decoding order reaches their first member
    all_groups, _, all_tables, _ = wobble_ref.with_singletons(L, groups, weights, tables, cb)
    group_of = {j: k for k, g in enumerate(all_groups) for j in g}
    step_of = {}
    for r in out["decoding_order"][0].tolist():
        step_of.setdefault(group_of[r], len(step_of))
    check_draws(S, U, draws, lambda k: all_tables[k], fd1, lambda k, g: step_of[k], "wobble beside states")
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)


def test_wobble_refusals(weights_np):
    dev = torch.device("cuda:0")
    cx, fd_cpu, pairs = make_case(40, 1, 0.5, 2, seed=3140, fixed_every=0)
    fd_cpu["paired_wobble"] = True
    m = make_model(weights_np, 24, dev)
    fd = to_dev(fd_cpu, dev)
    with pytest.raises(ValueError, match="pair_bias is not supported together with paired_residues"):
        m.sample(dict(fd, pair_bias=torch.zeros(1, 40, 33, 40, 33, device=dev)))
    i, j = pairs[0]
    other = next(r for r in range(40) if r not in (i, j) and r not in pairs[1])
    with pytest.raises(ValueError, match="wobble pairs do not join symmetry groups"):
        m.sample(dict(fd, symmetry_residues=[[j, other]], symmetry_weights=[[0.5, 0.5]]))
    from na_mpnn_amd import hip
    t = torch.zeros(64 + 40 + 64, dtype=torch.int32, device=dev)
    assert hip.lib().namp_sample_class_tables(t.data_ptr(), 1, 65) != 0       # more classes than lanes
    assert hip.lib().namp_sample_class_tables(t.data_ptr(), 0, 35) != 0
    assert hip.lib().namp_sample_class_tables(None, 0, 0) == 0                # detaches


def test_cli_paired_wobble(tmp_path):
    """--paired_strands A:B --paired_wobble 1 on a synthetic all-RNA 2 x 12 duplex: every pair of every sample is canonical or G-U,
    and pairs of both kinds are drawn (the synthetic weights put nearly all mass on G-C: the bias of 4 makes G-U about as likely); the
    same run without the flag stays canonical-only."""
    from na_mpnn_amd import cli, pdbio
    n = 12
    cx = synth.make_complex(seed=77, n=2 * n, n_chains=1, frac_protein=0.0, frac_dna=0.0)
    assert cx["rna_mask"].all()
    path = os.path.join(str(tmp_path), "duplex.pdb")
    pdbio.write_pdb(path, cx["X"], cx["X_m"], [spec.RESTYPES[t] for t in cx["S"]], ["A"] * n + ["B"] * n, list(range(1, n + 1)) * 2)
    l1 = spec.RESTYPE_3TO1
    canonical = {(l1["A"], l1["U"]), (l1["U"], l1["A"]), (l1["C"], l1["G"]), (l1["G"], l1["C"])}
    gu = {(l1["G"], l1["U"]), (l1["U"], l1["G"])}
    # (synthetic weights know no chemistry: the amino-acid letters are omitted)
    common = ["--pdb_path", path, "--random_init_seed", "0", "--seed", "11", "--batch_size", "3", "--temperature", "0.5", "--output_pdbs", "0",
              "--paired_strands", "A:B", "--omit_AA", "ARNDCQEGHILKMFPSTWYVX"]

    def pair_letters(folder):
        lines = open(os.path.join(folder, "seqs", "duplex.fa")).read().splitlines()
        assert len(lines) == 2 * (1 + 3)
        out = []
        for a, b in (ln.split("/") for ln in lines[3::2]):                    # (the samples: the first record is the input)
            assert len(a) == len(b) == n
            out += list(zip(a, reversed(b)))                                  # antiparallel
        return out

    out_w = os.path.join(str(tmp_path), "out_wobble")
    cli.main(common + ["--out_folder", out_w, "--paired_wobble", "1", "--paired_wobble_bias", "4.0"])
    got = pair_letters(out_w)
    assert all(p in canonical or p in gu for p in got), got
    assert any(p in gu for p in got) and any(p in canonical for p in got), got
    out_c = os.path.join(str(tmp_path), "out_canonical")
    cli.main(common + ["--out_folder", out_c])
    assert all(p in canonical for p in pair_letters(out_c))
