"""GPU tests of multi-state design — ProteinMPNN.sample with feature_dict["state_weights"]: one sequence tied across M backbone states —
against the per-state CPU oracle (tied_states_ref), across the routes of the plan (namp_states_plan on the device, the host route
with and without split groups, per-level launches), against plain sample() at M = 1, and through the CLI's --multi_state."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
from tied_states_ref import make_states, oracle_tied, state_fd, states_fd, to_dev, write_multimodel

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli")


def make_model(weights_np, k, dev, n_dec=3):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, num_decoder_layers=n_dec, atom_dict=spec.atom_dict(),
                    restype_to_int=spec.restype_to_int(), polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def maxdiff(a, b):
    return float((torch.as_tensor(a).cpu().float() - torch.as_tensor(b).cpu().float()).abs().max())


def case_fd(L, M, bs, T, weights=None, masked_frac=0.0, sym=None):
    cx = synth.make_complex(seed=2100 + L, n=L, masked_frac=masked_frac)
    cx["chain_mask"][::9] = 0                                              # every case has fixed residues
    rng = np.random.default_rng(L + M)
    w = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, np.float64)
    assert np.abs(w).sum() / T <= 4.0                                      # what keeps the sampler's 1e-3 bar valid for the tied sum
    return cx, states_fd(cx, make_states(cx, M, seed=L + 7 * M), w, bs, T, rng.standard_normal((bs, L)).astype(np.float32), sym=sym)


def check_against_oracle(m, weights_np, cx, fd_cpu, K, out, check_score=True):
    """One sequence; fixed residues keep S; no special token; draws follow sampling_probs through the inverse CDF of `uniform`; the
    per-state oracle teacher-forced with the sampled S agrees within 1e-3 on log_probs and sampling_probs; per state, score() on that
    state with the sampled S reproduces its log_probs on designed residues within 2e-4."""
    dev = out["S"].device
    M, L = fd_cpu["X"].shape[:2]
    bs = fd_cpu["batch_size"]
    S, P, U, order = out["S"].cpu(), out["sampling_probs"].cpu(), out["uniform"].cpu(), out["decoding_order"].cpu()
    LP = out["log_probs"].cpu()
    assert S.shape == (bs, L) and P.shape == (bs, L, 33) and LP.shape == (bs, M, L, 33) and U.shape == (bs, L) and order.shape == (bs, L)
    assert torch.isfinite(LP).all() and m.sample_walk_status() == 0
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    assert torch.equal(S[:, ~cm], torch.from_numpy(cx["S"].astype(np.int64))[~cm].expand(bs, -1))
    for tok in (20, 25, 30, 31, 32):
        assert not (S[:, cm] == tok).any()
    assert (LP[:, :, ~cm] == 0).all() and (P[:, ~cm] == 0).all()
    sym = fd_cpu["symmetry_residues"]
    in_group = {i: g for g in sym for i in g}
    steps, seen = [], set()                                                # the residue whose visit closes each step's group
    for i in order[0].tolist():
        if i not in seen:
            g = in_group.get(i, [i])
            seen.update(g); steps.append(g)
    for b in range(bs):
        for t, g in enumerate(steps):
            for i in g:
                if not cm[i]:
                    continue
                cdf = torch.cumsum(P[b, i].double(), 0)
                u = float(U[b, t])
                expect = int((cdf > u).nonzero()[0]) if (cdf > u).any() else int(P[b, i].nonzero()[-1])
                if expect != int(S[b, i]):
                    assert abs(float(cdf[min(expect, int(S[b, i]))]) - u) < 1e-5, (b, t, i)
    w = {k_: torch.from_numpy(v) for k_, v in weights_np.items()}
    lp_ref, p_ref, order_ref = oracle_tied(w, fd_cpu, K, S)
    if len(in_group) == 0:
        assert torch.equal(order_ref, order)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(LP[:, :, valid], lp_ref[:, :, valid]), maxdiff(P[:, valid], p_ref[:, valid])
    d_sc = 0.0
    if check_score:
        for mi in range(M):
            for b in range(bs):
                fdb = to_dev(state_fd(fd_cpu, mi), dev)
                fdb.update(batch_size=1, S=S[b:b + 1].to(dev), randn=fdb["randn"][:1])
                d_sc = max(d_sc, maxdiff(m.score(fdb)["log_probs"][0].cpu()[cm], LP[b, mi][cm]))
    print(f"tied states L={L} K={K} M={M} bs={bs}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; score() max|dlogp| = {d_sc:.3e}; "
          f"levels {int(out['levels'])}, work items {out['work_items']}")
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)
    assert d_sc < 2e-4, d_sc


@pytest.mark.parametrize("L,K,M,bs,T,weights,mf", [(60, 24, 3, 2, 0.5, (0.5, 0.3, 0.2), 0.0), (30, 48, 2, 3, 1.0, (0.6, 0.4), 0.0),
                                                   (97, 32, 4, 1, 0.3, None, 0.03), (200, 48, 8, 2, 0.8, None, 0.0)])
def test_tied_states_free_running(weights_np, L, K, M, bs, T, weights, mf):
    """Free-running tied-states sampling on the device route against the per-state oracle (see check_against_oracle).
    Measured (MI355X, split-bf16): oracle max |dlogp| 3.2e-5 / 3.2e-5 / 3.4e-5 / 4.2e-5, max |dp| 8.0e-6 / 3.8e-6 / 1.0e-5 / 3.2e-6,
    score() max |dlogp| 3.8e-5 / 4.0e-5 / 4.1e-5 / 5.2e-5 in the four cases; exact fp32 (60, 24, 3): 3.3e-6, 6.0e-7, 1.9e-6."""
    dev = torch.device("cuda:0")
    cx, fd_cpu = case_fd(L, M, bs, T, weights, mf)
    m = make_model(weights_np, K, dev)
    torch.manual_seed(5)
    out = m.sample(to_dev(fd_cpu, dev))
    assert out["work_items"] == bs * M * L
    check_against_oracle(m, weights_np, cx, fd_cpu, K, out)


@pytest.mark.parametrize("L,K,M,bs,T,mf", [(60, 24, 3, 2, 0.5, 0.0), (97, 32, 4, 1, 0.3, 0.03), (200, 48, 8, 2, 0.8, 0.0)])
def test_tied_states_routes_are_bit_identical(weights_np, L, K, M, bs, T, mf):
    """The device plan, the host route with walk + split groups, the host route without split and the per-level launches (walk off)
    give bit-identical S, sampling_probs and log_probs under the same uniforms; the walks' barriers complete; the routes count the same
    levels, fewer than L; the split routes decode every (stream, state, residue) as a work item of its own."""
    dev = torch.device("cuda:0")
    _, fd_cpu = case_fd(L, M, bs, T, None, mf)
    fd = to_dev(fd_cpu, dev)
    m = make_model(weights_np, K, dev)
    outs = {}
    for name, (plan, split, walk) in {"device": (True, True, True), "host_split": (False, True, True), "host_whole": (False, False, True),
                                      "per_level": (False, True, False)}.items():
        m.sample_states_device_plan, m.sample_split_groups, m.sample_level_walk = plan, split, walk
        torch.manual_seed(21)
        outs[name] = m.sample(fd)
        if walk:
            assert m.sample_walk_status() == 0
        if name == "device":                              # twice: the workspace and the barrier words are reused
            torch.manual_seed(21)
            again = m.sample(fd)
            assert torch.equal(again["S"], outs[name]["S"]) and torch.equal(again["log_probs"], outs[name]["log_probs"])
    ref = outs["per_level"]
    assert torch.isfinite(ref["log_probs"]).all()
    for name, o in outs.items():
        assert torch.equal(o["uniform"], ref["uniform"]) and torch.equal(o["decoding_order"], ref["decoding_order"]), name
        assert torch.equal(o["S"], ref["S"]), name
        assert torch.equal(o["sampling_probs"], ref["sampling_probs"]), name
        assert torch.equal(o["log_probs"], ref["log_probs"]), name
        assert int(o["levels"]) == int(ref["levels"]) and int(o["levels"]) < L, name
    assert outs["device"]["work_items"] == outs["host_split"]["work_items"] == bs * M * L
    assert outs["host_whole"]["work_items"] == bs * L


@pytest.mark.parametrize("contexts", [False, True])
def test_walk_fallback_equals_the_per_level_sampler(weights_np, contexts):
    """With `sample_check_walk`, a tied-states walk whose grid barrier gave up (reported here by a patched `sample_walk_status`; no
    real timeout is provoked) is decoded again with one launch per level and the same uniforms: the result is the per-level
    sampler's, with a warning, and the model's switches are left as they were — as test_gpu_model's test of the plain path.
    contexts: state_S (state 1 holds other tokens at the fixed residues) and state_mask (state 1 lacks three residues) beside."""
    dev = torch.device("cuda:0")
    L, K, M, bs = 30, 16, 2, 2
    _, fd_cpu = case_fd(L, M, bs, 0.5)
    if contexts:
        fixed = (fd_cpu["chain_mask"][0] == 0).nonzero().view(-1)
        fd_cpu["state_S"] = fd_cpu["S"].long().repeat(M, 1)
        fd_cpu["state_S"][1, fixed] = (fd_cpu["state_S"][1, fixed] + 1) % 20
        fd_cpu["state_mask"] = fd_cpu["mask"].repeat(M, 1)
        fd_cpu["state_mask"][1, [5, 12, 18]] = 0                           # (a fixed one among them; state 0 has all: mask stays the OR)
        assert (fd_cpu["mask"][0, [5, 12, 18]] != 0).all()
        fd_cpu["X"] = fd_cpu["X"] * fd_cpu["state_mask"][:, :, None, None].to(fd_cpu["X"].dtype)
        fd_cpu["X_m"] = fd_cpu["X_m"] * fd_cpu["state_mask"][:, :, None].to(fd_cpu["X_m"].dtype)
    fd = to_dev(fd_cpu, dev)
    m = make_model(weights_np, K, dev)
    m.sample_level_walk = False
    torch.manual_seed(8)
    ref = m.sample(fd)
    m.sample_level_walk, m.sample_check_walk = True, True
    codes, real_status = [0x102], m.sample_walk_status
    m.sample_walk_status = lambda: codes.pop() if codes else real_status()
    torch.manual_seed(8)
    with pytest.warns(UserWarning, match="timed out"):
        out = m.sample(fd)
    assert not codes and m.sample_level_walk and out["levels"] == ref["levels"]
    assert ("S_states" in ref) == contexts
    for key in ("uniform", "decoding_order", "S", "sampling_probs", "log_probs") + (("S_states",) if contexts else ()):
        assert torch.equal(out[key], ref[key]), key


def test_one_state_equals_plain_sample(weights_np):
    """M = 1 with weight 1.0 is plain sample() given the same repeated randn row and the same uniforms: same S, log-probs within 1e-5
    (the same kernels on the same graph; the group sum 1.0 * z and the deferred draw may reorder nothing but are other code paths)."""
    dev = torch.device("cuda:0")
    L, K, bs = 80, 32, 3
    cx, fd_cpu = case_fd(L, 1, bs, 0.5, (1.0,))
    fd = to_dev(fd_cpu, dev)
    m = make_model(weights_np, K, dev)
    torch.manual_seed(9)
    out = m.sample(fd)
    torch.manual_seed(9)
    plain = m.sample(to_dev(state_fd(fd_cpu, 0), dev))
    assert torch.equal(out["uniform"], plain["uniform"]) and torch.equal(out["decoding_order"], plain["decoding_order"])
    assert torch.equal(out["S"], plain["S"])
    assert maxdiff(out["log_probs"][:, 0], plain["log_probs"]) < 1e-5
    assert maxdiff(out["sampling_probs"], plain["sampling_probs"]) < 1e-5


def test_tied_states_with_symmetry_residues(weights_np):
    """States together with symmetry_residues: the groups are the unions across states, the weights w_m * w_sym."""
    dev = torch.device("cuda:0")
    L, K, M, bs, T = 60, 24, 2, 2, 0.5
    sym = ([[3, 17, 40], [8, 10]], [[0.4, 0.3, 0.3], [0.5, 0.5]])        # (all designable; total weight per group 1: sum |w| / T = 2)
    cx, fd_cpu = case_fd(L, M, bs, T, (0.6, 0.4), sym=sym)
    m = make_model(weights_np, K, dev)
    torch.manual_seed(13)
    out = m.sample(to_dev(fd_cpu, dev))
    S = out["S"].cpu()
    for g in sym[0]:
        assert all(torch.equal(S[:, g[0]], S[:, i]) for i in g)
    check_against_oracle(m, weights_np, cx, fd_cpu, K, out, check_score=False)   # (score() knows no ties: the oracle carries this case)


def test_tied_states_exact_fp32(weights_np):
    dev = torch.device("cuda:0")
    L, K, M, bs, T = 60, 24, 3, 2, 0.5
    cx, fd_cpu = case_fd(L, M, bs, T, (0.5, 0.3, 0.2))
    m = make_model(weights_np, K, dev)
    m.message_precision = "fp32"
    torch.manual_seed(5)
    check_against_oracle(m, weights_np, cx, fd_cpu, K, m.sample(to_dev(fd_cpu, dev)))


def test_tied_states_with_four_decoder_layers():
    """The depth the plain sampler's test covers (test_sampler_with_more_than_three_decoder_layers)."""
    dev = torch.device("cuda:0")
    L, K, M, bs, T = 60, 24, 3, 2, 0.5
    w4 = synth.make_weights(0, 3, 4)
    cx, fd_cpu = case_fd(L, M, bs, T, (0.5, 0.3, 0.2))
    m = make_model(w4, K, dev, n_dec=4)
    torch.manual_seed(5)
    check_against_oracle(m, w4, cx, fd_cpu, K, m.sample(to_dev(fd_cpu, dev)))


def test_cli_multi_state(tmp_path):
    """--multi_state 1 on a three-model file: one FASTA whose sequences are what sample() returns for the same seed and the file's
    states; --multi_state 0 leaves the CLI's output byte-identical (the golden FASTA) and reads model 1 of a multi-model file."""
    from na_mpnn_amd import cli, pdbio
    dev = torch.device("cuda:0")
    path = os.path.join(str(tmp_path), "ens.pdb")
    write_multimodel(path, os.path.join(GOLD, "input.pdb"), 3, seed=5)
    out = os.path.join(str(tmp_path), "out")
    args_for = lambda pdb, folder: ["--pdb_path", pdb, "--out_folder", folder, "--random_init_seed", "0", "--seed", "11", "--batch_size", "2",
                                    "--temperature", "0.5", "--fixed_residues", "A0 A1", "--output_pdbs", "0"]
    cli.main(args_for(path, out) + ["--multi_state", "1", "--state_weights", "0.5,0.3,0.2", "--save_stats", "1"])
    lines = open(os.path.join(out, "seqs", "ens.fa")).read().splitlines()
    assert len(lines) == 2 * (1 + 2)
    # the same call by hand
    P = pdbio.parse_states(path)
    L = len(P["S"])
    encoded = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    chain_mask = np.array([int(e not in ("A0", "A1")) for e in encoded], np.int32)
    rti = spec.restype_to_int(True)
    m = make_model(synth.make_weights(0), 32, dev)
    fd = pdbio.to_feature_dict(dict(P, X=P["X"][0], X_m=P["X_m"][0]), chain_mask, dev)
    alphabet = [spec.RESTYPE_3TO1[r] for r in spec.RESTYPES]
    omit = torch.tensor([float(c in "X" + "bdhuy") for c in alphabet], device=dev)
    fd.update({"X": torch.as_tensor(P["X"], device=dev), "X_m": torch.as_tensor(P["X_m"], dtype=torch.int32, device=dev),
               "state_weights": [0.5, 0.3, 0.2], "batch_size": 2, "temperature": 0.5, "bias": (-1e8 * omit[None, None, :]).repeat(1, L, 1),
               "symmetry_residues": [[]], "symmetry_weights": [[]]})
    torch.manual_seed(11)
    fd["randn"] = torch.randn(2, L, device=dev)
    res = m.sample(fd)
    str_to_int = {spec.RESTYPE_3TO1[k]: v for k, v in rti.items()}
    int_to_str = {}
    for k, v in str_to_int.items():
        int_to_str.setdefault(v, k)
    dna_to_rna = {spec.RESTYPE_3TO1[d]: spec.RESTYPE_3TO1[r] for d, r in (("DA", "A"), ("DC", "C"), ("DG", "G"), ("DT", "U"), ("DX", "RX"))}
    for ix in range(2):
        want = cli.seq_string(res["S"][ix].cpu().numpy(), P["rna_mask_for_token_conversion"], int_to_str, dna_to_rna, P["chain_letters"])
        assert lines[3 + 2 * ix] == want
        assert lines[2 + 2 * ix].startswith(f">ens, id={ix + 1}, T=0.5, seed=11, overall_confidence=")
        # overall_confidence: exp of the weight-averaged per-state log-prob of the drawn tokens over the designed residues
        cmask = (fd["mask"] * fd["chain_mask"]).float()[0]
        lp = torch.gather(res["log_probs"][ix], -1, res["S"][ix][None, :, None].expand(3, L, 1))[..., 0]
        loss = -((lp * torch.tensor([0.5, 0.3, 0.2], device=dev)[:, None]).sum(0) * cmask).sum() / (cmask.sum() + 1e-8)
        conf = float(lines[2 + 2 * ix].split("overall_confidence=")[1].split()[0])
        assert abs(conf - float(torch.exp(-loss))) < 2e-4
    stats = torch.load(os.path.join(out, "stats", "ens.pt"), weights_only=False)
    assert tuple(stats["log_probs"].shape) == (2, 3, L, 33) and torch.equal(stats["generated_sequences"], res["S"].cpu())
    # --multi_state 0: the golden run, byte for byte; and model 1 of the multi-model file
    out0 = os.path.join(str(tmp_path), "out0")
    cli.main(["--pdb_path", os.path.join(GOLD, "input.pdb"), "--out_folder", out0, "--random_init_seed", "0", "--seed", "7", "--batch_size", "2",
              "--temperature", "1.0", "--fixed_residues", "A0 A1", "--forced_draws_npz", os.path.join(GOLD, "forced_draws.npz"),
              "--multi_state", "0"])
    assert open(os.path.join(out0, "seqs", "input.fa"), "rb").read() == open(os.path.join(GOLD, "expected.fa"), "rb").read()
    out1 = os.path.join(str(tmp_path), "out1")
    single = os.path.join(str(tmp_path), "m1.pdb")
    body = open(path).read().split("ENDMDL")[0].splitlines()[1:]
    open(single, "w").write("\n".join(body + ["END"]) + "\n")
    cli.main(args_for(path, out1) + ["--multi_state", "0"])
    cli.main(args_for(single, out1 + "s"))
    a, b = (open(os.path.join(o_, "seqs", n_ + ".fa")).read().replace(n_, "x") for o_, n_ in ((out1, "ens"), (out1 + "s", "m1")))
    assert a == b


@pytest.mark.parametrize("L,K,M,bs", [(150, 32, 4, 3), (70, 48, 12, 2), (33, 48, 2, 1), (300, 24, 1, 2)])
def test_states_plan_equals_the_host_route(L, K, M, bs):
    """namp_states_plan against the host route's building blocks on random neighbour lists: the same flattened neighbour lists, visit
    plan, weights, levels (namp_sample_levels_dep on the flattened graph) and level-sorted lists (level_work_lists with split groups).
    12 states x 48 neighbours = 576 look-ups per step: more than the 512 a wave requests ahead."""
    from na_mpnn_amd import hip
    from na_mpnn_amd.model import level_work_lists, symmetry_visits
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(L * M)
    Kk, N = min(K, L), M * L
    E = np.stack([np.stack([rng.permutation(L)[:Kk] for _ in range(L)]) for _ in range(M)]).astype(np.int32)
    order0 = rng.permutation(L).astype(np.int32)
    rank0 = np.empty(L, np.int32); rank0[order0] = np.arange(L, dtype=np.int32)
    w = rng.uniform(0.1, 1.0, M).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    E_d, o_d, r_d, w_d = t(E), t(order0), t(rank0), t(w)
    i32e = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    E_f, sym_w, work_n, level = i32e(N, Kk), torch.full((N,), -7.0, device=dev), i32e(bs * N), i32e(L)
    order_f, rank_f, gf, gl = i32e(bs, N), i32e(bs, N), i32e(bs, N), i32e(bs, N)
    work, level_off, n_levels, close, close_off = i32e(bs * N, 2), i32e(N + 2), i32e(1), i32e(bs * L, 2), i32e(N + 2)
    Lb = hip.lib()
    hip.check(Lb.namp_states_plan(E_d.data_ptr(), o_d.data_ptr(), r_d.data_ptr(), w_d.data_ptr(), E_f.data_ptr(), order_f.data_ptr(),
                                  rank_f.data_ptr(), gf.data_ptr(), gl.data_ptr(), sym_w.data_ptr(), work_n.data_ptr(), level.data_ptr(),
                                  work.data_ptr(), level_off.data_ptr(), n_levels.data_ptr(), close.data_ptr(), close_off.data_ptr(),
                                  bs, M, L, Kk, hip.current_stream()), "states_plan")
    groups = [[i + m * L for m in range(M)] for i in range(L)]
    visits, gf_h, gl_h, wl = symmetry_visits(groups, [list(map(float, w))] * L, order0.tolist(), N)
    order_h = torch.tensor(visits, dtype=torch.int32, device=dev).repeat(bs, 1)
    gf_t = torch.tensor(gf_h, dtype=torch.int32, device=dev).repeat(bs, 1).contiguous()
    gl_t = torch.tensor(gl_h, dtype=torch.int32, device=dev).repeat(bs, 1).contiguous()
    rank_h = ProteinMPNN.ranks_of(order_h.long()).to(torch.int32).contiguous()
    E_h = (E_d + (torch.arange(M, dtype=torch.int32, device=dev) * L)[:, None, None]).view(N, Kk).contiguous()
    lvl_h = torch.empty(bs, N, dtype=torch.int32, device=dev)
    hip.check(Lb.namp_sample_levels_dep(E_h.data_ptr(), order_h.data_ptr(), rank_h.data_ptr(), None, 0, gf_t.data_ptr(), gl_t.data_ptr(),
                                        lvl_h.data_ptr(), bs, 1, N, Kk, hip.current_stream()), "sample_levels")
    sel, flat, wn_h, close_h, coff_h = level_work_lists(lvl_h, gf_t, gl_t, order_h[0], E_h.long(), split=True)
    assert torch.equal(E_f, E_h) and torch.equal(order_f, order_h) and torch.equal(rank_f, rank_h)
    assert torch.equal(gf, gf_t) and torch.equal(gl, gl_t) and torch.equal(sym_w.cpu(), torch.tensor(wl))
    assert torch.equal(level, lvl_h[0, ::M]) and int(n_levels) == int(lvl_h.max()) + 1
    assert sel.numel() == bs * N and torch.equal(work_n, wn_h.to(torch.int32))
    assert torch.equal(work, torch.stack((sel // N, sel % N), 1).to(torch.int32))
    hist = torch.zeros(N + 1, dtype=torch.int64, device=dev).scatter_add_(0, flat, torch.ones_like(flat))
    assert torch.equal(level_off, torch.cat((hist.new_zeros(1), hist.cumsum(0))).to(torch.int32))
    assert torch.equal(close, close_h) and torch.equal(close_off, coff_h)
