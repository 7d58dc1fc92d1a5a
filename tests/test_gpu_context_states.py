"""GPU tests of context states — ProteinMPNN.sample / score_tied with feature_dict["state_S"] (per-state fixed tokens)
and ["state_mask"] (per-state presence) beside "state_weights" — against the per-state CPU oracle (context_states_ref): the GPU runs
free with a given `uniform`, the oracle is teacher-forced with the GPU's sequence, every draw must be the inverse CDF of the ORACLE's
distribution; the plan's routes, the three routes of score_tied, the call with equal rows, M = 1 and the CLI, bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import paired_ref
import real_structures
from context_states_ref import (case, context_probs, context_state_fd, contexts_fd, model_of, oracle_contexts, oracle_score_tied,
                                other_tokens, token_rows, write_models)
from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
from tied_states_ref import make_states, state_fd, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
TOL = 1e-3            # log_probs and sampling_probs against the oracle (test_gpu_tied_states.py)
TOL_SCORE = 2e-4      # score_tied's rows against the oracle; two GPU routes against each other (test_gpu_tied_score.py)
CDF_MARGIN = 1e-5     # a draw may differ from the oracle's where u lies this close to a boundary of its CDF: at most one per case
SPECIAL = list(cpu_ref.SPECIAL_TOKENS)
_models = {}


def model(weights_np, k, prec="x3"):
    if (k, prec) not in _models:
        m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                        polytype_to_int=spec.polytype_to_int())
        m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
        m = m.to(DEV).eval()
        m.message_precision = prec
        _models[(k, prec)] = m
    m = _models[(k, prec)]
    m.sample_states_device_plan, m.sample_split_groups, m.sample_level_walk = True, True, True
    return m


def maxdiff(a, b):
    return float((torch.as_tensor(a).cpu().double() - torch.as_tensor(b).cpu().double()).abs().max())


@functools.lru_cache(maxsize=None)
def _weights_t():
    return cpu_ref.to_torch(synth.make_weights(0))


_runs = {}


def run(weights_np, name):
    """The case's design call on the device plan (given uniforms) and the oracle teacher-forced with its sequence, once per case."""
    if name not in _runs:
        cx, fd_cpu, K = case(name)
        m = model(weights_np, K)
        bs, L = fd_cpu["batch_size"], fd_cpu["S"].shape[1]
        u = torch.rand(bs, L, generator=torch.Generator().manual_seed(L)).to(DEV)
        out = m._sample(to_dev(fd_cpu, DEV), True, uniform=u)
        assert m.sample_walk_status() == 0
        S = out["S"].cpu()
        _runs[name] = (out, oracle_contexts(_weights_t(), fd_cpu, K, S))
    return _runs[name]


def check_against_oracle(fd_cpu, out, ref, what):
    """The properties of a context call against the oracle (lp_ref [bs, M, L, V], p_ref [bs, L, V], order [L])."""
    lp_ref, p_ref, order_ref = ref
    M, L = fd_cpu["X"].shape[:2]
    bs = fd_cpu["batch_size"]
    S, Ss, P, LP, U, order = (out[k].cpu() for k in ("S", "S_states", "sampling_probs", "log_probs", "uniform", "decoding_order"))
    assert S.shape == (bs, L) and Ss.shape == (bs, M, L) and Ss.dtype == torch.int64 and P.shape == (bs, L, 33)
    assert LP.shape == (bs, M, L, 33) and U.shape == (bs, L)
    assert torch.isfinite(LP).all()                                            # absent members are multiplied by zero, not skipped
    cm = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0] != 0
    present = fd_cpu["state_mask"] != 0 if "state_mask" in fd_cpu else fd_cpu["mask"].expand(M, L) != 0
    # every state's copy: the one drawn token where the design draws, its own state_S elsewhere; S is state 0's block
    assert torch.equal(Ss, token_rows(fd_cpu, S)) and torch.equal(S, Ss[:, 0])
    for tok in SPECIAL:
        assert not (S[:, cm] == tok).any()
    scored = cm[None, :] & present
    assert (LP[:, ~scored] == 0).all() and (P[:, ~cm] == 0).all()
    assert torch.equal(order[0], order_ref) and all(torch.equal(order[0], order[b]) for b in range(bs))
    excepted = 0
    for b in range(bs):
        for t, i in enumerate(order_ref.tolist()):
            if not cm[i]:
                continue
            cdf = torch.cumsum(p_ref[b, i], 0)
            u = float(U[b, t])
            expect = int((cdf > u).nonzero()[0]) if (cdf > u).any() else int(p_ref[b, i].nonzero()[-1])
            if expect != int(S[b, i]):
                assert abs(float(cdf[min(expect, int(S[b, i]))]) - u) < CDF_MARGIN, (what, b, t, i)
                excepted += 1
    d_lp, d_p = maxdiff(LP[:, scored], lp_ref[:, scored]), maxdiff(P, p_ref)
    print(f"context states {what}: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}; draws near a CDF boundary: {excepted}; "
          f"levels {int(out['levels'])}, work items {out['work_items']}")
    assert excepted <= 1, excepted
    assert d_lp < TOL and d_p < TOL, (d_lp, d_p)
    return d_lp, d_p


@pytest.mark.parametrize("name", ["tokens", "tokens_deformed", "unbound", "LltK"])
def test_context_states_free_running(weights_np, name):
    """Cases 1 to 3 of the issue on the device plan.  Measured (MI355X, split-bf16): see the printed line of each case."""
    cx, fd_cpu, K = case(name)
    out, ref = run(weights_np, name)
    M, L = fd_cpu["X"].shape[:2]
    assert out["work_items"] == fd_cpu["batch_size"] * M * L
    check_against_oracle(fd_cpu, out, ref, name)


def test_per_state_tokens_are_felt(weights_np):
    """Case 1 against the call whose rows are equal: same backbone, same uniforms, the fixed tokens of state 1 alone differ — the
    results differ, and by more than the tolerance: the oracle of the equal rows is far from the context call."""
    _, fd_ctx, K = case("tokens")
    _, fd_eq, _ = case("tokens_equal_rows")
    out, (lp_ref, p_ref, _) = run(weights_np, "tokens")
    out_eq, _ = run(weights_np, "tokens_equal_rows")
    assert torch.equal(out["uniform"], out_eq["uniform"]) and torch.equal(out["decoding_order"], out_eq["decoding_order"])
    assert not torch.equal(out["log_probs"][:, 1], out_eq["log_probs"][:, 1])
    assert not torch.equal(out["sampling_probs"], out_eq["sampling_probs"])
    cm = (fd_ctx["mask"] * fd_ctx["chain_mask"])[0] != 0
    lp_wrong, _, _ = oracle_contexts(_weights_t(), fd_eq, K, out["S"].cpu())     # the same sequence under shared tokens
    gap = maxdiff(out["log_probs"].cpu()[:, :, cm], lp_wrong[:, :, cm])
    print(f"per-state tokens: the shared-token oracle is {gap:.3e} from the context call")
    assert gap > 10 * TOL


@pytest.mark.parametrize("name", ["tokens", "unbound", "LltK"])
def test_context_routes_are_bit_identical(weights_np, name):
    """The device plan, the host plan and walk=False give equal bits on every returned tensor."""
    _, fd_cpu, K = case(name)
    ref, _ = run(weights_np, name)
    m = model(weights_np, K)
    fd = to_dev(fd_cpu, DEV)
    for what, (plan, split, walk) in {"host plan": (False, True, True), "host plan, whole groups": (False, False, True),
                                      "per-level launches": (False, True, False)}.items():
        m.sample_states_device_plan, m.sample_split_groups = plan, split
        out = m._sample(fd, walk, uniform=ref["uniform"])
        if walk:
            assert m.sample_walk_status() == 0
        for k in ("S", "S_states", "sampling_probs", "log_probs", "decoding_order", "uniform"):
            assert torch.equal(out[k], ref[k]), (name, what, k)
        assert int(out["levels"]) == int(ref["levels"]), (name, what)
    model(weights_np, K)


def test_equal_rows_give_the_bits_of_the_plain_multi_state_call(weights_np):
    """state_S / state_mask with all rows equal (given both, or either alone) are today's call: every tensor it returns, bit for bit —
    also with masked residues, and with symmetry_residues beside the states."""
    for masked_frac, sym in ((0.0, None), (0.05, None), (0.0, ([[3, 17, 31], [8, 10]], [[0.4, 0.3, 0.3], [0.5, 0.5]]))):
        L, K, M, bs = 60, 24, 3, 2
        cx = synth.make_complex(seed=2100 + L, n=L, masked_frac=masked_frac)
        cx["chain_mask"][::9] = 0
        if sym is not None:
            cx["chain_mask"][[i for g in sym[0] for i in g]] = 1
        rng = np.random.default_rng(L)
        plain = contexts_fd(cx, make_states(cx, M, seed=L), (0.5, 0.3, 0.2), bs, 0.5, rng.standard_normal((bs, L)).astype(np.float32), sym=sym)
        sS, sm = plain["S"].long().repeat(M, 1), plain["mask"].repeat(M, 1)
        m = model(weights_np, K)
        u = torch.rand(bs, L, generator=torch.Generator().manual_seed(3)).to(DEV)
        want = m._sample(to_dev(plain, DEV), True, uniform=u)
        assert "S_states" not in want
        for keys in ({"state_S": sS, "state_mask": sm}, {"state_S": sS}, {"state_mask": sm}):
            got = m._sample(to_dev(dict(plain, **keys), DEV), True, uniform=u)
            for k in want:
                same = torch.equal(got[k], want[k]) if torch.is_tensor(want[k]) else got[k] == want[k]
                assert same, (masked_frac, sorted(keys), k)
            assert torch.equal(got["S_states"], got["S"][:, None, :].expand(bs, M, L))


def test_one_state_with_the_keys_equals_plain_sample(weights_np):
    """M = 1 with the keys: the sequence of plain sample() and its rows within 1e-5 — what test_one_state_equals_plain_sample asks of
    M = 1 without them (the group sum 1.0 * z and the deferred draw are other code paths) —, and the bits of M = 1 without the keys."""
    L, K, bs = 80, 32, 3
    cx = synth.make_complex(seed=2100 + L, n=L)
    cx["chain_mask"][::9] = 0
    rng = np.random.default_rng(L + 1)
    fd_cpu = contexts_fd(cx, make_states(cx, 1, seed=L + 7), (1.0,), bs, 0.5, rng.standard_normal((bs, L)).astype(np.float32))
    keys = {"state_S": fd_cpu["S"].long().clone(), "state_mask": fd_cpu["mask"].clone()}
    m = model(weights_np, K)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(9)).to(DEV)
    out = m._sample(to_dev(dict(fd_cpu, **keys), DEV), True, uniform=u)
    bare = m._sample(to_dev(fd_cpu, DEV), True, uniform=u)
    for k in bare:
        assert (torch.equal(out[k], bare[k]) if torch.is_tensor(bare[k]) else out[k] == bare[k]), k
    plain = m._sample(to_dev(state_fd(fd_cpu, 0), DEV), True, uniform=u)
    assert torch.equal(out["decoding_order"], plain["decoding_order"]) and torch.equal(out["S"], plain["S"])
    assert maxdiff(out["log_probs"][:, 0], plain["log_probs"]) < 1e-5 and maxdiff(out["sampling_probs"], plain["sampling_probs"]) < 1e-5


# ---- score_tied -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tokens", "unbound", "LltK"])
def test_score_tied_with_context_states(weights_np, name):
    """score_tied on its three routes: token_log_probs at designed positions, member_log_probs where a copy is present and
    state_log_likelihood (per counted position) within 2e-4 of the oracle; the routes within 2e-4 of each other; token_log_probs equal
    the log of the sampler's teacher-forced distribution at T = 1 with zero bias (the sampler removes the special tokens and
    renormalises: the oracle's mass of them is put back)."""
    cx, fd_cpu, K = case(name)
    out, _ = run(weights_np, name)
    M, L = fd_cpu["X"].shape[:2]
    rng = np.random.default_rng(7)
    S_lib = torch.cat((out["S"].cpu(), torch.from_numpy(rng.integers(0, 20, (2, L)))))       # the design's sequences and two random ones
    n = S_lib.shape[0]
    ref = oracle_score_tied(_weights_t(), fd_cpu, K, S_lib)
    cm = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0] != 0
    present = fd_cpu["state_mask"] != 0
    counted = cm[None, :] & present
    m = model(weights_np, K)
    fd = to_dev(fd_cpu, DEV)
    outs = {}
    for route in ("items", "stream", "sampler"):
        o = outs[route] = m.score_tied(fd, S_lib.to(DEV), method=route)
        assert o["method"] == route and int(o["units"]) == int(cm.sum()) and bool(o["consistent"].all())
        assert tuple(o["token_log_probs"].shape) == (n, L) and tuple(o["state_log_likelihood"].shape) == (n, M)
        assert torch.equal(o["leader"].cpu(), torch.arange(L))
        own = o["member_log_probs"].cpu()
        assert (own[:, ~present & (fd_cpu["mask"] != 0)] == 0).all()                           # an absent copy scores nothing
        d = (maxdiff(o["token_log_probs"][:, cm], ref["token_log_probs"][:, cm]), maxdiff(own[:, present], ref["member_log_probs"][:, present]),
             maxdiff(o["state_log_likelihood"].cpu() / counted.sum(-1), ref["state_log_likelihood"] / counted.sum(-1)),
             maxdiff(o["log_likelihood"].cpu() / cm.sum(), ref["log_likelihood"] / cm.sum()))
        print(f"score_tied {name} {route}: units {d[0]:.2e} members {d[1]:.2e} state ll / position {d[2]:.2e} ll / unit {d[3]:.2e}")
        assert max(d) < TOL_SCORE, (route, d)
    for other in ("stream", "sampler"):
        d = (maxdiff(outs["items"]["token_log_probs"][:, cm], outs[other]["token_log_probs"][:, cm]),
             maxdiff(outs["items"]["member_log_probs"], outs[other]["member_log_probs"]),
             maxdiff(outs["items"]["state_log_likelihood"], outs[other]["state_log_likelihood"]) / int(cm.sum()))
        print(f"score_tied {name} items vs {other}: units {d[0]:.2e} members {d[1]:.2e} state ll / position {d[2]:.2e}")
        assert max(d) < TOL_SCORE, (other, d)
    # the sampler's own teacher-forced distribution at T = 1 with zero bias
    forced = m._sample(dict(fd, temperature=1.0, bias=torch.zeros(1, L, 33, device=DEV), batch_size=n, S_forced=S_lib.to(DEV),
                            randn=fd["randn"][:1].repeat(n, 1)), True)
    assert torch.equal(forced["S"].cpu()[:, cm], S_lib[:, cm])
    p = forced["sampling_probs"].cpu().double().gather(2, S_lib[:, :, None])[:, :, 0]
    lp_all, _ = oracle_contexts(_weights_t(), fd_cpu, K, S_lib)[:2]
    kept = 1.0 - context_probs(lp_all, fd_cpu, T=1.0, bias=torch.zeros(1, 1, 33), special=())[:, :, SPECIAL].sum(-1)
    d = maxdiff(torch.log(p[:, cm] * kept[:, cm]), outs["items"]["token_log_probs"].cpu()[:, cm])
    print(f"score_tied {name}: against the log of the sampler's distribution {d:.2e}")
    assert d < TOL_SCORE


def test_score_tied_weighted_single_copy(weights_np):
    """A designable residue present in ONE state whose weight is not 1 draws from softmax(w_m logits_m): the stream and sampler routes
    score it so (2e-4 of the oracle), auto avoids the item route, which refuses."""
    cx, fd_cpu, K = case("LltK")
    sm = fd_cpu["state_mask"].clone()
    sm[0, 7] = 0
    sm[1, 7] = 0                                                               # residue 7 is left to state 2 (weight 0.1)
    fd_cpu = dict(fd_cpu, state_mask=sm, X=fd_cpu["X"] * sm[:, :, None, None].float(), X_m=fd_cpu["X_m"] * sm[:, :, None])
    S_lib = torch.from_numpy(np.random.default_rng(3).integers(0, 20, (3, fd_cpu["S"].shape[1])))
    ref = oracle_score_tied(_weights_t(), fd_cpu, K, S_lib)
    cm = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0] != 0
    m = model(weights_np, K)
    fd = to_dev(fd_cpu, DEV)
    with pytest.raises(NotImplementedError):
        m.score_tied(fd, S_lib.to(DEV), method="items")
    assert m.score_tied(fd, S_lib.to(DEV))["method"] == "stream"
    for route in ("stream", "sampler"):
        o = m.score_tied(fd, S_lib.to(DEV), method=route)
        d = maxdiff(o["token_log_probs"][:, cm], ref["token_log_probs"][:, cm])
        print(f"weighted single copy, {route}: {d:.2e}")
        assert d < TOL_SCORE


# ---- pairs beside contexts ----------------------------------------------------------------------------------------------------------------

def test_pairs_beside_context_states(weights_np):
    """Case 4: a 2 x 12 DNA duplex, designable and paired, and 30 fixed protein residues whose tokens differ per state.  The oracle is
    paired_ref's — cpu_ref.sample_symmetric on the mapped groups, per state with the state's tokens — recombined over the states."""
    L, K, M, bs, T, sw = 54, 24, 2, 2, 1.0, (1.0, -0.5)
    cx = synth.make_complex(seed=4100, n=L, n_chains=3, frac_protein=30 / 54, frac_dna=24 / 54)
    prot, dna = np.nonzero(cx["protein_mask"])[0], np.nonzero(cx["dna_mask"])[0]
    assert len(prot) == 30 and len(dna) == 24
    cx["mask"][:] = 1
    cx["chain_mask"][:] = 0
    cx["chain_mask"][dna] = 1
    cx["chain_labels"] = np.where(cx["protein_mask"] == 1, 0, np.where(np.arange(L) < dna[12], 1, 2)).astype(np.int32)
    pairs = [(int(dna[i]), int(dna[23 - i])) for i in range(12)]
    rti = spec.restype_to_int()
    rng = np.random.default_rng(41)
    bias = torch.zeros(1, L, 33)
    bias[0, dna] = -1e8
    for i in dna:
        bias[0, i, [rti[n_] for n_ in ("DA", "DC", "DG", "DT")]] = 0.0         # (synthetic weights know no chemistry: see paired_ref.make_case)
    sS = np.tile(cx["S"], (M, 1))
    sS[1] = other_tokens(cx["S"], prot, rng)
    fd_cpu = contexts_fd(cx, make_states(cx, M, seed=5), sw, bs, T, rng.standard_normal((bs, L)).astype(np.float32), state_S=sS, bias=bias)
    fd_cpu["paired_residues"] = pairs
    m = model(weights_np, K)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(4)).to(DEV)
    out = m._sample(to_dev(fd_cpu, DEV), True, uniform=u)
    assert m.sample_walk_status() == 0
    S, Ss, P, LP = (out[k].cpu() for k in ("S", "S_states", "sampling_probs", "log_probs"))
    assert torch.isfinite(LP).all() and torch.equal(Ss, token_rows(fd_cpu, S))
    canon = set(spec.na_canonical_base_pair_ints(rti))
    assert all((int(S[b, i]), int(S[b, j])) in canon for b in range(bs) for i, j in pairs)
    w = _weights_t()
    lps = []
    for mi in range(M):
        fdm = dict(context_state_fd(fd_cpu, mi), paired_residues=pairs)
        fdm.pop("state_S")
        lp_m, _, _, (groups, weights, maps), lp_g = paired_ref.oracle_paired(w, fdm, K, Ss[:, mi], rti)
        lps.append(lp_m)
    lp_ref = torch.stack(lps, 1)
    fd1 = dict(state_fd(fd_cpu, 0))
    p_ref = paired_ref.paired_probs(lp_ref, fd1, groups, weights, maps, state_weights=sw)
    d_lp, d_p = maxdiff(LP, lp_ref), maxdiff(P, p_ref)
    print(f"pairs beside context states: oracle max|dlogp| = {d_lp:.3e}, max|dp| = {d_p:.3e}")
    assert d_lp < TOL and d_p < TOL, (d_lp, d_p)
    # the protein's tokens of state 1 are felt: the same call with shared tokens gives other rows for state 1
    shared = m._sample(to_dev({k: v for k, v in fd_cpu.items() if k != "state_S"}, DEV), True, uniform=u)
    assert not torch.equal(shared["log_probs"][:, 1], out["log_probs"][:, 1])


# ---- a real structure -----------------------------------------------------------------------------------------------------------------

def real_case():
    """Case 5: the DNA duplex and the bound protein chain of 1AM9 (118 residues); state 0 the complex, state 1 the protein alone; the
    protein is designed, the DNA fixed."""
    cx = real_structures.variant("1am9_crop")
    L = len(cx["S"])
    cx["chain_mask"] = cx["protein_mask"].astype(np.int32)
    sm = np.stack([cx["mask"], cx["mask"] * cx["protein_mask"]]).astype(np.int32)
    rng = np.random.default_rng(118)
    Xs = np.stack([cx["X"], cx["X"]]).astype(np.float32)
    return cx, contexts_fd(cx, Xs, (1.0, -0.5), 1, 0.5, rng.standard_normal((1, L)).astype(np.float32), state_mask=sm), 32


def test_real_structure_bound_against_unbound(weights_np):
    cx, fd_cpu, K = real_case()
    m = model(weights_np, K)
    L = fd_cpu["S"].shape[1]
    u = torch.rand(1, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = m._sample(to_dev(fd_cpu, DEV), True, uniform=u)
    assert m.sample_walk_status() == 0
    ref = oracle_contexts(_weights_t(), fd_cpu, K, out["S"].cpu())
    check_against_oracle(fd_cpu, out, ref, "1AM9 bound / unbound")
    sc = m.score_tied(to_dev(fd_cpu, DEV), out["S"])
    want = oracle_score_tied(_weights_t(), fd_cpu, K, out["S"].cpu())
    cm = (fd_cpu["mask"] * fd_cpu["chain_mask"])[0] != 0
    d = maxdiff(sc["token_log_probs"][:, cm], want["token_log_probs"][:, cm])
    print(f"1AM9 bound / unbound: score_tied ({sc['method']}) against the oracle {d:.2e}")
    assert d < TOL_SCORE


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------

def test_cli_state_contexts(tmp_path):
    """--multi_state 1 --state_contexts 1 on a two-MODEL file (model 2: a renamed base and no second strand) equals the API call on
    parse_states(contexts=True), bit for bit; the stats file carries S_states."""
    from na_mpnn_amd import cli, pdbio
    cx = real_structures.variant("1am9_crop")
    letters = [real_structures.chain_letters("1am9")[i] for i in real_structures.rows_of_chains("1am9", real_structures.CROP_CHAINS)]
    names = [spec.RESTYPES[int(t)] for t in cx["S"]]
    rows = np.r_[0:12, 21:33, 38:68]
    keep = np.r_[0:12, 38:68]
    other = "DG" if names[5] != "DG" else "DA"
    path = os.path.join(str(tmp_path), "ctx.pdb")
    write_models(path, [model_of(cx, names, letters, rows), model_of(cx, names, letters, keep, rename={5: other})])
    out_dir = os.path.join(str(tmp_path), "out")
    cli.main(["--pdb_path", path, "--out_folder", out_dir, "--random_init_seed", "0", "--seed", "11", "--batch_size", "2", "--temperature", "0.5",
              "--chains_to_design", "A", "--output_pdbs", "0", "--multi_state", "1", "--state_contexts", "1", "--state_weights", "1,-0.5",
              "--save_stats", "1"])
    P = pdbio.parse_states(path, contexts=True)
    L = len(P["S"])
    assert L == len(rows) and not P["state_mask"][1, 12:24].any() and P["state_S"][1, 5] != P["state_S"][0, 5]
    chain_mask = np.array([int(c == "A") for c in P["chain_letters"]], np.int32)
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=32, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in synth.make_weights(0).items()})
    m = m.to(DEV).eval()
    m.sample_check_walk = True
    fd = pdbio.to_feature_dict(dict(P, X=P["X"][0], X_m=P["X_m"][0]), chain_mask, DEV)
    alphabet = [spec.RESTYPE_3TO1[r] for r in spec.RESTYPES]
    omit = torch.tensor([float(c in "X" + "bdhuy") for c in alphabet], device=DEV)
    fd.update({"X": torch.as_tensor(P["X"], device=DEV), "X_m": torch.as_tensor(P["X_m"], dtype=torch.int32, device=DEV),
               "state_weights": [1.0, -0.5], "state_S": torch.as_tensor(P["state_S"], dtype=torch.int64, device=DEV),
               "state_mask": torch.as_tensor(P["state_mask"], dtype=torch.int32, device=DEV), "batch_size": 2, "temperature": 0.5,
               "bias": (-1e8 * omit[None, None, :]).repeat(1, L, 1), "symmetry_residues": [[]], "symmetry_weights": [[]]})
    torch.manual_seed(11)
    fd["randn"] = torch.randn(2, L, device=DEV)
    res = m.sample(fd)
    stats = torch.load(os.path.join(out_dir, "stats", "ctx.pt"), weights_only=False)
    assert torch.equal(stats["generated_sequences"], res["S"].cpu()) and torch.equal(stats["S_states"], res["S_states"].cpu())
    assert torch.equal(stats["log_probs"], res["log_probs"].cpu()) and torch.equal(stats["sampling_probs"], res["sampling_probs"].cpu())
    assert torch.equal(stats["S_states"][:, 1, 5], torch.full((2,), int(P["state_S"][1, 5])))
    lines = open(os.path.join(out_dir, "seqs", "ctx.fa")).read().splitlines()
    assert len(lines) == 2 * (1 + 2)
    rti = spec.restype_to_int(True)
    int_to_str = {}
    for k, v in rti.items():
        int_to_str.setdefault(v, spec.RESTYPE_3TO1[k])
    dna_to_rna = {spec.RESTYPE_3TO1[d]: spec.RESTYPE_3TO1[r] for d, r in (("DA", "A"), ("DC", "C"), ("DG", "G"), ("DT", "U"), ("DX", "RX"))}
    for ix in range(2):
        assert lines[3 + 2 * ix] == cli.seq_string(res["S"][ix].cpu().numpy(), P["rna_mask_for_token_conversion"], int_to_str, dna_to_rna,
                                                   P["chain_letters"])
