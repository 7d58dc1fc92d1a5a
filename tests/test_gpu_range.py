"""GPU tests of every precision mode at the activation scales of a trained model: the shapes and entry points the suite already runs, with
the weight variants of tests/weight_variants.py, which push GELU pre-activations past the exact form's clamp and the bf16-mode polynomial's
checked range, feed LayerNorms rows with |mean| / std in the hundreds, and drive |log p| to 50 (tests/test_weight_variants_host.py asserts
that reach on the CPU).  Every comparison is against the CPU oracle evaluated in fp64, computed once per (variant, input)."""
import functools

import numpy as np
import pytest
import torch

import weight_variants as wv
from na_mpnn_amd import hip, spec, synth, train
from na_mpnn_amd.model import ProteinMPNN
from na_mpnn_amd.pack import PackedWeights
from oracle import cpu_ref, cpu_ref_mixed
from test_gpu_parity import TOL_ACT, TOL_LOGP, run_encdec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
GRAPH_VARIANTS = ("base", "gain2", "gain4", "shift", "affine", "head")
MAX_NEAR_TIES = 0.02                 # share of the unmasked residues the arg-max rule may leave out


# ------------------------------------------------------------------------------------------------------------------------------------
# shared, cached inputs and fp64 oracles
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def session_weights():
    return synth.make_weights(0)


@functools.lru_cache(maxsize=None)
def graph_inputs(shape):
    t = wv.graph_case(shape)
    return t, {k: v.to(DEV) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def graph_oracle64(name, shape):
    return wv.graph_oracle(wv.torch_weights(session_weights(), name, F64), graph_inputs(shape)[0])


@functools.lru_cache(maxsize=None)
def graph_autocast(name, shape):
    """The reference's own whole-model bf16 autocast on the same inputs, against the fp64 oracle: (max |dlogp|, arg-max agreement) on the
    unmasked residues — the accuracy class the bf16 throughput mode is held to."""
    t = graph_inputs(shape)[0]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        lp = wv.graph_oracle(wv.torch_weights(session_weights(), name), t)["log_probs"].double()
    ref = graph_oracle64(name, shape)["log_probs"]
    valid = t["mask"].bool()
    return float((lp - ref)[valid].abs().max()), float((lp.argmax(-1) == ref.argmax(-1))[valid].float().mean())


@functools.lru_cache(maxsize=None)
def packed_weights(name):
    return PackedWeights({k: v.to(DEV) for k, v in wv.torch_weights(session_weights(), name).items()}, 3, 3, 33, torch.device(DEV))


@functools.lru_cache(maxsize=None)
def coords_oracle64(name):
    fd = wv.coords_case()
    w, fd64 = wv.torch_weights(session_weights(), name, F64), cpu_ref.to_dtype(fd, F64)
    with torch.no_grad():
        _, E, E_idx = cpu_ref.features(w, fd64, wv.COORDS_K)
        return {"E": E, "E_idx": E_idx, "score": cpu_ref.score(w, fd64, wv.COORDS_K),
                "unconditional": cpu_ref.unconditional_probs(w, fd64, wv.COORDS_K)["log_probs"]}


@functools.lru_cache(maxsize=None)
def train_oracle64(name):
    fd, randn = wv.train_case()
    return cpu_ref.train_loss_and_grads(wv.torch_weights(session_weights(), name, F64), cpu_ref.to_dtype(fd, F64), wv.TRAIN_K, randn,
                                        spec.restype_to_int())


@functools.lru_cache(maxsize=None)
def train_oracle_mixed(name):
    fd, randn = wv.train_case()
    return cpu_ref_mixed.train_loss_and_grads(wv.torch_weights(session_weights(), name), fd, wv.TRAIN_K, randn, spec.restype_to_int())


def make_model(name, k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict(wv.torch_weights(session_weights(), name))
    return m.to(DEV)


def on_device(fd):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def check_log_probs(tag, logp, ref, valid):
    """The parity bars on log-probabilities: finite, rows normalised, within TOL_LOGP on unmasked residues, arg-max identical wherever the
    fp64 oracle's top two are at least 2 TOL_LOGP apart — and that rule may leave out at most MAX_NEAR_TIES of the unmasked residues."""
    logp = logp.detach().cpu()
    assert torch.isfinite(logp).all(), tag
    assert float(torch.logsumexp(logp.double(), -1).abs().max()) < 1e-5, tag
    err = float((logp.double() - ref)[valid].abs().max())
    decided = valid & (wv.top2_margin(ref) >= 2 * TOL_LOGP)
    left_out = int(valid.sum()) - int(decided.sum())
    print(f"RANGE {tag}: max|dlogp| = {err:.2e}; arg-max rule leaves out {left_out} of {int(valid.sum())} unmasked residues")
    assert left_out <= MAX_NEAR_TIES * int(valid.sum()), tag
    assert err < TOL_LOGP, (tag, err)
    assert torch.equal(logp.argmax(-1)[decided], ref.argmax(-1)[decided]), tag
    return err


# ------------------------------------------------------------------------------------------------------------------------------------
# a. graph path, parity modes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("name", GRAPH_VARIANTS)
def test_graph_path_parity_modes(name, shape, joint, prec):
    """(V, E, E_idx) -> h_V, h_E, log-probs as namp_encoder_fwd + namp_decoder_fwd and as the joint namp_encdec_fwd, split-bf16 and exact
    fp32, on the fused path (2 x 120, K = 30) and in the unfused regime (3 x 840 = 2,520 residues, K = 17: two tiles with padding rows)."""
    L = hip.lib()
    B, N, K, _ = wv.GRAPH_SHAPES[shape]
    if shape == "large":
        assert B * N > L.namp_fused_tail_max_residues()
    t, d = graph_inputs(shape)
    ref = graph_oracle64(name, shape)
    P = packed_weights(name)
    P.set_precision(prec)
    try:
        hV, hE, logp, order = run_encdec(L, torch.device(DEV), P, d, B, N, K, joint)
    finally:
        P.set_precision("x3")
    tag = f"graph {name} {shape} {'joint' if joint else 'separate'} {prec}"
    assert torch.isfinite(hV).all() and torch.isfinite(hE).all(), tag
    assert torch.equal(order.cpu(), ref["decoding_order"]), tag
    stride = max(1, N // 16)
    d_hv, d_he = maxdiff(hV, ref["h_V"]), maxdiff(hE[:, ::stride], ref["h_E"][:, ::stride])
    print(f"RANGE {tag}: max|dh_V| = {d_hv:.2e}, max|dh_E| = {d_he:.2e}")
    check_log_probs(tag, logp, ref["log_probs"], t["mask"].bool())
    assert d_hv < TOL_ACT and d_he < TOL_ACT, (tag, d_hv, d_he)


# ------------------------------------------------------------------------------------------------------------------------------------
# b. graph path, bf16 throughput mode
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,joint", [("small", False), ("large", True)])
@pytest.mark.parametrize("name", GRAPH_VARIANTS)
def test_graph_path_bf16_mode(name, shape, joint):
    """bf16 MFMA per-edge GEMMs (separate calls, small shape; joint call, large shape) against the fp64 oracle.  (The joint call stores h_E
    and the gathered tables as bf16 only with more edge workgroups than two per compute unit: 3 x 840 x 17 has 420, so on 256 compute units
    it runs the large-batch launches with h_E in fp32 — tests/test_gpu_solvable.py asserts which path a shape takes.)  Bar: the accuracy class of the reference's own whole-model bf16 autocast evaluated on the same inputs
    (cpu_ref under torch.autocast against the fp64 oracle), margin 1 x: max |dlogp| <= max(0.055, autocast's), arg-max agreement >=
    min(0.99, autocast's).  On `shift` and `head` autocast itself falls apart (max |dlogp| above 0.6): finiteness and normalisation only."""
    L = hip.lib()
    B, N, K, _ = wv.GRAPH_SHAPES[shape]
    t, d = graph_inputs(shape)
    ref = graph_oracle64(name, shape)["log_probs"]
    valid = t["mask"].bool()
    P = packed_weights(name)
    P.set_precision("bf16")
    try:
        hV, hE, logp, _ = run_encdec(L, torch.device(DEV), P, d, B, N, K, joint)
    finally:
        P.set_precision("x3")
    logp = logp.cpu()
    err = float((logp.double() - ref)[valid].abs().max())
    agree = float((logp.argmax(-1) == ref.argmax(-1))[valid].float().mean())
    ac_err, ac_agree = graph_autocast(name, shape)
    print(f"RANGE bf16 {name} {shape} {'joint' if joint else 'separate'}: max|dlogp| = {err:.4f}, arg-max agreement = {agree:.4f}; "
          f"the reference's autocast: {ac_err:.4f} / {ac_agree:.4f}")
    assert torch.isfinite(logp).all() and torch.isfinite(hV).all()
    assert float(torch.logsumexp(logp.double(), -1).abs().max()) < 1e-5
    if name not in ("shift", "head"):
        assert err <= max(0.055, ac_err), (name, shape, err, ac_err)
        assert agree >= min(0.99, ac_agree), (name, shape, agree, ac_agree)


# ------------------------------------------------------------------------------------------------------------------------------------
# c. from coordinates
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", wv.NAMES)
def test_from_coordinates(name, prec):
    """model.score and model.unconditional_probs on a 70-residue complex with masked residues and missing atoms, K = 24: the featuriser
    (its LayerNorm sees the large-mean rows of `feat`), encoder, decoder and output head."""
    fd_cpu = wv.coords_case()
    fd = on_device(fd_cpu)
    ref = coords_oracle64(name)
    valid = fd_cpu["mask"][0].bool()
    m = make_model(name, wv.COORDS_K).eval()
    m.message_precision = prec
    with torch.no_grad():
        V, E, E_idx = m.featurize(fd)
        out = m.score(fd)
        up = m.unconditional_probs(fd)
    # neighbour lists: a masked residue's distance row is all-equal, so its list is an arbitrary tie-break on either device
    E_idx, ref_idx = E_idx[0].cpu().long(), ref["E_idx"][0]
    assert torch.equal(E_idx[valid], ref_idx[valid])
    d_e = maxdiff(E[0][valid], ref["E"][0][valid])
    tag = f"coords {name} {prec}"
    print(f"RANGE {tag}: max|dE| = {d_e:.2e}")
    assert torch.equal(out["decoding_order"].cpu(), ref["score"]["decoding_order"])
    check_log_probs(tag + " score", out["log_probs"], ref["score"]["log_probs"], fd_cpu["mask"].bool())
    check_log_probs(tag + " unconditional", up["log_probs"], ref["unconditional"], fd_cpu["mask"].bool())
    assert torch.isfinite(E).all() and d_e < TOL_ACT, (tag, d_e)


# ------------------------------------------------------------------------------------------------------------------------------------
# d. sampler
# ------------------------------------------------------------------------------------------------------------------------------------
OMITTED = (10, 11, 12, 13)


def sample_case(T):
    n, bs = 60, 3
    cx = synth.make_complex(seed=500, n=n, n_chains=2)
    cx["chain_mask"][:7] = 0
    rng = np.random.default_rng(n)
    bias = np.zeros((1, n, 33), np.float32)
    bias[:, :, OMITTED] = -1e8                                           # omitted letters
    allowed = [a for a in range(33) if a not in OMITTED and a not in cpu_ref.SPECIAL_TOKENS]
    bias[0, np.arange(n), rng.choice(allowed, n)] = 30.0                 # one strongly favoured letter per residue
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd.update({"batch_size": bs, "temperature": T, "bias": torch.from_numpy(bias), "symmetry_residues": [[]], "symmetry_weights": [[]],
               "randn": torch.from_numpy(rng.standard_normal((bs, n)).astype(np.float32))})
    return cx, fd


@pytest.mark.parametrize("T", [0.05, 1.0])
@pytest.mark.parametrize("name", ["base", "gain4", "head"])
def test_sampler(name, T):
    """model.sample (n = 60, K = 16, three streams, seven fixed residues) with a bias that omits letters (-1e8) and favours one letter per
    residue (+30), at T = 0.05 (logits / T of several hundred) and T = 1: the checks of test_sample_free_running — (i) draws follow the
    returned distributions through the inverse CDF of the returned uniforms, (ii) fixed residues keep their tokens, special and omitted
    tokens never appear, (iv) the fp64 oracle teacher-forced with the sampled sequence gives the same log_probs / sampling_probs within 1e-3
    — once decoded by the level walk and once sequentially, the two bit-identical."""
    k = 16
    cx, fd_cpu = sample_case(T)
    fd = on_device(fd_cpu)
    n, bs = cx["S"].shape[0], fd_cpu["batch_size"]
    m = make_model(name, k).eval()
    outs = []
    with torch.no_grad():
        for lvl, walk in ((True, True), (False, False)):
            m.sample_level_parallel, m.sample_level_walk = lvl, walk
            torch.manual_seed(5)
            outs.append(m.sample(fd))
    out, seq = outs
    assert "levels" in out and "levels" not in seq
    for key in ("uniform", "decoding_order", "S", "sampling_probs", "log_probs"):
        assert torch.equal(out[key], seq[key]), key
    S, P, U = out["S"].cpu(), out["sampling_probs"].cpu(), out["uniform"].cpu()
    order = out["decoding_order"].cpu()
    assert torch.isfinite(P).all() and torch.isfinite(out["log_probs"]).all()
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    # (ii)
    assert torch.equal(S[:, ~cm], torch.from_numpy(cx["S"].astype(np.int64))[~cm].expand(bs, -1))
    for tok in cpu_ref.SPECIAL_TOKENS + OMITTED:
        assert not (S[:, cm] == tok).any()
        assert float(P[:, :, tok].abs().max()) == 0.0
    assert float((P[:, cm].double().sum(-1) - 1).abs().max()) < 1e-5
    # (i) inverse CDF
    for b in range(bs):
        for t in range(n):
            i = int(order[b, t])
            if not cm[i]:
                continue
            cdf = torch.cumsum(P[b, i].double(), 0)
            u = float(U[b, t])
            expect = int((cdf > u).nonzero()[0]) if (cdf > u).any() else int(P[b, i].nonzero()[-1])
            if expect != int(S[b, i]):
                assert abs(float(cdf[min(expect, int(S[b, i]))]) - u) < 1e-5, (b, t, i)
    # (iv) the fp64 oracle, teacher-forced
    with torch.no_grad():
        ref = cpu_ref.sample(wv.torch_weights(session_weights(), name, F64), cpu_ref.to_dtype(fd_cpu, F64), k, S_forced=S)
    assert ref["log_probs"].dtype == F64
    assert torch.equal(ref["decoding_order"], order)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp = maxdiff(out["log_probs"][:, valid], ref["log_probs"][:, valid])
    d_p = maxdiff(out["sampling_probs"][:, valid], ref["sampling_probs"][:, valid])
    print(f"RANGE sampler {name} T={T}: max|dlogp| = {d_lp:.2e}, max|dp| = {d_p:.2e}, max|logit / T| = "
          f"{float(ref['log_probs'].abs().max()) / T:.0f}")
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)


# ------------------------------------------------------------------------------------------------------------------------------------
# e. training
# ------------------------------------------------------------------------------------------------------------------------------------
def train_step_on_device(name, prec, monkeypatch):
    monkeypatch.setattr(train, "X3", train.X3)               # forward_train sets the module's precision code: put it back for later tests
    fd, randn = wv.train_case()
    rti = spec.restype_to_int()
    m = make_model(name, wv.TRAIN_K).train()
    m.message_precision = prec
    rm, rn = train.polymer_restype_tables(rti, 33, DEV)
    no_loss = torch.tensor([rti[t] for t in cpu_ref.NO_LOSS_TOKENS], device=DEV)
    opt = train.get_std_opt(m.parameters(), 128, 0)
    with torch.enable_grad():
        loss, _ = train.train_step(m, opt, on_device(fd), rm, rn, no_loss, decoding_randn=randn.to(DEV))
    return float(loss), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", GRAPH_VARIANTS)
def test_training_step(name, prec, monkeypatch):
    """train.train_step on the padded batch of test_training_gradients_odd_shapes (40 + 33 residues, K = 17, masked residues) against
    cpu_ref.train_loss_and_grads in fp64, the existing bars: loss 1e-5 relative, every gradient within 2e-4 of its tensor's max."""
    loss_ref, _, g_ref = train_oracle64(name)
    loss, grads = train_step_on_device(name, prec, monkeypatch)
    worst = ("", 0.0)
    for key, gr in grads.items():
        assert torch.isfinite(gr).all(), key
        scale = float(g_ref[key].abs().max())
        if scale >= 1e-12:
            e = float((gr - g_ref[key]).abs().max()) / scale
            worst = max(worst, (key, e), key=lambda x: x[1])
    print(f"RANGE train {name} {prec}: loss {abs(loss - float(loss_ref)) / abs(float(loss_ref)):.1e} relative, worst gradient {worst[1]:.2e} "
          f"of its tensor's max ({worst[0]})")
    assert abs(loss - float(loss_ref)) <= 1e-5 * max(1e-3, abs(float(loss_ref)))
    for key, gr in grads.items():
        scale = float(g_ref[key].abs().max())
        if scale < 1e-12:
            assert float(gr.abs().max()) < 1e-9, key
        else:
            assert float((gr - g_ref[key]).abs().max()) / scale < 2e-4, (key, float((gr - g_ref[key]).abs().max()) / scale)


@pytest.mark.parametrize("name", ["base", "gain2", "gain4"])
def test_training_step_mixed_precision(name, monkeypatch):
    """message_precision "bf16" against the CPU emulation of its rounding points (oracle/cpu_ref_mixed.py), the bars of
    test_mixed_precision_training_mode: loss within 0.2 %, every gradient within 2 % of the emulation's (relative to its norm)."""
    l_em, _, g_em = train_oracle_mixed(name)
    loss, grads = train_step_on_device(name, "bf16", monkeypatch)
    gnorm = float(torch.cat([g.double().flatten() for g in g_em.values()]).norm())
    worst = ("", 0.0)
    for key, gb in grads.items():
        assert torch.isfinite(gb).all(), key
        ge = g_em[key].double()
        if float(ge.norm()) > 1e-6 * gnorm:
            worst = max(worst, (key, float((gb - ge).norm() / ge.norm())), key=lambda x: x[1])
    print(f"RANGE train {name} bf16 vs the CPU emulation: loss {loss:.6f} / {float(l_em):.6f}, worst gradient {worst[0]} {worst[1]:.4f}")
    assert abs(loss - float(l_em)) < 2e-3 * abs(float(l_em)), (loss, float(l_em))
    assert worst[1] < 0.02, worst
