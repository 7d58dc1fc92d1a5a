"""The tail-operand block of the fused edge stages (namp_kernels.h: EDGE_OPS_OFF, TOP_*) at the smallest shapes where staging can go wrong.

The fp32-class edge launches with the 4- / 8-row residue tail copy the tail's small operands (LayerNorm weights, b_in, b_out, m3_b, the
message b2, the bias row of every projection) to LDS when the stage starts; mask words, tokens and token rows are still read per residue.
What can go wrong is which vector lands where and who reads it: a partly filled last workgroup, workgroups whose residues belong to
different complexes, projections with and without a bias or a token table (tokens at the ends of the table), masked residues, a null
logits output, and the capacity of the bias rows (8 blocks at four decoder layers).  Every case, for "fp32" and "x3":

  * log-probs against oracle/cpu_ref.encdec_from_graph within 1e-3, h_V / h_E within 2e-4 (the bars of tests/test_gpu_parity.py), for
    namp_encdec_fwd and for namp_encoder_fwd + namp_decoder_fwd;
  * equal bits: namp_encdec_fwd with and without logits; the persistent launch against the launch chain where the library has a persistent
    form (3 + 3 layers, at most four residues per workgroup); the encoder outputs h_V / h_E of the one call and of the two calls in exact fp32.

The one call and the two calls do NOT give equal log-probs bit for bit, before this block existed or after it: the two-call decoder takes its
layer-0 tables from node_linear (16x16x4 MFMA order), the one call from the last encoder tail (4x4x1 MFMA order), and the split-bf16 encoder
of the two calls evaluates its residue tables differently.  Measured on all 36 cases here, with the same figures before and after the
block: fp32 differs in log_probs only (<= 1.9e-6), x3 in h_V (<= 2.3e-5), h_E (<= 4.0e-5) and log_probs (<= 3.0e-5).  They are held to
the oracle's bars and to each other within the same bars instead.

K may exceed N here (neighbour lists with repeats): the per-workgroup residue count is set by K alone (12 waves / ceil(K / 16) tiles), and
K = 33 .. 48 gives the four-residue tail, K = 17 .. 32 the six-residue one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, synth
from na_mpnn_amd.pack import PackedWeights
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_LOGP = 1e-3
TOL_ACT = 2e-4
VOCAB = 33


def stream():
    return hip.current_stream()


def _ln_rows(x):
    mu = x.mean(-1, keepdims=True)
    return ((x - mu) / np.sqrt(x.var(-1, keepdims=True) + 1e-5)).astype(np.float32)


def make_case(B, N, K, tokens, mask_mode, seed):
    rng = np.random.default_rng(seed)
    g = {"V": _ln_rows(rng.standard_normal((B, N, 128))), "E": _ln_rows(rng.standard_normal((B, N, K, 128))),
         "E_idx": rng.integers(0, N, (B, N, K)).astype(np.int32)}
    if tokens == "zeros":
        S = np.zeros((B, N), np.int32)
    elif tokens == "last":
        S = np.full((B, N), VOCAB - 1, np.int32)
    else:
        S = rng.integers(0, VOCAB, (B, N)).astype(np.int32)
        S.flat[0], S.flat[-1] = VOCAB - 1, 0
    mask = np.ones((B, N), np.int32)
    if mask_mode == "half":                       # about half masked, and the last residue — inside the partly filled workgroup — among them
        mask[rng.random((B, N)) < 0.5] = 0
        mask[-1, -1] = 0
        mask[0, 0] = 1
    elif mask_mode == "complex":                  # the last complex fully masked
        mask[-1] = 0
    g.update(S=S, mask=mask, chain_mask=np.ones((B, N), np.int32), randn=rng.standard_normal((B, N)).astype(np.float32))
    return {k: torch.from_numpy(v) for k, v in g.items()}


_models = {}


def model(depth, dev):
    """(weights on the host, PackedWeights) per (n_enc, n_dec): built once, shared."""
    if depth not in _models:
        w = {k: torch.from_numpy(v) for k, v in synth.make_weights(0, depth[0], depth[1]).items()}
        _models[depth] = (w, PackedWeights({k: v.to(dev) for k, v in w.items()}, depth[0], depth[1], VOCAB, dev))
    return _models[depth]


def run_joint(L, P, d, rank, B, N, K, want_logits, dev):
    hV = torch.full((B, N, 128), float("nan"), device=dev)
    hE = torch.full((B, N, K, 128), float("nan"), device=dev)
    logp = torch.full((B, N, VOCAB), float("nan"), device=dev)
    logits = torch.full((B, N, VOCAB), float("nan"), device=dev) if want_logits else None
    ws = torch.full((2 * L.namp_workspace_bytes(B, B, N, K),), 0xCD, dtype=torch.uint8, device=dev)     # poisoned barrier state
    hip.check(L.namp_encdec_fwd(P.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(),
                                d["S"].data_ptr(), rank.data_ptr(), hV.data_ptr(), hE.data_ptr(), logp.data_ptr(),
                                logits.data_ptr() if want_logits else None, ws.data_ptr(), ws.numel(), B, N, K, stream()))
    torch.cuda.synchronize()
    return hV, hE, logp, logits, ws


def run_separate(L, P, d, rank, B, N, K, dev):
    hV = torch.full((B, N, 128), float("nan"), device=dev)
    hE = torch.full((B, N, K, 128), float("nan"), device=dev)
    logp = torch.full((B, N, VOCAB), float("nan"), device=dev)
    ws = torch.empty(2 * L.namp_workspace_bytes(B, B, N, K), dtype=torch.uint8, device=dev)
    hip.check(L.namp_encoder_fwd(P.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(),
                                 hV.data_ptr(), hE.data_ptr(), ws.data_ptr(), ws.numel(), B, N, K, stream()))
    hip.check(L.namp_decoder_fwd(P.model(), hV.data_ptr(), hE.data_ptr(), d["E_idx"].data_ptr(), d["S"].data_ptr(), d["mask"].data_ptr(),
                                 rank.data_ptr(), logp.data_ptr(), None, None, ws.data_ptr(), ws.numel(), B, B, N, K, stream()))
    torch.cuda.synchronize()
    return hV, hE, logp


# (B, N, K, tokens, mask, (n_enc, n_dec))
CASES = [
    # partly filled last workgroup, four residues per workgroup (N below one workgroup included)
    (1, 5, 48, "mixed", "none", (3, 3)), (1, 3, 40, "mixed", "none", (3, 3)), (1, 7, 33, "mixed", "none", (3, 3)),
    (1, 5, 48, "mixed", "half", (3, 3)), (1, 7, 33, "zeros", "none", (3, 3)), (1, 7, 33, "last", "none", (3, 3)),
    # six residues per workgroup (the 8-row tail)
    (1, 9, 32, "mixed", "none", (3, 3)), (1, 13, 17, "mixed", "none", (3, 3)), (1, 13, 17, "last", "half", (3, 3)),
    (1, 13, 17, "zeros", "none", (3, 3)),
    # workgroups that straddle complexes: token rows and mask words of different complexes in one workgroup
    (2, 7, 48, "mixed", "none", (3, 3)), (2, 7, 48, "last", "complex", (3, 3)), (3, 5, 20, "mixed", "half", (3, 3)),
    (3, 5, 20, "zeros", "complex", (3, 3)),
    # depths: four decoder layers = 8 projection blocks in the last encoder tail (the capacity of the staged bias rows); one decoder layer
    (1, 7, 33, "mixed", "half", (3, 4)), (1, 9, 32, "mixed", "none", (3, 4)), (2, 7, 48, "mixed", "none", (3, 1)),
    (1, 13, 17, "mixed", "half", (3, 1)),
]


@pytest.mark.parametrize("prec", ["fp32", "x3"])
@pytest.mark.parametrize("B,N,K,tokens,mask_mode,depth", CASES,
                         ids=[f"b{c[0]}n{c[1]}k{c[2]}-{c[3]}-{c[4]}-{c[5][0]}x{c[5][1]}" for c in CASES])
def test_staged_tail_operands(B, N, K, tokens, mask_mode, depth, prec):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dev = torch.device("cuda:0")
    L = hip.lib()
    w, P = model(depth, dev)
    t = make_case(B, N, K, tokens, mask_mode, seed=7000 + 131 * B + 17 * N + K)
    d = {k: v.to(dev) for k, v in t.items()}
    order = torch.argsort((d["mask"] * d["chain_mask"] + 0.0001) * torch.abs(d["randn"]))
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(N, device=dev).expand(B, -1))
    rank = rank.to(torch.int32)

    prev = L.namp_set_persistent(0)
    P.set_precision(prec)
    try:
        hV, hE, logp, logits, _ = run_joint(L, P, d, rank, B, N, K, True, dev)
        hV2, hE2, logp2, _, _ = run_joint(L, P, d, rank, B, N, K, False, dev)
        hV3, hE3, logp3 = run_separate(L, P, d, rank, B, N, K, dev)
        pers = None
        if depth == (3, 3) and (K + 15) // 16 >= 3:           # the library's persistent form: 3 + 3 layers, <= 4 residues per workgroup
            L.namp_set_persistent(1)
            pers = run_joint(L, P, d, rank, B, N, K, True, dev)
            code = C.c_int32(-1)
            hip.check(L.namp_persistent_status(pers[4].data_ptr(), pers[4].numel(), B, N, K, C.byref(code)))
            assert code.value == 0, hex(code.value)
    finally:
        P.set_precision("x3")
        L.namp_set_persistent(prev)

    # one result, whichever way the call is made
    for name, a_, b_ in (("h_V", hV, hV2), ("h_E", hE, hE2), ("log_probs", logp, logp2)):
        assert torch.equal(a_, b_), f"{name}: with and without logits differ"
    if prec == "fp32":
        assert torch.equal(hV, hV3) and torch.equal(hE, hE3), "encoder outputs: namp_encdec_fwd and namp_encoder_fwd differ"
    print(f"tail operands {prec} B={B} N={N} K={K}: one call against two calls: |dh_V| {float((hV - hV3).abs().max()):.2e} "
          f"|dh_E| {float((hE - hE3).abs().max()):.2e} |dlogp| {float((logp - logp3).abs().max()):.2e}")
    for name, a_, b_, tol in (("h_V", hV, hV3, TOL_ACT), ("h_E", hE, hE3, TOL_ACT), ("log_probs", logp, logp3, TOL_LOGP)):
        assert float((a_ - b_).abs().max()) < tol, f"{name}: namp_encdec_fwd and encoder + decoder differ"
    if pers is not None:
        for name, a_, b_ in (("h_V", hV, pers[0]), ("h_E", hE, pers[1]), ("log_probs", logp, pers[2]), ("logits", logits, pers[3])):
            assert torch.equal(a_, b_), f"{name}: the persistent launch differs from the launch chain"

    # against the oracle
    rV, rE = cpu_ref.encode_from_graph(w, t["V"], t["E"], t["E_idx"].long(), t["mask"])
    ref = cpu_ref.encdec_from_graph(w, t["V"], t["E"], t["E_idx"].long(), t["S"], t["mask"], t["chain_mask"], t["randn"])
    valid = t["mask"].bool()
    assert torch.isfinite(logp).all() and torch.isfinite(logits).all() and torch.isfinite(logp3).all()
    d_v = max(float((x.cpu().double() - rV.double()).abs().max()) for x in (hV, hV3))
    d_e = max(float((x.cpu().double() - rE.double()).abs().max()) for x in (hE, hE3))
    d_lp = max(float((x.cpu().double()[valid] - ref["log_probs"].double()[valid]).abs().max()) for x in (logp, logp3)) if valid.any() else 0.0
    print(f"tail operands {prec} B={B} N={N} K={K} {tokens} {mask_mode} {depth}: |dh_V| {d_v:.2e} |dh_E| {d_e:.2e} |dlogp| {d_lp:.2e}")
    assert d_v < TOL_ACT and d_e < TOL_ACT, (d_v, d_e)
    assert d_lp < TOL_LOGP, d_lp
    # log_softmax of the logits is the log-probs the call returns
    assert float((torch.log_softmax(logits, -1) - logp).abs().max()) < 1e-5
