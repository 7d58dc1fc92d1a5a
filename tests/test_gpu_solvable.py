"""GPU tests of the bf16 throughput mode on exactly solvable weights (tests/solvable.py): every weight matrix a signed, scaled permutation,
so that every product is exact in bf16 and an MFMA result depends neither on the precision mode nor on the accumulation order.  The
kernels must then equal the fp64 evaluation of an emulation that rounds where they round, except on the sparse set of elements that lie
within fp32 rounding of a bf16 tie — a missing bias, a wrong LayerNorm constant, a padding row in a K-sum or a misplaced rounding moves a
tenth of a tensor and more (tests/test_solvable_host.py).  Through PackedWeights and run_encdec like tests/test_gpu_range.py.

Bars, per observable (h_V, h_E, log-probs) and form, computed at run time from the emulation's own fp32-against-fp64 figures (premise (d)
of tests/test_solvable_host.py): the share of elements off by more than 1e-5 max|ref| at most max(10 x the reference's share, 1e-3); the
largest difference at most max(2 x the reference's largest, 2^-7 max|ref|).  Every test prints the kernel's figures beside the reference's."""
import ctypes as C
import functools
import importlib.util
import os

import pytest
import torch

import solvable as sv
from na_mpnn_amd import hip
from na_mpnn_amd.pack import PackedWeights
from test_gpu_parity import TOL_ACT, TOL_LOGP, run_encdec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
F64 = torch.float64
H = sv.H


@functools.lru_cache(maxsize=None)
def frag_perm():
    """position -> channel of the bf16 rows' fragment order B: the one statement of it, in tools/bf16s32_check.py."""
    spec_ = importlib.util.spec_from_file_location("bf16s32_check", os.path.join(sv.ROOT, "tools", "bf16s32_check.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod.frag_perm()


@functools.lru_cache(maxsize=None)
def packed(variant, nl):
    w = sv.solvable_weights(0, nl[0], nl[1], variant)
    return PackedWeights({k: torch.from_numpy(v).to(DEV) for k, v in w.items()}, nl[0], nl[1], 33, torch.device(DEV))


@functools.lru_cache(maxsize=None)
def inputs(shape):
    t = sv.solvable_graph(shape)
    return t, {k: v.to(DEV) for k, v in t.items()}


@functools.lru_cache(maxsize=2)
def reference(variant, nl, shape, form):
    """The fp64 emulation of one case, and per observable the fp32 evaluation's own (share, largest difference) against it."""
    w, t = sv.solvable_weights(0, nl[0], nl[1], variant), inputs(shape)[0]
    valid = t["mask"].bool()
    e64, e32 = sv.emulate(w, t, form, F64), sv.emulate(w, t, form, torch.float32)
    return e64, {k: sv.figures(sv.select(e32, k, valid), sv.select(e64, k, valid)) for k in sv.OBSERVABLES}


def unpermuted_bf16_rows(hE, rows):
    """The bf16 rows the storage path leaves in the first half of the caller's h_E buffer, in channel order, as fp32."""
    raw = hE.reshape(-1).view(torch.bfloat16)[:rows * H].view(rows, H)
    out = torch.empty_like(raw)
    out[:, frag_perm().to(raw.device)] = raw
    return out.float()


def check(tag, key, got, ref, ref_figs):
    share, mx = sv.figures(got, ref)
    bar_share, bar_max = sv.bars(*ref_figs)
    print(f"SOLVABLE {tag} {key}: kernel share {share:.2e} / largest {mx:.2f} units; reference (fp32 vs fp64) share {ref_figs[0]:.2e} / largest "
          f"{ref_figs[1]:.2f} units; bars {bar_share:.2e} / {bar_max:.2f} units")
    return share <= bar_share and mx <= bar_max


@pytest.mark.parametrize("case", sv.bf16_cases(), ids=sv.case_id)
def test_bf16_forms_against_the_emulation(case):
    """set_precision("bf16") on solvable weights against the fp64 emulation of the form the call takes: the fused small-batch launches
    (2 x 120, K = 30), the large-batch launches with h_E in fp32 (namp_encoder_fwd + namp_decoder_fwd; 3 x 840, K = 17: two tiles per
    residue with 15 padding rows; 3 x 841, K = 33: three tiles, an odd tile total) and the one-call path, which stores h_E and the
    gathered tables as bf16 where the batch has more edge workgroups than two per compute unit (3 x 841 x 33, 4 x 840 x 17 — not
    3 x 840 x 17 on 256 compute units: that call keeps h_E in fp32, and is held to that form).  Which path ran is asserted from the
    h_E buffer: bf16 rows in fragment order in its first half, or fp32 rows.  Masked residues' rows of h_V are exactly the emulation's.
    The three-layer model runs in every form with all matrices zero (no ties at any depth: every bias path, the 1/30 weights and the table
    slots of all layers, exactly); with dense matrices, the depths whose reference tie rate passes premise (d) (solvable.bf16_cases)."""
    variant, nl, shape, form, joint = case
    L = hip.lib()
    B, N, K = sv.SHAPES[shape]
    assert L.namp_fused_tail_max_residues() == sv.FUSED_TAIL_MAX_RESIDUES
    if form == "one_call":
        form = sv.one_call_form(shape, torch.cuda.get_device_properties(0).multi_processor_count)
    assert (B * N <= sv.FUSED_TAIL_MAX_RESIDUES) == (form == "bf16_fused")
    t, d = inputs(shape)
    ref, figs = reference(variant, nl, shape, form)
    valid = t["mask"].bool()
    P = packed(variant, nl)
    P.set_precision("bf16")
    try:
        hV, hE, logp, order = run_encdec(L, torch.device(DEV), P, d, B, N, K, joint)
    finally:
        P.set_precision("x3")
    tag = sv.case_id((variant, nl, shape, form, "joint" if joint else "separate"))
    hV, logp = hV.cpu(), logp.cpu()
    assert torch.isfinite(hV).all() and torch.isfinite(logp).all(), tag
    assert torch.equal(order.cpu(), ref["decoding_order"]), tag
    # which path ran: the buffer read as the OTHER format is nowhere near the emulation
    as_bf16 = unpermuted_bf16_rows(hE, B * N * K).view(B, N, K, H).cpu()
    as_fp32 = torch.nan_to_num(hE.cpu(), nan=0.0, posinf=0.0, neginf=0.0)
    hE_got, hE_other = (as_bf16, as_fp32) if form == "bf16_storage" else (as_fp32, as_bf16)
    # (all matrices zero: every h_E row is LayerNorm 3's bias, and the reading in the other format need not be far from it.  The path of
    # those cases rests on one_call_form — asserted on the other variants at the same shapes — and on the values below: fp32 rows read
    # as bf16 pairs, or the reverse, are garbage and fail the bars)
    if variant != "zero_matrix":
        assert sv.figures(hE_other, ref["h_E"])[0] > 0.25, (tag, "the h_E buffer does not hold what the intended path leaves there")
    ok = [check(tag, "h_V", hV[valid], ref["h_V"][valid], figs["h_V"]),
          check(tag, "h_E", hE_got, ref["h_E"], figs["h_E"]),
          check(tag, "log_probs", logp[valid], ref["log_probs"][valid], figs["log_probs"])]
    assert torch.equal(hV[~valid].double(), ref["h_V"][~valid]), tag               # masked residues: zero rows
    assert float(torch.logsumexp(logp.double(), -1).abs().max()) < 1e-5, tag
    assert all(ok), (tag, ok)


def run_one_call_persistent(L, P, d, B, N, K):
    """namp_encdec_fwd with the persistent single launch enabled, on a workspace whose barrier state is poisoned: returns the outputs, the
    timeout word (namp_persistent_status) and the top arrival counter.  The launch chain never touches those words, so a timeout
    word of 0 and a small arrival count there mean that the persistent kernel ran and no grid barrier gave up."""
    dev = torch.device(DEV)
    order = torch.argsort((d["mask"] * d["chain_mask"] + 0.0001) * torch.abs(d["randn"]))
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(N, device=dev).expand(B, -1))
    rank = rank.to(torch.int32)
    ws = torch.full((2 * L.namp_workspace_bytes(B, B, N, K),), 0xCD, dtype=torch.uint8, device=dev)
    hV = torch.full((B, N, H), float("nan"), device=dev)
    hE = torch.full((B, N, K, H), float("nan"), device=dev)
    logp = torch.full((B, N, 33), float("nan"), device=dev)
    prev = L.namp_set_persistent(1)
    try:
        hip.check(L.namp_encdec_fwd(P.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(),
                                    d["S"].data_ptr(), rank.data_ptr(), hV.data_ptr(), hE.data_ptr(), logp.data_ptr(), None,
                                    ws.data_ptr(), ws.numel(), B, N, K, hip.current_stream()))
        torch.cuda.synchronize()
    finally:
        L.namp_set_persistent(prev)
    code = C.c_int32(-1)
    hip.check(L.namp_persistent_status(ws.data_ptr(), ws.numel(), B, N, K, C.byref(code)))
    top = int(ws[:256].view(torch.int32)[8].item())
    return (hV, hE, logp, order), code.value, top


@pytest.mark.parametrize("case", sv.control_cases(), ids=sv.case_id)
def test_parity_modes_as_controls(case):
    """Exact fp32 and split-bf16 on the same weights and inputs through the one call, against the emulation without roundings (x3: with
    the split-bf16 truncations): the suite's own bars, 2e-4 on h_V / h_E and 1e-3 on log-probs.  A harness mistake (weights, inputs, the
    decoding order, the comparison) would show here.  The three-layer model at (2, 120, 33) — a shape that qualifies: four residues per
    edge workgroup, 60 workgroups — runs as the launch chain and as the persistent single launch; that the latter ran is asserted from the
    poisoned barrier words of the workspace (timeout word 0, the arrival counter re-initialised and counted up), as
    test_persistent_forward_equals_launch_chain does, and its outputs equal the chain's to the bit."""
    variant, nl, shape, form = case
    L = hip.lib()
    B, N, K = sv.SHAPES[shape]
    t, d = inputs(shape)
    ref, _ = reference(variant, nl, shape, form)
    valid = t["mask"].bool()
    P = packed(variant, nl)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    runs = []
    prev = L.namp_set_persistent(0)
    P.set_precision(form)
    try:
        runs.append(("chain", run_encdec(L, torch.device(DEV), P, d, B, N, K, True)))
        if shape == "small33":
            assert nl == (3, 3) and sv.persistent_eligible(shape, cus)
            out, code, top = run_one_call_persistent(L, P, d, B, N, K)
            print(f"SOLVABLE control {sv.case_id(case)}: persistent status {code:#x}, top arrival counter {top}")
            assert code == 0 and 0 < top <= 8 * 5, (hex(code & 0xFFFFFFFF), top)      # (poison: 0xCDCDCDCD; at most 8 groups x 5 barriers)
            for a_, b_, name in zip(out, runs[0][1], ("h_V", "h_E", "log_probs", "order")):
                assert torch.equal(a_, b_), name
            runs.append(("persistent", out))
    finally:
        P.set_precision("x3")
        L.namp_set_persistent(prev)
    for how, (hV, hE, logp, order) in runs:
        hV, hE, logp = hV.cpu().double(), hE.cpu().double(), logp.cpu().double()
        assert torch.equal(order.cpu(), ref["decoding_order"])
        d_hv, d_he = float((hV - ref["h_V"]).abs().max()), float((hE - ref["h_E"]).abs().max())
        d_lp = float((logp - ref["log_probs"])[valid].abs().max())
        print(f"SOLVABLE control {sv.case_id(case)} {how}: max|dh_V| = {d_hv:.2e}, max|dh_E| = {d_he:.2e}, max|dlogp| = {d_lp:.2e}")
        assert d_hv < TOL_ACT and d_he < TOL_ACT and d_lp < TOL_LOGP, (case, how, d_hv, d_he, d_lp)


@pytest.mark.parametrize("B,N,K", sv.MESSAGE_SHAPES)
def test_bf16_storage_message_kernel_on_solvable_weights(B, N, K):
    """namp_bf16s_message, both message modes, called as tools/bf16s32_check.py calls it, with W1 and W2 signed permutations and the
    restatement using the kernel's GELU polynomial (tests/solvable.py: message_case, message_restate): the K-sums of every residue
    (fp32 sums of up to 80 terms) against the fp64 restatement under the bars of this file, measured from the restatement's own fp32
    evaluation; every tile's weight sum EQUAL to its restatement in the kernel's order (rows of fp32(1/30) or 0 through the xor-shuffle
    tree).  Odd tile counts, K % 16 != 0 and random neighbour indices included."""
    L = hip.lib()
    dev = torch.device(DEV)
    c = sv.message_case(B, N, K)
    G, tpn = c["G"], c["tpn"]
    perm = frag_perm()
    dense = lambda cols, vals: torch.zeros(H, H).index_put_((torch.arange(H), cols), vals).contiguous().to(dev)
    W1, W2, b2 = dense(c["c1"], c["v1"]), dense(c["c2"], c["v2"]), c["b2"].to(dev).contiguous()
    i1 = torch.empty(H * H, dtype=torch.bfloat16, device=dev)
    i2 = torch.empty_like(i1)
    st = hip.current_stream()
    hip.check(L.namp_pack_image_bf16_32(W1.data_ptr(), H, 0, i1.data_ptr(), st))
    hip.check(L.namp_pack_image_bf16_32(W2.data_ptr(), H, 0, i2.data_ptr(), st))
    tb = [c[k][:, perm].contiguous().to(dev) for k in ("hE", "Pa", "Pj0", "Pj1")]
    idx_d, mask_d, rank_d = c["idx"].to(dev), c["mask"].to(dev), c["rank"].to(dev)
    for mode in (0, 1):
        part = torch.full((G * tpn * 129 + 4,), float("nan"), device=dev)
        hip.check(L.namp_bf16s_message(mode, tb[0].data_ptr(), idx_d.data_ptr(), mask_d.data_ptr(), rank_d.data_ptr(), tb[1].data_ptr(),
                                       tb[2].data_ptr(), tb[3].data_ptr(), i1.data_ptr(), i2.data_ptr(), b2.data_ptr(), part.data_ptr(),
                                       B, B, N, K, st), "bf16s_message")
        torch.cuda.synchronize()
        S = part[:G * tpn * H].view(G, tpn, H).sum(1).cpu()
        ws = part[G * tpn * H:G * tpn * 129].view(G, tpn).cpu()
        ref = sv.message_restate(c, mode, F64)
        ref_figs = sv.figures(sv.message_restate(c, mode, torch.float32), ref)
        assert float(ref.abs().max()) > 1.0
        ok = check(f"bf16s_message mode {mode} B={B} N={N} K={K}", "K-sums", S, ref, ref_figs)
        ws_ref = sv.message_weight_sums(c, mode)
        print(f"SOLVABLE bf16s_message mode {mode}: weight sums of {G * tpn} tiles, largest deviation from the restatement "
              f"{float((ws - ws_ref).abs().max()):.1e}")
        assert torch.equal(ws, ws_ref), mode
        assert ok, (mode, B, N, K)
