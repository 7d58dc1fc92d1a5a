"""CPU premises of the exactly-solvable-weights tests (tests/solvable.py, tests/test_gpu_solvable.py): the staged emulation is the oracle's
function, the weights are what they claim, the network they give is not degenerate, the reference's own tie rate (fp32 against fp64
arithmetic) leaves the GPU bars far below what one misplaced rounding point moves, and the emulation is sensitive to a dropped bias, a moved
rounding point and a swapped channel block."""
import functools

import numpy as np
import pytest
import torch

import solvable as sv
from oracle import cpu_ref

torch.set_grad_enabled(False)
F64 = torch.float64
H = sv.H


@functools.lru_cache(maxsize=None)
def small_graph():
    return sv.solvable_graph("small")


# ----------------------------------------------------------------------------------------------------------------------------------------
# (a) the restatement is the oracle's function
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [(1, 1), (3, 3), (2, 1)])
@pytest.mark.parametrize("variant", ["base", "zero_bias"])
def test_emulation_without_roundings_is_the_oracle(variant, nl):
    """Every rounding point off, exact-erf GELU, fp64: h_V, h_E and the log-probs of cpu_ref on the same weights and graph within 1e-10 —
    the hoisted first-layer tables, layer 3 behind the K-sum and the implicit decoder context are the reference's function."""
    w = sv.solvable_weights(0, nl[0], nl[1], variant)
    g = small_graph()
    wt = {k: torch.from_numpy(v).double() for k, v in w.items()}
    V, E, idx, mask = g["V"].double(), g["E"].double(), g["E_idx"].long(), g["mask"].double()
    hV, hE = cpu_ref.encode_from_graph(wt, V, E, idx, mask)
    ref = cpu_ref.score_from_encoded(wt, hV, hE, idx, g["S"], mask, g["chain_mask"].double(), g["randn"])
    em = sv.emulate(w, g, {"gelu.edge": "erf"}, F64)
    assert torch.equal(em["decoding_order"][0], ref["decoding_order"])
    for name, a, b in (("h_V", em["h_V"], hV), ("h_E", em["h_E"], hE), ("log_probs", em["log_probs"], ref["log_probs"])):
        assert a.dtype == F64 and float((a - b).abs().max()) < 1e-10, (name, float((a - b).abs().max()))
    assert sv.FORMS["fp32"] == {"gelu.edge": "erf"}


def test_fp64_rounding_helpers():
    """round_bf16 on fp64 bit patterns is round-to-nearest-even onto the bf16 grid (equal to torch's fp32 -> bf16 cast on every fp32 value,
    ties and negative values included); x3 keeps 16 bits; the polynomial GELU is within its documented 1.4e-3 of the exact form."""
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(200000, generator=g) * 4, torch.tensor([0.0, -0.0, 1.00390625, 1.01171875, -1.00390625, -3.0234375, 2.0 ** -20])])
    assert torch.equal(sv.round_bf16(x.double()).float(), x.to(torch.bfloat16).float())
    assert torch.equal(sv.round_bf16(x.double()), sv.round_bf16(sv.round_bf16(x.double())))
    assert float(((sv.round_x3(x.double()) - x.double()).abs() / x.double().abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    xs = torch.linspace(-14, 14, 56001, dtype=F64)
    assert float((sv.gelu_poly(xs) - torch.nn.functional.gelu(xs)).abs().max()) <= 1.4e-3


# ----------------------------------------------------------------------------------------------------------------------------------------
# (b) the weights are what they claim
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_weights_are_exactly_solvable():
    base = sv.solvable_weights(0, 3, 3, "base")
    ref = sv.synth.make_weights(0, 3, 3)
    assert set(base) == set(ref)
    used_blocks = {}
    for key, W in base.items():
        if key not in sv.replaced_keys(base):
            assert np.array_equal(W, ref[key]), key                  # biases, LayerNorm parameters, features.*: untouched
            continue
        if key == "W_s.weight":
            assert np.array_equal(W * 64.0, np.round(W * 64.0)) and np.abs(W).max() > 0
            continue
        blocks = [W[:, c:c + H] for c in range(0, W.shape[1], H)] if W.shape[0] == H and not key.endswith("dense.W_out.weight") else [W]
        for blk in blocks:
            assert int((blk != 0).sum(1).max()) <= 1 and int((blk != 0).sum(1).min()) == 1, key
            assert set(np.unique(blk[blk != 0]).tolist()) <= set(sv.VALUES), key
        if W.shape[0] == W.shape[1] or (W.shape[0] == H and not key.endswith("dense.W_out.weight")):
            for blk in blocks:
                assert int((blk != 0).sum(0).max()) == 1, key             # a permutation: every input is used once
        if key.endswith("dense.W_out.weight"):
            used_blocks[key] = set((np.nonzero(W)[1] // H).tolist())
    assert used_blocks and all(v == {0, 1, 2, 3} for v in used_blocks.values()), used_blocks
    vals = np.concatenate([W[W != 0] for k, W in base.items() if k in sv.replaced_keys(base) and k != "W_s.weight"])
    assert set(np.unique(vals).tolist()) == set(sv.VALUES)               # both signs, both scales
    zb, zm = sv.solvable_weights(0, 3, 3, "zero_bias"), sv.solvable_weights(0, 3, 3, "zero_matrix")
    for key in base:
        lin_bias = key.endswith(".bias") and "norm" not in key and not key.startswith("features.")
        assert np.array_equal(zb[key], np.zeros_like(base[key]) if lin_bias else base[key]), key
        assert np.array_equal(zm[key], np.zeros_like(base[key]) if key in sv.replaced_keys(base) else base[key]), key
    assert sum(k.endswith(".bias") and "norm" not in k and not k.startswith("features.") for k in base) == 3 + 5 * 3 + 8 * 3
    # V, E and W_s survive a bf16 round trip
    for shape in sv.SHAPES:
        g = sv.solvable_graph(shape)
        assert tuple(g["E"].shape[:3]) == sv.SHAPES[shape]
        for k in ("V", "E"):
            assert torch.equal(g[k].to(torch.bfloat16).float(), g[k])
        assert 0.05 < 1.0 - float(g["mask"].float().mean()) < 0.15
    ws = torch.from_numpy(base["W_s.weight"])
    assert torch.equal(ws.to(torch.bfloat16).float(), ws)


# ----------------------------------------------------------------------------------------------------------------------------------------
# (c) the network is not degenerate
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [(1, 1), (3, 3)])
@pytest.mark.parametrize("variant", ["base", "zero_bias"])
def test_network_is_not_degenerate(variant, nl):
    g = small_graph()
    out = sv.emulate(sv.solvable_weights(0, nl[0], nl[1], variant), g, "fp32", F64)
    valid = g["mask"].bool()
    lp = out["log_probs"][valid]
    entropy = float(-(lp.exp() * lp).sum(-1).mean())
    tokens = len(set(lp.argmax(-1).tolist()))
    std = float(out["h_V"][valid].std())
    print(f"SOLVABLE {variant} {nl}: mean row entropy {entropy:.2f} nats, {tokens} distinct arg-max tokens, h_V std {std:.2f}, "
          f"max |h_V| {float(out['h_V'].abs().max()):.1f}, max |h_E| {float(out['h_E'].abs().max()):.1f}, min log p {float(lp.min()):.1f}")
    assert 1.0 <= entropy <= 3.4 and tokens >= 8 and 0.3 <= std <= 3.0


# ----------------------------------------------------------------------------------------------------------------------------------------
# (d) the reference's own tie rate, and the bars derived from it
# ----------------------------------------------------------------------------------------------------------------------------------------
def reference_figures(variant, nl, shape, form):
    """{observable: (share, max in units of 2^-8 max|ref|)} of emulate in fp32 against fp64, and the fp64 outputs."""
    w, g = sv.solvable_weights(0, nl[0], nl[1], variant), sv.solvable_graph(shape)
    valid = g["mask"].bool()
    e64, e32 = sv.emulate(w, g, form, F64), sv.emulate(w, g, form, torch.float32)
    return {k: sv.figures(sv.select(e32, k, valid), sv.select(e64, k, valid)) for k in sv.OBSERVABLES}, e64


def _premise_cases():
    seen, out = set(), []
    for variant, nl, shape, form, _ in sv.bf16_cases():
        key = (variant, nl, shape, sv.one_call_form(shape) if form == "one_call" else form)
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out + [c for c in sv.control_cases()]


@pytest.mark.parametrize("case", _premise_cases(), ids=sv.case_id)
def test_reference_tie_rate_and_derived_bars(case):
    """For every form and shape of the GPU tests: the share of elements of the fp32 evaluation of the emulation that differ from its fp64
    evaluation by more than 1e-5 max|ref|, and the largest difference in units of 2^-8 max|ref| — what fp32 arithmetic alone moves across
    bf16 ties.  The GPU bars are max(10 x share, 1e-3) and max(2 x largest, one bf16 step at the top of the range); a misplaced rounding
    point moves a quarter of a tensor's elements and more, so every share bar must stay a factor of 20 below 0.25."""
    variant, nl, shape, form = case
    figs, _ = reference_figures(variant, nl, shape, form)
    for k, (share, mx) in figs.items():
        bar_share, bar_max = sv.bars(share, mx)
        print(f"SOLVABLE reference {sv.case_id(case)} {k}: share {share:.2e}, largest {mx:.2f} units -> bars {bar_share:.2e} / {bar_max:.2f} units")
    for k, (share, mx) in figs.items():
        bar_share, bar_max = sv.bars(share, mx)
        assert bar_share * 20.0 <= 0.25, (k, share, bar_share)
        assert bar_max <= 4.0, (k, mx)          # ties move an element by one bf16 step of its own value: at most 2 units of 2^-8 max|ref|


@pytest.mark.parametrize("B,N,K", sv.MESSAGE_SHAPES)
def test_message_restatement_tie_rate_and_derived_bars(B, N, K):
    """The same premise for the namp_bf16s_message cases: the K-sum restatement's fp32 evaluation against its fp64 evaluation, both modes;
    the weight sums in the kernel's order are count x fp32(1/30) to fp32 rounding."""
    c = sv.message_case(B, N, K)
    for mode in (0, 1):
        ref = sv.message_restate(c, mode, F64)
        share, mx = sv.figures(sv.message_restate(c, mode, torch.float32), ref)
        bar_share, bar_max = sv.bars(share, mx)
        print(f"SOLVABLE reference bf16s_message mode {mode} B={B} N={N} K={K}: share {share:.2e}, largest {mx:.2f} units -> bars "
              f"{bar_share:.2e} / {bar_max:.2f} units")
        assert float(ref.abs().max()) > 1.0
        assert bar_share * 20.0 <= 0.25 and bar_max <= 4.0
        ws, count = sv.message_weight_sums(c, mode).double().sum(1), sv.message_attended(c, mode).double().sum(1)
        assert float((ws - count / 30.0).abs().max()) <= 2.0 ** -21 * (K / 30.0)


def test_one_call_forms_of_the_shapes():
    """What namp_encdec_fwd does with each shape under set_precision("bf16") on the 256 compute units of an MI355X: (3, 840, 17) is past
    the fused tail but its 420 edge workgroups (6 residues each) are not more than two per compute unit, so it keeps h_E in fp32;
    (3, 841, 33) (631 workgroups of 4 residues) and (4, 840, 17) (560 of 6) take the bf16 storage path."""
    assert [sv.one_call_form(s) for s in ("small", "large17", "large33", "wide17")] == \
        ["bf16_fused", "bf16_separate", "bf16_storage", "bf16_storage"]
    # the persistent single launch: (2, 120, 30) holds six residues per workgroup and does not qualify, (2, 120, 33) holds four
    assert [sv.persistent_eligible(s) for s in ("small", "small33", "large17")] == [False, True, False]
    assert sv.one_call_form("large17", cus=128) == "bf16_storage"


# ----------------------------------------------------------------------------------------------------------------------------------------
# (e) sensitivity of the emulation
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sensitivity_reference(form="bf16_storage"):
    return sv.emulate(sv.solvable_weights(0, 1, 1, "base"), small_graph(), form, F64)


def moved_shares(out, form="bf16_storage"):
    ref, valid = sensitivity_reference(form), small_graph()["mask"].bool()
    return {k: sv.figures(sv.select(out, k, valid), sv.select(ref, k, valid))[0] for k in sv.OBSERVABLES}


BIASES = ["W_v.bias", "W_e.bias", "W_out.bias", "encoder_layers.0.W1.bias", "encoder_layers.0.W2.bias", "encoder_layers.0.W3.bias",
          "encoder_layers.0.W11.bias", "encoder_layers.0.W12.bias", "encoder_layers.0.W13.bias", "encoder_layers.0.dense.W_in.bias",
          "encoder_layers.0.dense.W_out.bias", "decoder_layers.0.W1.bias", "decoder_layers.0.W2.bias", "decoder_layers.0.W3.bias",
          "decoder_layers.0.dense.W_in.bias", "decoder_layers.0.dense.W_out.bias"]


@pytest.mark.parametrize("key", BIASES)
def test_sensitivity_dropped_bias(key):
    w = sv.solvable_weights(0, 1, 1, "base")
    assert key in w and np.abs(w[key]).max() > 0
    w[key] = np.zeros_like(w[key])
    shares = moved_shares(sv.emulate(w, small_graph(), "bf16_storage", F64))
    print(f"SOLVABLE sensitivity, {key} dropped: {shares}")
    assert max(shares.values()) > 0.10, (key, shares)
    assert max(shares.values()) > 100 * sv.SHARE_FLOOR


S_, F_ = "bf16_storage", "bf16_fused"
MOVES = [(S_, "msg.a1", None), (S_, "msg.a2", "bf16"), (S_, "edge.a1", None), (S_, "edge.a2", None), (S_, "hE.store", None),
         (S_, "tab.store", None), (S_, "node.S", None), (S_, "node.x1", None), (S_, "node.hid", None), (S_, "node.proj", None),
         (S_, "first.h", None), (S_, "dec.first.h", None), (S_, "node.S", "x3"), (S_, "gelu.edge", "erf"), (S_, "first.V", None),
         (S_, "embed.E", None), (F_, "msg.hE", None), (F_, "edge.hE", None), (F_, "msg.a1", None), (F_, "msg.a2", "bf16"),
         (F_, "node.S", "bf16"), (F_, "hE.store", "bf16"), (F_, "tab.store", "bf16")]


@pytest.mark.parametrize("form,point,to", MOVES, ids=[f"{f}:{p}->{t}" for f, p, t in MOVES])
def test_sensitivity_moved_rounding_point(form, point, to):
    """One entry of a form's table changed (a rounding dropped, added, or weakened to split-bf16; the edge GELU's form): more than a tenth
    of some observable's elements move beyond 1e-5 max|ref|.  (V and E are bf16 values already: `first.V` and `embed.E` are no-ops on
    these inputs and are listed to show it; `msg.hE` / `edge.hE` are no-ops behind `hE.store` and are moved in the fused form's table.  A split-bf16 truncation
    (2^-17 relative) is below what the share resolves: the x3 entries of a table are read from the code, not confirmed by measurement.)"""
    table = dict(sv.FORMS[form])
    assert table.get(point) != to
    if to is None:
        del table[point]
    else:
        table[point] = to
    shares = moved_shares(sv.emulate(sv.solvable_weights(0, 1, 1, "base"), small_graph(), table, F64), form)
    print(f"SOLVABLE sensitivity, {form}: {point} -> {to}: {shares}")
    if point in ("first.V", "embed.E"):
        assert max(shares.values()) == 0.0
    else:
        assert max(shares.values()) > 0.10, (point, to, shares)


SWAPS = ["encoder_layers.0.W2.weight", "encoder_layers.0.W12.weight", "encoder_layers.0.W3.weight", "encoder_layers.0.dense.W_in.weight",
         "decoder_layers.0.W2.weight", "W_e.weight"]


@pytest.mark.parametrize("key", SWAPS)
def test_sensitivity_swapped_channel_blocks(key):
    """Input channels 0..15 and 16..31 of one matrix swapped (one 16-channel tile taken for another)."""
    w = sv.solvable_weights(0, 1, 1, "base")
    W = w[key].copy()
    W[:, 0:16], W[:, 16:32] = w[key][:, 16:32], w[key][:, 0:16]
    assert not np.array_equal(W, w[key])
    w[key] = W
    shares = moved_shares(sv.emulate(w, small_graph(), "bf16_storage", F64))
    print(f"SOLVABLE sensitivity, {key} blocks swapped: {shares}")
    assert max(shares.values()) > 0.10, (key, shares)
