"""Exactly solvable weights for the bf16 kernels, and a staged emulation of the graph path with named rounding points — TEST INFRASTRUCTURE.

With dense random weights every bf16 GEMM output carries the rounding noise of 128 products, so a kernel and an emulation of it agree only
statistically.  Here every weight matrix (per 128-wide input block) has at most ONE non-zero per output row, with a value in {+-1, +-0.5}:
every product is exact in bf16, every dot product has a single term, and an MFMA result depends neither on the precision mode nor on the
accumulation order.  What is left of a precision mode is deterministic: WHERE values are rounded (to bf16, or split-bf16 truncated), which
GELU form an edge MLP uses, and fp32 LayerNorms / softmax / K-sums.  `emulate` restates the graph path (encoder, decoder tables, decoder,
head) in the hoisted form the kernels evaluate (first-layer tables per residue, layer 3 behind the K-sum, implicit decoder context) with a
table of named rounding points per form (FORMS); evaluated in fp64 it must equal the kernels except on the sparse set of elements where a
value lies within fp32 rounding of a bf16 tie.  DESIGN.md section 2, "Exactly solvable weights", holds the table with the launches it was
read from."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from na_mpnn_amd import synth
from oracle import cpu_ref, cpu_ref_mixed

H = 128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = (1.0, -1.0, 0.5, -0.5)
VARIANTS = ("base", "zero_bias", "zero_matrix")
SHAPES = {"small": (2, 120, 30), "small33": (2, 120, 33), "large17": (3, 840, 17), "large33": (3, 841, 33), "wide17": (4, 840, 17)}    # (B, N, K)
MASKED_FRAC = 0.1


# ----------------------------------------------------------------------------------------------------------------------------------------
# weights and inputs
# ----------------------------------------------------------------------------------------------------------------------------------------
def _one_per_row(rng, n_out, n_in):
    """[n_out, n_in] with one non-zero per row from VALUES; a signed, scaled permutation when square, stacked permutations when taller."""
    if n_out <= n_in:
        cols = rng.permutation(n_in)[:n_out]
    else:
        cols = np.concatenate([rng.permutation(n_in) for _ in range(n_out // n_in)])
    W = np.zeros((n_out, n_in), np.float32)
    W[np.arange(n_out), cols] = rng.choice(VALUES, n_out)
    return W


def replaced_keys(w):
    return [k for k, v in w.items() if v.ndim == 2 and not k.startswith("features.")]


def solvable_weights(seed=0, n_enc=3, n_dec=3, variant="base"):
    """synth.make_weights(seed, n_enc, n_dec) with every matrix outside features.* replaced: each 128-wide input block of a [128, n] matrix
    by a signed permutation (+-1 / +-0.5), W_in and the head W_out by one non-zero per row, dense.W_out by one non-zero per row in a random
    one of its four hidden blocks, W_s rounded to multiples of 1/64.  Biases and LayerNorm parameters stay.  Variants: "zero_bias" (every
    Linear bias zero), "zero_matrix" (every replaced matrix zero: the outputs are functions of biases, masks and K-sum weights alone)."""
    assert variant in VARIANTS, variant
    w = synth.make_weights(seed, n_enc, n_dec)
    rng = np.random.default_rng(1000 + seed)
    for key in replaced_keys(w):
        n_out, n_in = w[key].shape
        if key == "W_s.weight":
            new = np.round(w[key] * 64.0) / 64.0
        elif key.endswith("dense.W_out.weight"):
            new = np.zeros((n_out, n_in), np.float32)
            new[np.arange(n_out), H * rng.integers(0, n_in // H, n_out) + rng.permutation(H)[:n_out]] = rng.choice(VALUES, n_out)
        elif n_in > H and n_out == H:
            new = np.concatenate([_one_per_row(rng, n_out, H) for _ in range(n_in // H)], 1)
        else:
            new = _one_per_row(rng, n_out, n_in)
        w[key] = (np.zeros_like(new) if variant == "zero_matrix" else new).astype(np.float32)
    if variant == "zero_bias":
        for key in w:
            if key.endswith(".bias") and ".norm" not in key and "norm_" not in key and not key.startswith("features."):
                w[key] = np.zeros_like(w[key])
    return w


def solvable_graph(shape, seed=0):
    """synth.make_graph at SHAPES[shape] with V and E rounded to bf16 and a masked fraction of 0.1, as torch CPU tensors."""
    B, N, K = SHAPES[shape]
    g = synth.make_graph(seed=5200 + 7 * seed + N + K, batch=B, n=N, k=K, masked_frac=MASKED_FRAC)
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    for k in ("V", "E"):
        t[k] = t[k].to(torch.bfloat16).to(torch.float32)
    return t


# ----------------------------------------------------------------------------------------------------------------------------------------
# roundings and GELU forms
# ----------------------------------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    """Round to nearest even onto the bf16 grid, in x's own dtype.  fp64 values are rounded directly (on the bit pattern: a detour through
    fp32 would round twice)."""
    if x.dtype == torch.float32:
        return x.to(torch.bfloat16).to(torch.float32)
    assert x.dtype == torch.float64
    bits = x.contiguous().view(torch.int64)
    bits = (bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)
    return bits.view(torch.float64)


def round_x3(x):
    """The split-bf16 operand: hi = bf16(x), mid = bf16(x - hi), value hi + mid (namp_device.h, split_x3)."""
    hi = round_bf16(x)
    return hi + round_bf16(x - hi)


ROUNDINGS = {None: lambda x: x, "bf16": round_bf16, "x3": round_x3}


def gelu4_constants():
    """Q0..Q4 of the bf16 mode's GELU polynomial, parsed from namp_device.h (no second copy of them)."""
    return cpu_ref_mixed.gelu4_constants()


def gelu_poly(x):
    """gelu4_bf16mode: x * clamp01(1/2 + x Q(x^2)), Q of degree 4."""
    q0, q1, q2, q3, q4 = gelu4_constants()
    t = x * x
    q = (((q4 * t + q3) * t + q2) * t + q1) * t + q0
    return x * torch.clamp(x * q + 0.5, 0.0, 1.0)


GELUS = {"erf": F.gelu, "poly": gelu_poly}

# ----------------------------------------------------------------------------------------------------------------------------------------
# the rounding points, per form.  A point that a form does not name is not rounded.
#   first.V     V, operand of W_v                                  first.h    h_V = W_v.V + b, operand of layer 0's W1a / W1c
#   embed.E     E, operand of W_e                                  hE.store   h_E as stored: after the embedding and after every LayerNorm 3
#   tab.store   every gathered first-layer table as stored (Pa, Pc, edge-update Pa / Pc, decoder Pa, Pbw, Pfw)
#   msg.hE / msg.a1 / msg.a2    message MLP: the h_E operand of W1b / W1e, gelu(z1) as the operand of W2, gelu(z2) in front of the K-sum
#   edge.hE / edge.a1 / edge.a2 edge update: the h_E operand of W11b (the residual takes the stored row), the operands of W12 and W13
#   node.S / node.x1 / node.hid / node.proj   residue update: the K-sum as the operand of W3, LayerNorm 1's rows as the operand of W_in,
#               gelu(hidden) as the operand of W_out, the new h_V as the operand of the next tables' projections
#   dec.first.h the encoder's h_V as the operand of the decoder's first tables (Pfw_l, layer 0's Pa / Pbw)
#   gelu.edge   the GELU of the per-edge MLPs ("erf" | "poly"); the residue update's FFN is exact-erf in every form
# ----------------------------------------------------------------------------------------------------------------------------------------
_EDGE_BF16 = {"gelu.edge": "poly", "msg.hE": "bf16", "msg.a1": "bf16", "edge.hE": "bf16", "edge.a1": "bf16", "edge.a2": "bf16"}
_NODE = ("node.S", "node.x1", "node.hid", "node.proj")
FORMS = {
    # exact fp32 everywhere
    "fp32": {"gelu.edge": "erf"},
    # split-bf16: the activation operand of every product that runs out of an x3 image, large-batch table (the fused small-batch launches
    # keep some residue-level products in exact fp32; 2^-17 relative, far below the controls' bars)
    "x3": dict({"gelu.edge": "erf", "first.V": "x3", "first.h": "x3", "embed.E": "x3", "dec.first.h": "x3", "msg.hE": "x3", "msg.a1": "x3",
                "edge.hE": "x3", "edge.a1": "x3", "edge.a2": "x3"}, **{p: "x3" for p in _NODE}),
    # set_precision("bf16"), at most NAMP_FUSED_TAIL_MAX_RESIDUES residues: bf16 per-edge products, everything per residue in exact fp32
    "bf16_fused": dict(_EDGE_BF16),
    # ... on a large batch through namp_encoder_fwd + namp_decoder_fwd: h_E and tables in fp32, the residue update on x3 images
    "bf16_separate": dict(_EDGE_BF16, **{p: "x3" for p in _NODE}),
    # ... on a large batch through namp_encdec_fwd (encdec_bf16_storage): h_E and the gathered tables stored as bf16, hi . hi residue products
    "bf16_storage": dict(_EDGE_BF16, **{p: "bf16" for p in _NODE},
                         **{"first.V": "bf16", "first.h": "bf16", "embed.E": "bf16", "hE.store": "bf16", "tab.store": "bf16",
                            "dec.first.h": "bf16"}),
}
POINTS = ("first.V", "first.h", "embed.E", "hE.store", "tab.store", "msg.hE", "msg.a1", "msg.a2", "edge.hE", "edge.a1", "edge.a2") + _NODE + \
    ("dec.first.h",)


class _Weights:
    """The state dict in `dtype`; a matrix block with at most one non-zero per row is applied as a gather (the same values as the dense
    product: every other term is an exact zero)."""

    def __init__(self, w, dtype):
        self.w = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(dtype) for k, v in w.items()}
        self.cache = {}

    def __getitem__(self, key):
        return self.w[key]

    def lin(self, x, key, c0=0, c1=None, bias=True):
        W = self.w[key + ".weight"]
        c1 = W.shape[1] if c1 is None else c1
        ck = (key, c0, c1)
        if ck not in self.cache:
            blk = W[:, c0:c1]
            nz = blk != 0
            if int(nz.sum(1).max()) <= 1:
                cols = nz.to(torch.int8).argmax(1)
                self.cache[ck] = (cols, blk[torch.arange(blk.shape[0]), cols])
            else:
                self.cache[ck] = (None, blk)
        cols, vals = self.cache[ck]
        y = x[..., cols] * vals if cols is not None else x @ vals.t()
        b = self.w.get(key + ".bias") if bias else None
        return y + b if b is not None else y

    def ln(self, x, key):
        return F.layer_norm(x, (x.size(-1),), self.w[key + ".weight"], self.w[key + ".bias"], 1e-5)


def emulate(weights, graph, form, dtype=torch.float64):
    """(V, E, E_idx, S, mask, ...) -> {"h_V", "h_E", "log_probs", "decoding_order"} in `dtype`, with the roundings and the edge GELU of
    `form`: a name in FORMS or such a table itself."""
    table = FORMS[form] if isinstance(form, str) else form
    unknown = set(table) - set(POINTS) - {"gelu.edge"}
    assert not unknown, unknown
    r = lambda name, x: ROUNDINGS[table.get(name)](x)
    gelu_e = GELUS[table.get("gelu.edge", "erf")]
    W = _Weights(weights, dtype)
    n_enc, n_dec = cpu_ref.n_layers(weights, "encoder"), cpu_ref.n_layers(weights, "decoder")
    V, E, idx = graph["V"].to(dtype), graph["E"].to(dtype), graph["E_idx"].long()
    mask = graph["mask"].to(dtype)
    K = idx.shape[-1]
    gat = lambda t: cpu_ref.gather_nodes(t, idx)

    def edge_mlp(p, n1, n2, pt, hE, Pa, Pj):
        z1 = W.lin(r(pt + ".hE", hE), p + n1, H, 2 * H, bias=False) + Pa.unsqueeze(-2) + Pj
        a1 = r(pt + ".a1", gelu_e(z1))
        return r(pt + ".a2", gelu_e(W.lin(a1, p + n2)))

    def node_update(p, hV, S, ws):
        dh = W.lin(r("node.S", S), p + "W3", bias=False) + ws.unsqueeze(-1) * W[p + "W3.bias"]
        x1 = W.ln(hV + dh, p + "norm1")
        hid = F.gelu(W.lin(r("node.x1", x1), p + "dense.W_in"))
        x2 = W.ln(x1 + W.lin(r("node.hid", hid), p + "dense.W_out"), p + "norm2")
        return mask.unsqueeze(-1) * x2

    with torch.no_grad():
        # ---- encoder
        hV = W.lin(r("first.V", V), "W_v")
        hE = r("hE.store", W.lin(r("embed.E", E), "W_e"))
        w_att = mask.unsqueeze(-1) * gat(mask.unsqueeze(-1)).squeeze(-1) / cpu_ref.SCALE
        hp = r("first.h", hV)
        for l in range(n_enc):
            p = f"encoder_layers.{l}."
            Pa = r("tab.store", W.lin(hp, p + "W1", 0, H))
            Pc = r("tab.store", W.lin(hp, p + "W1", 2 * H, 3 * H, bias=False))
            a2 = edge_mlp(p, "W1", "W2", "msg", hE, Pa, gat(Pc))
            hV = node_update(p, hV, (w_att.unsqueeze(-1) * a2).sum(-2), w_att.sum(-1))
            hp = r("node.proj", hV)
            ePa = r("tab.store", W.lin(hp, p + "W11", 0, H))
            ePc = r("tab.store", W.lin(hp, p + "W11", 2 * H, 3 * H, bias=False))
            a2 = edge_mlp(p, "W11", "W12", "edge", hE, ePa, gat(ePc))
            hE = r("hE.store", W.ln(hE + W.lin(a2, p + "W13"), p + "norm3"))
        hV_enc = hV
        # ---- decoder
        order = cpu_ref.decoding_order_of(graph["mask"] * graph["chain_mask"], graph["randn"])
        bw = cpu_ref.backward_mask(order, idx).to(dtype)
        S_tok = graph["S"].long()
        tok = lambda p: (W["W_s.weight"] @ W[p + "W1.weight"][:, 2 * H:3 * H].t())[S_tok]
        hp = r("dec.first.h", hV_enc)
        Pfw = [r("tab.store", W.lin(hp, f"decoder_layers.{l}.W1", 3 * H, 4 * H, bias=False)) for l in range(n_dec)]
        for l in range(n_dec):
            p = f"decoder_layers.{l}."
            Pa = r("tab.store", W.lin(hp, p + "W1", 0, H))
            Pbw = r("tab.store", W.lin(hp, p + "W1", 3 * H, 4 * H, bias=False) + tok(p))
            a2 = edge_mlp(p, "W1", "W2", "msg", hE, Pa, bw * gat(Pbw) + (1.0 - bw) * gat(Pfw[l]))
            hV = node_update(p, hV, a2.sum(-2) / cpu_ref.SCALE, torch.full(hV.shape[:2], K / cpu_ref.SCALE, dtype=dtype))
            hp = r("node.proj", hV)
        logits = W.lin(hV, "W_out")
        return {"h_V": hV_enc, "h_E": hE, "log_probs": F.log_softmax(logits, -1), "decoding_order": order}


# ----------------------------------------------------------------------------------------------------------------------------------------
# the two figures every comparison reports, and the bars derived from the reference's own
# ----------------------------------------------------------------------------------------------------------------------------------------
SHARE_EPS = 1e-5              # an element "differs" beyond this fraction of max |ref|
SHARE_FLOOR = 1e-3
SHARE_MARGIN = 10.0           # another operation order in fp32 (FMA contraction, Horner form, three-term sums): more chances to cross a tie
MAX_FLOOR_UNITS = 2.0         # 2^-7 max |ref| = one bf16 step at the top of the range, in units of 2^-8 max |ref|
OBSERVABLES = ("h_V", "h_E", "log_probs")


def figures(got, ref):
    """(share of elements with |got - ref| > 1e-5 max|ref|, largest difference in units of 2^-8 max|ref|); `ref` in fp64."""
    got, ref = got.double(), ref.double()
    scale = float(ref.abs().max())
    if ref.numel() == 0 or scale == 0.0:
        return 0.0, 0.0
    d = (got - ref).abs()
    return float((d > SHARE_EPS * scale).double().mean()), float(d.max()) / (scale / 256.0)


def bars(ref_share, ref_max_units):
    return max(SHARE_MARGIN * ref_share, SHARE_FLOOR), max(2.0 * ref_max_units, MAX_FLOOR_UNITS)


def select(out, key, valid):
    """The elements of observable `key` the shares are taken over: the unmasked residues' rows of h_V and the log-probs (a masked residue's
    are constants), every row of h_E (a masked residue's edges are updated like any other's)."""
    return out[key] if key == "h_E" else out[key][valid]


# ----------------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_solvable.py (tests/test_solvable_host.py measures the reference's own tie rate on the same list)
# ----------------------------------------------------------------------------------------------------------------------------------------
MI355X_CUS = 256
FUSED_TAIL_MAX_RESIDUES = 2500          # NAMP_FUSED_TAIL_MAX_RESIDUES (asserted against the library by the GPU tests)


def one_call_form(shape, cus=MI355X_CUS):
    """The form namp_encdec_fwd takes under set_precision("bf16") at SHAPES[shape] on a device of `cus` compute units (namp.hip: the bf16
    storage path needs more than NAMP_FUSED_TAIL_MAX_RESIDUES residues AND more edge workgroups than two per compute unit, a workgroup
    holding 12 // tiles-per-residue residues)."""
    B, N, K = SHAPES[shape]
    G, tpn = B * N, (K + 15) // 16
    grid = -(-G // max(12 // tpn, 1))
    if G <= FUSED_TAIL_MAX_RESIDUES:
        return "bf16_fused"
    return "bf16_storage" if grid > 2 * cus else "bf16_separate"


def bf16_cases():
    """(variant, (n_enc, n_dec), shape, form, joint); form "one_call" = whatever one_call_form gives on the device.  One-layer models on
    every variant, so that each stage is observable on its own; the three-layer model in every form on the zero-matrix variant (every
    bias path, the 1/30 weights and the table slots of all layers, exactly); with dense matrices, models of more layers where the
    reference's own tie rate leaves the bars meaningful ("Exactly solvable weights")."""
    out = []
    for variant in VARIANTS:
        out += [(variant, (1, 1), "small", "bf16_fused", False), (variant, (1, 1), "large17", "bf16_separate", False),
                (variant, (1, 1), "large33", "bf16_separate", False), (variant, (1, 1), "large17", "one_call", True),
                (variant, (1, 1), "large33", "one_call", True), (variant, (1, 1), "wide17", "one_call", True)]
    out += [("base", (3, 3), "small", "bf16_fused", False), ("base", (2, 2), "large33", "bf16_separate", False),
            ("base", (1, 2), "large33", "one_call", True)]
    out += [("zero_matrix", (3, 3), "small", "bf16_fused", False), ("zero_matrix", (3, 3), "large33", "bf16_separate", False),
            ("zero_matrix", (3, 3), "large33", "one_call", True), ("zero_matrix", (3, 3), "wide17", "one_call", True)]
    return out


def control_cases():
    """(variant, (n_enc, n_dec), shape, form): exact fp32 and split-bf16 on the same inputs, through the one-call path.  (2, 120, 33) —
    three tiles, four residues per workgroup, 60 workgroups — is a shape whose three-layer call may run as the persistent single launch."""
    return [("base", nl, shape, form) for nl in ((1, 1), (3, 3)) for shape in ("small", "large17") for form in ("fp32", "x3")] + \
        [("base", (3, 3), "small33", form) for form in ("fp32", "x3")]


def persistent_eligible(shape, cus=MI355X_CUS):
    """namp_encdec_fwd's condition for the persistent single launch besides 3 + 3 layers: at most four residues per edge workgroup and at
    most one workgroup per compute unit."""
    B, N, K = SHAPES[shape]
    npw = max(12 // ((K + 15) // 16), 1)
    return B * N <= FUSED_TAIL_MAX_RESIDUES and npw <= 4 and -(-B * N // npw) <= cus


def case_id(case):
    return "-".join(f"{x[0]}x{x[1]}" if isinstance(x, tuple) else str(x) for x in case)


# ----------------------------------------------------------------------------------------------------------------------------------------
# namp_bf16s_message on permutation weights: inputs, the restatement of its K-sums, its weight sums in the kernel's own order
# ----------------------------------------------------------------------------------------------------------------------------------------
MESSAGE_SHAPES = [(3, 333, 48), (2, 257, 30), (1, 75, 16), (5, 201, 70)]


def message_case(B, N, K):
    """CPU inputs of one namp_bf16s_message call: bf16 rows and tables, W1 / W2 as (column, value) of a signed permutation, random
    neighbour indices, 5 % masked residues, a decoding rank per residue."""
    G = B * N
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + K)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = {"B": B, "N": N, "K": K, "G": G, "tpn": (K + 15) // 16}
    c["hE"], c["Pa"], c["Pj0"], c["Pj1"] = rn(G * K, H).bfloat16(), rn(G, H).bfloat16(), rn(G, H).bfloat16(), rn(G, H).bfloat16()
    for n in ("1", "2"):
        c["c" + n], c["v" + n] = torch.randperm(H, generator=g), torch.tensor(VALUES)[torch.randint(0, 4, (H,), generator=g)]
    c["b2"] = rn(H) * 0.1
    c["idx"] = torch.randint(0, N, (B, N, K), generator=g).to(torch.int32)
    c["mask"] = (torch.rand(G, generator=g) > 0.05).to(torch.int32)
    c["rank"] = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32).contiguous()
    c["jg"] = torch.arange(B).repeat_interleave(N)[:, None] * N + c["idx"].view(G, K).long()          # [G, K] global neighbour rows
    return c


def message_attended(c, mode):
    """[G, K] 0 / 1: mask_i mask_j in the encoder mode, every neighbour in the decoder mode."""
    return (c["mask"][:, None] * c["mask"][c["jg"]]) if mode == 0 else torch.ones(c["G"], c["K"], dtype=torch.int32)


def message_restate(c, mode, dtype):
    """The K-sums [G, 128] of the layer-2 activations with the kernel's rounding points and its GELU polynomial, in `dtype`."""
    G, K, jg = c["G"], c["K"], c["jg"]
    x = c["hE"].to(dtype).view(G, K, H)
    if mode == 0:
        pj = c["Pj0"].to(dtype)[jg]
    else:
        bwd = (c["rank"].view(-1)[jg] < c["rank"].view(-1)[:, None])[..., None]
        pj = torch.where(bwd, c["Pj0"].to(dtype)[jg], c["Pj1"].to(dtype)[jg])
    z1 = x[..., c["c1"]] * c["v1"].to(dtype) + c["Pa"].to(dtype)[:, None, :] + pj
    a1 = round_bf16(gelu_poly(z1))
    a2 = gelu_poly(a1[..., c["c2"]] * c["v2"].to(dtype) + c["b2"].to(dtype))
    return ((message_attended(c, mode).to(dtype) / 30.0)[..., None] * a2).sum(1)


def message_weight_sums(c, mode):
    """[G, tpn] fp32: every 16-row tile's weight sum in the kernel's own order — rows weigh fp32(1/30) or 0 (padding rows too), summed by
    the xor-shuffle tree over 1, 2, 4, 8 lanes — so that the comparison can be exact."""
    G, K, tpn = c["G"], c["K"], c["tpn"]
    w = torch.zeros(G, tpn * 16, dtype=torch.float32)
    w[:, :K] = message_attended(c, mode).float() * torch.tensor(1.0 / 30.0, dtype=torch.float32)
    w = w.view(G, tpn, 16)
    lane = torch.arange(16)
    for o in (1, 2, 4, 8):
        w = w + w[..., lane ^ o]
    return w[..., 0].contiguous()
