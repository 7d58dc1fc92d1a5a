"""Exactly solvable weights for the mixed-precision TRAINING kernels: an explicit forward and backward of every per-edge stage with named
rounding points — TEST INFRASTRUCTURE (the backward counterpart of tests/solvable.py).

Every 128 x 128 matrix is a signed permutation (+-1 / +-0.5): each forward product bf16(x) . W and each data-gradient product bf16(g) . W
has ONE exact term, so what is left of `train.X3 == 2` is deterministic — where h_E, the activations, gelu' and the gradients are rounded
to bf16 before a product, a contraction over the edge rows or a store, which GELU form a launch evaluates, and fp32 sums.  `restate` writes
that down per stage, forward AND backward by hand (it is not autograd of a rounded forward: a rounding has no derivative, and the kernels
round gradients too); evaluated in fp64 it must equal the kernels except at bf16 ties and in the last bits of the long fp32 sums.  The
tables were read off csrc/namp_train_dw.h (message stages), csrc/namp_train_eu.h (edge update), csrc/namp_train.h (the row-tensor forms,
the row contractions, the gather of table gradients) and train.py (what the host hands to which launch); DESIGN.md section 2, "Exactly
solvable weights: training", holds them with the measured figures."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from na_mpnn_amd import synth
from oracle import cpu_ref
from solvable import H, _one_per_row, round_bf16, round_x3, gelu4_constants, figures, bars

ROUNDINGS = {None: lambda x: x, "bf16": round_bf16, "x3": round_x3}
MI355X_CUS = 256
ROUND_ROWS = 64                       # DW_ROWS: edge rows per round of a persistent workgroup
# (B, N, K): 10 rounds (most workgroups idle); 262.5 rounds (two rounds for some workgroups on 256 CUs, a ragged last round, K % 16 != 0);
# 1,050 rounds (several rounds per workgroup, K % 16 == 0, B > 1)
SHAPES = {"idle": (1, 40, 16), "ragged": (1, 560, 30), "multi": (2, 700, 48)}
STAGES = ("enc_msg", "dec_msg", "edge_update", "edge_linear", "embed_tail")
# The feature weight gradient runs as the chain edge_embedding -> _EdgeEmbedTail on a synthetic complex (synth.make_complex): its upstream
# gradient is the tail's dL/dy, handed over as bf16 operand tiles.  B complexes of N residues per case; the [E, 5200] feature rows of the
# restatement are regenerated FEAT_CHUNK edge rows at a time (dWf and the positional gradients are sums over edge rows), never held whole.
FEAT_STAGE = "feat_wgrad"
FEAT_SHAPES = ("idle", "ragged", "multi")
FEAT_CHUNK = 4096
MASKED_FRAC = 0.15
SEED_DROP = 4321


# ----------------------------------------------------------------------------------------------------------------------------------------
# the training path's counter-based dropout mask
# ----------------------------------------------------------------------------------------------------------------------------------------
def _mix32(x):
    """mix32 of csrc/namp_device.h on int64 tensors holding uint32 values."""
    M = 0xFFFFFFFF
    x = x ^ (x >> 16); x = (x * 0x7feb352d) & M
    x = x ^ (x >> 15); x = (x * 0x846ca68b) & M
    return x ^ (x >> 16)


def hash_dropout_factor(seed, E, p, dev):
    """The training path's counter-based dropout mask (drop_row_key / drop_factor, csrc/namp_device.h) restated in torch: [E,128] of
    0 or 1 / (1 - p).  Edge rows < 2^32, so the key's high-word term is mix32(0x9E3779B9)."""
    M = 0xFFFFFFFF
    e = torch.arange(E, device=dev, dtype=torch.int64)
    hi = _mix32(torch.full((1,), 0x9E3779B9, device=dev, dtype=torch.int64))
    key = _mix32((int(seed) & M) ^ e ^ hi)
    ch = torch.arange(128, device=dev, dtype=torch.int64)
    h = _mix32((key[:, None] + ch[None, :] * 0x9E3779B9) & M)
    thresh = int(float(p) * 4294967296.0)
    return (h >= thresh).double() / (1.0 - p)


# ----------------------------------------------------------------------------------------------------------------------------------------
# GELU forms: value and derivative
# ----------------------------------------------------------------------------------------------------------------------------------------
def _phi(x):
    return torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def _Phi_poly(x):
    q0, q1, q2, q3, q4 = gelu4_constants()
    t = x * x
    q = (((q4 * t + q3) * t + q2) * t + q1) * t + q0
    return torch.clamp(x * q + 0.5, 0.0, 1.0)


def _Phi_erf(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _Phi_as(x):
    """Phi of gelu_val_grad (csrc/namp_train.h): erf by Abramowitz-Stegun 7.1.26 with the kernel's fp32 constants, |error| <= 1.5e-7 —
    small, but four times what fp32 arithmetic leaves, and so visible as bf16 tie crossings of everything that is rounded behind it."""
    f = lambda v: float(np.float32(v))
    v = x * f(0.84932180028801904)
    e = torch.exp2(-(v * v))
    t = 1.0 / (v.abs() * f(0.27273943) + 1.0)
    q = (((f(1.061405429) * t + f(-1.453152027)) * t + f(1.421413741)) * t + f(-0.284496736)) * t + f(0.254829592)
    y = 1.0 - (q * t) * e
    return 0.5 + torch.where(x < 0, -0.5, 0.5) * y


def gelu_val_grad(x, form):
    """(gelu(x), gelu'(x)).  "poly": dw_gelu_split4_bf16 — value x Phi with the clamped degree-4 Phi of the bf16 mode, derivative that Phi
    plus x phi with phi exact (NOT the derivative of the polynomial).  "erf": the exact form.  "as": the row-tensor launches' form, the
    exact one but for the Abramowitz-Stegun erf.  "poly_erf_phi": a seeded fault — the polynomial's value with the exact Phi inside the
    derivative."""
    if form == "poly":
        P = _Phi_poly(x)
        return x * P, P + x * _phi(x)
    if form == "erf":
        P = _Phi_erf(x)
        return x * P, P + x * _phi(x)
    if form == "as":
        P = _Phi_as(x)
        return x * P, P + x * _phi(x)
    assert form == "poly_erf_phi", form
    return x * _Phi_poly(x), _Phi_erf(x) + x * _phi(x)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the rounding points.  A point that a table does not name is not rounded.
#   fwd.hE    h_E as the operand of W1b / W11b (the edge update's residual takes the fp32 row)      fwd.x   x as the operand of W_e (embed_tail:
#             x = LayerNorm(y))
#   fwd.a1    gelu(z1) as the operand of W2 / W12, in the forward launch and in every recomputation
#   fwd.a2    edge update: gelu(z2) as the operand of W13
#   fwd.S     message stages: the K-sum of gelu(z2) as the operand of W3 (node_linear_kernel, split-bf16 products in the mixed mode too)
#   bwd.g     message stages: dL/d(out) as the operand of W3^T (the same launch, transposed image);  edge_linear: g as the operand of W_e^T
#   bwd.d2    gelu'(z2) as it multiplies W3^T g3 (edge update: packed to bf16 across the LayerNorm; message stages: fp32 registers)
#   bwd.d1    gelu'(z1) as it multiplies W2^T g2 (packed to bf16 across the second product)
#   bwd.g3    edge update: dL/dz3 as the operand of W13^T and of the dW13 / db13 contraction
#   bwd.g2    dL/dz2 as the operand of W2^T and of the dW2 / db2 contraction (edge update: the bf16 G2 rows between the two launches)
#   bwd.g1    dL/dz1 as the operand of W1b^T, of the dW1b contraction, and as stored in the bf16 G1 rows the gather of dL/dPj reads
#   dPa.g1    dL/dz1 as summed over k into dL/dPa — fp32 registers in every form: never rounded (named so that a fault can round it)
#   dW3.g / dW3.S   message stages: the two operands of the residue-level contraction dW3 = g^T S (wgrad_x3_multi_kernel<MID = false>)
#   dW3.a2 / dW2.a1 / dW1.hE / dW.x   the activation operand of a contraction over edge rows (the gradient operand is bwd.g3 / g2 / g1)
#   dW.g      edge_linear: g as the operand of dW_e (its bias gradient sums the fp32 rows)
#   featW.g / featW.x   dL/dy (the tail's bf16 tiles) and the regenerated [positional | RBF] features as operands of the 5200 -> 128 weight gradient
#   gelu.fwd / gelu.bwd   the GELU of the forward launch / of the backward launch's recomputation
# ----------------------------------------------------------------------------------------------------------------------------------------
_MIXED_COMMON = {"gelu.fwd": "poly", "fwd.hE": "bf16", "fwd.a1": "bf16", "bwd.g2": "bf16", "bwd.g1": "bf16", "dW2.a1": "bf16", "dW1.hE": "bf16"}
TABLES = {
    # train.X3 == 2, DW_ONCHIP (and DW_ONCHIP_EDGE): edge_bwd_dw16_kernel; edge_update_bwd_a16_kernel + edge_update_bwd_b16_kernel
    "mixed": {
        "enc_msg": dict(_MIXED_COMMON, **{"gelu.bwd": "poly", "fwd.S": "x3", "bwd.g": "x3", "dW3.g": "bf16", "dW3.S": "bf16", "bwd.d1": "bf16"}),
        "edge_update": dict(_MIXED_COMMON, **{"gelu.bwd": "poly", "fwd.a2": "bf16", "bwd.g3": "bf16", "dW3.a2": "bf16", "bwd.d2": "bf16",
                                              "bwd.d1": "bf16"}),
        "edge_linear": {"fwd.x": "bf16", "bwd.g": "bf16", "dW.g": "bf16", "dW.x": "bf16"},
        # _EdgeEmbedTail (edge_mlp_kernel<MODE_EMBED> with the LayerNorm in front, embed_ln_bwd_kernel<2>, wgrad_x3_ln_kernel<false>): the same four
        # points with x = LayerNorm(y), which both launches re-derive from y in fp32; the LayerNorm's own backward and its sums stay fp32
        "embed_tail": {"fwd.x": "bf16", "bwd.g": "bf16", "dW.g": "bf16", "dW.x": "bf16"},
        # ... followed by namp_train_feat_wgrad on the tail's bf16 tiles of dL/dy (feat_wgrad_t16_kernel: hi . hi products, the 5184 RBF and
        # 16 positional features regenerated in fp32 and rounded to bf16 as MFMA operands) and namp_train_pos_grad (exact fp32 throughout)
        "feat_wgrad": {"fwd.x": "bf16", "bwd.g": "bf16", "dW.g": "bf16", "dW.x": "bf16", "featW.g": "bf16", "featW.x": "bf16"},
    },
    # train.X3 == 2 with the row-tensor forms (DW_ONCHIP = False / DW_ONCHIP_EDGE = False): edge_chain_bwd_kernel<., 2> recomputes with the
    # Abramowitz-Stegun erf GELU ("as"), keeps gelu' in fp32 registers (edge update: gelu'(z1) parked in a bf16 row), stores A1 / A2 / G1 / G2 / G3 as
    # bf16 rows and leaves the contractions to wgrad_bf16_kernel
    "mixed_rows": {
        "enc_msg": dict(_MIXED_COMMON, **{"gelu.bwd": "as", "fwd.S": "x3", "bwd.g": "x3", "dW3.g": "bf16", "dW3.S": "bf16"}),
        "edge_update": dict(_MIXED_COMMON, **{"gelu.bwd": "as", "fwd.a2": "bf16", "bwd.g3": "bf16", "dW3.a2": "bf16", "bwd.d1": "bf16"}),
        "edge_linear": {"fwd.x": "bf16", "bwd.g": "bf16", "dW.g": "bf16", "dW.x": "bf16"},
    },
    # exact fp32 and split-bf16 products: no rounding point the controls' bars (2e-5 / 5e-5 of the largest entry) could see
    "exact": {s: {"gelu.fwd": "erf", "gelu.bwd": "erf"} for s in ("enc_msg", "edge_update", "edge_linear", "embed_tail", "feat_wgrad")},
}
for _t in TABLES.values():
    _t["dec_msg"] = _t["enc_msg"]
POINTS = ("fwd.hE", "fwd.x", "fwd.a1", "fwd.a2", "fwd.S", "bwd.g", "bwd.d2", "bwd.d1", "bwd.g3", "bwd.g2", "bwd.g1", "dPa.g1", "dW3.g", "dW3.S",
          "dW3.a2", "dW2.a1", "dW1.hE", "dW.x", "dW.g", "featW.g", "featW.x")

# what a comparison reports per observable: row tensors differ from the fp64 evaluation at bf16 ties only (share of elements, largest
# difference in bf16 steps: solvable.figures / solvable.bars); sums over edge rows by the largest difference relative to the largest entry
ROW_OBSERVABLES = ("out", "d_hE", "d_x", "d_y", "d_Pj0", "d_Pj1")
SUM_OBSERVABLES = ("d_Pa", "dW1", "dW2", "db2", "dW3", "db3", "d_lnw", "d_lnb", "dW", "db", "dWf", "d_posw", "d_posb")
SUM_MARGIN = 4.0                      # another summation order in fp32 (<= 256 per-workgroup partials, 32-row MFMA blocks) plus tie crossings
# Floor of a sum's bar: ONE bf16 step of its largest single term, relative to the sum's largest entry.  Every term of dW*, db2, db13, dL/dPa
# and d(ln weight) is a product of factors behind a rounding point; where one factor sits within fp32 rounding of a bf16 tie, another fp32
# operation order takes the other side and the term moves by one step of that factor, at most 2^-7 of the term.  The term is bounded row by
# row: max over rows of max_c |g[row, c]| x max_d |a[row, d]| (_largest_term).  The reference's fp32 evaluation meets a handful of such ties
# per tensor — at 640 rows often none at all where the kernel meets one (measured, enc_msg at 1 x 40 x 16: dW2 2.7e-6 in the reference,
# 1.4e-4 on the kernel) —, so 4 x its figure alone would hold the kernel to having FEWER tie crossings than another evaluation order has.
# Sums with no rounding point upstream (d(ln bias), the message stages' db3, edge_linear's dW / db, the tail's d(ln weight), the positional
# gradients) get no floor.
TIE_STEP = 2.0 ** -7
SHARE_BAR_LIMIT = 0.25 / 20.0         # a case whose share bar comes closer to 0.25 than a factor of 20 says nothing: it is left out
SENSITIVITY = 3.0                     # every seeded fault must move some observable to this many bars


# ----------------------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------------------
def signed_permutation(rng):
    return torch.from_numpy(_one_per_row(rng, H, H))


def rounds_per_workgroup(shape, cus=MI355X_CUS):
    """(rounds, largest number of rounds one persistent workgroup walks, rows of the last round) at SHAPES[shape] on `cus` compute units."""
    B, N, K = SHAPES[shape] if isinstance(shape, str) else shape
    E = B * N * K
    rounds = -(-E // ROUND_ROWS)
    grid = min(rounds, cus)
    return rounds, -(-rounds // grid), E - (rounds - 1) * ROUND_ROWS


def ragged_shape(cus=MI355X_CUS):
    """(1, N, 30) with more rounds than compute units, fewer than two per unit, and a ragged last round: (1, 560, 30) on 256 units, the
    smallest such N on any other device."""
    N = SHAPES["ragged"][1]
    ok = lambda n: cus < -(-n * 30 // ROUND_ROWS) < 2 * cus and (n * 30) % ROUND_ROWS != 0
    if not ok(N):
        N = next(n for n in range(31, 100000) if ok(n))
    return (1, N, 30)


def make_case(stage, shape, p=0.0, seed=0):
    if stage == FEAT_STAGE:
        return feat_case(feat_inputs(shape, seed), seed)
    return _make_case(stage, shape, p, seed)


def _make_case(stage, shape, p=0.0, seed=0):
    """CPU inputs of one stage at `shape` (a name in SHAPES or (B, N, K)): dense random rows, tables, biases, LayerNorm parameters and
    upstream gradients; signed-permutation matrices; neighbour lists with a hub (every residue lists residue 0 first) and otherwise
    random distinct neighbours; 15 % masked residues, one unmasked residue whose whole neighbourhood is masked (`lonely`); a random rank."""
    assert stage in STAGES, stage
    B, N, K = SHAPES[shape] if isinstance(shape, str) else shape
    G, E = B * N, B * N * K
    g = torch.Generator(device="cpu").manual_seed(7000 + 131 * STAGES.index(stage) + 17 * N + K + 1000003 * seed)
    rng = np.random.default_rng(4000 + 131 * STAGES.index(stage) + N + K + 7919 * seed)
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g)
    c = {"stage": stage, "B": B, "N": N, "K": K, "G": G, "E": E, "p": float(p), "seed": SEED_DROP}
    if stage == "edge_linear":
        c.update(x=rn(B, N, K, H), W=signed_permutation(rng), b=rn(H, sc=0.1), R=rn(B, N, K, H))
        return c
    if stage == "embed_tail":
        c.update(y=rn(B, N, K, H, sc=2.0) + 0.5, ln_w=1.0 + rn(H, sc=0.2), ln_b=rn(H, sc=0.2), W=signed_permutation(rng), b=rn(H, sc=0.1),
                 R=rn(B, N, K, H))
        return c
    idx = torch.rand(B, N, N, generator=g).argsort(-1)[..., :K].contiguous()
    idx[:, :, 0] = 0                                                            # the hub: N incoming edges
    mask = (torch.rand(B, N, generator=g) > MASKED_FRAC)
    mask[:, 1] = True                                                           # `lonely`: unmasked, every listed neighbour masked
    mask[:, 2] = False
    masked = [torch.nonzero(~mask[b]).view(-1) for b in range(B)]
    for b in range(B):
        idx[b, 1] = masked[b][torch.randint(0, len(masked[b]), (K,), generator=g)]
    c.update(h_E=rn(B, N, K, H), Pa=rn(B, N, H), Pj0=rn(B, N, H), Pj1=rn(B, N, H),
             W1=signed_permutation(rng), W2=signed_permutation(rng), W3=signed_permutation(rng), b2=rn(H, sc=0.1), b3=rn(H, sc=0.1),
             ln_w=1.0 + rn(H, sc=0.1), ln_b=rn(H, sc=0.1), E_idx=idx, mask=mask.to(torch.int32),
             rank=torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32), lonely=1)
    c["jg"] = (torch.arange(B)[:, None, None] * N + idx).view(G, K)             # [G, K] global neighbour rows
    if stage == "edge_update":
        c["R"] = rn(B, N, K, H)
    else:
        c["R"], c["R2"] = rn(B, N, H), rn(B, N, K, H)
    return c


def feat_complexes(shape, seed=0):
    """The feature dict of B synthetic complexes of N residues each (synth.make_complex; two chains, 5 % missing atoms, 4 % masked
    residues), stacked, as CPU tensors."""
    B, N, K = SHAPES[shape] if isinstance(shape, str) else shape
    cxs = [synth.make_complex(seed=31 + N + seed + 101 * b, n=N, n_chains=2, missing_atom_frac=0.05, masked_frac=0.04) for b in range(B)]
    return {k: torch.from_numpy(np.stack([np.ascontiguousarray(cx[k]) for cx in cxs])) for k in cxs[0]}


def feat_inputs(shape, seed=0):
    """feat_complexes featurised on the CPU in fp32: what feat_case needs, with y = feat . Wedge^T."""
    B, N, K = SHAPES[shape] if isinstance(shape, str) else shape
    fd = feat_complexes(shape, seed)
    w = {k: torch.from_numpy(v) for k, v in synth.make_weights(0, 1, 1).items() if k.startswith("features.")}
    X, A = fd["X"].float(), cpu_ref.ATOM
    Cb = cpu_ref._virtual_atom(X[:, :, A["N"]], X[:, :, A["CA"]], X[:, :, A["C"]], -0.58273431, 0.56802827, -0.54067466)
    Nna = cpu_ref._virtual_atom(X[:, :, A["O4'"]], X[:, :, A["C1'"]], X[:, :, A["C2'"]], -0.56967352, 0.51055973, -0.53122153)
    X18 = torch.cat((X, Cb[:, :, None], Nna[:, :, None]), -2)
    M18 = torch.cat((fd["X_m"], fd["protein_mask"][:, :, None], (fd["rna_mask"] + fd["dna_mask"])[:, :, None]), -1).float()
    _, E_idx = cpu_ref.knn(X[:, :, A["CA"]] + X[:, :, A["C1'"]], fd["mask"].float(), K)
    t = dict(E_idx=E_idx, X18=X18, M18=M18, R_idx=fd["R_idx"], chain=fd["chain_labels"], pos_w=w["features.embeddings.linear.weight"],
             pos_b=w["features.embeddings.linear.bias"], Wedge=w["features.edge_embedding.weight"])
    t["y"] = torch.cat([feat_rows(t, torch.float32, e0, e1) @ t["Wedge"].t() for e0, e1 in feat_chunks(t)]).view(B, N, K, H)
    return t


def feat_classes(t):
    """[E] relative-position class of every edge: clip(R_i - R_j + 32, 0, 64) on the same chain, 65 across chains."""
    idx = t["E_idx"].long()
    bidx = torch.arange(idx.shape[0])[:, None, None]
    R_idx, ch = t["R_idx"].long(), t["chain"].long()
    same = (ch[:, :, None] == ch[bidx, idx]).long()
    return (torch.clip(R_idx[:, :, None] - R_idx[bidx, idx] + 32, 0, 64) * same + (1 - same) * 65).view(-1)


def feat_chunks(t):
    E = t["E_idx"].numel()
    return [(e0, min(e0 + FEAT_CHUNK, E)) for e0 in range(0, E, FEAT_CHUNK)]


def feat_rows(t, dtype, e0=0, e1=None, rounding=lambda x: x):
    """Rows e0 .. e1 of the [E, 5200] features [E_pos (16) | RBF (18 x 18 x 16)] on the flat edge list: E_pos = W[:, class] + b in fp32 (one
    addition, the kernel's), the RBFs exp(-((D_ab - mu_r) / 1.25)^2) mask_a mask_b of cpu_ref.rbf_all_pairs in `dtype`; `rounding` is
    applied to every value (on the present pairs only: it keeps zeros)."""
    B, N, K = t["E_idx"].shape
    e1 = B * N * K if e1 is None else e1
    i = torch.arange(e0, e1) // K                                               # global residue of the edge, global neighbour
    j = (i // N) * N + t["E_idx"].reshape(-1)[e0:e1].long()
    X, M = t["X18"].reshape(B * N, 18, 3).to(dtype), t["M18"].reshape(B * N, 18).to(dtype)
    D = torch.sqrt(torch.sum((X[i][:, :, None, :] - X[j][:, None, :, :]) ** 2, -1) + 1e-6)
    mu = torch.linspace(2., 22., 16, dtype=dtype)
    present = (M[i][:, :, None] * M[j][:, None, :]) != 0                       # 0 / 1 masks: an absent pair's 16 RBFs are exact zeros
    rbf = torch.zeros(e1 - e0, 18, 18, 16, dtype=dtype)
    rbf[present] = rounding(torch.exp(-((D[present].unsqueeze(-1) - mu) / 1.25) ** 2))
    cls = t["cls"] if "cls" in t else feat_classes(t)
    pos = rounding((t["pos_w"].t()[cls[e0:e1]] + t["pos_b"]).to(dtype))
    return torch.cat((pos, rbf.reshape(e1 - e0, -1)), -1)


def feat_case(t, seed=0):
    """The feat_wgrad case on the featurised complex `t` (feat_inputs on the CPU; the device's own y, E_idx, X18, M18 on the GPU): the tail's
    LayerNorm parameters, a signed-permutation W_e, its bias and the upstream gradient."""
    B, N, K = t["E_idx"].shape
    g = torch.Generator(device="cpu").manual_seed(9100 + 17 * N + K + 1000003 * seed)
    rng = np.random.default_rng(9200 + N + K + 7919 * seed)
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g)
    c = {"stage": FEAT_STAGE, "B": B, "N": N, "K": K, "G": B * N, "E": B * N * K, "p": 0.0, "seed": SEED_DROP}
    c.update(t)
    c.update(ln_w=1.0 + rn(H, sc=0.2), ln_b=rn(H, sc=0.2), W=signed_permutation(rng), b=rn(H, sc=0.1), R=rn(B, N, K, H), cls=feat_classes(t))
    return c


def case_matrices(c):
    return [c[k] for k in ("W", "W1", "W2", "W3") if k in c]


# ----------------------------------------------------------------------------------------------------------------------------------------
# seeded faults (tests/test_solvable_train_host.py, premise (d)): name -> the stages it applies to
# ----------------------------------------------------------------------------------------------------------------------------------------
_EDGE3 = ("enc_msg", "dec_msg", "edge_update")
FAULTS = {
    "row_missing": STAGES + (FEAT_STAGE,),           # one edge row missing from every contraction over edge rows
    "last_round_missing": STAGES + (FEAT_STAGE,),    # the ragged last round missing from every contraction (shapes with one)
    "padding_row_counted": STAGES + (FEAT_STAGE,),   # the clamped copy of the last row (a padding row past E) contributing to the contractions
    "no_db2": _EDGE3, "no_db3": _EDGE3, "no_db": ("edge_linear", "embed_tail"),
    "no_d_lnb": ("edge_update", "embed_tail"),
    "dropout_forward_only": ("edge_update",),
    "W1_for_W1T": _EDGE3, "W2_for_W2T": _EDGE3, "W3_for_W3T": _EDGE3, "W_for_WT": ("edge_linear", "embed_tail"),
    "blocks_swapped": STAGES,                # two 16-channel blocks of one transposed image swapped (W2^T; edge_linear: W_e^T)
    "masked_edge_counted": ("enc_msg",),     # one edge with mask_i mask_j = 0 weighed 1/30 in the backward
    "Pj1_for_Pj0": ("dec_msg",),
}
SOFT_FAULTS = {
    "erf_phi_in_gelu_grad": _EDGE3,          # exact-erf Phi inside gelu'
    "g2_unrounded_in_dW2": _EDGE3,           # the upstream gradient left unrounded in a contraction
    "g_unrounded_in_dW": ("edge_linear", "embed_tail"),
}


def _swap_blocks(W):
    """rows 0..15 and 16..31 of W exchanged: what a transposed image with two 16-channel blocks swapped multiplies by."""
    Wp = W.clone()
    Wp[0:16], Wp[16:32] = W[16:32], W[0:16]
    return Wp


# ----------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------------------------
def restate(case, dtype, points="mixed", fault=None, keep=False, terms=False):
    """Forward and backward of `case` in `dtype` with the rounding points of `points` (a name in TABLES or a table itself) -> {observable:
    tensor}; `fault` seeds one of FAULTS / SOFT_FAULTS; keep=True adds "z1", the first product, which the host premises look at;
    terms=True adds "_terms": per sum over edge rows that has a rounding point upstream, a bound on its largest single term (bars_of).
    Observables: out; d_hE (edge_linear: d_x); d_Pa, d_Pj0 (, d_Pj1); dW1, dW2, db2, dW3, db3 (edge_linear: dW, db); d_lnw, d_lnb.
    The message stages' d_hE includes the pass-through gradient R2, as the launch adds it."""
    stage = case["stage"]
    table = dict(TABLES[points][stage] if isinstance(points, str) else points)
    unknown = set(table) - set(POINTS) - {"gelu.fwd", "gelu.bwd"}
    assert not unknown, unknown
    assert fault is None or stage in dict(FAULTS, **SOFT_FAULTS)[fault], (fault, stage)
    r = lambda name, x: ROUNDINGS[table.get(name)](x)
    with torch.no_grad():
        fn = _restate_linear if stage in ("edge_linear", "embed_tail", FEAT_STAGE) else _restate_edge
        out = fn(case, dtype, table, r, fault, keep)
        if not terms:
            out.pop("_terms", None)
        return out


def _row_weights(case, fault, dtype):
    """[E] weights of the edge rows inside the contractions: ones, but for the bookkeeping faults."""
    E = case["E"]
    cw = torch.ones(E, dtype=dtype)
    if fault == "row_missing":
        e = (2 * E) // 3 + 5
        if case["stage"] == "enc_msg":                          # a row that takes part: mask_i mask_j = 1
            att = (case["mask"].view(-1)[:, None] * case["mask"].view(-1)[case["jg"]]).view(-1)
            e += int(torch.nonzero(att[e:])[0])
        cw[e] = 0.0
    elif fault == "last_round_missing":
        assert E % ROUND_ROWS != 0, "this shape has no ragged last round"
        cw[E - E % ROUND_ROWS:] = 0.0
    elif fault == "padding_row_counted":
        cw[E - 1] = 2.0
    return cw


def _largest_term(G, A):
    """Bound on the largest single term of G^T A (rows = edge rows or residues): max over rows of max_c |G[row, c]| x max_d |A[row, d]|."""
    return float((G.abs().amax(-1) * A.abs().amax(-1)).max())


def _restate_linear(c, dtype, table, r, fault, keep):
    E = c["E"]
    W, b, g = c["W"].to(dtype), c["b"].to(dtype), c["R"].to(dtype).view(E, H)
    cw = _row_weights(c, fault, dtype)[:, None]
    Wt = W.t() if fault == "W_for_WT" else _swap_blocks(W) if fault == "blocks_swapped" else W
    tail = c["stage"] in ("embed_tail", FEAT_STAGE)
    if tail:                                                   # x = LayerNorm(y): re-derived from y by the forward and by both backward launches
        y, ln_w, ln_b = c["y"].to(dtype).view(E, H), c["ln_w"].to(dtype), c["ln_b"].to(dtype)
        yc = y - y.mean(-1, keepdim=True)
        rstd = torch.rsqrt((yc * yc).mean(-1, keepdim=True) + 1e-5)
        xhat = yc * rstd
        x = xhat * ln_w + ln_b
    else:
        x = c["x"].to(dtype).view(E, H)
    gx = r("bwd.g", g) @ Wt
    out = {"out": r("fwd.x", x) @ W.t() + b}
    if tail:
        out["d_lnw"] = (cw * gx * xhat).sum(0)
        out["d_lnb"] = torch.zeros(H, dtype=dtype) if fault == "no_d_lnb" else (cw * gx).sum(0)
        gw = gx * ln_w
        out["d_y"] = (gw - gw.mean(-1, keepdim=True) - xhat * (gw * xhat).mean(-1, keepdim=True)) * rstd
        out["_terms"] = {"dW": _largest_term(g, x)}                               # LayerNorm(y) is computed, so its rounding meets ties
    else:
        out["d_x"] = gx
    gq = g if fault == "g_unrounded_in_dW" else r("dW.g", g)
    out["dW"] = (cw * gq).t() @ r("dW.x", x)
    out["db"] = torch.zeros(H, dtype=dtype) if fault == "no_db" else (cw * g).sum(0)
    if c["stage"] == FEAT_STAGE:
        gpre = out["d_y"]
        gq, dWf, term = cw * r("featW.g", gpre), torch.zeros(H, c["Wedge"].shape[1], dtype=dtype), 0.0
        for e0, e1 in feat_chunks(c):                                       # the feature rows a chunk at a time: dWf is a sum over edge rows
            feat = feat_rows(c, dtype, e0, e1, ROUNDINGS[table.get("featW.x")])
            dWf += gq[e0:e1].t() @ feat
            term = max(term, _largest_term(gq[e0:e1], feat))
        out["dWf"] = dWf
        gp = cw * (gpre @ c["Wedge"][:, :16].to(dtype))                     # exact fp32 on the device: no rounding point
        out["d_posw"] = torch.zeros(16, c["pos_w"].shape[1], dtype=dtype).index_add_(1, c["cls"], gp.t())
        out["d_posb"] = gp.sum(0)
        out["_terms"]["dWf"] = term
    if keep:
        out["z1"] = r("fwd.x", x) @ W.t()
    return out


def _restate_edge(c, dtype, table, r, fault, keep):
    stage = c["stage"]
    G, K, E, jg = c["G"], c["K"], c["E"], c["jg"]
    t = lambda k: c[k].to(dtype)
    hE, Pa, Pj0, Pj1 = t("h_E").view(G, K, H), t("Pa").view(G, H), t("Pj0").view(G, H), t("Pj1").view(G, H)
    W1, W2, W3, b2, b3 = t("W1"), t("W2"), t("W3"), t("b2"), t("b3")
    gelu_f, gelu_b = table.get("gelu.fwd", "erf"), table.get("gelu.bwd", "erf")
    gelu_bd = "poly_erf_phi" if fault == "erf_phi_in_gelu_grad" else gelu_b
    W1T = W1.t() if fault == "W1_for_W1T" else W1                  # the matrix a "W^T . g" product multiplies g with from the right
    W2T = W2.t() if fault == "W2_for_W2T" else _swap_blocks(W2) if fault == "blocks_swapped" else W2
    W3T = W3.t() if fault == "W3_for_W3T" else W3
    cw = _row_weights(c, fault, dtype).view(G, K, 1)
    flat = lambda x: x.reshape(E, H)
    out = {}

    # ---- tables and row weights
    sel = None
    if stage == "dec_msg":
        sel = (c["rank"].view(-1)[jg] < c["rank"].view(-1)[:, None])              # the neighbour comes earlier: first table
        pj = Pj1[jg] if fault == "Pj1_for_Pj0" else torch.where(sel[..., None], Pj0[jg], Pj1[jg])
        att = torch.ones(G, K, dtype=dtype)
    elif stage == "enc_msg":
        pj = Pj0[jg]
        att = (c["mask"].view(-1)[:, None] * c["mask"].view(-1)[jg]).to(dtype)
    else:
        pj = Pj0[jg]
    # ---- forward
    z1 = r("fwd.hE", hE) @ W1.t() + (Pa[:, None, :] + pj)
    a1 = gelu_val_grad(z1, gelu_f)[0]
    z2 = r("fwd.a1", a1) @ W2.t() + b2
    a2 = gelu_val_grad(z2, gelu_f)[0]
    # ---- the backward launch's recomputation (its own GELU form; the same values when the two forms agree)
    if gelu_b == gelu_f and gelu_bd == gelu_b:
        a1b, a2b = a1, a2
        d1, d2 = gelu_val_grad(z1, gelu_b)[1], gelu_val_grad(z2, gelu_b)[1]
    else:
        a1b = gelu_val_grad(z1, gelu_b)[0]
        d1 = gelu_val_grad(z1, gelu_bd)[1]
        z2b = r("fwd.a1", a1b) @ W2.t() + b2
        a2b = gelu_val_grad(z2b, gelu_b)[0]
        d2 = gelu_val_grad(z2b, gelu_bd)[1]

    if stage == "edge_update":
        ln_w, ln_b, g = t("ln_w"), t("ln_b"), t("R").view(G, K, H)
        D = hash_dropout_factor(c["seed"], E, c["p"], "cpu").to(dtype).view(G, K, H) if c["p"] > 0.0 else None
        z3 = r("fwd.a2", a2) @ W3.t() + b3
        x = hE + (z3 * D if D is not None else z3)                              # the residual takes the fp32 row
        xc = x - x.mean(-1, keepdim=True)
        rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
        xhat = xc * rstd
        out["out"] = xhat * ln_w + ln_b
        # the backward launch recomputes z3 from ITS a2 (the same LayerNorm statistics unless the GELU forms differ)
        if a2b is not a2:
            z3b = r("fwd.a2", a2b) @ W3.t() + b3
            xb = hE + (z3b * D if D is not None else z3b)
            xc = xb - xb.mean(-1, keepdim=True)
            rstd = torch.rsqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
            xhat = xc * rstd
        out["d_lnb"] = torch.zeros(H, dtype=dtype) if fault == "no_d_lnb" else (cw * g).sum((0, 1))
        out["d_lnw"] = (cw * g * xhat).sum((0, 1))
        gw = g * ln_w
        dx = (gw - gw.mean(-1, keepdim=True) - xhat * (gw * xhat).mean(-1, keepdim=True)) * rstd
        g3 = dx * D if (D is not None and fault != "dropout_forward_only") else dx
        g3r = r("bwd.g3", g3)
        out["dW3"] = flat(cw * g3r).t() @ flat(r("dW3.a2", a2b))
        out["db3"] = torch.zeros(H, dtype=dtype) if fault == "no_db3" else (cw * g3r).sum((0, 1))
        g2 = (g3r @ W3T) * r("bwd.d2", d2)
        residual = dx
    else:
        g, R2 = t("R").view(G, H), t("R2").view(G, K, H)
        w = att / 30.0
        S, wsum = (w[..., None] * a2).sum(1), w.sum(1)
        out["out"] = r("fwd.S", S) @ W3.t() + wsum[:, None] * b3                 # layer 3 behind the K-sum, per residue
        out["dW3"] = r("dW3.g", g).t() @ r("dW3.S", S)
        out["db3"] = torch.zeros(H, dtype=dtype) if fault == "no_db3" else (g * wsum[:, None]).sum(0)
        gS = r("bwd.g", g) @ W3T                                                # dL/d(K-sum), per residue
        wb = w
        if fault == "masked_edge_counted":
            i0 = int(torch.nonzero((att.view(-1) == 0) & (c["mask"].view(-1)[:, None].expand(G, K).reshape(-1) == 1))[7])
            wb = w.clone()
            wb.view(-1)[i0] = 1.0 / 30.0
        g2 = (gS[:, None, :] * wb[..., None]) * r("bwd.d2", d2)
        residual = R2
    g2r = r("bwd.g2", g2)
    out["dW2"] = flat(cw * (g2 if fault == "g2_unrounded_in_dW2" else g2r)).t() @ flat(r("dW2.a1", a1b))
    out["db2"] = torch.zeros(H, dtype=dtype) if fault == "no_db2" else (cw * g2r).sum((0, 1))
    g1 = (g2r @ W2T) * r("bwd.d1", d1)
    g1r = r("bwd.g1", g1)
    out["dW1"] = flat(cw * g1r).t() @ flat(r("dW1.hE", hE))
    out["d_Pa"] = (cw * r("dPa.g1", g1)).sum(1)
    rows = flat(cw * g1r)
    if sel is not None:
        s = sel.reshape(E, 1).to(dtype)
        out["d_Pj0"] = torch.zeros(G, H, dtype=dtype).index_add_(0, jg.reshape(-1), rows * s)
        out["d_Pj1"] = torch.zeros(G, H, dtype=dtype).index_add_(0, jg.reshape(-1), rows * (1.0 - s))
    else:
        out["d_Pj0"] = torch.zeros(G, H, dtype=dtype).index_add_(0, jg.reshape(-1), rows)
    out["d_hE"] = g1r @ W1T + residual
    mx = lambda x: float(x.abs().max())
    tm = {"dW2": _largest_term(g2r, a1b), "db2": mx(g2r), "dW1": _largest_term(g1r, hE), "d_Pa": mx(g1)}
    if stage == "edge_update":
        tm.update({"dW3": _largest_term(g3r, a2b), "db3": mx(g3r), "d_lnw": mx(g * xhat)})
    else:
        tm["dW3"] = _largest_term(g, S)
    out["_terms"] = tm
    if keep:
        out["z1"] = r("fwd.hE", hE) @ W1.t()
    return out


def dense_autograd(case):
    """fp64 torch autograd of the dense formulas (exact-erf GELU, F.layer_norm, the hash dropout mask) -> the observables of `restate`."""
    stage = case["stage"]
    D_ = torch.float64
    with torch.enable_grad():
        if stage == "edge_linear":
            x, W, b = (case[k].to(D_).requires_grad_(True) for k in ("x", "W", "b"))
            y = x @ W.t() + b
            (y * case["R"].to(D_)).sum().backward()
            return {"out": y.detach().view(-1, H), "d_x": x.grad.view(-1, H), "dW": W.grad, "db": b.grad}
        if stage == "embed_tail":
            y0, lw, lb, W, b = (case[k].to(D_).requires_grad_(True) for k in ("y", "ln_w", "ln_b", "W", "b"))
            out = F.linear(F.layer_norm(y0, (H,), lw, lb, 1e-5), W, b)
            (out * case["R"].to(D_)).sum().backward()
            return {"out": out.detach().view(-1, H), "d_y": y0.grad.view(-1, H), "d_lnw": lw.grad, "d_lnb": lb.grad, "dW": W.grad, "db": b.grad}
        if stage == FEAT_STAGE:
            # y = [one_hot(class) . pos_w^T + pos_b | RBF] . Wedge^T on the CPU's own features, then the tail; the case's y is NOT used
            lw, lb, W, b, We, pw, pb = (case[k].to(D_).requires_grad_(True) for k in ("ln_w", "ln_b", "W", "b", "Wedge", "pos_w", "pos_b"))
            # (E_pos enters the backward launch as fp32 rows whose one addition was made in fp32: the same values here, as a constant beside the
            # graph to pos_w and pos_b)
            feat = feat_rows(case, D_)
            pos = pw.t()[case["cls"]] + pb
            y0 = torch.cat((pos + (feat[:, :16] - pos).detach(), feat[:, 16:]), -1) @ We.t()
            y0.retain_grad()
            out = F.linear(F.layer_norm(y0, (H,), lw, lb, 1e-5), W, b)
            (out * case["R"].to(D_).view(-1, H)).sum().backward()
            return {"out": out.detach(), "d_y": y0.grad, "d_lnw": lw.grad, "d_lnb": lb.grad, "dW": W.grad, "db": b.grad, "dWf": We.grad,
                    "d_posw": pw.grad, "d_posb": pb.grad}
        B, N, K, G, E = (case[k] for k in "BNKGE")
        idx = case["E_idx"]
        bidx = torch.arange(B)[:, None, None]
        names = ["h_E", "Pa", "Pj0", "Pj1", "W1", "W2", "b2", "W3", "b3", "ln_w", "ln_b"]
        hE, pa, pj0, pj1, w1, w2, bb2, w3, bb3, lw, lb = leaves = [case[k].to(D_).requires_grad_(True) for k in names]
        if stage == "dec_msg":
            rank = case["rank"].long()
            bw = (rank[bidx, idx] < rank[:, :, None]).unsqueeze(-1)
            pj = torch.where(bw, pj0[bidx, idx], pj1[bidx, idx])
        else:
            pj = pj0[bidx, idx]
        z3 = F.gelu(F.gelu(hE @ w1.t() + pa[:, :, None] + pj) @ w2.t() + bb2) @ w3.t() + bb3
        if stage == "edge_update":
            drop = hash_dropout_factor(case["seed"], E, case["p"], "cpu").view(B, N, K, H) if case["p"] > 0.0 else 1.0
            y = F.layer_norm(hE + z3 * drop, (H,), lw, lb, 1e-5)
            (y * case["R"].to(D_)).sum().backward()
        else:
            mask = case["mask"].bool()
            wgt = (mask[:, :, None] & mask[bidx, idx]).to(D_) if stage == "enc_msg" else torch.ones(B, N, K, dtype=D_)
            y = (wgt.unsqueeze(-1) * z3).sum(2) / 30.0
            ((y * case["R"].to(D_)).sum() + (hE * case["R2"].to(D_)).sum()).backward()
        gr = dict(zip(names, [l.grad for l in leaves]))
        out = {"out": y.detach().reshape(-1, K, H) if stage == "edge_update" else y.detach().reshape(G, H),
               "d_hE": gr["h_E"].view(G, K, H), "d_Pa": gr["Pa"].view(G, H), "d_Pj0": gr["Pj0"].view(G, H), "dW1": gr["W1"], "dW2": gr["W2"],
               "db2": gr["b2"], "dW3": gr["W3"], "db3": gr["b3"]}
        if stage == "dec_msg":
            out["d_Pj1"] = gr["Pj1"].view(G, H)
        if stage == "edge_update":
            out["d_lnw"], out["d_lnb"] = gr["ln_w"], gr["ln_b"]
        return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# figures and bars
# ----------------------------------------------------------------------------------------------------------------------------------------
def observables(case):
    stage = case["stage"]
    if stage == "edge_linear":
        return ("out", "d_x", "dW", "db")
    if stage == "embed_tail":
        return ("out", "d_y", "d_lnw", "d_lnb", "dW", "db")
    if stage == FEAT_STAGE:
        return ("out", "d_y", "d_lnw", "d_lnb", "dW", "db", "dWf", "d_posw", "d_posb")
    names = ["out", "d_hE", "d_Pa", "d_Pj0"] + (["d_Pj1"] if stage == "dec_msg" else []) + ["dW1", "dW2", "db2", "dW3", "db3"]
    return tuple(names + (["d_lnw", "d_lnb"] if stage == "edge_update" else []))


def rel_max(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def measure(got, ref64):
    """{observable: (share, units) for a row tensor | (rel,) for a sum over edge rows} of `got` against the fp64 restatement."""
    out = {}
    for k, v in ref64.items():
        if k in ROW_OBSERVABLES:
            out[k] = figures(got[k].reshape(v.shape).cpu(), v)
        elif k in SUM_OBSERVABLES:
            out[k] = (rel_max(got[k].reshape(v.shape).cpu(), v),)
    return out


def bars_of(ref_figures, ref64, terms):
    """The bars a kernel is held to, from the reference's own figures (its fp32 evaluation against its fp64 evaluation): solvable.bars for
    row tensors; for the sums over edge rows SUM_MARGIN x the reference's figure, or one bf16 step of the sum's largest term (TIE_STEP)
    where that is more."""
    floor = lambda k: TIE_STEP * terms[k] / float(ref64[k].abs().max()) if k in terms else 0.0
    return {k: bars(*f) if len(f) == 2 else (max(SUM_MARGIN * f[0], floor(k)),) for k, f in ref_figures.items()}


def ratios(figs, bar):
    """{observable: the figure furthest over its bar, as a multiple of the bar}"""
    return {k: max((f / b if b > 0 else (0.0 if f == 0 else float("inf"))) for f, b in zip(figs[k], bar[k])) for k in figs}


def reference(case, points="mixed"):
    """(fp64 restatement, the fp32 evaluation's figures against it, the bars)"""
    ref64 = restate(case, torch.float64, points, terms=True)
    terms = ref64.pop("_terms", {})
    figs = measure(restate(case, torch.float32, points), ref64)
    return ref64, figs, bars_of(figs, ref64, terms)


def line(tag, name, figs, ref_figs, bar):
    """one SOLVABLE line in the format of tests/test_gpu_solvable.py"""
    if len(figs) == 2:
        return (f"SOLVABLE {tag} {name}: share {figs[0]:.2e} (reference {ref_figs[0]:.2e}, bar {bar[0]:.2e}), "
                f"max {figs[1]:.2f} units (reference {ref_figs[1]:.2f}, bar {bar[1]:.2f})")
    return f"SOLVABLE {tag} {name}: rel {figs[0]:.2e} (reference {ref_figs[0]:.2e}, bar {bar[0]:.2e})"
