"""Weight variants that move the network out of the narrow numeric band of synth.make_weights (Xavier matrices, 0.1-sigma biases,
LayerNorm affine terms near (1, 0): GELU pre-activations below 6.5, LayerNorm rows with |mean| / std near 0.3, |log p| below 8) towards
the activation scales of a trained model.  variant(weights_np, name) returns a modified COPY of the session weights; the reach of each
variant on the fp64 oracle is asserted by tests/test_weight_variants_host.py, so that the GPU tests built on them (tests/test_gpu_range.py)
cannot silently lose it.

"Layer" tensors are the keys under encoder_layers. / decoder_layers.; "norm" tensors are the keys containing "norm".

    base    unchanged
    gain2   every layer non-norm tensor (matrices and biases) x 2: GELU pre-activations past the exact form's clamp (5.6) and past the
            range the bf16-mode polynomial was checked on (12)
    gain4   the same x 4: pre-activations of 60-250, the polynomial's overflow region
    shift   + 40 on the layer biases of W3, W13 and dense.W_out: rows entering norm1 / norm2 / norm3 with |mean| / std in the hundreds
    affine  every norm weight x 3, every norm bias + 2 sign(r), r drawn per tensor (in key order) from default_rng(123)
    head    W_out.* and W_s.* x 8: |log p| of 30-50; at T = 0.05 the sampler's logits / T reach ~1000
    feat    features.edge_embedding.weight x 4 and + 4.0 on every channel of the row entering features.norm_edges.  The edge embedding has
            no bias, so the shift goes in as a constant column driven by a bias of the positional encoding: column FEAT_SHIFT_COLUMN of the
            (scaled) edge embedding is set to 1.0 and features.embeddings.linear.bias[FEAT_SHIFT_COLUMN] is raised by 4.0, i.e. every
            channel of the row receives 4.0 + that positional channel's own (small) value in place of the column's former random term.
"""
import numpy as np
import torch

from na_mpnn_amd import shard, synth
from oracle import cpu_ref

NAMES = ("base", "gain2", "gain4", "shift", "affine", "head", "feat")
FEAT_SHIFT = 4.0
FEAT_SHIFT_COLUMN = 15          # the last of the 16 positional-encoding channels
FEAT_SHIFT_VIA = "features.embeddings.linear.bias"


def _is_layer(key):
    return key.startswith("encoder_layers.") or key.startswith("decoder_layers.")


def _is_norm(key):
    return "norm" in key


def variant(weights_np, name):
    w = {k: v.copy() for k, v in weights_np.items()}
    if name == "base":
        pass
    elif name in ("gain2", "gain4"):
        f = np.float32(2.0 if name == "gain2" else 4.0)
        for k in w:
            if _is_layer(k) and not _is_norm(k):
                w[k] *= f
    elif name == "shift":
        for k in w:
            if _is_layer(k) and k.endswith((".W3.bias", ".W13.bias", ".dense.W_out.bias")):
                w[k] += np.float32(40.0)
    elif name == "affine":
        rng = np.random.default_rng(123)
        for k in w:
            if _is_norm(k):
                if k.endswith(".weight"):
                    w[k] *= np.float32(3.0)
                else:
                    w[k] += (2.0 * np.sign(rng.standard_normal(w[k].shape))).astype(np.float32)
    elif name == "head":
        for k in w:
            if k.startswith(("W_out.", "W_s.")):
                w[k] *= np.float32(8.0)
    elif name == "feat":
        w["features.edge_embedding.weight"] *= np.float32(4.0)
        assert "features.edge_embedding.bias" not in w
        w["features.edge_embedding.weight"][:, FEAT_SHIFT_COLUMN] = 1.0
        w[FEAT_SHIFT_VIA][FEAT_SHIFT_COLUMN] += np.float32(FEAT_SHIFT)
    else:
        raise KeyError(name)
    return w


# ----------------------------------------------------------------------------------------------------------------------------------------
# the inputs the range tests share (shapes the suite already runs; only the weights change), as CPU feature_dicts / graphs
# ----------------------------------------------------------------------------------------------------------------------------------------
GRAPH_SHAPES = {"small": (2, 120, 30, 0.05), "large": (3, 840, 17, 0.1)}      # (B, N, K, masked fraction)
COORDS_K = 24
TRAIN_NS, TRAIN_K = (40, 33), 17


def graph_case(shape):
    """synth.make_graph inputs of GRAPH_SHAPES[shape] as torch CPU tensors."""
    B, N, K, mf = GRAPH_SHAPES[shape]
    g = synth.make_graph(seed=4100 + N, batch=B, n=N, k=K, masked_frac=mf)
    return {k: torch.from_numpy(v) for k, v in g.items()}


def coords_case():
    """The from-coordinates input: one 70-residue complex with masked residues and missing atoms, batch dimension added."""
    cx = synth.make_complex(seed=41, n=70, masked_frac=0.05, missing_atom_frac=0.05)
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd["batch_size"] = 1
    return fd


def train_case():
    """(feature_dict, decoding-order noise) of the padded training batch, as test_training_gradients_odd_shapes builds it."""
    cxs = [synth.make_complex(seed=600 + 10 * i + n, n=n, n_chains=3, masked_frac=0.1) for i, n in enumerate(TRAIN_NS)]
    fd = shard.pad_batch(cxs)
    fd["S"] = fd["S"].long()
    randn = torch.randn(len(TRAIN_NS), max(TRAIN_NS), generator=torch.Generator().manual_seed(TRAIN_K))
    return fd, randn


def torch_weights(weights_np, name, dtype=None):
    w = {k: torch.from_numpy(v) for k, v in variant(weights_np, name).items()}
    return w if dtype is None else {k: v.to(dtype) for k, v in w.items()}


def graph_oracle(w, t):
    """cpu_ref on a graph_case in the dtype of `w`: h_V, h_E, log_probs and the decoding order of every batch member."""
    V, E = t["V"].to(w["W_v.weight"].dtype), t["E"].to(w["W_v.weight"].dtype)
    idx = t["E_idx"].long()
    with torch.no_grad():
        h_V, h_E = cpu_ref.encode_from_graph(w, V, E, idx, t["mask"])
        out = cpu_ref.score_from_encoded(w, h_V, h_E, idx, t["S"], t["mask"], t["chain_mask"], t["randn"])
    order = cpu_ref.decoding_order_of(t["mask"] * t["chain_mask"], t["randn"])
    return {"h_V": h_V, "h_E": h_E, "log_probs": out["log_probs"], "decoding_order": order}


def top2_margin(log_probs):
    """Gap between the two largest entries of every row."""
    top = log_probs.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]
