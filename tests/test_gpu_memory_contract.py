"""The memory contract of every ABI entry point (include/namp.h), checked with guarded buffers (tests/guarded.py).

Every buffer that crosses the ABI is carved from one arena with a 256 KiB guard band on each side; a call runs under two fills
(guards NaN / 1e30 beside float buffers, 0 / 1 beside integer ones; outputs and workspaces pre-filled with NaN bytes / zeros) and must
  1. leave every guard byte and every `const` input as it was,
  2. write outputs that are bit-identical under both fills (nothing outside the declared inputs reaches an output),
  3. leave no NaN / Inf in an output,
  4. return NAMP_OK.
Sizes come from include/namp.h alone: const-ness, the size comments and the *_bytes / *_groups / *_chunks / *_rows functions.  A
workspace is allocated at exactly the declared byte count, partial-sum buffers at exactly the declared row count.

The contract table is TABLE below: one row (a builder function) per entry point.  A builder registers the arguments with their role
(`inp` = const input, `out`, `inout`, `ws`) and shape and returns the call.  Packed weights live outside the arena; their buffer is
compared with a snapshot after every case.

Entry points that are NOT bit-reproducible (fp32 atomics into the table gradients) are listed in NONREPRO with the buffers concerned
and the tolerance those borrow from tests/test_gpu_train.py; every other output and every other row is compared to the bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from guarded import Arena, GuardError, run_contract

f32, i32, i64, bf16, u8, f64 = torch.float32, torch.int32, torch.int64, torch.bfloat16, torch.uint8, torch.float64
H, V33 = 128, 33

# (B, N, K): the smallest shapes with a ragged tail at every granule — 16 neighbours per tile, 16/32/64-row residue tiles, K clipped to N
SHAPES = [(1, 1, 1), (1, 17, 48), (1, 33, 15), (1, 33, 16), (3, 65, 17), (2, 129, 33), (1, 97, 48)]
# ... and one pair straddling namp_fused_tail_max_residues(): B = 2 with N = limit / 2 and limit / 2 + 1 at K = 17 (resolved at run time)
FUSED_PAIR = [("F", 0), ("F", 1)]
ROWS = [1, 63, 64, 65, "chunk+1"]                    # row-count kernels; "one chunk" is probed from the entry point's *_groups / *_chunks
SAMPLER = [(33, 1), (33, 3), (97, 1), (97, 3)]       # (N, batch_size) of the sampler and plan rows (K = 17, one complex)

TABLE = {}
EXEMPT = {
    "namp_persistent_status": "synchronous read-back of the barrier words into a HOST int; exercised by test_persistent_forward_equals_launch_chain",
    "namp_profile_collect": "measurement hook: waits for events and writes HOST arrays only",
    "namp_sample_token_maps": "attaches a pointer to the calling thread's next sampler call; launches nothing and touches no memory itself",
    "namp_sample_class_tables": "attaches a pointer to the calling thread's next sampler call; launches nothing and touches no memory itself",
}
# the entry points the contract must cover by a row (none of them may be exempt)
REQUIRED = """namp_gather_nodes_f32 namp_gather_rows_f32 namp_gather_edges_f32 namp_cat_neighbors_nodes_f32 namp_node_linear namp_edge_embed
namp_edge_embed_prec namp_edge_embed_ln namp_logits_log_softmax namp_pack_images namp_enc_layer_fwd namp_dec_layer_fwd namp_encoder_fwd
namp_decoder_fwd namp_encdec_fwd namp_bf16s_message namp_featurize namp_featurize_ordered namp_decoding_order namp_sample_levels
namp_sample_levels_dep namp_sample_work_lists namp_decoder_sample namp_decoder_sample_levels namp_decoder_sample_walk namp_states_plan
namp_pairs_plan namp_pairs_work_lists namp_decoder_loo namp_train_edge_fwd namp_train_edge_bwd namp_train_edge_bwd_dw
namp_train_edge_update_bwd namp_train_edge_update_bwd_dw namp_train_tail_fwd namp_train_tail_bwd namp_train_ln_rows_fwd namp_train_ln_rows_bwd
namp_train_wgrad namp_train_wgrad_ln namp_train_wgrad_multi namp_train_scatter_rows namp_train_scatter_rows_bf16 namp_train_reverse_adjacency
namp_train_embed_ln_bwd namp_train_feat_wgrad namp_train_pos_features namp_train_pos_grad namp_train_class_sums namp_train_wcolsum
namp_reduce_sum namp_train_loss_smoothed namp_train_adam_step namp_train_metrics namp_canonical_pair_accuracy""".split()

# Entry points that are NOT bit-reproducible: they accumulate the table gradients dL/dPa (when K % 16 != 0; per-tile plain stores
# otherwise) and dL/dPj / dL/dPc (when the caller passes those buffers) with fp32 atomics, in no fixed order.  Only these buffers are
# compared at a tolerance, relative to the largest entry; every other output of these rows, and every other row, is compared to the bit.
TOL_SPLIT = 5e-5     # tests/test_gpu_train.py::test_edge_mlp_backward_matches_autograd: the bar of every gradient, fp32 / split-bf16 products
TOL_BF16 = 3e-2      # tests/test_gpu_train.py::test_on_chip_backward_matches_fp64_autograd: the bar of the bf16-product backward
NONREPRO = {
    "namp_train_edge_bwd": "g_Pa (K % 16 != 0), g_Pj0, g_Pj1",
    "namp_train_edge_bwd_dw": "g_Pa (K % 16 != 0)",
    "namp_train_edge_update_bwd": "g_Pa (K % 16 != 0), g_Pc",
    "namp_train_edge_update_bwd_dw": "g_Pa (K % 16 != 0)",
}


def atomic(prec, *names):
    """Options of a case whose buffers `names` are accumulated with fp32 atomics at precision code `prec`."""
    names = [n for n in names if n]
    return dict(tol=TOL_BF16 if prec == 2 else TOL_SPLIT, tol_buffers=set(names)) if names else {}


class Row:
    def __init__(self, symbol, build, cases):
        self.symbol, self.build, self.cases = symbol, build, cases


def row(symbol, cases):
    """Register the builder of one entry point.  cases: [(id, case)]."""
    def deco(fn):
        assert symbol not in TABLE
        TABLE[symbol] = Row(symbol, fn, cases)
        return fn
    return deco


def ids(cases):
    return [("-".join(str(x) for x in (c if isinstance(c, tuple) else (c,))), c) for c in cases]


def cross(*lists):
    out = [()]
    for lst in lists:
        out = [a + (b if isinstance(b, tuple) else (b,)) for a in out for b in lst]
    return out


# ---- environment ---------------------------------------------------------------------------------------------------------
class Env:
    def __init__(self, weights_np):
        from na_mpnn_amd import hip
        from na_mpnn_amd.pack import PackedWeights
        assert torch.cuda.is_available(), "gpu tests need a HIP device"
        self.hip, self.L, self.dev = hip, hip.lib(), torch.device("cuda:0")
        self.packed = PackedWeights({k: torch.from_numpy(v).to(self.dev) for k, v in weights_np.items()}, 3, 3, V33, self.dev)
        torch.cuda.synchronize()
        self.snapshot = self.packed.flat.clone()              # packed weights count as `in`: compared after every case
        self.limit = self.L.namp_fused_tail_max_residues()

    def s(self):
        return self.hip.current_stream()

    def a(self, name):
        return self.packed.addr(name)

    def shape(self, case3):
        if case3[0] == "F":
            return 2, self.limit // 2 + case3[1], 17
        return case3

    def img(self, prec, name):
        """Image of a packed [128 x 128] block in the operand format of precision code `prec` (0 fp32, 1 split-bf16, 2 bf16)."""
        return self.a(name + ("_img", "_ximg", "_bimg")[prec])


@pytest.fixture(scope="module")
def env(weights_np):
    return Env(weights_np)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, sc=1.0):
    return sc * torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=16)
def graph_case(B, N, K):
    """Synthetic graph after featurisation with the masks the issue asks for: every complex after the first has a mask-0 padded tail of
    its own length, and 5-10 % of the residues inside are masked."""
    from na_mpnn_amd import synth
    g = synth.make_graph(seed=4000 + 131 * B + 7 * N + K, batch=B, n=N, k=K, masked_frac=0.08 if N >= 17 else 0.0)
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    for b in range(1, B):
        t["mask"][b, N - (3 * b + 2):] = 0
    order = torch.argsort((t["mask"] * t["chain_mask"] + 0.0001) * t["randn"].abs(), dim=1)
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(N).expand(B, -1))
    t["order"], t["rank"] = order.to(i32), rank.to(i32)
    t["K"] = t["E_idx"].shape[-1]
    return t


def rand_idx(g, B, N, K):
    """[B, N, K] int32 neighbour lists (distinct per residue), K already clipped to N."""
    return torch.stack([torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(N)]) for _ in range(B)]).to(i32)


def padded_mask(g, B, N):
    m = (torch.rand(B, N, generator=g) > 0.08).to(i32) if N >= 17 else torch.ones(B, N, dtype=i32)
    for b in range(1, B):
        m[b, N - (3 * b + 2):] = 0
    return m


# ==== copies and heads ======================================================================================================
@row("namp_gather_nodes_f32", ids(cross(SHAPES, [16, 3])))
def _gather_nodes(ar, env, case):
    B, N, K, Cn = case
    K = min(K, N)
    g = gen(1)
    nodes, idx = ar.inp("nodes", rn(g, B, N, Cn)), ar.inp("idx", rand_idx(g, B, N, K))
    out = ar.out("out", f32, (B, N, K, Cn))
    return lambda: env.L.namp_gather_nodes_f32(nodes.ptr, idx.ptr, out.ptr, B, N, K, Cn, env.s())


@row("namp_gather_rows_f32", ids(cross(SHAPES, [8, 5])))
def _gather_rows(ar, env, case):
    B, N, K, Cn = case
    K = min(K, N)
    g = gen(2)
    T, R, M = B * 2, N, K                                     # T tables of R rows, M look-ups per table
    tables = ar.inp("tables", rn(g, T, R, Cn))
    idx = ar.inp("idx", torch.randint(0, R, (T, M), generator=g).to(i32))
    out = ar.out("out", f32, (T, M, Cn))
    return lambda: env.L.namp_gather_rows_f32(tables.ptr, idx.ptr, out.ptr, T, R, M, Cn, env.s())


@row("namp_gather_edges_f32", ids(cross(SHAPES, [4, 1])))
def _gather_edges(ar, env, case):
    B, N, K, Cn = case
    K = min(K, N)
    g = gen(3)
    edges, idx = ar.inp("edges", rn(g, B, N, N, Cn)), ar.inp("idx", rand_idx(g, B, N, K))
    out = ar.out("out", f32, (B, N, K, Cn))
    return lambda: env.L.namp_gather_edges_f32(edges.ptr, idx.ptr, out.ptr, B, N, K, Cn, env.s())


@row("namp_cat_neighbors_nodes_f32", ids(cross(SHAPES, [(16, 16), (5, 3)])))
def _cat(ar, env, case):
    B, N, K, C1, C2 = case
    K = min(K, N)
    g = gen(4)
    nodes, nbrs = ar.inp("h_nodes", rn(g, B, N, C2)), ar.inp("h_neighbors", rn(g, B, N, K, C1))
    idx = ar.inp("idx", rand_idx(g, B, N, K))
    out = ar.out("out", f32, (B, N, K, C1 + C2))
    return lambda: env.L.namp_cat_neighbors_nodes_f32(nodes.ptr, nbrs.ptr, idx.ptr, out.ptr, B, N, K, C1, C2, env.s())


@row("namp_node_linear", ids(SHAPES))
def _node_linear(ar, env, case):
    B, N, K = case
    t = graph_case(B, N, K)
    X, S = ar.inp("X", t["V"]), ar.inp("S", t["S"])
    pre = ar.out("pre.out", f32, (B * N, H))
    outs = [ar.out(f"proj{q}.out", f32, (B * N, H)) for q in range(3)]
    NP = env.hip.NampProj

    def call():
        proj = (NP * 3)(NP(env.a("enc0.W1a_img"), env.a("enc0.b1"), None, outs[0].ptr), NP(env.a("enc0.W1c_img"), None, None, outs[1].ptr),
                        NP(env.a("dec1.W1v_img"), None, env.a("dec1.tok"), outs[2].ptr))
        p = NP(env.a("Wv_img"), env.a("Wv_b"), None, pre.ptr)
        return env.L.namp_node_linear(X.ptr, S.ptr, B, B, N, proj, 3, C.byref(p), env.s())
    return call


@row("namp_edge_embed", ids(SHAPES))
def _edge_embed(ar, env, case):
    B, N, K = case
    t = graph_case(B, N, K)
    K = t["K"]
    E, hE = ar.inp("E", t["E"]), ar.out("h_E", f32, (B, N, K, H))
    return lambda: env.L.namp_edge_embed(env.a("We_img"), env.a("We_b"), E.ptr, hE.ptr, B, N, K, env.s())


@row("namp_edge_embed_prec", ids(cross(SHAPES, [0, 1, 2])))
def _edge_embed_prec(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K = t["K"]
    E, hE = ar.inp("E", t["E"]), ar.out("h_E", f32, (B, N, K, H))
    return lambda: env.L.namp_edge_embed_prec(env.img(prec, "We"), env.a("We_b"), E.ptr, hE.ptr, prec, B, N, K, env.s())


@row("namp_edge_embed_ln", ids(cross(SHAPES, [0, 1, 2])))
def _edge_embed_ln(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K = t["K"]
    Y, hE = ar.inp("Y", 2.0 * t["E"] + 0.5), ar.out("h_E", f32, (B, N, K, H))
    return lambda: env.L.namp_edge_embed_ln(env.img(prec, "We"), env.a("We_b"), env.a("feat.ln_g"), env.a("feat.ln_b"), Y.ptr, hE.ptr, prec,
                                            B, N, K, env.s())


@row("namp_logits_log_softmax", ids(cross(SHAPES, ["logits", "nologits"])))
def _logits(ar, env, case):
    B, N, K, want = case
    G = B * N
    hV = ar.inp("h_V", graph_case(B, N, K)["V"])
    lp = ar.out("log_probs", f32, (G, V33))
    lg = ar.out("logits", f32, (G, V33)) if want == "logits" else None
    return lambda: env.L.namp_logits_log_softmax(env.a("Wout_w"), env.a("Wout_b"), hV.ptr, lp.ptr, lg.ptr if lg else None, G, V33, env.s())


@row("namp_pack_images", ids(["all_kinds"]))
def _pack_images(ar, env, case):
    g = gen(5)
    W1 = ar.inp("W1", rn(g, H, 3 * H))                        # [128 x 384]: column blocks as PackedWeights slices them
    Win = ar.inp("Win", rn(g, 4 * H, H))
    # (source, element offset, ld, out_f, in_f, kind, transposed, floats of output): x3 / bf16 of a [128 x 128] block, x3 of a general block
    descs = [(W1, H, 3 * H, H, H, 1, 0, H * H), (W1, H, 3 * H, H, H, 1, 1, H * H), (W1, 0, 3 * H, H, H, 2, 0, H * H // 2),
             (W1, 2 * H, 3 * H, H, H, 2, 1, H * H // 2), (Win, 0, H, 4 * H, H, 3, 0, 4 * H * H), (Win, 0, H, H, 4 * H, 3, 1, 4 * H * H)]
    imgs = [ar.out(f"img{q}", f32, (d[7],)) for q, d in enumerate(descs)]
    NP = env.hip.NampPack
    table = ar.inp("table", torch.zeros(C.sizeof(NP) * len(descs), dtype=u8))
    ar.build("A")                                             # fixes the addresses the descriptors hold
    arr, first = (NP * len(descs))(), 0
    for q, (src, off, ld, out_f, in_f, kind, tr, _n) in enumerate(descs):
        arr[q] = NP(src.ptr + 4 * off, imgs[q].ptr, ld, out_f, in_f, kind, tr, first)
        first += (out_f * in_f + 255) // 256
    table.data = torch.frombuffer(bytearray(bytes(arr)), dtype=u8).clone()
    return lambda: env.L.namp_pack_images(table.ptr, len(descs), first, env.s())


# ==== layer and graph level =================================================================================================
PRECS = ["x3", "fp32", "bf16"]
GRAPH_SHAPES = SHAPES + FUSED_PAIR


class precision:
    def __init__(self, env, prec):
        self.env, self.prec = env, prec

    def __enter__(self):
        self.env.packed.set_precision(self.prec)

    def __exit__(self, *exc):
        self.env.packed.set_precision("x3")


def with_precision(env, prec, fn):
    def call():
        with precision(env, prec):
            return fn()
    return call


@row("namp_enc_layer_fwd", ids(cross(GRAPH_SHAPES, PRECS)))
def _enc_layer(ar, env, case):
    B, N, K = env.shape(case[:-1])
    t = graph_case(B, N, K)
    K = t["K"]
    hV, hE, idx, mask = ar.inp("h_V", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"])
    oV, oE = ar.out("h_V_out", f32, (B, N, H)), ar.out("h_E_out", f32, (B, N, K, H))
    ws = ar.ws("ws", env.L.namp_workspace_bytes(B, B, N, K))
    return with_precision(env, case[-1], lambda: env.L.namp_enc_layer_fwd(
        env.packed.enc_layer(1), hV.ptr, hE.ptr, idx.ptr, mask.ptr, None, oV.ptr, oE.ptr, ws.ptr, ws.nbytes, B, N, K, env.s()))


@row("namp_dec_layer_fwd", ids(SHAPES))
def _dec_layer(ar, env, case):
    B, N, K = case
    t = graph_case(B, N, K)
    K = t["K"]
    g = gen(6)
    hV, ctx = ar.inp("h_V", t["V"]), ar.inp("h_ESV", rn(g, B, N, K, 3 * H))
    mV = ar.inp("mask_V", t["mask"])
    ma = ar.inp("mask_attend", torch.randint(0, 2, (B, N, K), generator=g).float())
    out = ar.out("h_V_out", f32, (B, N, H))
    ws = ar.ws("ws", env.L.namp_workspace_bytes(B, B, N, K))
    return lambda: env.L.namp_dec_layer_fwd(env.packed.dec_layer(0), hV.ptr, ctx.ptr, mV.ptr, ma.ptr, out.ptr, ws.ptr, ws.nbytes, B, N, K, env.s())


@row("namp_encoder_fwd", ids(cross(GRAPH_SHAPES, PRECS)))
def _encoder(ar, env, case):
    B, N, K = env.shape(case[:-1])
    t = graph_case(B, N, K)
    K = t["K"]
    Vv, E, idx, mask = ar.inp("V", t["V"]), ar.inp("E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"])
    oV, oE = ar.out("h_V", f32, (B, N, H)), ar.out("h_E", f32, (B, N, K, H))
    ws = ar.ws("ws", env.L.namp_workspace_bytes(B, B, N, K))
    return with_precision(env, case[-1], lambda: env.L.namp_encoder_fwd(
        env.packed.model(), Vv.ptr, E.ptr, idx.ptr, mask.ptr, oV.ptr, oE.ptr, ws.ptr, ws.nbytes, B, N, K, env.s()))


@row("namp_decoder_fwd", ids(cross(GRAPH_SHAPES, PRECS)))
def _decoder(ar, env, case):
    B, N, K = env.shape(case[:-1])
    t = graph_case(B, N, K)
    K = t["K"]
    hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
    S, mask, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
    lp, lg, hd = ar.out("log_probs", f32, (B, N, V33)), ar.out("logits", f32, (B, N, V33)), ar.out("h_V_dec", f32, (B * N, H))
    ws = ar.ws("ws", env.L.namp_workspace_bytes(B, B, N, K))
    return with_precision(env, case[-1], lambda: env.L.namp_decoder_fwd(
        env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, mask.ptr, rank.ptr, lp.ptr, lg.ptr, hd.ptr, ws.ptr, ws.nbytes, B, B, N, K, env.s()))


@row("namp_encdec_fwd", ids(cross(GRAPH_SHAPES, PRECS, ["chain", "persistent"])))
def _encdec(ar, env, case):
    B, N, K = env.shape(case[:-2])
    prec, persistent = case[-2], case[-1] == "persistent"
    t = graph_case(B, N, K)
    K = t["K"]
    Vv, E, idx, mask = ar.inp("V", t["V"]), ar.inp("E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"])
    S, rank = ar.inp("S", t["S"]), ar.inp("rank", t["rank"])
    oV, oE = ar.out("h_V", f32, (B, N, H)), ar.out("h_E", f32, (B, N, K, H))
    lp, lg = ar.out("log_probs", f32, (B, N, V33)), ar.out("logits", f32, (B, N, V33))
    ws = ar.ws("ws", 2 * env.L.namp_workspace_bytes(B, B, N, K))

    def call():
        old = env.L.namp_set_persistent(1 if persistent else 0)
        try:
            with precision(env, prec):
                return env.L.namp_encdec_fwd(env.packed.model(), Vv.ptr, E.ptr, idx.ptr, mask.ptr, S.ptr, rank.ptr, oV.ptr, oE.ptr, lp.ptr, lg.ptr,
                                             ws.ptr, ws.nbytes, B, N, K, env.s())
        finally:
            env.L.namp_set_persistent(old)
    return call


@row("namp_bf16s_message", ids(cross(SHAPES, [0, 1])))
def _bf16s_message(ar, env, case):
    B, N, K, mode = case
    t = graph_case(B, N, K)
    K = t["K"]
    g = gen(7)
    G, tpn = B * N, (K + 15) // 16
    hE = ar.inp("hE16", t["E"].to(bf16))                      # rows of 128 bf16 (fragment order: any permutation of a row's channels)
    idx, mask, rank = ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
    Pa, P0, P1 = (ar.inp(nm, rn(g, G, H).to(bf16)) for nm in ("Pa16", "Pj016", "Pj116"))
    partial = ar.out("partial", f32, (G * tpn * (H + 1),))    # [G][tpn][128] K-sums + [G][tpn] weight sums
    lay = "enc1." if mode == 0 else "dec1."
    w1 = env.a(lay + ("W1b_simg" if mode == 0 else "W1e_simg"))
    return lambda: env.L.namp_bf16s_message(mode, hE.ptr, idx.ptr, mask.ptr, rank.ptr if mode else None, Pa.ptr, P0.ptr, P1.ptr if mode else None,
                                            w1, env.a(lay + "W2_simg"), env.a(lay + "b2"), partial.ptr, B, B, N, K, env.s())


# ---- the building blocks the layer-level operators are made of ---------------------------------------------------------------
def table_inputs(ar, G, g, names):
    return [ar.inp(nm, rn(g, G, H)) for nm in names]


def partial_floats(G, K):
    return G * ((K + 15) // 16) * (H + 1)                     # [G][ceil(K/16)][128] K-sums + [G][ceil(K/16)] weight sums


@row("namp_enc_message", ids(cross(SHAPES, PRECS)))
def _enc_message(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K = t["K"]
    hE, idx, mask = ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"])
    Pa, Pc = table_inputs(ar, B * N, gen(60), ("Pa", "Pc"))
    partial = ar.out("partial", f32, (partial_floats(B * N, K),))
    return with_precision(env, prec, lambda: env.L.namp_enc_message(env.packed.enc_layer(1), hE.ptr, idx.ptr, mask.ptr, None, Pa.ptr, Pc.ptr,
                                                                    partial.ptr, B, N, K, env.s()))


@row("namp_enc_edge_update", ids(cross(SHAPES, PRECS)))
def _enc_edge_update(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K = t["K"]
    hE, idx = ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
    Pa, Pc = table_inputs(ar, B * N, gen(61), ("Pa", "Pc"))
    out = ar.out("h_E_out", f32, (B, N, K, H))
    return with_precision(env, prec, lambda: env.L.namp_enc_edge_update(env.packed.enc_layer(1), hE.ptr, idx.ptr, Pa.ptr, Pc.ptr, out.ptr,
                                                                        B, N, K, env.s()))


def enc_projs(env, outs, lay="enc1."):
    NP = env.hip.NampProj
    a = lambda nm: env.a(lay + nm)
    return (NP * 3)(NP(a("W11a_img"), a("b11"), None, outs[0].ptr), NP(a("W11c_img"), None, None, outs[1].ptr),
                    NP(a("W1a_img"), a("b1"), None, outs[2].ptr))


@row("namp_node_update", ids(cross(SHAPES, ["m3", "whole"])))
def _node_update(ar, env, case):
    B, N, K, kind = case
    t = graph_case(B, N, K)
    K, G = t["K"], B * N
    g = gen(62)
    hV, mask = ar.inp("h_V", t["V"]), ar.inp("mask", t["mask"])
    tpn = (K + 15) // 16
    # m3 given: K-sums + weight sums as namp_enc_message writes them; m3 NULL: [G][T][128] whole messages
    partial = ar.inp("partial", rn(g, partial_floats(G, K), sc=0.1) if kind == "m3" else rn(g, G, tpn, H, sc=0.1))
    hVo = ar.out("h_V_out", f32, (G, H))
    outs = [ar.out(f"proj{q}.out", f32, (G, H)) for q in range(3)]
    a = lambda nm: env.a("enc1." + nm)
    return lambda: env.L.namp_node_update(a("ln1_g"), a("ln1_b"), a("Win_img"), a("b_in"), a("Wout_img"), a("b_out"), a("ln2_g"), a("ln2_b"), hV.ptr,
                                          partial.ptr, a("W3_img") if kind == "m3" else None, a("b3") if kind == "m3" else None, mask.ptr, hVo.ptr,
                                          enc_projs(env, outs), 3, None, G, K, env.s())


@row("namp_dec_message", ids(cross(SHAPES, PRECS)))
def _dec_message(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K = t["K"]
    hE, idx, rank = ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("rank", t["rank"])
    Pa, Pbw, Pfw = table_inputs(ar, B * N, gen(63), ("Pa", "Pbw", "Pfw"))
    partial = ar.out("partial", f32, (partial_floats(B * N, K),))
    return with_precision(env, prec, lambda: env.L.namp_dec_message(env.packed.dec_layer(1), hE.ptr, idx.ptr, rank.ptr, Pa.ptr, Pbw.ptr, Pfw.ptr,
                                                                    partial.ptr, B, B, N, K, env.s()))


@row("namp_enc_message_update", ids(cross(SHAPES, PRECS)))
def _enc_message_update(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K, G = t["K"], B * N
    hE, idx, mask, hV = ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"]), ar.inp("h_V", t["V"])
    Pa, Pc = table_inputs(ar, G, gen(64), ("Pa", "Pc"))
    hVo = ar.out("h_V_out", f32, (G, H))
    outs = [ar.out(f"proj{q}.out", f32, (G, H)) for q in range(3)]
    return with_precision(env, prec, lambda: env.L.namp_enc_message_update(env.packed.enc_layer(1), hE.ptr, idx.ptr, mask.ptr, None, Pa.ptr, Pc.ptr,
                                                                           hV.ptr, hVo.ptr, enc_projs(env, outs), 3, B, N, K, env.s()))


@row("namp_enc_edge_message_update", ids(SHAPES))
def _enc_edge_message_update(ar, env, case):
    B, N, K = case
    t = graph_case(B, N, K)
    K, G = t["K"], B * N
    hE = ar.inout("h_E", t["E"])                              # updated IN PLACE
    idx, mask, hV = ar.inp("E_idx", t["E_idx"]), ar.inp("mask", t["mask"]), ar.inp("h_V", t["V"])
    ePa, ePc, Pa, Pc = table_inputs(ar, G, gen(65), ("ePa", "ePc", "Pa", "Pc"))
    hVo = ar.out("h_V_out", f32, (G, H))
    outs = [ar.out(f"proj{q}.out", f32, (G, H)) for q in range(3)]
    return with_precision(env, "fp32", lambda: env.L.namp_enc_edge_message_update(
        env.packed.enc_layer(1), ePa.ptr, ePc.ptr, hE.ptr, env.packed.enc_layer(2), idx.ptr, mask.ptr, None, Pa.ptr, Pc.ptr, hV.ptr, hVo.ptr,
        enc_projs(env, outs, "enc2."), 3, B, N, K, env.s()))


@row("namp_dec_message_update", ids(cross(SHAPES, PRECS, ["head", "nohead"])))
def _dec_message_update(ar, env, case):
    B, N, K, prec, head = case
    t = graph_case(B, N, K)
    K, G = t["K"], B * N
    hE, idx, rank = ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"]), ar.inp("rank", t["rank"])
    hV, mask, S = ar.inp("h_V", t["V"]), ar.inp("mask", t["mask"]), ar.inp("S", t["S"])
    Pa, Pbw, Pfw = table_inputs(ar, G, gen(66), ("Pa", "Pbw", "Pfw"))
    hVo = ar.out("h_V_out", f32, (G, H))
    outs = [ar.out(f"proj{q}.out", f32, (G, H)) for q in range(2)]
    lp = ar.out("log_probs", f32, (G, V33)) if head == "head" else None
    lg = ar.out("logits", f32, (G, V33)) if head == "head" else None
    NP = env.hip.NampProj
    b = lambda nm: env.a("dec1." + nm)

    def call():
        proj = (NP * 2)(NP(b("W1a_img"), b("b1"), None, outs[0].ptr), NP(b("W1v_img"), None, b("tok"), outs[1].ptr))
        return env.L.namp_dec_message_update(env.packed.dec_layer(1), hE.ptr, idx.ptr, rank.ptr, Pa.ptr, Pbw.ptr, Pfw.ptr, hV.ptr, mask.ptr, hVo.ptr,
                                             proj, 2, S.ptr, env.a("Wout_w") if lp else None, env.a("Wout_b") if lp else None,
                                             lp.ptr if lp else None, lg.ptr if lg else None, V33, B, B, N, K, env.s())
    return with_precision(env, prec, call)


@row("namp_node_linear_prec", ids(cross(SHAPES, [0, 1, 2])))
def _node_linear_prec(ar, env, case):
    B, N, K, prec = case
    G = B * N
    X = ar.inp("X", graph_case(B, N, K)["V"])
    outs = [ar.out(f"proj{q}.out", f32, (G, H)) for q in range(2)]
    NP = env.hip.NampProj
    sfx = "_img" if prec == 0 else "_ximg"                    # fp32 fragment images for code 0, x3 images for 1 / 2

    def call():
        proj = (NP * 2)(NP(env.a("enc0.W1a" + sfx), env.a("enc0.b1"), None, outs[0].ptr), NP(env.a("enc0.W1c" + sfx), None, None, outs[1].ptr))
        return env.L.namp_node_linear_prec(X.ptr, G, proj, 2, prec, env.s())
    return call


@row("namp_node_linear_sum", ids(cross(SHAPES, [0, 1, 2])))
def _node_linear_sum(ar, env, case):
    B, N, K, prec = case
    G = B * N
    Xs = table_inputs(ar, G, gen(67), ("X0", "X1", "X2"))
    out = ar.out("out", f32, (G, H))
    sfx = "_img" if prec == 0 else "_ximg"
    arr = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)
    return lambda: env.L.namp_node_linear_sum(arr([x.ptr for x in Xs]), arr([env.a("enc0." + nm + sfx) for nm in ("W1a", "W1c", "W11a")]), 3,
                                              out.ptr, G, prec, env.s())


# ---- weight packing ------------------------------------------------------------------------------------------------------------
def _pack_row(symbol, floats, general=False):
    @row(symbol, ids(["col0_0", "col0_128"] if not general else ["512x128", "128x512", "128x128_col128"]))
    def build(ar, env, case):
        g = gen(68)
        if general:
            out_f, in_f, ld, col0 = {"512x128": (4 * H, H, H, 0), "128x512": (H, 4 * H, 4 * H, 0), "128x128_col128": (H, H, 3 * H, H)}[case]
        else:
            out_f, in_f, ld, col0 = H, H, 3 * H, (0 if case == "col0_0" else H)
        W = ar.inp("W", rn(g, out_f, ld))
        img = ar.out("img", f32, (out_f * in_f if general else floats,))
        fn = getattr(env.L, symbol)
        if general:
            return lambda: fn(W.ptr, ld, col0, out_f, in_f, img.ptr, env.s())
        return lambda: fn(W.ptr, ld, col0, img.ptr, env.s())
    return build


_pack_row("namp_pack_image", None, general=True)
_pack_row("namp_pack_image_x3_general", None, general=True)
_pack_row("namp_pack_image_bf16", H * H // 2)                 # 32 KiB
_pack_row("namp_pack_image_bf16_32", H * H // 2)
_pack_row("namp_pack_image_x3", H * H)                        # 64 KiB


@row("namp_pack_feat_x3", ids(["edge_embedding"]))
def _pack_feat_x3(ar, env, case):
    W = ar.inp("W", rn(gen(69), H, 5200, sc=0.05))
    img = ar.out("img", f32, (H * 5200,))
    return lambda: env.L.namp_pack_feat_x3(W.ptr, 5200, img.ptr, env.s())



# ==== from coordinates ======================================================================================================
@functools.lru_cache(maxsize=4)
def complex_case(B, L):
    from na_mpnn_amd import synth
    cx = [synth.make_complex(seed=600 + 17 * b + L, n=L, n_chains=min(3, L), masked_frac=0.08 if L >= 17 else 0.0, missing_atom_frac=0.05)
          for b in range(B)]
    t = {k: torch.from_numpy(np.stack([c[k] for c in cx])) for k in cx[0]}
    for b in range(1, B):
        t["mask"][b, L - (3 * b + 2):] = 0
    return t


FEAT_INTS = ("X_m", "mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask")


def _featurize_common(ar, env, case):
    B, L, top_k, what, split, prec = case
    t = complex_case(B, L)
    K = min(top_k, L)
    X = ar.inp("X", t["X"])
    ints = [ar.inp(nm, t[nm].to(i32)) for nm in FEAT_INTS]
    idx = ar.out("E_idx", i32, (B, L, K))
    E = ar.out("E", f32, (B, L, K, H)) if what in ("E", "both") else None
    hE = ar.out("h_E", f32, (B, L, K, H)) if what in ("hE", "both") else None
    nbytes = env.L.namp_featurize_workspace_bytes(B, L) + (env.L.namp_featurize_split_bytes(B, L, top_k) if split == "split" else 0)
    ws = ar.ws("ws", nbytes)
    head = lambda: (env.packed.model(), X.ptr, *[x.ptr for x in ints], top_k, 15, idx.ptr, E.ptr if E else None, hE.ptr if hE else None,
                    ws.ptr, ws.nbytes, B, L)
    return head, t


FEAT_CASES = ids(cross(SHAPES, ["E", "hE", "both"], ["nosplit", "split"], ["x3"]) + cross([(3, 65, 17), (1, 97, 48)], ["both"], ["split"], ["fp32"]))


@row("namp_featurize", FEAT_CASES)
def _featurize(ar, env, case):
    head, _t = _featurize_common(ar, env, case)
    return with_precision(env, case[-1], lambda: env.L.namp_featurize(*head(), env.s()))


@row("namp_featurize_ordered", FEAT_CASES)
def _featurize_ordered(ar, env, case):
    B, L = case[0], case[1]
    head, t = _featurize_common(ar, env, case)
    g = gen(8)
    om = ar.inp("order_mask", t["mask"].float())
    ocm = ar.inp("order_chain_mask", (torch.rand(B, L, generator=g) > 0.3).float())
    randn = ar.inp("randn", rn(g, B, L))
    o64, o32, r32 = ar.out("order64", i64, (B, L)), ar.out("order32", i32, (B, L)), ar.out("rank32", i32, (B, L))
    return with_precision(env, case[-1], lambda: env.L.namp_featurize_ordered(*head(), om.ptr, ocm.ptr, randn.ptr, o64.ptr, o32.ptr, r32.ptr, B,
                                                                              env.s()))


# ==== sampler and plans =====================================================================================================
KS = 17


@functools.lru_cache(maxsize=4)
def sampler_case(N, bs):
    """One complex, `bs` streams: fixed residues (chain_mask 0), masked residues, one symmetry group of three residues; every stream walks
    the visit order of stream 0 (as symmetry-tied sampling does)."""
    from na_mpnn_amd.model import symmetry_visits
    t = dict(graph_case(1, N, KS))
    g = gen(900 + N + bs)
    chain = (torch.rand(1, N, generator=g) > 0.2).to(i32)
    order0 = t["order"][0].tolist()
    visits, gf, gl, wl = symmetry_visits([[3, 10, 20]], [[0.5, 0.3, 0.2]], order0, N)
    order = torch.tensor(visits, dtype=i32).repeat(bs, 1)
    rank = torch.empty_like(order).scatter_(1, order.long(), torch.arange(N, dtype=i32).expand(bs, -1).contiguous())
    t.update(chain_mask=chain * t["mask"], order=order, rank=rank, group_first=torch.tensor(gf, dtype=i32).repeat(bs, 1),
             group_last=torch.tensor(gl, dtype=i32).repeat(bs, 1), sym_w=torch.tensor(wl, dtype=f32).view(1, N),
             uniform=torch.rand(bs, N, generator=g), bias=rn(g, 1, N, V33, sc=0.1), mask_dec=t["mask"].repeat(bs, 1),
             order_plain=t["order"].repeat(bs, 1) if bs == 1 else torch.stack([torch.randperm(N, generator=g) for _ in range(bs)]).to(i32))
    rp = torch.empty_like(t["order_plain"]).scatter_(1, t["order_plain"].long(), torch.arange(N, dtype=i32).expand(bs, -1).contiguous())
    t["rank_plain"] = rp
    return t


SPECIAL = sum(1 << k for k in (20, 25, 30, 31, 32))          # a set of never-drawn tokens (the model's UNK / DX / RX / MAS / PAD lanes)


@row("namp_decoding_order", ids(cross(SAMPLER, ["chain", "nochain"])))
def _decoding_order(ar, env, case):
    N, bs, chain = case
    g = gen(9)
    Bm = 1
    mask = ar.inp("mask", (torch.rand(Bm, N, generator=g) > 0.1).float())
    cm = ar.inp("chain_mask", (torch.rand(Bm, N, generator=g) > 0.3).float()) if chain == "chain" else None
    randn = ar.inp("randn", rn(g, bs, N))
    o64, o32, r32 = ar.out("order64", i64, (bs, N)), ar.out("order32", i32, (bs, N)), ar.out("rank32", i32, (bs, N))
    return lambda: env.L.namp_decoding_order(mask.ptr, cm.ptr if cm else None, randn.ptr, o64.ptr, o32.ptr, r32.ptr, bs, Bm, N, env.s())


@row("namp_sample_levels", ids(SAMPLER))
def _sample_levels(ar, env, case):
    N, bs = case
    t = sampler_case(N, bs)
    idx, order, rank = ar.inp("E_idx", t["E_idx"]), ar.inp("order", t["order_plain"]), ar.inp("rank", t["rank_plain"])
    level = ar.out("level", i32, (bs, N))
    return lambda: env.L.namp_sample_levels(idx.ptr, order.ptr, rank.ptr, level.ptr, bs, 1, N, KS, env.s())


def dep_idx_of(N, g):
    d = torch.full((1, N, 2), -1, dtype=i32)
    d[0, ::5, 0] = torch.randint(0, N, (len(range(0, N, 5)),), generator=g).to(i32)
    return d


@row("namp_sample_levels_dep", ids(cross(SAMPLER, ["plain", "groups", "deps"])))
def _sample_levels_dep(ar, env, case):
    N, bs, kind = case
    t = sampler_case(N, bs)
    grouped = kind == "groups"
    idx = ar.inp("E_idx", t["E_idx"])
    order, rank = ar.inp("order", t["order" if grouped else "order_plain"]), ar.inp("rank", t["rank" if grouped else "rank_plain"])
    dep = ar.inp("dep_idx", dep_idx_of(N, gen(10))) if kind == "deps" else None
    gf = ar.inp("group_first", t["group_first"]) if grouped else None
    gl = ar.inp("group_last", t["group_last"]) if grouped else None
    level = ar.out("level", i32, (bs, N))
    return lambda: env.L.namp_sample_levels_dep(idx.ptr, order.ptr, rank.ptr, dep.ptr if dep else None, 2 if dep else 0, gf.ptr if gf else None,
                                                gl.ptr if gl else None, level.ptr, bs, 1, N, KS, env.s())


def device_levels(env, t, bs, N, grouped):
    """Levels by visit, computed by the library on plain device tensors (an input of the rows below, not under test there)."""
    d = lambda x: x.to(env.dev).contiguous()
    idx, order, rank = d(t["E_idx"]), d(t["order" if grouped else "order_plain"]), d(t["rank" if grouped else "rank_plain"])
    gf, gl = (d(t["group_first"]), d(t["group_last"])) if grouped else (None, None)
    level = torch.empty(bs, N, dtype=i32, device=env.dev)
    env.hip.check(env.L.namp_sample_levels_dep(idx.data_ptr(), order.data_ptr(), rank.data_ptr(), None, 0, env.hip.ptr(gf), env.hip.ptr(gl),
                                               level.data_ptr(), bs, 1, N, KS, env.s()), "sample_levels_dep")
    torch.cuda.synchronize()
    return level.cpu()


def sort_items_within_levels(work, level_off, nwork):
    """namp_sample_work_lists leaves the order inside a level undefined (its items are independent): compare the sorted levels."""
    w = work.view(-1, 2).long()
    key = w[:, 0] * (1 << 20) + w[:, 1]
    pos = torch.arange(w.shape[0], device=w.device)
    seg = torch.searchsorted(level_off.long().contiguous(), pos, right=True)
    perm = torch.argsort(seg * (1 << 40) + key)
    return work.view(-1, 2)[perm].contiguous()


@row("namp_sample_work_lists", ids(SAMPLER))
def _sample_work_lists(ar, env, case):
    N, bs = case
    level = ar.inp("level", device_levels(env, sampler_case(N, bs), bs, N, False))
    work, off, nl = ar.out("work", i32, (bs * N, 2)), ar.out("level_off", i32, (N + 2,)), ar.out("n_levels", i32, (1,))
    call = lambda: env.L.namp_sample_work_lists(level.ptr, work.ptr, off.ptr, nl.ptr, bs, N, env.s())

    def canon(outs):
        outs["work"] = sort_items_within_levels(outs["work"], outs["level_off"], bs * N)
        return outs
    return call, dict(canon=canon)


def sampler_args(ar, env, t, N, bs, grouped, forced):
    """The arguments the three samplers share (include/namp.h: namp_decoder_sample), registered in the arena."""
    g = gen(11)
    a = dict(h_V=ar.inp("h_V_enc", t["V"]), h_E=ar.inp("h_E", t["E"]), idx=ar.inp("E_idx", t["E_idx"]), mask=ar.inp("mask", t["mask"]),
             mask_dec=ar.inp("mask_dec", t["mask_dec"]), chain=ar.inp("chain_mask", t["chain_mask"]), S_true=ar.inp("S_true", t["S"]),
             bias=ar.inp("bias", t["bias"]), order=ar.inp("order", t["order" if grouped else "order_plain"]),
             rank=ar.inp("rank", t["rank" if grouped else "rank_plain"]), uniform=ar.inp("uniform", t["uniform"]),
             forced=ar.inp("S_forced", torch.randint(0, 20, (bs, N), generator=g).to(i32)) if forced else None,
             gf=ar.inp("group_first", t["group_first"]) if grouped else None, gl=ar.inp("group_last", t["group_last"]) if grouped else None,
             sw=ar.inp("sym_weights", t["sym_w"]) if grouped else None)
    a["S_out"], a["probs"], a["logp"] = ar.out("S_out", i32, (bs, N)), ar.out("probs_out", f32, (bs, N, V33)), ar.out("logp_out", f32, (bs, N, V33))
    a["ws"] = ar.ws("ws", env.L.namp_sample_workspace_bytes_n(1, bs, N, KS, env.packed.n_dec))     # the model's real n_dec, not the 8-layer bound
    p = lambda b: b.ptr if b is not None else None
    common = lambda: (env.packed.model(), a["h_V"].ptr, a["h_E"].ptr, a["idx"].ptr, a["mask"].ptr, a["mask_dec"].ptr, a["chain"].ptr, a["S_true"].ptr,
                      a["bias"].ptr, a["order"].ptr, a["rank"].ptr, a["uniform"].ptr, p(a["forced"]), p(a["gf"]), p(a["gl"]), p(a["sw"]), None)
    tail = lambda: (0.7, SPECIAL, a["S_out"].ptr, a["probs"].ptr, a["logp"].ptr, a["ws"].ptr, a["ws"].nbytes, bs, 1, N, KS, env.s())
    return common, tail


@row("namp_decoder_sample", ids(cross(SAMPLER, ["plain", "groups", "forced"])))
def _decoder_sample(ar, env, case):
    N, bs, kind = case
    common, tail = sampler_args(ar, env, sampler_case(N, bs), N, bs, kind == "groups", kind == "forced")
    return lambda: env.L.namp_decoder_sample(*common(), *tail())


def host_work_lists(env, t, bs, N, grouped, split):
    from na_mpnn_amd.model import level_work_lists
    level = device_levels(env, t, bs, N, grouped)
    gf, gl = (t["group_first"], t["group_last"]) if grouped else (None, None)
    order0 = (t["order"] if grouped else t["order_plain"])[0]
    sel, flat, work_n, close, close_off = level_work_lists(level, gf, gl, order0, t["E_idx"][0].long(), split=split)
    work = torch.stack((sel // N, sel % N), 1).to(i32).contiguous()
    hist = torch.zeros(N + 1, dtype=i64).scatter_add_(0, flat, torch.ones_like(flat))
    level_off = torch.cat((hist.new_zeros(1), hist.cumsum(0))).to(i32).contiguous()
    return work, work_n, level_off, close, close_off, torch.bincount(flat).tolist()


@row("namp_decoder_sample_levels", ids(cross(SAMPLER, ["plain", "groups"])))
def _decoder_sample_levels(ar, env, case):
    N, bs, kind = case
    t = sampler_case(N, bs)
    grouped = kind == "groups"
    work_t, work_n_t, _off, _c, _co, counts = host_work_lists(env, t, bs, N, grouped, False)
    common, tail = sampler_args(ar, env, t, N, bs, grouped, False)
    work = ar.inp("work", work_t)
    work_n = ar.inp("work_n", work_n_t.to(i32)) if grouped else None
    counts_c = (C.c_int32 * len(counts))(*counts)             # HOST array (the header says so): outside the arena
    return lambda: env.L.namp_decoder_sample_levels(*common(), work.ptr, work_n.ptr if work_n else None, counts_c, len(counts), *tail())


@row("namp_decoder_sample_walk", ids(cross(SAMPLER, ["plain", "groups", "deferred"])))
def _decoder_sample_walk(ar, env, case):
    N, bs, kind = case
    t = sampler_case(N, bs)
    grouped = kind != "plain"
    assert env.L.namp_decoder_sample_walk_grid(bs, N, KS) > 0
    work_t, work_n_t, off_t, close_t, close_off_t, _counts = host_work_lists(env, t, bs, N, grouped, kind == "deferred")
    common, tail = sampler_args(ar, env, t, N, bs, grouped, False)
    work, off = ar.inp("work", work_t), ar.inp("level_off", off_t)
    work_n = ar.inp("work_n", work_n_t.to(i32)) if grouped else None
    close = close_off = zbuf = None
    if kind == "deferred":
        close, close_off = ar.inp("close", close_t), ar.inp("close_off", close_off_t)
        zbuf = ar.ws("zbuf", bs * N * V33 * 4)                # scratch (float [B_dec][N][vocab])
    nwork = work_t.shape[0]
    p = lambda b: b.ptr if b is not None else None
    return lambda: env.L.namp_decoder_sample_walk(*common(), work.ptr, p(work_n), nwork, off.ptr, p(close), p(close_off), p(zbuf), *tail())


@row("namp_states_plan", ids(SAMPLER))
def _states_plan(ar, env, case):
    N, bs = case
    M, K = 2, KS
    t = graph_case(2, N, K)
    idx = ar.inp("E_idx", t["E_idx"])
    order0, rank0 = ar.inp("order0", t["order"][0]), ar.inp("rank0", t["rank"][0])
    wts = ar.inp("weights", torch.tensor([0.6, 0.4]))
    o = lambda nm, dt, *shape: ar.out(nm, dt, shape)
    E_flat = o("E_flat", i32, M * N, K)
    order, rank, gf, gl = (o(nm, i32, bs, M * N) for nm in ("order", "rank", "group_first", "group_last"))
    sym_w, work_n, level = o("sym_w", f32, M * N), o("work_n", i32, bs * M * N), o("level", i32, N)
    work, level_off, n_levels = o("work", i32, bs * M * N, 2), o("level_off", i32, M * N + 2), o("n_levels", i32, 1)
    close, close_off = o("close", i32, bs * N, 2), o("close_off", i32, M * N + 2)
    return lambda: env.L.namp_states_plan(idx.ptr, order0.ptr, rank0.ptr, wts.ptr, E_flat.ptr, order.ptr, rank.ptr, gf.ptr, gl.ptr, sym_w.ptr,
                                          work_n.ptr, level.ptr, work.ptr, level_off.ptr, n_levels.ptr, close.ptr, close_off.ptr, bs, M, N, K, env.s())


def two_strands(N):
    """One two-strand pair set: residues 2..9 paired with 29..22 (antiparallel), the strand listed first flagged."""
    partner, first = [-1] * N, [0] * N
    for i in range(2, 10):
        j = 31 - i
        partner[i], partner[j], first[i] = j, i, 1
    return torch.tensor(partner, dtype=i32), torch.tensor(first, dtype=i32), 8


@row("namp_pairs_plan", ids(SAMPLER))
def _pairs_plan(ar, env, case):
    N, bs = case
    t = graph_case(1, N, KS)
    partner_t, first_t, _np = two_strands(N)
    partner, first = ar.inp("partner", partner_t), ar.inp("first", first_t)
    order0, rank0 = ar.inp("order0", t["order"][0]), ar.inp("rank0", t["rank"][0])
    order, rank, gf, gl = (ar.out(nm, i32, (bs, N)) for nm in ("order", "rank", "group_first", "group_last"))
    return lambda: env.L.namp_pairs_plan(partner.ptr, first.ptr, order0.ptr, rank0.ptr, order.ptr, rank.ptr, gf.ptr, gl.ptr, bs, N, env.s())


@row("namp_pairs_work_lists", ids(SAMPLER))
def _pairs_work_lists(ar, env, case):
    N, bs = case
    t = graph_case(1, N, KS)
    partner_t, first_t, npairs = two_strands(N)
    d = lambda x: x.to(env.dev).contiguous()
    pa, fi, o0, r0, idx = d(partner_t), d(first_t), d(t["order"][0]), d(t["rank"][0]), d(t["E_idx"])
    po, pr, pgf, pgl, plevel = (torch.empty(bs, N, dtype=i32, device=env.dev) for _ in range(5))
    env.hip.check(env.L.namp_pairs_plan(pa.data_ptr(), fi.data_ptr(), o0.data_ptr(), r0.data_ptr(), po.data_ptr(), pr.data_ptr(), pgf.data_ptr(),
                                        pgl.data_ptr(), bs, N, env.s()), "pairs_plan")
    env.hip.check(env.L.namp_sample_levels_dep(idx.data_ptr(), po.data_ptr(), pr.data_ptr(), None, 0, pgf.data_ptr(), pgl.data_ptr(),
                                               plevel.data_ptr(), bs, 1, N, KS, env.s()), "sample_levels_dep")
    torch.cuda.synchronize()
    level, gf = ar.inp("level", plevel[0].cpu()), ar.inp("group_first", pgf.cpu())
    items = bs * (N - npairs)                                 # the header: "the number of items is B_dec * (N - pairs)"
    work, work_n = ar.out("work", i32, (bs * N, 2), compare=2 * items), ar.out("work_n", i32, (bs * N,), compare=items)
    off, nl = ar.out("level_off", i32, (N + 2,)), ar.out("n_levels", i32, (1,))
    return lambda: env.L.namp_pairs_work_lists(level.ptr, gf.ptr, work.ptr, work_n.ptr, off.ptr, nl.ptr, bs, N, env.s())


@row("namp_decoder_loo", ids(cross(SHAPES, ["x3", "fp32"])))
def _decoder_loo(ar, env, case):
    B, N, K, prec = case
    t = graph_case(B, N, K)
    K = t["K"]
    hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
    S, mask, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
    lp, counts = ar.out("log_probs", f32, (B, N, V33)), ar.out("counts", i32, (2,))
    ws = ar.ws("ws", env.L.namp_loo_workspace_bytes(B, N, K, env.packed.n_dec))
    return with_precision(env, prec, lambda: env.L.namp_decoder_loo(env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, mask.ptr, rank.ptr, lp.ptr,
                                                                    counts.ptr, ws.ptr, ws.nbytes, B, N, K, env.s()))


# ==== training ==============================================================================================================
def row_dtype(prec):
    return bf16 if prec == 2 else f32


def edge_inputs(ar, B, N, K, seed):
    g = gen(seed)
    K = min(K, N)
    d = dict(h_E=ar.inp("h_E", rn(g, B, N, K, H)), idx=ar.inp("E_idx", rand_idx(g, B, N, K)), mask=ar.inp("mask", padded_mask(g, B, N)),
             rank=ar.inp("rank", torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(i32)),
             Pa=ar.inp("Pa", rn(g, B * N, H)), Pj0=ar.inp("Pj0", rn(g, B * N, H)), Pj1=ar.inp("Pj1", rn(g, B * N, H)))
    return d, K, g


@row("namp_train_edge_fwd", ids(cross(SHAPES, [0, 1, 2], [0, 1, 2])))
def _train_edge_fwd(ar, env, case):
    B, N, K, mode, prec = case
    d, K, g = edge_inputs(ar, B, N, K, 20)
    G, tpn = B * N, (K + 15) // 16
    out = ar.out("out", f32, (G * tpn * (H + 1),) if mode != 2 else (G * K, H))
    ln = mode == 2
    lay = "enc1."
    imgs = [env.img(prec, lay + nm) for nm in (("W11b", "W12", "W13") if ln else ("W1b", "W2", "W3"))]
    return lambda: env.L.namp_train_edge_fwd(
        mode, d["h_E"].ptr, d["idx"].ptr, d["mask"].ptr if mode == 0 else None, None, d["rank"].ptr if mode == 1 else None, d["Pa"].ptr,
        d["Pj0"].ptr, d["Pj1"].ptr if mode == 1 else None, *imgs, env.a(lay + "b2"), env.a(lay + "b3"), env.a(lay + "ln3_g") if ln else None,
        env.a(lay + "ln3_b") if ln else None, 0.1 if ln else 0.0, 77, out.ptr, prec, B, N, K, env.s())


@row("namp_train_edge_bwd", ids(cross(SHAPES, [0, 1, 2], [1, 2])))
def _train_edge_bwd(ar, env, case):
    B, N, K, mode, prec = case
    d, K, g = edge_inputs(ar, B, N, K, 21)
    G, E, rdt = B * N, B * N * min(K, N), row_dtype(prec)
    g_out = ar.inp("g_out", rn(g, E, H) if mode == 2 else rn(g, G, H))
    g_in = ar.inp("g_hE_in", rn(g, E, H)) if mode != 2 else None
    A1, G1, G2 = (ar.out(nm, rdt, (E, H)) for nm in ("A1", "G1", "G2"))
    A2 = ar.out("A2", rdt, (E, H)) if mode == 2 else None
    g_hE = ar.out("g_hE", f32, (E, H))
    tiles = K % 16 == 0
    g_Pa = ar.out("g_Pa", f32, (E // 16, H)) if tiles else ar.inout("g_Pa", torch.zeros(G, H))
    g_Pj0 = ar.inout("g_Pj0", torch.zeros(G, H))
    g_Pj1 = ar.inout("g_Pj1", torch.zeros(G, H)) if mode == 1 else None
    lay = "enc1."
    nm = ("W11b", "W12", "W13") if mode == 2 else ("W1b", "W2", "W3")
    i1, i2, i3 = (env.img(prec, lay + x) for x in nm)         # (any image of the operand format serves as the transposed block's)
    p = lambda b: b.ptr if b is not None else None
    code = prec | (4 if mode != 2 else 0) | (8 if tiles else 0)
    call = lambda: env.L.namp_train_edge_bwd(
        mode, d["h_E"].ptr, d["idx"].ptr, d["mask"].ptr if mode == 0 else None, None, d["rank"].ptr if mode == 1 else None, d["Pa"].ptr,
        d["Pj0"].ptr, d["Pj1"].ptr if mode == 1 else None, i1, i2, i3 if mode == 2 else None, i2, i1, env.a(lay + "b2"), g_out.ptr, A1.ptr, p(A2),
        G1.ptr, G2.ptr, None, g_hE.ptr, p(g_in), g_Pa.ptr, g_Pj0.ptr, p(g_Pj1), None, None, code, B, N, K, env.s())
    return call, atomic(prec, None if tiles else "g_Pa", "g_Pj0", "g_Pj1" if mode == 1 else None)


@row("namp_train_edge_bwd_dw", ids(cross(SHAPES, [0, 1], [1, 2])))
def _train_edge_bwd_dw(ar, env, case):
    B, N, K, mode, prec = case
    d, K, g = edge_inputs(ar, B, N, K, 24)
    G, E = B * N, B * N * K
    Ep, n = env.L.namp_train_edge_bwd_dw_rows(B, N, K), env.L.namp_train_edge_bwd_dw_groups(B, N, K)
    g_out, g_in = ar.inp("g_out", rn(g, G, H)), ar.inp("g_hE_in", rn(g, E, H))
    # G1 and g_hE hold namp_train_edge_bwd_dw_rows() rows: the launch stores whole 64-row rounds, the rows past B*N*K are padding
    G1 = ar.out("G1", row_dtype(prec), (Ep, H), compare=E * H)
    g_hE = ar.out("g_hE", f32, (Ep, H), compare=E * H)
    tiles = K % 16 == 0
    g_Pa = ar.out("g_Pa", f32, (Ep // 16, H), compare=(E // 16) * H) if tiles else ar.inout("g_Pa", torch.zeros(G, H))
    dW, db = ar.out("dW_part", f32, (n, 2, H, H)), ar.out("db_part", f32, (n, H))
    lay = "enc1." if mode == 0 else "dec1."
    i1, i2 = env.img(prec, lay + ("W1b" if mode == 0 else "W1e")), env.img(prec, lay + "W2")
    code = prec | 4 | (8 if tiles else 0)
    return lambda: env.L.namp_train_edge_bwd_dw(
        mode, d["h_E"].ptr, d["idx"].ptr, d["mask"].ptr if mode == 0 else None, None, d["rank"].ptr if mode == 1 else None, d["Pa"].ptr,
        d["Pj0"].ptr, d["Pj1"].ptr if mode == 1 else None, i1, i2, i2, i1, env.a(lay + "b2"), g_out.ptr, G1.ptr, g_hE.ptr, g_in.ptr, g_Pa.ptr,
        dW.ptr, db.ptr, code, B, N, K, env.s()), atomic(prec, None if tiles else "g_Pa")


@row("namp_train_edge_update_bwd", ids(cross(SHAPES, [1, 2], [0.0, 0.1])))
def _train_edge_update_bwd(ar, env, case):
    B, N, K, prec, p_drop = case
    d, K, g = edge_inputs(ar, B, N, K, 22)
    G, E, rdt = B * N, B * N * K, row_dtype(prec)
    g_out = ar.inp("g_out", rn(g, E, H))
    A1, A2, G1, G2, G3 = (ar.out(nm, rdt, (E, H)) for nm in ("A1", "A2", "G1", "G2", "G3"))
    g_hE = ar.out("g_hE", f32, (E, H))
    tiles = K % 16 == 0
    g_Pa = ar.out("g_Pa", f32, (E // 16, H)) if tiles else ar.inout("g_Pa", torch.zeros(G, H))
    g_Pc = ar.inout("g_Pc", torch.zeros(G, H))
    part = ar.out("dgb_part", f32, (env.L.namp_train_edge_update_bwd_groups(B, N, K), 2, H))
    lay = "enc1."
    i1, i2, i3 = (env.img(prec, lay + x) for x in ("W11b", "W12", "W13"))
    return lambda: env.L.namp_train_edge_update_bwd(
        d["h_E"].ptr, d["idx"].ptr, d["Pa"].ptr, d["Pj0"].ptr, i1, i2, i3, i3, i2, i1, env.a(lay + "b12"), env.a(lay + "b13"), env.a(lay + "ln3_g"),
        p_drop, 4321, 0, g_out.ptr, A1.ptr, A2.ptr, G1.ptr, G2.ptr, G3.ptr, g_hE.ptr, g_Pa.ptr, g_Pc.ptr, part.ptr, prec | (8 if tiles else 0),
        B, N, K, env.s()), atomic(prec, None if tiles else "g_Pa", "g_Pc")


@row("namp_train_edge_update_bwd_dw", ids(cross(SHAPES, [0.0, 0.1])))
def _train_edge_update_bwd_dw(ar, env, case):
    B, N, K, p_drop = case
    d, K, g = edge_inputs(ar, B, N, K, 23)
    G, E = B * N, B * N * K
    Ep, n = env.L.namp_train_edge_bwd_dw_rows(B, N, K), env.L.namp_train_edge_bwd_dw_groups(B, N, K)
    g_out = ar.inp("g_out", rn(g, E, H))
    # row buffers hold namp_train_edge_bwd_dw_rows() rows: the launches store whole 64-row rounds, the rows past B*N*K are padding
    G2, G1 = ar.out("G2", bf16, (Ep, H), compare=E * H), ar.out("G1", bf16, (Ep, H), compare=E * H)
    g_hE = ar.out("g_hE", f32, (Ep, H), compare=E * H)
    tiles = K % 16 == 0
    g_Pa = ar.out("g_Pa", f32, (Ep // 16, H), compare=(E // 16) * H) if tiles else ar.inout("g_Pa", torch.zeros(G, H))
    dW, db, dgb = ar.out("dW_part", f32, (3 * n, H, H)), ar.out("db_part", f32, (2 * n, H)), ar.out("dgb_part", f32, (n, 2, H))
    lay = "enc1."
    i1, i2, i3 = (env.img(2, lay + x) for x in ("W11b", "W12", "W13"))
    return lambda: env.L.namp_train_edge_update_bwd_dw(
        d["h_E"].ptr, d["idx"].ptr, d["Pa"].ptr, d["Pj0"].ptr, i1, i2, i3, i3, i2, i1, env.a(lay + "b12"), env.a(lay + "b13"), env.a(lay + "ln3_g"),
        p_drop, 4321, g_out.ptr, G2.ptr, G1.ptr, g_hE.ptr, g_Pa.ptr, dW.ptr, db.ptr, dgb.ptr, 2 | (8 if tiles else 0), B, N, K, env.s()), \
        atomic(2, None if tiles else "g_Pa")


def probe_chunk(fn):
    """Rows per chunk / group of a row-count kernel, probed from its *_groups / *_chunks function (not read from the kernel source)."""
    r = 1
    while fn(r) == 1:
        r *= 2
    lo, hi = r // 2, r                                        # fn(lo) == 1 < fn(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fn(mid) == 1 else (lo, mid)
    return lo


def rows_of(case_rows, fn):
    return probe_chunk(fn) + 1 if case_rows == "chunk+1" else case_rows


@row("namp_train_tail_fwd", ids(cross(ROWS, [0.0, 0.1])))
def _train_tail_fwd(ar, env, case):
    G = rows_of(case[0], env.L.namp_train_tail_groups)
    g = gen(24)
    hV, dh, mask = ar.inp("h_V", rn(g, G, H)), ar.inp("dh", rn(g, G, H)), ar.inp("mask", padded_mask(g, 1, G).view(-1))
    out, x1, z, y = ar.out("out", f32, (G, H)), ar.out("x1", f32, (G, H)), ar.out("z", f32, (4, G, H)), ar.out("y", f32, (G, H))
    a = lambda nm: env.a("enc1." + nm)
    return lambda: env.L.namp_train_tail_fwd(hV.ptr, dh.ptr, mask.ptr, a("ln1_g"), a("ln1_b"), a("Win_ximg"), a("b_in"), a("Wout_ximg"), a("b_out"),
                                             a("ln2_g"), a("ln2_b"), case[1], 11, 12, out.ptr, x1.ptr, z.ptr, y.ptr, G, env.s())


@row("namp_train_tail_bwd", ids(cross(ROWS, [0.0, 0.1])))
def _train_tail_bwd(ar, env, case):
    G = rows_of(case[0], env.L.namp_train_tail_groups)
    g = gen(25)
    hV, dh, mask = ar.inp("h_V", rn(g, G, H)), ar.inp("dh", rn(g, G, H)), ar.inp("mask", padded_mask(g, 1, G).view(-1))
    x1, z, y, g_out = ar.inp("x1", rn(g, G, H)), ar.inp("z", rn(g, 4, G, H)), ar.inp("y", rn(g, G, H)), ar.inp("g_out", rn(g, G, H))
    g_hV, g_dh, g_f = (ar.out(nm, f32, (G, H)) for nm in ("g_hV", "g_dh", "g_f"))
    g_z, h = ar.out("g_z", f32, (4, G, H)), ar.out("h", f32, (4, G, H))
    part = ar.out("part", f32, (env.L.namp_train_tail_groups(G), 4, H))
    a = lambda nm: env.a("enc1." + nm)
    # (the images of the transposed blocks: W_out^T is [512 x 128] like W_in, W_in^T is [128 x 512] like W_out)
    return lambda: env.L.namp_train_tail_bwd(hV.ptr, dh.ptr, mask.ptr, a("ln1_g"), a("ln2_g"), a("Win_ximg"), a("Wout_ximg"), case[1], 11, 12,
                                             x1.ptr, z.ptr, y.ptr, g_out.ptr, g_hV.ptr, g_dh.ptr, g_f.ptr, g_z.ptr, h.ptr, part.ptr, G, env.s())


@row("namp_train_ln_rows_fwd", ids(ROWS))
def _ln_rows_fwd(ar, env, case):
    rows = rows_of(case, env.L.namp_train_ln_rows_groups)
    x, out = ar.inp("x", rn(gen(26), rows, H)), ar.out("out", f32, (rows, H))
    return lambda: env.L.namp_train_ln_rows_fwd(x.ptr, env.a("feat.ln_g"), env.a("feat.ln_b"), out.ptr, rows, env.s())


@row("namp_train_ln_rows_bwd", ids(ROWS))
def _ln_rows_bwd(ar, env, case):
    rows = rows_of(case, env.L.namp_train_ln_rows_groups)
    g = gen(27)
    x, gg = ar.inp("x", rn(g, rows, H)), ar.inp("g", rn(g, rows, H))
    gx, part = ar.out("gx", f32, (rows, H)), ar.out("dgb_part", f32, (env.L.namp_train_ln_rows_groups(rows), 2, H))
    return lambda: env.L.namp_train_ln_rows_bwd(x.ptr, gg.ptr, env.a("feat.ln_g"), gx.ptr, part.ptr, rows, env.s())


# precision argument of the row contractions: 0 exact fp32, 1 split-bf16, 2 bf16 on fp32 rows, +16 G in bf16, +32 A in bf16; "gelu" = gelu_A with code 0
WGRAD_CODES = [0, 1, 2, 2 | 16, 2 | 16 | 32, "gelu"]


@row("namp_train_wgrad", ids(cross(ROWS, WGRAD_CODES, ["bias", "nobias"])))
def _wgrad(ar, env, case):
    rows = rows_of(case[0], env.L.namp_train_wgrad_chunks)
    code, want_b = case[1], case[2] == "bias"
    g = gen(28)
    gelu, code = (1, 0) if code == "gelu" else (0, code)
    Gm = ar.inp("G", rn(g, rows, H).to(bf16 if code & 16 else f32))
    A = ar.inp("A", rn(g, rows, H).to(bf16 if code & 32 else f32))
    n = env.L.namp_train_wgrad_chunks(rows)
    dW = ar.out("dW_part", f32, (n, H, H))
    db = ar.out("db_part", f32, (n, H)) if want_b else None
    return lambda: env.L.namp_train_wgrad(Gm.ptr, A.ptr, gelu, code, rows, dW.ptr, db.ptr if db else None, env.s())


@row("namp_train_wgrad_ln", ids(cross(ROWS, [1, 2])))
def _wgrad_ln(ar, env, case):
    rows = rows_of(case[0], env.L.namp_train_wgrad_chunks)
    g = gen(29)
    Gm, Y = ar.inp("G", rn(g, rows, H)), ar.inp("Y", rn(g, rows, H, sc=2.0) + 0.5)
    y = Y.data.view(rows, H)
    stats = ar.inp("ln_stats", torch.stack((y.mean(1), (y.var(1, unbiased=False) + 1e-5).rsqrt()), 1))
    n = env.L.namp_train_wgrad_chunks(rows)
    dW, db = ar.out("dW_part", f32, (n, H, H)), ar.out("db_part", f32, (n, H))
    return lambda: env.L.namp_train_wgrad_ln(Gm.ptr, Y.ptr, stats.ptr, env.a("feat.ln_g"), env.a("feat.ln_b"), case[1], rows, dW.ptr, db.ptr, env.s())


@row("namp_train_wgrad_multi", ids(cross(ROWS, [1, 2], ["default", "chunks3", "add"])))
def _wgrad_multi(ar, env, case):
    rows = rows_of(case[0], env.L.namp_train_wgrad_chunks)
    prec, kind = case[1], case[2]
    g = gen(30)
    nq = 3
    Gs, As = [ar.inp(f"G{q}", rn(g, rows, H)) for q in range(nq)], [ar.inp(f"A{q}", rn(g, rows, H)) for q in range(nq)]
    chunks = 3 if kind == "chunks3" else 0
    n = chunks or env.L.namp_train_wgrad_chunks(rows)
    add = kind == "add"                                       # bit 6: add to the partials an earlier launch left there
    mk = (lambda nm, shape: ar.inout(nm, rn(g, *shape))) if add else (lambda nm, shape: ar.out(nm, f32, shape))
    dWs = [mk(f"dW_part{q}", (n, H, H)) for q in range(nq)]
    dbs = [mk(f"db_part{q}", (n, H)) if q != 1 else None for q in range(nq)]
    arr = lambda bufs: (C.c_void_p * len(bufs))(*[b.ptr if b is not None else None for b in bufs])
    return lambda: env.L.namp_train_wgrad_multi(arr(Gs), arr(As), nq, prec | (64 if add else 0), rows, chunks, arr(dWs), arr(dbs), env.s())


def reverse_adjacency_of(E_idx):
    B, N, K = E_idx.shape
    j = (E_idx.long() + (torch.arange(B) * N)[:, None, None]).view(-1)
    edges = torch.argsort(j, stable=True).to(i32)
    offsets = torch.cat([torch.zeros(1, dtype=i64), torch.bincount(j, minlength=B * N).cumsum(0)]).to(i32)
    return edges, offsets


def _scatter_rows(symbol, dt):
    @row(symbol, ids(cross(SHAPES, ["sel", "nosel"])))
    def build(ar, env, case):
        B, N, K, sel_kind = case
        g = gen(31)
        K = min(K, N)
        idx = rand_idx(g, B, N, K)
        idx[:, :, 0] = 0                                      # a hub row
        edges_t, off_t = reverse_adjacency_of(idx)
        G, E = B * N, B * N * K
        G1 = ar.inp("G1", rn(g, E, H).to(dt))
        edges, off = ar.inp("rev_edge", edges_t), ar.inp("rev_off", off_t)
        sel = ar.inp("sel", torch.randint(0, 2, (E,), generator=g).to(u8)) if sel_kind == "sel" else None
        out0 = ar.out("out0", f32, (G, H))
        out1 = ar.out("out1", f32, (G, H)) if sel else None
        fn = getattr(env.L, symbol)
        return lambda: fn(G1.ptr, edges.ptr, off.ptr, sel.ptr if sel else None, out0.ptr, out1.ptr if out1 else None, G, env.s())
    return build


_scatter_rows("namp_train_scatter_rows", f32)
_scatter_rows("namp_train_scatter_rows_bf16", bf16)


@row("namp_train_reverse_adjacency", ids(SHAPES))
def _reverse_adjacency(ar, env, case):
    B, N, K = case
    K = min(K, N)
    t = rand_idx(gen(32), B, N, K)
    t[:, :, 0] = 0
    idx = ar.inp("E_idx", t)
    off, edges = ar.out("offsets", i32, (B * N + 1,)), ar.out("edges", i32, (B * N * K,))
    ws = ar.ws("ws", 4 * (2 * B * N + B * N * K))             # "2*B*N + B*N*K int32 of scratch"
    return lambda: env.L.namp_train_reverse_adjacency(idx.ptr, off.ptr, edges.ptr, ws.ptr, B, N, K, env.s())


@row("namp_train_embed_ln_bwd", ids(cross(ROWS, [(1, "nog16"), (2, "nog16"), (1, "g16"), (2, "g16")])))
def _embed_ln_bwd(ar, env, case):
    rows = rows_of(case[0], env.L.namp_train_embed_ln_bwd_groups)
    prec, want16 = case[1], case[2] == "g16"
    g = gen(33)
    gg, Y = ar.inp("g", rn(g, rows, H)), ar.inp("Y", rn(g, rows, H, sc=2.0) + 0.5)
    g_pre, stats = ar.out("g_pre", f32, (rows, H)), ar.out("ln_stats", f32, (rows, 2))
    part = ar.out("dgb_part", f32, (env.L.namp_train_embed_ln_bwd_groups(rows), 2, H))
    g16 = None
    if want16:                                                # the tail tile zeroed by the caller when rows % 64 != 0 (the header): data, hence inout
        ne = env.L.namp_train_g16_elems(rows)
        g16 = ar.inout("g16", torch.zeros(2 if prec == 1 else 1, ne, dtype=bf16))
    return lambda: env.L.namp_train_embed_ln_bwd(gg.ptr, Y.ptr, env.img(prec, "We"), env.a("feat.ln_g"), g_pre.ptr, stats.ptr, part.ptr,
                                                 g16.ptr if g16 else None, prec, rows, env.s())


@row("namp_train_feat_wgrad", ids(cross(SHAPES, [0, 1, 2])))
def _feat_wgrad(ar, env, case):
    B, L, K, prec = case
    K = min(K, L)
    g = gen(34)
    E = B * L * K
    X18, M18 = rn(g, B * L, 18, 3, sc=3.0), (torch.rand(B * L, 18, generator=g) > 0.2).float()
    if prec:                                                  # packed atoms (x, y, z, mask): split-bf16 / bf16 only
        Xb, Mb = ar.inp("X18", torch.cat((X18, M18.unsqueeze(-1)), -1)), None
    else:
        Xb, Mb = ar.inp("X18", X18), ar.inp("M18", M18)
    idx = ar.inp("E_idx", rand_idx(g, B, L, K))
    E_pos, g_pre = ar.inp("E_pos", rn(g, E, 16)), ar.inp("g_pre", rn(g, E, H))
    dW = ar.out("dW_part", f32, (env.L.namp_train_feat_wgrad_chunks(E), H, 5200))
    tws = ar.ws("tile_ws", 4 * env.L.namp_train_feat_wgrad_ws_ints(E))
    return lambda: env.L.namp_train_feat_wgrad(Xb.ptr, Mb.ptr if Mb else None, idx.ptr, E_pos.ptr, g_pre.ptr, None, dW.ptr, tws.ptr, prec, B, L, K,
                                               env.s())


@row("namp_train_pos_features", ids(SHAPES))
def _pos_features(ar, env, case):
    B, L, K = case
    K = min(K, L)
    g = gen(35)
    R = ar.inp("R_idx", torch.cumsum(torch.randint(1, 4, (B, L), generator=g), 1).to(i32))
    ch = ar.inp("chain", (torch.arange(L)[None, :] // 20 + torch.arange(B)[:, None]).to(i32))
    idx = ar.inp("E_idx", rand_idx(g, B, L, K))
    d, E_pos = ar.out("d_out", i32, (B, L, K)), ar.out("E_pos", f32, (B, L, K, 16))
    return lambda: env.L.namp_train_pos_features(R.ptr, ch.ptr, idx.ptr, env.a("feat.pos_w"), env.a("feat.pos_b"), d.ptr, E_pos.ptr, B, L, K, env.s())


@row("namp_train_pos_grad", ids(ROWS))
def _pos_grad(ar, env, case):
    edges = rows_of(case, env.L.namp_train_pos_grad_groups)
    g = gen(36)
    gg, W = ar.inp("g", rn(g, edges, H)), ar.inp("Wedge", rn(g, H, 5200, sc=0.05))
    d = ar.inp("d", torch.randint(0, 66, (edges,), generator=g).to(i32))
    part = ar.out("part", f32, (env.L.namp_train_pos_grad_groups(edges), 67, 16))
    return lambda: env.L.namp_train_pos_grad(gg.ptr, W.ptr, 5200, d.ptr, part.ptr, edges, env.s())


@row("namp_train_class_sums", ids(cross(ROWS, [6, 33, 64])))
def _class_sums(ar, env, case):
    rows = rows_of(case[0], env.L.namp_train_rows_groups)
    ncls = case[1]
    g = gen(37)
    x = ar.inp("g", rn(g, rows, H))
    idx = ar.inp("idx", torch.randint(0, ncls, (rows,), generator=g).to(i32))
    part = ar.out("part", f32, (env.L.namp_train_rows_groups(rows), ncls, H))
    return lambda: env.L.namp_train_class_sums(x.ptr, idx.ptr, ncls, rows, part.ptr, env.s())


@row("namp_train_wcolsum", ids(ROWS))
def _wcolsum(ar, env, case):
    rows = rows_of(case, env.L.namp_train_rows_groups)
    g = gen(38)
    x, w = ar.inp("g", rn(g, rows, H)), ar.inp("w", rn(g, rows))
    part = ar.out("part", f32, (env.L.namp_train_rows_groups(rows), H))
    return lambda: env.L.namp_train_wcolsum(x.ptr, w.ptr, rows, part.ptr, env.s())


@row("namp_reduce_sum", ids(["four_segments"]))
def _reduce_sum(ar, env, case):
    g = gen(39)
    # (src shape, A, Mb, sa, sn, n): [n][M] partials; per-tile rows [G][T][128] -> [G][128]; a scalar (Mb = 1) segment; an odd-sized one
    segs = [((37, H * H), 1, H * H, 0, H * H, 37), ((65, 3, H), 65, H, 3 * H, H, 3), ((97, 3), 97, 1, 3, 1, 3), ((5, 7, 33), 5, 33, 7 * 33, 33, 7)]
    src = [ar.inp(f"src{q}", rn(g, *s[0])) for q, s in enumerate(segs)]
    dst = [ar.out(f"dst{q}", f32, (s[1], s[2])) for q, s in enumerate(segs)]
    NR = env.hip.NampReduce

    def call():
        arr = (NR * len(segs))(*[NR(src[q].ptr, dst[q].ptr, s[1], s[2], s[3], s[4], s[5], 0) for q, s in enumerate(segs)])
        return env.L.namp_reduce_sum(arr, len(segs), env.s())
    return call


@row("namp_train_loss_smoothed", ids(cross([1, 63, 64, 65, 1000], ["fwd", "bwd", "fwd_ppm"])))
def _loss_smoothed(ar, env, case):
    G = case[0]                                               # (no *_groups function to probe: 1000 rows stand for "several workgroups")
    kind = case[1]
    g = gen(40)
    S = ar.inp("S", torch.randint(0, 30, (G,), generator=g).to(i32))
    poly = torch.randint(0, 3, (G,), generator=g)
    pm = [ar.inp(nm, (poly == k).float()) for k, nm in enumerate(("protein_mask", "dna_mask", "rna_mask"))]
    rt = [ar.inp(nm, torch.tensor([1.0 if lo <= v < hi else 0.0 for v in range(V33)]))
          for nm, lo, hi in (("protein_restypes", 0, 21), ("dna_restypes", 21, 26), ("rna_restypes", 26, 31))]
    eps3 = (C.c_float * 3)(0.1 / 21, 0.1 / 5, 0.1 / 5)        # HOST array
    ppm = ar.inp("ppm_mask", torch.randint(0, 2, (G,), generator=g).to(i32)) if kind == "fwd_ppm" else None
    appm = ar.inp("aligned_ppm", torch.softmax(rn(g, G, V33), -1).double()) if kind == "fwd_ppm" else None
    p = lambda b: b.ptr if b is not None else None
    if kind == "bwd":
        g_loss, g_lp = ar.inp("g_loss", rn(g, G).double()), ar.out("g_log_probs", f32, (G, V33))
        return lambda: env.L.namp_train_loss_smoothed(1, S.ptr, None, *[x.ptr for x in pm], *[x.ptr for x in rt], eps3, 0.1, None, None, None,
                                                      g_loss.ptr, g_lp.ptr, G, V33, env.s())
    lp, loss = ar.inp("log_probs", torch.log_softmax(rn(g, G, V33), -1)), ar.out("loss", f64, (G,))
    return lambda: env.L.namp_train_loss_smoothed(0, S.ptr, lp.ptr, *[x.ptr for x in pm], *[x.ptr for x in rt], eps3, 0.1, p(ppm), p(appm), loss.ptr,
                                                  None, None, G, V33, env.s())


@row("namp_train_adam_step", ids(["noclip", "clip"]))
def _adam_step(ar, env, case):
    g = gen(41)
    chunk = env.L.namp_train_adam_chunk()
    numels = [1, 33, chunk, chunk + 1, 2 * chunk + 63]
    tens = [[ar.inout(f"{kind}{q}", (rn(g, n).abs() * 0.01 if kind == "exp_avg_sq" else rn(g, n))) for q, n in enumerate(numels)]
            for kind in ("param", "grad", "exp_avg", "exp_avg_sq")]
    bt = [q for q, n in enumerate(numels) for _ in range(0, n, chunk)]
    bo = [off for n in numels for off in range(0, n, chunk)]
    blk_t, blk_o = ar.inp("blk_tensor", torch.tensor(bt, dtype=i32)), ar.inp("blk_off", torch.tensor(bo, dtype=i64))
    numel = ar.inp("numel", torch.tensor(numels, dtype=i64))
    ptrs = ar.inp("ptrs", torch.zeros(4, len(numels), dtype=i64))
    ws = ar.out("ws", f32, (len(bt) + 2,), compare=2) if case == "clip" else None   # ws[0] = gradient norm, ws[1] = clip coefficient
    ar.build("A")                                             # fixes the addresses the pointer table holds
    ptrs.data = torch.tensor([[b.ptr for b in kind] for kind in tens], dtype=i64).view(-1)
    return lambda: env.L.namp_train_adam_step(blk_t.ptr, blk_o.ptr, numel.ptr, ptrs.ptr, len(numels), len(bt), 1.0 if case == "clip" else 0.0,
                                              0.9, 0.999, 1e-3 / 0.1, 0.001 ** 0.5, 1e-8, ws.ptr if ws else None, env.s())


def metric_batch(ar, env, G, Lr, g, with_lp):
    """NampMetricBatch over arena buffers (one complex row of Lr tokens per G / Lr)."""
    hip = env.hip
    ref = lambda b, dt: hip.NampTensorRef(b.ptr, hip.NAMP_DT[dt], 0)
    bufs = dict(S=ar.inp("S", torch.randint(0, 30, (G,), generator=g).to(i32)),
                mask=ar.inp("mask_for_loss", (torch.rand(G, generator=g) > 0.1).float()),
                cbp_mask=ar.inp("cbp_mask", torch.randint(0, 2, (G,), generator=g).to(i64)),
                poly=ar.inp("row_polymer0", torch.randint(0, 2, (G,), generator=g).to(torch.bool), dtype=torch.bool),
                iface=ar.inp("row_interface0", torch.randint(0, 2, (G,), generator=g).to(i32)))
    if with_lp:
        bufs["lp"] = ar.inp("log_probs", torch.log_softmax(rn(g, G, V33), -1))
        bufs["cbp_index"] = ar.inp("cbp_index", torch.randint(0, Lr, (G,), generator=g).to(i64))
    else:
        bufs.update(loss=ar.inp("loss", rn(g, G).abs().double()), acc=ar.inp("accuracy", torch.randint(0, 2, (G,), generator=g).float()),
                    cacc=ar.inp("cbp_accuracy", torch.randint(0, 2, (G,), generator=g).to(i64)),
                    spred=ar.inp("S_pred", torch.randint(0, 30, (G,), generator=g).to(i64)))

    def make():
        m = hip.NampMetricBatch()
        m.G, m.L, m.V = G, Lr, V33 if with_lp else 1
        m.S, m.mask_for_loss = ref(bufs["S"], "int32"), ref(bufs["mask"], "float32")
        m.cbp_mask = ref(bufs["cbp_mask"], "int64")
        m.row_polymer[0], m.row_interface[0] = ref(bufs["poly"], "bool"), ref(bufs["iface"], "int32")
        m.n_polymer, m.n_interface, m.n_res = 1, 1, 2
        m.res[0], m.res[1] = 21, 26
        for a_, b_ in ((21, 24), (24, 21), (22, 23), (23, 22)):
            m.pair_bits[a_] |= 1 << b_
        if with_lp:
            m.log_probs, m.cbp_index = bufs["lp"].ptr, ref(bufs["cbp_index"], "int64")
        else:
            m.loss, m.accuracy = ref(bufs["loss"], "float64"), ref(bufs["acc"], "float32")
            m.cbp_accuracy, m.S_pred = ref(bufs["cacc"], "int64"), ref(bufs["spred"], "int64")
        return m
    return make


@row("namp_train_metrics", ids(cross([(1, 33), (3, 65), (2, 129)], ["given"])))
def _train_metrics(ar, env, case):
    B, Lr, _kind = case
    G = B * Lr
    g = gen(42)
    make = metric_batch(ar, env, G, Lr, g, False)
    nrows, ncols = 4, 5 + 2 * 2
    table = ar.inout("table", rn(g, nrows + 1, ncols).double())
    wsp = ar.ws("workspace", 8 * env.L.namp_train_metrics_workspace(G, nrows, 2))
    err = ar.inout("err", torch.zeros(1, dtype=i32))
    row_of, col_of = (C.c_int32 * nrows)(0, 1, 2, 4), (C.c_int32 * ncols)(0, 1, 2, 3, -1, 5, 6, 7, 8)
    return lambda: env.L.namp_train_metrics(C.byref(make()), table.ptr, ncols, row_of, col_of, wsp.ptr, err.ptr, env.s())


@row("namp_canonical_pair_accuracy", ids([(1, 33), (3, 65), (2, 129)]))
def _pair_accuracy(ar, env, case):
    B, Lr = case
    G = B * Lr
    make = metric_batch(ar, env, G, Lr, gen(43), True)
    out, err = ar.out("out", i64, (G,)), ar.inout("err", torch.zeros(1, dtype=i32))
    return lambda: env.L.namp_canonical_pair_accuracy(C.byref(make()), out.ptr, err.ptr, env.s())


# ==== the test ==============================================================================================================
pytestmark = pytest.mark.gpu
PARAMS = [pytest.param(sym, case, id=f"{sym}-{cid}") for sym, r in TABLE.items() for cid, case in r.cases]


@pytest.mark.parametrize("symbol,case", PARAMS)
def test_memory_contract(env, symbol, case):
    r = TABLE[symbol]
    ar = Arena(env.dev)
    built = r.build(ar, env, case)
    call, opts = built if isinstance(built, tuple) else (built, {})
    assert not opts.get("tol_buffers") or symbol in NONREPRO, f"{symbol} compares with a tolerance but is not listed as irreproducible"
    try:
        _outs, reproducible = run_contract(lambda a: call(), ar, **opts)
    finally:
        torch.cuda.synchronize()
        assert torch.equal(env.packed.flat, env.snapshot), f"{symbol} wrote into the packed weights"
    print(f"{symbol} {case}: arena {ar.mem.numel() / 2 ** 20:.1f} MiB, {len(ar.buffers)} buffers, bit-reproducible: {reproducible}")
    assert reproducible or opts.get("tol_buffers"), f"{symbol} is not bit-reproducible, and its row does not say so"


# ---- sensitivity: the harness catches a real kernel (both stay inside memory the arena owns) ---------------------------------
def test_harness_reports_a_kernel_writing_past_an_understated_output(env):
    """namp_gather_nodes_f32 told N rows while the output registered in the arena is one row shorter: a trailing-guard write on `out`,
    of exactly that row."""
    B, N, K, Cn = 1, 33, 16, 16
    g = gen(50)
    ar = Arena(env.dev)
    nodes, idx = ar.inp("nodes", rn(g, B, N, Cn)), ar.inp("idx", rand_idx(g, B, N, K))
    out = ar.out("out", f32, (B, N - 1, K, Cn))
    with pytest.raises(GuardError) as e:
        run_contract(lambda a: env.L.namp_gather_nodes_f32(nodes.ptr, idx.ptr, out.ptr, B, N, K, Cn, env.s()), ar)
    assert len(e.value.failures) == 1, e.value.failures
    f = e.value.failures[0]
    assert f["buffer"] == "out" and f["side"] == "trailing" and f["kind"].startswith("guard write")
    assert f["first"] >= 0 and f["last"] < K * Cn * 4 and f["count"] <= K * Cn * 4      # inside the one missing row


def test_harness_reports_a_kernel_reading_past_an_understated_input(env):
    """`nodes` registered one row short with an index that selects the last row: the gathered row comes from the guard band, so the
    outputs of fill A (NaN) and fill B (1e30) differ — and nothing else is reported."""
    B, N, K, Cn = 1, 33, 16, 16
    g = gen(51)
    ar = Arena(env.dev)
    nodes = ar.inp("nodes", rn(g, B, N - 1, Cn))
    idx_t = torch.randint(0, N - 1, (B, N, K), generator=g).to(i32)
    idx_t[0, 5, 3] = N - 1
    idx = ar.inp("idx", idx_t)
    out = ar.out("out", f32, (B, N, K, Cn))
    with pytest.raises(GuardError) as e:
        run_contract(lambda a: env.L.namp_gather_nodes_f32(nodes.ptr, idx.ptr, out.ptr, B, N, K, Cn, env.s()), ar)
    first = (5 * K + 3) * Cn
    kinds = sorted(f["kind"].split(" (")[0] for f in e.value.failures)
    assert kinds == ["NaN/Inf", "fill-dependent output"], e.value.failures
    for f in e.value.failures:
        assert f["buffer"] == "out" and (f["first"], f["last"], f["count"]) == (first, first + Cn - 1, Cn), f
