"""GPU parity tests: HIP kernels (through the C ABI of libnamp_hip.so) vs the CPU oracle and the
committed goldens.  Run on an MI355X with  python -m pytest tests -m gpu.

Tolerances (BASELINE.json north_star): argmax sequences identical; logits / log-probs within
1e-3 in fp32 mode.  Copy kernels (gather) are bit-exact.  Intermediate activations are
checked at 2e-4 (observed ~1e-5: fp32 MFMA with a different but fixed summation order).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.pack import PackedWeights, image_index
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_LOGP = 1e-3
TOL_ACT = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    return hip.lib()


@pytest.fixture(scope="module")
def wt(weights_np):
    return {k: torch.from_numpy(v) for k, v in weights_np.items()}


@pytest.fixture(scope="module")
def packed(wt, dev):
    return PackedWeights({k: v.to(dev) for k, v in wt.items()}, 3, 3, 33, dev)


def stream():
    return hip.current_stream()


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def graph(dev, **kw):
    g = synth.make_graph(**kw)
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    d = {k: v.to(dev) for k, v in t.items()}
    return t, d


# ------------------------------------------------------------------------------------------
def test_pack_image_matches_host_permutation(L, dev):
    rng = np.random.default_rng(5)
    for out_f, in_f, ld, col0 in [(128, 128, 384, 128), (512, 128, 128, 0), (128, 512, 512, 0)]:
        W = rng.standard_normal((out_f, ld)).astype(np.float32)
        Wd = torch.from_numpy(W).to(dev)
        img = torch.empty(out_f * in_f, device=dev)
        hip.check(L.namp_pack_image(Wd.data_ptr(), ld, col0, out_f, in_f, img.data_ptr(), stream()))
        n, k = image_index(out_f, in_f)
        assert np.array_equal(img.cpu().numpy(), W[n, col0 + k])


def test_gather_and_cat_bit_exact(L, dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_gather.npz"))
    nodes, nbrs = torch.from_numpy(g["nodes"]).to(dev), torch.from_numpy(g["nbrs"]).to(dev)
    idx = torch.from_numpy(g["idx"].astype(np.int32)).to(dev)
    B, N, K = idx.shape
    out = torch.empty(B, N, K, 16, device=dev)
    hip.check(L.namp_gather_nodes_f32(nodes.data_ptr(), idx.data_ptr(), out.data_ptr(), B, N, K, 16, stream()))
    assert np.array_equal(out.cpu().numpy(), g["gather_nodes"])
    cat = torch.empty(B, N, K, 32, device=dev)
    hip.check(L.namp_cat_neighbors_nodes_f32(nodes.data_ptr(), nbrs.data_ptr(), idx.data_ptr(), cat.data_ptr(),
                                             B, N, K, 16, 16, stream()))
    assert np.array_equal(cat.cpu().numpy(), g["cat"])
    # channel counts that are not multiples of 4 (the reference gathers C=1 masks and C=54 coordinates)
    for c in (1, 54, 18):
        x = torch.randn(B, N, c, device=dev)
        o = torch.empty(B, N, K, c, device=dev)
        hip.check(L.namp_gather_nodes_f32(x.data_ptr(), idx.data_ptr(), o.data_ptr(), B, N, K, c, stream()))
        ref = cpu_ref.gather_nodes(x.cpu(), idx.cpu().long())
        assert torch.equal(o.cpu(), ref)
    # empty input is a no-op, not an error
    hip.check(L.namp_gather_nodes_f32(nodes.data_ptr(), idx.data_ptr(), out.data_ptr(), 0, N, K, 16, stream()))


def test_reference_named_gather_helpers(dev):
    """na_mpnn_amd.ops: gather_edges / gather_nodes / gather_nodes_t / cat_neighbors_nodes with the reference's names and
    shapes (model_utils.py:707-732), float and integer payloads, bit-exact against the oracle's torch.gather forms."""
    from na_mpnn_amd import ops
    g = torch.Generator().manual_seed(3)
    B, N, K = 2, 37, 9
    idx = torch.randint(0, N, (B, N, K), generator=g)
    for C in (1, 3, 54, 128):
        nodes = torch.randn(B, N, C, generator=g)
        edges = torch.randn(B, N, N, C, generator=g)
        nbrs = torch.randn(B, N, K, 5 if C % 4 else 8, generator=g)
        assert torch.equal(ops.gather_nodes(nodes.to(dev), idx.to(dev)).cpu(), cpu_ref.gather_nodes(nodes, idx))
        assert torch.equal(ops.gather_edges(edges.to(dev), idx.to(dev)).cpu(), cpu_ref.gather_edges(edges, idx))
        assert torch.equal(ops.cat_neighbors_nodes(nodes.to(dev), nbrs.to(dev), idx.to(dev)).cpu(),
                           cpu_ref.cat_neighbors_nodes(nodes, nbrs, idx))
        it = torch.randint(0, N, (B, 11), generator=g)
        ref_t = torch.gather(nodes, 1, it.unsqueeze(-1).expand(-1, -1, C))
        assert torch.equal(ops.gather_nodes_t(nodes.to(dev), it.to(dev)).cpu(), ref_t)
    # integer payloads (the reference gathers the int32 mask and int64 offset matrices this way)
    mask = torch.randint(0, 2, (B, N, 1), generator=g, dtype=torch.int32)
    out = ops.gather_nodes(mask.to(dev), idx.to(dev))
    assert out.dtype == torch.int32 and torch.equal(out.cpu(), cpu_ref.gather_nodes(mask, idx))
    off = torch.randint(-50, 50, (B, N, N, 1), generator=g, dtype=torch.int32)
    assert torch.equal(ops.gather_edges(off.to(dev), idx.to(dev)).cpu(), cpu_ref.gather_edges(off, idx))


def test_gather_cat_full_size(L, dev):
    """cfg2-sized [1,1000,48,128|128] concat, bit-exact vs torch on the same device data."""
    t, d = graph(dev, seed=11, batch=2, n=1000, k=48)
    hV = torch.randn(2, 1000, 128, device=dev)
    out = torch.empty(2, 1000, 48, 256, device=dev)
    hip.check(L.namp_cat_neighbors_nodes_f32(hV.data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(), out.data_ptr(),
                                             2, 1000, 48, 128, 128, stream()))
    ref = cpu_ref.cat_neighbors_nodes(hV.cpu(), t["E"], t["E_idx"].long())
    assert torch.equal(out.cpu(), ref)


def test_node_linear_and_token_table(L, dev, wt, packed):
    t, d = graph(dev, seed=12, batch=2, n=77, k=16)
    X = d["V"]
    outs = [torch.empty(2, 77, 128, device=dev) for _ in range(3)]
    S = d["S"]
    proj = (hip.NampProj * 3)(
        hip.NampProj(packed.addr("enc0.W1a_img"), packed.addr("enc0.b1"), None, outs[0].data_ptr()),
        hip.NampProj(packed.addr("enc0.W1c_img"), None, None, outs[1].data_ptr()),
        hip.NampProj(packed.addr("dec1.W1v_img"), None, packed.addr("dec1.tok"), outs[2].data_ptr()))
    hip.check(L.namp_node_linear(X.data_ptr(), S.data_ptr(), 2, 2, 77, proj, 3, None, stream()))
    W1, W1d = wt["encoder_layers.0.W1.weight"], wt["decoder_layers.1.W1.weight"]
    r0 = t["V"] @ W1[:, :128].T + wt["encoder_layers.0.W1.bias"]
    r1 = t["V"] @ W1[:, 256:384].T
    tok = wt["W_s.weight"] @ W1d[:, 256:384].T
    r2 = t["V"] @ W1d[:, 384:].T + tok[t["S"].long()]
    assert maxdiff(outs[0], r0) < 1e-5 and maxdiff(outs[1], r1) < 1e-5 and maxdiff(outs[2], r2) < 1e-5
    assert maxdiff(packed.view("dec1.tok").view(33, 128), tok) < 1e-5


def test_edge_embed(L, dev, wt, packed):
    for n, k in [(50, 48), (33, 30), (20, 7)]:
        t, d = graph(dev, seed=13 + n, batch=2, n=n, k=k)
        kk = t["E_idx"].shape[-1]
        out = torch.empty_like(d["E"])
        hip.check(L.namp_edge_embed(packed.addr("We_img"), packed.addr("We_b"), d["E"].data_ptr(), out.data_ptr(),
                                    2, n, kk, stream()))
        ref = torch.nn.functional.linear(t["E"], wt["W_e.weight"], wt["W_e.bias"])
        assert maxdiff(out, ref) < 1e-5, (n, k)


def test_enc_layer_golden(L, dev, wt, packed, golden_dir):
    """a4: EncLayer.forward with partial masks vs the reference golden (G2)."""
    g = np.load(os.path.join(golden_dir, "g2_layers.npz"))
    t, d = graph(dev, seed=202, batch=1, n=128, k=48, masked_frac=0.1)
    hV, hE = torch.empty_like(d["V"]), torch.empty_like(d["E"])
    ws = torch.empty(L.namp_workspace_bytes(1, 1, 128, 48), dtype=torch.uint8, device=dev)
    hip.check(L.namp_enc_layer_fwd(packed.enc_layer(1), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(),
                                   d["mask"].data_ptr(), None, hV.data_ptr(), hE.data_ptr(), ws.data_ptr(), ws.numel(),
                                   1, 128, 48, stream()))
    dv = maxdiff(hV[0], torch.from_numpy(g["enc_hV"]))
    de = maxdiff(hE[0, ::16], torch.from_numpy(g["enc_hE_rows"]))
    assert dv < TOL_ACT and de < TOL_ACT, (dv, de)
    # explicit mask_attend (arbitrary 0/1 pattern) is honoured too
    rng = np.random.default_rng(3)
    ma = torch.from_numpy(rng.integers(0, 2, (1, 128, 48)).astype(np.int32))
    ma_d = ma.to(dev)
    hip.check(L.namp_enc_layer_fwd(packed.enc_layer(1), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(),
                                   d["mask"].data_ptr(), ma_d.data_ptr(), hV.data_ptr(), hE.data_ptr(),
                                   ws.data_ptr(), ws.numel(), 1, 128, 48, stream()))
    rV, rE = cpu_ref.enc_layer(wt, "encoder_layers.1.", t["V"], t["E"], t["E_idx"].long(), t["mask"], ma)
    assert maxdiff(hV, rV) < TOL_ACT and maxdiff(hE, rE) < TOL_ACT


def test_dec_layer_golden(L, dev, wt, packed, golden_dir):
    """a5: DecLayer.forward as an operator on a MATERIALISED 384-wide context (model_utils.py:636-657) vs the reference
    golden (G2 dec_hV: decoder_layers.2 on a seeded synthetic context with a partial mask_V), plus an explicit
    mask_attend and odd shapes (K not a multiple of 16, ragged last workgroup) vs the oracle."""
    g = np.load(os.path.join(golden_dir, "g2_layers.npz"))
    t, d = graph(dev, seed=202, batch=1, n=128, k=48, masked_frac=0.1)
    ctx = torch.from_numpy(np.random.default_rng(203).standard_normal((1, 128, 48, 384)).astype(np.float32))
    ctx_d = ctx.to(dev)
    out = torch.empty_like(d["V"])
    ws = torch.empty(L.namp_workspace_bytes(1, 1, 128, 48), dtype=torch.uint8, device=dev)
    hip.check(L.namp_dec_layer_fwd(packed.dec_layer(2), d["V"].data_ptr(), ctx_d.data_ptr(), d["mask"].data_ptr(), None,
                                   out.data_ptr(), ws.data_ptr(), ws.numel(), 1, 128, 48, stream()))
    dv = maxdiff(out[0], torch.from_numpy(g["dec_hV"]))
    assert dv < TOL_ACT, dv
    for (B, n, k, seed) in [(2, 37, 30, 5), (1, 21, 7, 6)]:
        rng = np.random.default_rng(seed)
        V = torch.from_numpy(rng.standard_normal((B, n, 128)).astype(np.float32))
        c = torch.from_numpy(rng.standard_normal((B, n, k, 384)).astype(np.float32))
        mV = torch.from_numpy(rng.integers(0, 2, (B, n)).astype(np.int32))
        ma = torch.from_numpy(rng.integers(0, 2, (B, n, k)).astype(np.float32))
        Vd, cd, mVd, mad = V.to(dev), c.to(dev), mV.to(dev), ma.to(dev)
        o = torch.empty_like(Vd)
        ws = torch.empty(L.namp_workspace_bytes(B, B, n, k), dtype=torch.uint8, device=dev)
        hip.check(L.namp_dec_layer_fwd(packed.dec_layer(0), Vd.data_ptr(), cd.data_ptr(), mVd.data_ptr(), mad.data_ptr(),
                                       o.data_ptr(), ws.data_ptr(), ws.numel(), B, n, k, stream()))
        ref = cpu_ref.dec_layer(wt, "decoder_layers.0.", V, c, mV.float(), ma)
        assert maxdiff(o, ref) < TOL_ACT, (B, n, k)


def run_encdec(L, dev, packed, d, B, N, K, joint=False):
    hV = torch.empty(B, N, 128, device=dev)
    hE = torch.empty(B, N, K, 128, device=dev)
    ws = torch.empty(2 * L.namp_workspace_bytes(B, B, N, K), dtype=torch.uint8, device=dev)
    if joint:        # the same path as ONE call, fused across the encoder/decoder boundary (namp_encdec_fwd)
        order = torch.argsort((d["mask"] * d["chain_mask"] + 0.0001) * torch.abs(d["randn"]))
        rank = torch.empty_like(order)
        rank.scatter_(1, order, torch.arange(N, device=dev).expand(B, -1))
        rank = rank.to(torch.int32)
        logp = torch.empty(B, N, 33, device=dev)
        hip.check(L.namp_encdec_fwd(packed.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(),
                                    d["mask"].data_ptr(), d["S"].data_ptr(), rank.data_ptr(), hV.data_ptr(), hE.data_ptr(),
                                    logp.data_ptr(), None, ws.data_ptr(), ws.numel(), B, N, K, stream()))
        torch.cuda.synchronize()
        return hV, hE, logp, order
    hip.check(L.namp_encoder_fwd(packed.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(),
                                 d["mask"].data_ptr(), hV.data_ptr(), hE.data_ptr(), ws.data_ptr(), ws.numel(),
                                 B, N, K, stream()))
    order = torch.argsort((d["mask"] * d["chain_mask"] + 0.0001) * torch.abs(d["randn"]))
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(N, device=dev).expand(B, -1))
    rank = rank.to(torch.int32)
    logp = torch.empty(B, N, 33, device=dev)
    hip.check(L.namp_decoder_fwd(packed.model(), hV.data_ptr(), hE.data_ptr(), d["E_idx"].data_ptr(), d["S"].data_ptr(),
                                 d["mask"].data_ptr(), rank.data_ptr(), logp.data_ptr(), None, None,
                                 ws.data_ptr(), ws.numel(), B, B, N, K, stream()))
    torch.cuda.synchronize()
    return hV, hE, logp, order


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("n,tag,mf,batch", [(256, "n256", 0.05, 1), (40, "n40_LltK", 0.0, 1),
                                             (200, "b3_n200", 0.1, 3), (1000, "n1000", 0.0, 1)])
def test_encoder_decoder_goldens(L, dev, packed, golden_dir, n, tag, mf, batch, joint, prec):
    """a7+a8, the BASELINE metric scope: (V,E,E_idx) -> log_probs vs reference goldens (G3); as namp_encoder_fwd +
    namp_decoder_fwd and as the single fused call namp_encdec_fwd (what bench.py times).  Both fp32-class evaluations of
    the per-edge GEMMs: split-bf16 products (the default) and exact fp32 MFMA — same bars."""
    g = np.load(os.path.join(golden_dir, f"g3_encdec_{tag}.npz"))
    t, d = graph(dev, seed=300 + n + batch, batch=batch, n=n, k=48, masked_frac=mf)
    K = t["E_idx"].shape[-1]
    packed.set_precision(prec)
    try:
        hV, hE, logp, order = run_encdec(L, dev, packed, d, batch, n, K, joint)
    finally:
        packed.set_precision("x3")
    stride = int(g["row_stride"])
    d_hv = maxdiff(hV[:, ::stride], torch.from_numpy(g["enc_hV_layers"][-1]))
    d_he = maxdiff(hE[:, ::max(1, n // 16)][:, :16], torch.from_numpy(g["enc_hE_rows"]))
    assert np.array_equal(order.cpu().numpy(), g["decoding_order"]), "decoding order differs from the reference"
    d_lp = maxdiff(logp, torch.from_numpy(g["log_probs"]))
    assert d_hv < TOL_ACT and d_he < TOL_ACT, (d_hv, d_he)
    assert d_lp < TOL_LOGP, d_lp
    valid = t["mask"].bool().numpy()
    assert np.array_equal(logp.argmax(-1).cpu().numpy()[valid], g["argmax"].astype(np.int64)[valid]), \
        "argmax sequence differs from the reference"


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("n,k,b,mf", [(1, 1, 1, 0.0), (2, 2, 3, 0.0), (5, 3, 2, 0.3), (16, 16, 1, 0.0), (17, 9, 4, 0.2), (31, 31, 2, 0.5),
                                      (63, 17, 3, 0.1), (100, 64, 2, 0.0), (130, 80, 1, 0.1), (257, 33, 2, 0.05), (300, 120, 1, 0.0)])
def test_random_shapes_against_the_oracle(L, dev, wt, packed, n, k, b, mf, joint):
    """(V, E, E_idx) -> log_probs against the CPU oracle over odd shapes: K from 1 to 120 (1..8 tiles per residue), K = N,
    batches, heavy masking; separate calls and the fused single call."""
    t, d = graph(dev, seed=9000 + 13 * n + k, batch=b, n=n, k=k, masked_frac=mf)
    K = t["E_idx"].shape[-1]
    hV, hE, logp, order = run_encdec(L, dev, packed, d, b, n, K, joint)
    ref = cpu_ref.encdec_from_graph(wt, t["V"], t["E"], t["E_idx"].long(), t["S"], t["mask"], t["chain_mask"], t["randn"])
    valid = t["mask"].bool()
    assert torch.isfinite(logp).all()
    if valid.any():
        assert maxdiff(logp.cpu()[valid], ref["log_probs"][valid]) < TOL_LOGP
        assert torch.equal(logp.cpu().argmax(-1)[valid], ref["log_probs"].argmax(-1)[valid])


def test_decoder_batch_replication_and_unconditional(L, dev, wt, packed):
    """B_dec = 3 x B_enc with different sequences / orders per decoder batch; rank = 0 -> unconditional."""
    t, d = graph(dev, seed=21, batch=1, n=90, k=32)
    hV_r, hE_r = cpu_ref.encode_from_graph(wt, t["V"], t["E"], t["E_idx"].long(), t["mask"])
    hV, hE = hV_r.to(dev), hE_r.to(dev)
    rng = np.random.default_rng(22)
    S = torch.from_numpy(rng.integers(0, 25, (3, 90)).astype(np.int32))
    randn = torch.from_numpy(rng.standard_normal((3, 90)).astype(np.float32))
    mask3 = t["mask"].repeat(3, 1)
    order = torch.argsort((mask3 + 0.0001) * randn.abs())
    rank = torch.empty_like(order); rank.scatter_(1, order, torch.arange(90).expand(3, -1))
    logp = torch.empty(3, 90, 33, device=dev)
    ws = torch.empty(L.namp_workspace_bytes(1, 3, 90, 32), dtype=torch.uint8, device=dev)
    S_d, mask_d, rank_d = S.to(dev), mask3.to(dev), rank.to(torch.int32).to(dev)   # keep the device buffers alive
    hip.check(L.namp_decoder_fwd(packed.model(), hV.data_ptr(), hE.data_ptr(), d["E_idx"].data_ptr(),
                                 S_d.data_ptr(), mask_d.data_ptr(), rank_d.data_ptr(),
                                 logp.data_ptr(), None, None, ws.data_ptr(), ws.numel(), 3, 1, 90, 32, stream()))
    E3 = t["E_idx"].long().repeat(3, 1, 1)
    ref, _ = cpu_ref.decode_parallel(wt, hV_r.repeat(3, 1, 1), hE_r.repeat(3, 1, 1, 1), E3, S.long(), mask3,
                                     cpu_ref.backward_mask(order, E3))
    assert maxdiff(logp, ref) < TOL_LOGP
    assert torch.equal(logp.argmax(-1).cpu(), ref.argmax(-1))
    zeros = torch.zeros(3, 90, dtype=torch.int32, device=dev)
    hip.check(L.namp_decoder_fwd(packed.model(), hV.data_ptr(), hE.data_ptr(), d["E_idx"].data_ptr(),
                                 zeros.data_ptr(), mask_d.data_ptr(), zeros.data_ptr(),
                                 logp.data_ptr(), None, None, ws.data_ptr(), ws.numel(), 3, 1, 90, 32, stream()))
    refu, _ = cpu_ref.decode_parallel(wt, hV_r.repeat(3, 1, 1), hE_r.repeat(3, 1, 1, 1), E3,
                                      torch.zeros(3, 90, dtype=torch.long), mask3, torch.zeros(3, 90, 32, 1))
    assert maxdiff(logp, refu) < TOL_LOGP


def test_full_size_invariants(L, dev, packed):
    """cfg2-sized (N=1000,K=48) size-independent properties: (i) neighbour-order permutation
    invariance of the message sums, (ii) batch independence (a complex scored alone == inside a batch)."""
    t, d = graph(dev, seed=31, batch=2, n=1000, k=48)
    _, _, logp, _ = run_encdec(L, dev, packed, d, 2, 1000, 48)
    # (ii) first complex alone
    d1 = {k: v[:1].contiguous() for k, v in d.items()}
    _, _, logp1, _ = run_encdec(L, dev, packed, d1, 1, 1000, 48)
    assert torch.equal(logp1[0], logp[0]), "batched and single-complex results differ (should be bit-identical)"
    # (i) permute the neighbour slots of every residue consistently in E and E_idx
    perm = torch.stack([torch.randperm(48, device=dev) for _ in range(2000)]).view(2, 1000, 48)
    dp = dict(d)
    dp["E_idx"] = torch.gather(d["E_idx"], 2, perm).contiguous()
    dp["E"] = torch.gather(d["E"], 2, perm[..., None].expand(-1, -1, -1, 128)).contiguous()
    _, _, logp_p, _ = run_encdec(L, dev, packed, dp, 2, 1000, 48)
    assert maxdiff(logp_p, logp) < 2e-4
    assert torch.isfinite(logp).all()
    assert maxdiff(torch.logsumexp(logp, -1), torch.zeros(2, 1000)) < 1e-5     # rows are normalised


@pytest.mark.parametrize("n,k,bdec", [(300, 48, 1), (130, 30, 1), (75, 16, 2)])
def test_fused_tail_matches_unfused(L, dev, packed, n, k, bdec):
    """namp_{enc,dec}_message_update (one launch) == namp_*_message + namp_node_update (two launches)."""
    t, d = graph(dev, seed=41 + n, batch=1, n=n, k=k, masked_frac=0.1)
    K = t["E_idx"].shape[-1]
    tpn = (K + 15) // 16
    G = n
    a = lambda nm: packed.addr("enc1." + nm)
    Pa, Pc = torch.randn(G, 128, device=dev), torch.randn(G, 128, device=dev)
    outs = [[torch.empty(G, 128, device=dev) for _ in range(3)] for _ in range(2)]
    hv = [torch.empty(G, 128, device=dev) for _ in range(2)]
    partial = torch.empty(G * tpn * 129 + 3, device=dev)      # K-sums [G][tpn][128] + weight sums [G][tpn] (include/namp.h)
    def projs(o):
        return (hip.NampProj * 3)(hip.NampProj(a("W11a_img"), a("b11"), None, o[0].data_ptr()),
                                  hip.NampProj(a("W11c_img"), None, None, o[1].data_ptr()),
                                  hip.NampProj(a("W1a_img"), a("b1"), None, o[2].data_ptr()))
    s = stream()
    hip.check(L.namp_enc_message_update(packed.enc_layer(1), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(),
                                        None, Pa.data_ptr(), Pc.data_ptr(), d["V"].data_ptr(), hv[0].data_ptr(),
                                        projs(outs[0]), 3, 1, n, K, s))
    hip.check(L.namp_enc_message(packed.enc_layer(1), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(), None,
                                 Pa.data_ptr(), Pc.data_ptr(), partial.data_ptr(), 1, n, K, s))
    hip.check(L.namp_node_update(a("ln1_g"), a("ln1_b"), a("Win_img"), a("b_in"), a("Wout_img"), a("b_out"), a("ln2_g"),
                                 a("ln2_b"), d["V"].data_ptr(), partial.data_ptr(), a("W3_img"), a("b3"), d["mask"].data_ptr(),
                                 hv[1].data_ptr(), projs(outs[1]), 3, None, G, K, s))
    # K <= 16: both forms run the same 16-row MFMA tail (bit-identical); K > 16: the fused form's tile has
    # <= 8 residues and uses the VALU tail (same math, different fp32 summation order)
    tol = 0.0 if K <= 16 else 2e-5
    assert maxdiff(hv[0], hv[1]) <= tol
    for x, y in zip(outs[0], outs[1]):
        assert maxdiff(x, y) <= tol
    # decoder form, with decoder-batch replication and token tables
    Gd = bdec * n
    b = lambda nm: packed.addr("dec1." + nm)
    rng = np.random.default_rng(n)
    S = torch.from_numpy(rng.integers(0, 33, (Gd,)).astype(np.int32)).to(dev)
    rank = torch.from_numpy(np.concatenate([rng.permutation(n) for _ in range(bdec)]).astype(np.int32)).to(dev)
    maskd = d["mask"].repeat(bdec, 1).contiguous()
    hVd = torch.randn(Gd, 128, device=dev)
    Pa, Pbw, Pfw = torch.randn(Gd, 128, device=dev), torch.randn(Gd, 128, device=dev), torch.randn(G, 128, device=dev)
    outs = [[torch.empty(Gd, 128, device=dev) for _ in range(2)] for _ in range(2)]
    hv = [torch.empty(Gd, 128, device=dev) for _ in range(2)]
    partial = torch.empty(Gd * tpn * 129 + 3, device=dev)
    lp = [torch.empty(Gd, 33, device=dev) for _ in range(2)]
    def dprojs(o):
        return (hip.NampProj * 2)(hip.NampProj(b("W1a_img"), b("b1"), None, o[0].data_ptr()),
                                  hip.NampProj(b("W1v_img"), None, b("tok"), o[1].data_ptr()))
    hip.check(L.namp_dec_message_update(packed.dec_layer(1), d["E"].data_ptr(), d["E_idx"].data_ptr(), rank.data_ptr(),
                                        Pa.data_ptr(), Pbw.data_ptr(), Pfw.data_ptr(), hVd.data_ptr(), maskd.data_ptr(),
                                        hv[0].data_ptr(), dprojs(outs[0]), 2, S.data_ptr(),
                                        packed.addr("Wout_w"), packed.addr("Wout_b"), lp[0].data_ptr(), None, 33,
                                        bdec, 1, n, K, s))
    hip.check(L.namp_dec_message(packed.dec_layer(1), d["E"].data_ptr(), d["E_idx"].data_ptr(), rank.data_ptr(),
                                 Pa.data_ptr(), Pbw.data_ptr(), Pfw.data_ptr(), partial.data_ptr(), bdec, 1, n, K, s))
    hip.check(L.namp_node_update(b("ln1_g"), b("ln1_b"), b("Win_img"), b("b_in"), b("Wout_img"), b("b_out"), b("ln2_g"),
                                 b("ln2_b"), hVd.data_ptr(), partial.data_ptr(), b("W3_img"), b("b3"), maskd.data_ptr(),
                                 hv[1].data_ptr(), dprojs(outs[1]), 2, S.data_ptr(), Gd, K, s))
    assert maxdiff(hv[0], hv[1]) <= tol
    for x, y in zip(outs[0], outs[1]):
        assert maxdiff(x, y) <= tol
    # fused output head == separate logits kernel on the same h_V'
    hip.check(L.namp_logits_log_softmax(packed.addr("Wout_w"), packed.addr("Wout_b"), hv[0].data_ptr(), lp[1].data_ptr(),
                                        None, Gd, 33, s))
    assert maxdiff(lp[0], lp[1]) <= 2e-6


@pytest.mark.parametrize("n,k", [(200, 48), (90, 30)])
def test_message_phase_writes_ksums_of_layer2_activations(L, dev, wt, packed, n, k):
    """namp_enc_message's `partial` (include/namp.h): per 16-neighbour tile the weighted K-sum of the layer-2 activations
    a_k = gelu(W2 gelu(W1 [h_V_i | h_E_ik | h_V_j] + b1) + b2), w_k = mask_i mask_j / 30, followed by the tiles' weight sums — and
    W3 . sum + b3 . wsum is the reference's message sum (model_utils.py:684-690), checked in fp64 from the raw weights."""
    t, d = graph(dev, seed=77 + n, batch=1, n=n, k=k, masked_frac=0.15)
    K = t["E_idx"].shape[-1]
    tpn, G = (K + 15) // 16, n
    W = {nm: wt["encoder_layers.1." + nm].to(dev).double() for nm in ("W1.weight", "W1.bias", "W2.weight", "W2.bias", "W3.weight", "W3.bias")}
    hV, hE = d["V"][0].double(), d["E"][0].double()                       # [n,128], [n,K,128] stand in for h_V, h_E
    idx, mask = d["E_idx"][0].long(), d["mask"][0].double()
    W1a, W1b, W1c = W["W1.weight"][:, :128], W["W1.weight"][:, 128:256], W["W1.weight"][:, 256:]
    Pa = (hV @ W1a.t() + W["W1.bias"]).float().contiguous()
    Pc = (hV @ W1c.t()).float().contiguous()
    partial = torch.zeros(G * tpn * 129 + 3, device=dev)
    hip.check(L.namp_enc_message(packed.enc_layer(1), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(), None,
                                 Pa.data_ptr(), Pc.data_ptr(), partial.data_ptr(), 1, n, K, stream()))
    gelu = torch.nn.functional.gelu
    z1 = hE @ W1b.t() + Pa.double()[:, None, :] + Pc.double()[idx]
    a2 = gelu(gelu(z1) @ W["W2.weight"].t() + W["W2.bias"])
    w = mask[:, None] * mask[idx] / 30.0                                   # [n,K]
    pad = tpn * 16 - K
    a2p = torch.nn.functional.pad(a2 * w[..., None], (0, 0, 0, pad)).view(n, tpn, 16, 128).sum(2)
    wp = torch.nn.functional.pad(w, (0, pad)).view(n, tpn, 16).sum(2)
    S = partial[:G * tpn * 128].view(n, tpn, 128).double()
    ws = partial[G * tpn * 128:G * tpn * 129].view(n, tpn).double()
    assert float((ws - wp).abs().max()) < 1e-6
    assert float((S - a2p).abs().max()) < 2e-4 * max(1.0, float(a2p.abs().max()))        # split-bf16 products: ~2^-16 per product
    dh_ref = ((a2 @ W["W3.weight"].t() + W["W3.bias"]) * w[..., None]).sum(1)
    dh = S.sum(1) @ W["W3.weight"].t() + W["W3.bias"] * ws.sum(1, keepdim=True)
    assert float((dh - dh_ref).abs().max()) < 2e-4 * max(1.0, float(dh_ref.abs().max()))


@pytest.mark.parametrize("n,k,b", [(300, 48, 1), (130, 30, 2), (75, 16, 1), (23, 48, 1)])
def test_fused_edge_message_matches_separate_launches(L, dev, packed, n, k, b):
    """namp_enc_edge_message_update (layer l-1's edge update + layer l's message + tail, one launch) ==
    namp_enc_edge_update followed by namp_enc_message_update: the same GEMMs on the same rows in the same order."""
    t, d = graph(dev, seed=77 + n, batch=b, n=n, k=k, masked_frac=0.1)
    K = t["E_idx"].shape[-1]
    G = b * n
    a = lambda nm: packed.addr("enc2." + nm)
    ePa, ePc, Pa, Pc = (torch.randn(G, 128, device=dev) for _ in range(4))
    hE = [d["E"].clone(), d["E"].clone()]
    outs = [[torch.empty(G, 128, device=dev) for _ in range(2)] for _ in range(2)]
    hv = [torch.empty(G, 128, device=dev) for _ in range(2)]
    def projs(o):
        return (hip.NampProj * 2)(hip.NampProj(a("W11a_img"), a("b11"), None, o[0].data_ptr()),
                                  hip.NampProj(a("W11c_img"), None, None, o[1].data_ptr()))
    s = stream()
    hip.check(L.namp_enc_edge_message_update(packed.enc_layer(1), ePa.data_ptr(), ePc.data_ptr(), hE[0].data_ptr(),
                                             packed.enc_layer(2), d["E_idx"].data_ptr(), d["mask"].data_ptr(), None,
                                             Pa.data_ptr(), Pc.data_ptr(), d["V"].data_ptr(), hv[0].data_ptr(),
                                             projs(outs[0]), 2, b, n, K, s))
    hip.check(L.namp_enc_edge_update(packed.enc_layer(1), hE[1].data_ptr(), d["E_idx"].data_ptr(), ePa.data_ptr(), ePc.data_ptr(),
                                     hE[1].data_ptr(), b, n, K, s))
    hip.check(L.namp_enc_message_update(packed.enc_layer(2), hE[1].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(),
                                        None, Pa.data_ptr(), Pc.data_ptr(), d["V"].data_ptr(), hv[1].data_ptr(),
                                        projs(outs[1]), 2, b, n, K, s))
    assert torch.equal(hE[0], hE[1])
    assert torch.equal(hv[0], hv[1])
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)
    # a projection must not overwrite a table the launch is still gathering
    bad = (hip.NampProj * 1)(hip.NampProj(a("W11a_img"), a("b11"), None, ePa.data_ptr()))
    rc = L.namp_enc_edge_message_update(packed.enc_layer(1), ePa.data_ptr(), ePc.data_ptr(), hE[0].data_ptr(),
                                        packed.enc_layer(2), d["E_idx"].data_ptr(), d["mask"].data_ptr(), None,
                                        Pa.data_ptr(), Pc.data_ptr(), d["V"].data_ptr(), hv[0].data_ptr(), bad, 1, b, n, K, s)
    assert rc == -1 and b"still gathers" in L.namp_last_error()


def test_unfused_path_large_batch(L, dev, wt, packed):
    """B*N above namp_fused_tail_max_residues() takes the two-launch path; same parity bar."""
    B, N = 6, 800
    assert B * N > L.namp_fused_tail_max_residues()
    t, d = graph(dev, seed=51, batch=B, n=N, k=32)
    _, _, logp, _ = run_encdec(L, dev, packed, d, B, N, 32)
    b = 4
    hV_r, hE_r = cpu_ref.encode_from_graph(wt, t["V"][b:b + 1], t["E"][b:b + 1], t["E_idx"][b:b + 1].long(), t["mask"][b:b + 1])
    ref = cpu_ref.score_from_encoded(wt, hV_r, hE_r, t["E_idx"][b:b + 1].long(), t["S"][b:b + 1], t["mask"][b:b + 1],
                                     t["chain_mask"][b:b + 1], t["randn"][b:b + 1])
    assert maxdiff(logp[b:b + 1], ref["log_probs"]) < TOL_LOGP
    assert torch.equal(logp[b].argmax(-1).cpu(), ref["log_probs"][0].argmax(-1))


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("B,N,K,mf", [(3, 901, 30, 0.1), (2, 1333, 48, 0.0), (5, 611, 17, 0.2), (7, 777, 64, 0.05)])
def test_unfused_regime_odd_shapes_against_the_oracle(L, dev, wt, packed, B, N, K, mf, joint):
    """Calls of more than namp_fused_tail_max_residues() residues with tile counts that divide nothing (persistent
    split-bf16 edge kernels with partly idle last rounds, the multi-tile split-bf16 residue update with a ragged last
    workgroup, K not a multiple of 16): one complex of the batch against the oracle, and the exact-fp32 evaluation of the
    same call against the default one."""
    assert B * N > L.namp_fused_tail_max_residues()
    t, d = graph(dev, seed=700 + N, batch=B, n=N, k=K, masked_frac=mf)
    _, _, logp, _ = run_encdec(L, dev, packed, d, B, N, K, joint)
    packed.set_precision("fp32")
    try:
        _, _, logp32, _ = run_encdec(L, dev, packed, d, B, N, K, joint)
    finally:
        packed.set_precision("x3")
    assert maxdiff(logp, logp32) < 3e-4
    b = B - 1
    hV_r, hE_r = cpu_ref.encode_from_graph(wt, t["V"][b:b + 1], t["E"][b:b + 1], t["E_idx"][b:b + 1].long(), t["mask"][b:b + 1])
    ref = cpu_ref.score_from_encoded(wt, hV_r, hE_r, t["E_idx"][b:b + 1].long(), t["S"][b:b + 1], t["mask"][b:b + 1],
                                     t["chain_mask"][b:b + 1], t["randn"][b:b + 1])
    assert maxdiff(logp[b:b + 1], ref["log_probs"]) < TOL_LOGP
    valid = t["mask"][b].bool()
    assert torch.equal(logp[b].argmax(-1).cpu()[valid], ref["log_probs"][0].argmax(-1)[valid])


def test_abi_error_reporting(L, dev, packed):
    x = torch.zeros(64 * 128 + 4, device=dev)
    out = torch.zeros(64 * 128, device=dev)
    proj = hip.NampProj(packed.addr("Wv_img"), None, None, out.data_ptr())
    rc = L.namp_node_linear(x.data_ptr() + 4, None, 1, 1, 64, C.byref(proj), 1, None, stream())     # misaligned
    assert rc == -1 and b"aligned" in L.namp_last_error()
    rc = L.namp_edge_embed(packed.addr("We_img"), packed.addr("We_b"), x.data_ptr(), out.data_ptr(), 1, 1, 500, stream())
    assert rc == -1 and b"NAMP_MAX_K" in L.namp_last_error()
    rc = L.namp_encoder_fwd(packed.model(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), out.data_ptr(),
                            out.data_ptr(), out.data_ptr(), 16, 1, 4, 2, stream())                   # tiny workspace
    assert rc == -3
    with pytest.raises(RuntimeError):
        hip.check(rc, "encoder_fwd")


@pytest.mark.parametrize("n,k", [(1, 1), (2, 2), (5, 3), (17, 16), (70, 64), (90, 80), (120, 100), (200, 130)])
def test_small_and_wide_neighbourhoods(L, dev, wt, packed, n, k):
    """Edge cases of the tiling: single-residue graphs, K below one tile, K = 64 / 80 / 100 / 130 (4..9 tiles per
    residue, i.e. 3 / 2 / 1 / 1 residues per workgroup) — encoder + decoder against the oracle."""
    t, d = graph(dev, seed=900 + n, batch=2, n=n, k=k, masked_frac=0.1 if n > 10 else 0.0)
    K = t["E_idx"].shape[-1]
    hV, hE, logp, order = run_encdec(L, dev, packed, d, 2, n, K)
    for b in range(2):
        sl = slice(b, b + 1)
        rV, rE = cpu_ref.encode_from_graph(wt, t["V"][sl], t["E"][sl], t["E_idx"][sl].long(), t["mask"][sl])
        ref = cpu_ref.score_from_encoded(wt, rV, rE, t["E_idx"][sl].long(), t["S"][sl], t["mask"][sl],
                                         t["chain_mask"][sl], t["randn"][sl])
        assert torch.equal(order[b].cpu(), ref["decoding_order"])
        assert maxdiff(hV[sl], rV) < TOL_ACT and maxdiff(hE[sl], rE) < TOL_ACT
        assert maxdiff(logp[sl], ref["log_probs"]) < TOL_LOGP
        valid = t["mask"][b].bool()
        assert torch.equal(logp[b].argmax(-1).cpu()[valid], ref["log_probs"][0].argmax(-1)[valid])


def test_cfg3_sized_batch(L, dev, wt, packed):
    """BASELINE configs[2] shape at the parity precisions: B=64 x N=1000, K=48 (3.07 M edges, unfused large-batch path).
    EXACT fp32 (the headline dtype): log-probs within 1e-3 of the oracle and arg-max sequences STRICTLY identical on the
    spot-checked complexes (north_star: "argmax sequences bit-exact").  Split-bf16 (the product's default): the same bar,
    except that a residue whose top two ORACLE log-probs are closer than 2e-3 may flip — the number of residues that used
    the exception is printed.  Whole batch: normalisation / finiteness / batch independence."""
    B, N, K = 64, 1000, 48
    parts = [synth.make_graph(seed=7000 + b, batch=1, n=N, k=K) for b in range(B)]
    g = {k_: np.concatenate([p[k_] for p in parts], 0) for k_ in parts[0]}
    t = {k_: torch.from_numpy(v) for k_, v in g.items()}
    d = {k_: v.to(dev) for k_, v in t.items()}
    _, _, logp, _ = run_encdec(L, dev, packed, d, B, N, K)                  # split-bf16 (the fixture's default precision)
    packed.set_precision("fp32")
    try:
        _, _, logp32, _ = run_encdec(L, dev, packed, d, B, N, K)            # exact fp32 MFMA
    finally:
        packed.set_precision("x3")
    for lp in (logp, logp32):
        assert torch.isfinite(lp).all()
        assert maxdiff(torch.logsumexp(lp, -1), torch.zeros(B, N)) < 1e-5
    near_ties_used = 0
    oracle_lp = {}
    for b in (0, 13, 31, 47, 63):
        sl = slice(b, b + 1)
        rV, rE = cpu_ref.encode_from_graph(wt, t["V"][sl], t["E"][sl], t["E_idx"][sl].long(), t["mask"][sl])
        ref = cpu_ref.score_from_encoded(wt, rV, rE, t["E_idx"][sl].long(), t["S"][sl], t["mask"][sl],
                                         t["chain_mask"][sl], t["randn"][sl])
        ar = ref["log_probs"][0].argmax(-1)
        oracle_lp[b] = ref["log_probs"][0]
        # exact fp32: strict
        assert maxdiff(logp32[sl], ref["log_probs"]) < TOL_LOGP
        assert torch.equal(logp32[b].argmax(-1).cpu(), ar), f"exact fp32: arg-max sequence of complex {b} differs from the oracle's"
        # split-bf16: arg-max identical, except where the oracle's own top two log-probs are closer than 2 x the tolerance
        assert maxdiff(logp[sl], ref["log_probs"]) < TOL_LOGP
        am = logp[b].argmax(-1).cpu()
        for i in torch.nonzero(am != ar).flatten().tolist():
            r = ref["log_probs"][0][i]
            assert abs(float(r[am[i]] - r[ar[i]])) < 2 * TOL_LOGP, (b, i, float(r[am[i]]), float(r[ar[i]]))
        assert int((am != ar).sum()) <= 1
        near_ties_used += int((am != ar).sum())
    print(f"cfg3-sized parity: exact fp32 arg-max identical on 5 x {N} residues; split-bf16 used the near-tie exception on "
          f"{near_ties_used} of {5 * N} residues")
    d1 = {k_: v[31:32].contiguous() for k_, v in d.items()}
    _, _, logp1, _ = run_encdec(L, dev, packed, d1, 1, N, K)          # fused small-batch path on the same complex
    assert maxdiff(logp1, logp[31:32]) < 5e-5
    # BASELINE configs[2] itself: the bf16 throughput mode AT this size, through the one-call path bench.py times (bf16
    # MFMA + bf16 storage of h_E and the gathered tables).  Bar = the bf16 accuracy class on all 64,000 residues.
    P = PackedWeights({k_: v.to(dev) for k_, v in wt.items()}, 3, 3, 33, dev)
    P.set_precision("bf16")
    _, _, lp16, _ = run_encdec(L, dev, P, d, B, N, K, joint=True)
    assert torch.isfinite(lp16).all()
    assert maxdiff(torch.logsumexp(lp16, -1), torch.zeros(B, N)) < 1e-5
    err = maxdiff(lp16, logp.cpu())
    agree = float((lp16.argmax(-1) == logp.argmax(-1)).float().mean())
    print(f"cfg3-sized bf16: max|dlogp| vs parity mode = {err:.4f}, arg-max agreement = {agree:.4f}")
    # the bf16 accuracy CLASS the reference's own whole-model autocast reaches (0.055, 99.3 %) — round 4 spends the
    # budget rounds 2-3 left unused (0.016 / 99.64 %): plain-bf16 residue-level GEMMs and a degree-4 GELU polynomial
    assert err <= 0.055 and agree >= 0.99
    # ... and against the ORACLE itself on the five spot-checked complexes (not only against the HIP parity mode): same class
    err_o = max(maxdiff(lp16[b], oracle_lp[b]) for b in oracle_lp)
    agree_o = float(np.mean([float((lp16[b].argmax(-1).cpu() == oracle_lp[b].argmax(-1)).float().mean()) for b in oracle_lp]))
    print(f"cfg3-sized bf16 vs the CPU oracle (5 complexes): max|dlogp| = {err_o:.4f}, arg-max agreement = {agree_o:.4f}")
    assert err_o <= 0.055 and agree_o >= 0.99


def test_bf16_throughput_mode(L, dev, wt, golden_dir):
    """BASELINE configs[2]: per-edge GEMMs on bf16 MFMA (fp32 accumulate).  Not the parity mode — the bar here is
    the accuracy class SURVEY F9 measured for bf16 (max |dlogp| 0.055, arg-max agreement 99.3 %): log-probs within
    0.15 of the fp32 reference and >= 97 % arg-max agreement; fp32 mode on the same packed weights is untouched."""
    g = np.load(os.path.join(golden_dir, "g3_encdec_n1000.npz"))
    t, d = graph(dev, seed=300 + 1000 + 1, batch=1, n=1000, k=48)
    P = PackedWeights({k_: v.to(dev) for k_, v in wt.items()}, 3, 3, 33, dev)
    P.set_precision("bf16")
    _, _, logp, _ = run_encdec(L, dev, P, d, 1, 1000, 48)
    ref = torch.from_numpy(g["log_probs"])
    err = maxdiff(logp, ref)
    agree = float((logp.argmax(-1).cpu() == ref.argmax(-1)).float().mean())
    print(f"bf16 mode: max|dlogp| = {err:.4f}, arg-max agreement = {agree:.4f}")
    assert err < 0.15 and agree >= 0.97
    P.set_precision("fp32")
    _, _, logp32, _ = run_encdec(L, dev, P, d, 1, 1000, 48)
    assert maxdiff(logp32, ref) < TOL_LOGP
    # large-batch (unfused) bf16 path
    t2, d2 = graph(dev, seed=61, batch=5, n=900, k=48)
    P.set_precision("bf16")
    _, _, lp_b, _ = run_encdec(L, dev, P, d2, 5, 900, 48)
    P.set_precision("fp32")
    _, _, lp_f, _ = run_encdec(L, dev, P, d2, 5, 900, 48)
    assert maxdiff(lp_b, lp_f) < 0.15 and float((lp_b.argmax(-1) == lp_f.argmax(-1)).float().mean()) >= 0.97
    # the single fused call additionally STORES h_E and the gathered tables in bf16 on such batches
    P.set_precision("bf16")
    _, _, lp_s, _ = run_encdec(L, dev, P, d2, 5, 900, 48, joint=True)
    err_s, agree_s = maxdiff(lp_s, lp_f), float((lp_s.argmax(-1) == lp_f.argmax(-1)).float().mean())
    print(f"bf16 storage mode: max|dlogp| = {err_s:.4f}, arg-max agreement = {agree_s:.4f}")
    assert err_s < 0.15 and agree_s >= 0.97
    # the persistent bf16 kernel on tile shapes with padding rows (K not a multiple of 16) and masked residues
    # (..., an odd number of row tiles in all — a trailing half pair in the 32-row kernels —, one tile per residue, eight tiles per residue)
    for (b, n, k, mf) in ((6, 700, 30, 0.1), (9, 520, 20, 0.0), (3, 1500, 70, 0.05), (3, 901, 16, 0.1), (1, 2600, 128, 0.0)):
        t3, d3 = graph(dev, seed=70 + k, batch=b, n=n, k=k, masked_frac=mf)
        P.set_precision("bf16")
        _, _, lp_b, _ = run_encdec(L, dev, P, d3, b, n, k)
        _, _, lp_s, _ = run_encdec(L, dev, P, d3, b, n, k, joint=True)            # bf16 storage path
        P.set_precision("fp32")
        _, _, lp_f, _ = run_encdec(L, dev, P, d3, b, n, k)
        valid = t3["mask"].bool().to(dev)
        for lp_x in (lp_b, lp_s):
            assert torch.isfinite(lp_x).all()
            assert maxdiff(lp_x[valid], lp_f[valid]) < 0.15, (b, n, k)
            assert float((lp_x.argmax(-1) == lp_f.argmax(-1))[valid].float().mean()) >= 0.97, (b, n, k)


@pytest.mark.parametrize("b,n,k,mf", [(5, 900, 48, 0.0), (6, 700, 30, 0.1), (3, 901, 16, 0.1), (1, 2600, 128, 0.0), (9, 520, 20, 0.0)])
def test_bf16p_equals_bf16s32(L, dev, wt, b, n, k, mf):
    """The round-6 sequencing of the bf16-storage edge launches (edge_mlp_bf16p_kernel: accumulator-major blocks, every MFMA slot carrying
    a slice of the previous block's epilogue) against the round-3 kernels it replaces (edge_mlp_bf16s32_kernel), through namp_encdec_fwd:
    same accumulation order, same rounding points, so h_V and the log-probabilities must agree to the BIT — incl. K % 16 != 0 (padding
    rows), an odd number of row tiles (a trailing half pair), masked residues, one and eight tiles per residue."""
    t, d = graph(dev, seed=70 + k, batch=b, n=n, k=k, masked_frac=mf)
    P = PackedWeights({k_: v.to(dev) for k_, v in wt.items()}, 3, 3, 33, dev)
    P.set_precision("bf16")
    prev = L.namp_set_bf16p(0)
    try:
        hV0, _, lp0, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
        for mask in (1, 2 | 16, 4, 7 | 16):              # (bit 4: the edge update's LayerNorm in the round-3 kernel's two-pass form)
            L.namp_set_bf16p(mask)
            hV1, _, lp1, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
            assert torch.isfinite(lp1).all()
            assert torch.equal(hV0, hV1), (mask, float((hV0 - hV1).abs().max()))
            assert torch.equal(lp0, lp1), (mask, float((lp0 - lp1).abs().max()))
        # the product's one-pass LayerNorm sums (var = E[x^2] - mean^2): same rows up to fp32 rounding of the statistics — a bf16 rounding of an
        # h_E element flips here and there, nothing more
        L.namp_set_bf16p(3)
        hV2, _, lp2, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
        valid = t["mask"].bool().to(dev)
        err = float((lp2 - lp0)[valid].abs().max())
        agree = float((lp2.argmax(-1) == lp0.argmax(-1))[valid].float().mean())
        print(f"one-pass LayerNorm 3 vs two-pass: max|dlogp| = {err:.2e}, arg-max agreement = {agree:.4f}")
        assert err < 0.03 and agree >= 0.99
    finally:
        L.namp_set_bf16p(prev)


@pytest.mark.parametrize("b,n,k,mf", [(5, 900, 48, 0.0), (6, 700, 30, 0.1), (3, 901, 16, 0.1), (9, 520, 20, 0.05)])
def test_node_update_w_matches_multi(L, dev, wt, b, n, k, mf):
    """The round-6 residue update of the bf16-storage path (node_update_w_kernel: one 16-row tile per wave end to end, weight blocks through
    an LDS ring) against the kernel it replaces there (node_update_multi_kernel<2, 2>), through namp_encdec_fwd: same operand rounding, fp32
    accumulation and LayerNorms; only the summation order of the FFN's second product differs (one chain over the four hidden blocks instead
    of eight per-wave partial sums) — which flips bf16 roundings downstream, so the two are two draws of the mode's rounding noise, not equal.
    Bar: EACH within the bf16 accuracy class of the exact-fp32 evaluation of the same launches (0.055 / 99 %), the new one no
    further from fp32 than 1.25 x the old one + 0.005, and the two within 0.05 / 98.5 % of each other; masked residues identical (zero rows);
    rows not a multiple of 64, K % 16 != 0 and masked residues included."""
    t, d = graph(dev, seed=170 + k, batch=b, n=n, k=k, masked_frac=mf)
    P = PackedWeights({k_: v.to(dev) for k_, v in wt.items()}, 3, 3, 33, dev)
    P.set_precision("fp32")
    _, _, lpf, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
    P.set_precision("bf16")
    prev = L.namp_set_bf16p(3)
    try:
        hV0, _, lp0, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
        L.namp_set_bf16p(11)
        hV1, _, lp1, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
    finally:
        L.namp_set_bf16p(prev)
    valid = t["mask"].bool().to(dev)
    assert torch.isfinite(lp1).all() and torch.isfinite(hV1).all()
    e0, e1 = float((lp0 - lpf)[valid].abs().max()), float((lp1 - lpf)[valid].abs().max())
    a0 = float((lp0.argmax(-1) == lpf.argmax(-1))[valid].float().mean())
    a1 = float((lp1.argmax(-1) == lpf.argmax(-1))[valid].float().mean())
    err = float((lp0 - lp1)[valid].abs().max())
    agree = float((lp0.argmax(-1) == lp1.argmax(-1))[valid].float().mean())
    print(f"vs exact fp32: multi {e0:.4f} / {a0:.4f}, node_update_w {e1:.4f} / {a1:.4f}; w vs multi: {err:.4f} / {agree:.4f}")
    assert e0 <= 0.055 and a0 >= 0.99 and e1 <= 0.055 and a1 >= 0.99
    assert e1 <= 1.25 * e0 + 0.005
    assert err <= 0.05 and agree >= 0.985
    assert torch.equal(hV1[~valid], hV0[~valid])              # masked residues: zero rows in both


@pytest.mark.parametrize("G,V,want_logits", [(5000, 33, True), (4099, 33, False), (64000, 33, False), (4100, 21, True), (100, 33, True)])
def test_logits_head_matches_torch(L, dev, G, V, want_logits):
    """namp_logits_log_softmax — the small-batch kernel (one token per lane) and, from 4,096 residues, logits_mfma_kernel (16-row tiles on the
    exact-fp32 matrix pipe, W_out as a fragment image built in LDS, the tile's [16][V] block written through LDS) — against torch in fp64:
    log-probs and logits within 2e-5, rows normalised; G not a multiple of 16 and a vocabulary of 21 (V * rows not a multiple of 4) included."""
    _logits_head_case(L, dev, G, V, want_logits, 1.0)


@pytest.mark.parametrize("G,V,want_logits", [(4100, 33, True), (100, 21, True)])
def test_logits_head_matches_torch_scaled(L, dev, G, V, want_logits):
    """The same with the rows x 20 (logits of +-100 and more: exp() of an unshifted logit would overflow), both kernels.  Bar: 2e-5, or
    4 x the deviation of torch's own fp32 CPU evaluation from fp64 on the same inputs where that is larger."""
    _logits_head_case(L, dev, G, V, want_logits, 20.0)


def _logits_head_case(L, dev, G, V, want_logits, scale):
    g = torch.Generator().manual_seed(G + V)
    h = (scale * torch.randn(G, 128, generator=g)).to(dev)
    W = (torch.randn(V, 128, generator=g) * 0.2).to(dev).contiguous()
    b = (torch.randn(V, generator=g) * 0.1).to(dev)
    lp = torch.full((G, V), float("nan"), device=dev)
    lg = torch.full((G, V), float("nan"), device=dev) if want_logits else None
    hip.check(L.namp_logits_log_softmax(W.data_ptr(), b.data_ptr(), h.data_ptr(), lp.data_ptr(), hip.ptr(lg), G, V, stream()))
    torch.cuda.synchronize()
    z = h.double() @ W.double().t() + b.double()
    ref = torch.log_softmax(z, -1)
    bar_lp = bar_lg = 2e-5
    if scale != 1.0:
        assert float(z.abs().max()) > 100.0
        zc = h.cpu() @ W.cpu().t() + b.cpu()
        dev_lp = float((torch.log_softmax(zc, -1).double() - ref.cpu()).abs().max())
        dev_lg = float((zc.double() - z.cpu()).abs().max())
        bar_lp, bar_lg = max(bar_lp, 4 * dev_lp), max(bar_lg, 4 * dev_lg)
        print(f"log-probs: error {float((lp.double() - ref).abs().max()):.2e}, bar {bar_lp:.2e} (torch fp32 on the CPU: {dev_lp:.2e}); "
              f"logits bar {bar_lg:.2e} (torch fp32 on the CPU: {dev_lg:.2e})")
    assert torch.isfinite(lp).all()
    assert float((lp.double() - ref).abs().max()) < bar_lp
    if want_logits:
        assert float((lg.double() - z).abs().max()) < bar_lg
    assert float((torch.logsumexp(lp.double(), -1)).abs().max()) < 1e-5


@pytest.mark.parametrize("b,n,k,mf", [(5, 900, 48, 0.0), (3, 901, 30, 0.1), (40, 75, 16, 0.05)])
def test_node_update_w_split_bf16(L, dev, wt, b, n, k, mf):
    """node_update_w_kernel<true> — the residue update of the split-bf16 (parity) mode on large batches, hi and mid planes of every weight block
    as separate LDS ring entries — against the exact-fp32 evaluation of the same launches and against node_update_multi_kernel<2, 1>, the kernel it
    replaces there: log-probs within 2e-4 of fp32 (the mode is fp32-equivalent to ~2^-16 per product; parity bar 1e-3), arg-max identical except
    at near-ties, and within 1e-4 of the kernel it replaces (another order of the three split products)."""
    t, d = graph(dev, seed=270 + k, batch=b, n=n, k=k, masked_frac=mf)
    P = PackedWeights({k_: v.to(dev) for k_, v in wt.items()}, 3, 3, 33, dev)
    P.set_precision("fp32")
    _, _, lpf, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
    P.set_precision("x3")
    prev = L.namp_set_bf16p(3)
    try:
        hV0, _, lp0, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
        L.namp_set_bf16p(11)
        hV1, _, lp1, _ = run_encdec(L, dev, P, d, b, n, k, joint=True)
    finally:
        L.namp_set_bf16p(prev)
    valid = t["mask"].bool().to(dev)
    e0, e1, e01 = (float((x - y)[valid].abs().max()) for x, y in ((lp0, lpf), (lp1, lpf), (lp0, lp1)))
    print(f"split-bf16 residue update: multi vs fp32 {e0:.2e}, node_update_w vs fp32 {e1:.2e}, w vs multi {e01:.2e}")
    assert torch.isfinite(lp1).all()
    assert e1 < 2e-4 and e01 < 1e-4
    flips = (lp1.argmax(-1) != lpf.argmax(-1)) & valid
    for bi, i in torch.nonzero(flips).tolist():
        top2 = lpf[bi, i].topk(2).values
        assert float(top2[0] - top2[1]) < 2e-3, (bi, i)
    assert torch.equal(hV1[~valid], hV0[~valid])


@pytest.mark.parametrize("B,N,K", [(3, 333, 48), (2, 257, 30), (1, 75, 16), (5, 201, 70)])
def test_bf16_storage_message_kernel(dev, B, N, K):
    """namp_bf16s_message (edge_mlp_bf16s32_kernel, v_mfma_f32_32x32x16_bf16 on rows stored in fragment order B) against a torch
    restatement with the kernel's rounding points (operands in bf16, fp32 accumulation, exact-erf GELU): K-sums of the layer-2
    activations of both message modes, incl. odd tile counts (a trailing half pair), K % 16 != 0 and random neighbour indices.
    Bar 5e-3 on sums of up to 48 activations weighted 1/30 (the bf16-mode GELU polynomial is within 1.3e-3 per value since round 4, its
    errors partly systematic in sign; measured 8.4e-4 with round 3's degree-6 form); the weight sums exact."""
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("bf16s32_check", os.path.join(os.path.dirname(__file__), "..", "tools", "bf16s32_check.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    for mode, (err, smax, _, dw) in mod.case(B, N, K, dev, seed=B * 1000 + K).items():
        print(f"bf16s32 {mode}: max abs dS = {err:.2e} (max abs S {smax:.2f})")
        assert err < 5e-3 and smax > 1.0, (mode, err, smax)
        assert dw < 1e-6, (mode, dw)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("B,N,K,mf", [(1, 1000, 48, 0.0), (1, 333, 40, 0.1), (2, 400, 48, 0.05), (1, 37, 35, 0.0), (1, 1024, 48, 0.0)])
def test_persistent_forward_equals_launch_chain(L, dev, wt, B, N, K, mf, prec):
    """namp_encdec_fwd as ONE persistent launch (h_E in registers across all six layers, in-kernel grid barriers) against
    the seven-launch chain on the same inputs: every output bit-identical, every grid barrier completed — repeated, so
    that a stale table line (a missing acquire) or a lost arrival would show."""
    t, d = graph(dev, seed=900 + N + K, batch=B, n=N, k=K, masked_frac=mf)
    KK = t["E_idx"].shape[-1]
    P = PackedWeights({k_: v.to(dev) for k_, v in wt.items()}, 3, 3, 33, dev)
    P.set_precision(prec)
    order = torch.argsort((d["mask"] * d["chain_mask"] + 0.0001) * torch.abs(d["randn"]))
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(N, device=dev).expand(B, -1))
    rank = rank.to(torch.int32)
    ws = torch.empty(2 * L.namp_workspace_bytes(B, B, N, KK), dtype=torch.uint8, device=dev)

    def run():
        hV = torch.full((B, N, 128), float("nan"), device=dev)
        hE = torch.full((B, N, KK, 128), float("nan"), device=dev)
        logp = torch.full((B, N, 33), float("nan"), device=dev)
        logits = torch.full((B, N, 33), float("nan"), device=dev)
        hip.check(L.namp_encdec_fwd(P.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(), d["mask"].data_ptr(),
                                    d["S"].data_ptr(), rank.data_ptr(), hV.data_ptr(), hE.data_ptr(), logp.data_ptr(), logits.data_ptr(),
                                    ws.data_ptr(), ws.numel(), B, N, KK, stream()))
        torch.cuda.synchronize()
        return hV, hE, logp, logits

    prev = L.namp_set_persistent(0)
    try:
        ref = run()
        L.namp_set_persistent(1)
        code = C.c_int32(-1)
        for rep in range(4):
            ws.fill_(0xCD)                                     # poison the barrier state: the launch must re-initialise it
            got = run()
            hip.check(L.namp_persistent_status(ws.data_ptr(), ws.numel(), B, N, KK, C.byref(code)))
            assert code.value == 0, hex(code.value)
            for a_, b_, name in zip(got, ref, ("h_V", "h_E", "log_probs", "logits")):
                assert torch.equal(a_, b_), (name, rep, float((a_ - b_).abs().max()))
    finally:
        L.namp_set_persistent(prev)
    assert torch.isfinite(ref[2]).all()
