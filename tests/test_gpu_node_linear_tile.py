"""node_linear at small G through the C ABI: node_linear_tile_kernel (one workgroup per 16-row tile, one wave per channel tile) serves
launches of one or two blocks, node_linear_kernel (one wave per (tile, block)) those of more; both are held to the same references.

The small-G kernel deals the eight channel tiles of every 128 x 128 product over eight waves and hands the `pre` product on through
LDS; the arithmetic per output element is that of node_linear_kernel (one wave per (tile, projection)): accumulator = bias, then the
fragments of the element's channel tile in image order.  Checked here

  * bitwise against that formulation evaluated on the host in the same order (fp32 products: for tk ascending, for r ascending, one
    v_mfma_f32_16x16x4_f32 adds the products of k = 16 tk + 4 g + r, g = 0..3 — MFMA_MODEL below states how one instruction rounds),
  * bitwise against node_linear_kernel itself: the same rows inside a launch of more tiles than the device has compute units, which
    the wave-per-unit kernel serves (exact fp32 only: large split-bf16 launches may take a third kernel),
  * against torch fp64 within 2e-4 of the largest reference value (exact fp32 and split-bf16; the figure of the issue), and for plain
    bf16 products (hi . hi) within the bound of the format: 2^-7 sum_k |W||x| per element (two operands rounded to 8 bits each).

Shapes: G = 1, 15, 16, 17, 250 (below, at and above one tile; a partly filled last tile; several workgroups), with and without `pre`,
nproj = 1, 2, 8 (8 = the capacity of the descriptor array), a token table on one projection with tokens at both ends of the table,
null and non-null biases, and a broadcast source (B_src = 1 feeding B_out = 2).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

H, VOCAB, GMAX = 128, 33, 250
REL_F64 = 2e-4
SIZES = [1, 15, 16, 17, 250]
TOK_AT, NOBIAS_AT = 0, 1           # projection 0 carries the token table (and a bias), projection 1 has no bias
# How one v_mfma_f32_16x16x4_f32 adds its four products to the accumulator: "fma4" = four fused multiply-adds in k order (one rounding
# each).  The other orders a matrix unit could use ("dot4": exact four-term dot product rounded once with the accumulator) are kept in
# host_products so that a reader can see what was ruled out on the device.
MFMA_MODEL = "fma4"


def stream():
    return hip.current_stream()


def host_products(W, x, bias, model=MFMA_MODEL):
    """out[row][n] of one 128 x 128 product in node_linear_kernel's order, fp32, on the host.  W [128 out][128 in], x [G][128]."""
    LD = np.longdouble                                             # 64-bit mantissa: a product of two fp32 is exact, a sum rounds at 2^-64
    acc = np.broadcast_to(bias if bias is not None else np.zeros(H, np.float32), (x.shape[0], H)).astype(np.float32).copy()
    Wl, xl = W.astype(LD), x.astype(LD)
    for tk in range(8):
        for r in range(4):
            ks = [16 * tk + 4 * g + r for g in range(4)]
            if model == "fma4":
                for k in ks:
                    acc = (xl[:, k:k + 1] * Wl[None, :, k] + acc.astype(LD)).astype(np.float32)
            elif model == "dot4":
                s = acc.astype(LD)
                for k in ks:
                    s = s + xl[:, k:k + 1] * Wl[None, :, k]
                acc = s.astype(np.float32)
            else:
                raise ValueError(model)
    return acc


class Case:
    """Weights, inputs and host references, built once and shared: rows are independent, so a G-row launch is the first G rows of the
    250-row problem and an nproj-block launch the first nproj blocks."""

    def __init__(self, dev):
        rng = np.random.default_rng(20251)
        self.dev = dev
        self.Wpre = (rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32)
        self.bpre = rng.standard_normal(H).astype(np.float32)
        self.W = (rng.standard_normal((8, H, H)) / np.sqrt(H)).astype(np.float32)
        self.b = rng.standard_normal((8, H)).astype(np.float32)
        self.tok = rng.standard_normal((VOCAB, H)).astype(np.float32)
        self.X = rng.standard_normal((GMAX, H)).astype(np.float32)
        S = rng.integers(0, VOCAB, GMAX).astype(np.int32)
        S[0], S[1], S[14], S[15], S[16], S[GMAX - 1] = 0, VOCAB - 1, VOCAB - 1, 0, VOCAB - 1, 0     # both ends of the table, around the tile edge
        self.S = S
        L = hip.lib()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d = {"X": t(self.X), "S": t(S), "b": t(self.b), "bpre": t(self.bpre), "tok": t(self.tok)}
        Wd = t(np.concatenate([self.Wpre[None], self.W]))
        self.img = torch.empty(9, H * H, device=dev)
        self.ximg = torch.empty(9, H * H, device=dev)              # x3 images: bf16 hi | bf16 mid, the size of the fp32 image
        for i in range(9):
            hip.check(L.namp_pack_image(Wd[i].data_ptr(), H, 0, H, H, self.img[i].data_ptr(), stream()))
            hip.check(L.namp_pack_image_x3(Wd[i].data_ptr(), H, 0, self.ximg[i].data_ptr(), stream()))
        torch.cuda.synchronize()
        self.keep = Wd
        self._host = {}

    def bias(self, q):
        return None if q == NOBIAS_AT else self.b[q]

    def host(self, pre):
        """(h or None, [8 projections]) bitwise references of all 250 rows."""
        if pre not in self._host:
            h = host_products(self.Wpre, self.X, self.bpre) if pre else None
            src = h if pre else self.X
            outs = []
            for q in range(8):
                o = host_products(self.W[q], src, self.bias(q))
                if q == TOK_AT:
                    o = o + self.tok[self.S]
                outs.append(o)
            self._host[pre] = (h, outs)
        return self._host[pre]

    def f64(self, pre):
        X = torch.from_numpy(self.X).double()
        h = X @ torch.from_numpy(self.Wpre).double().T + torch.from_numpy(self.bpre).double() if pre else None
        src = h if pre else X
        outs = []
        for q in range(8):
            o = src @ torch.from_numpy(self.W[q]).double().T
            if self.bias(q) is not None:
                o = o + torch.from_numpy(self.b[q]).double()
            if q == TOK_AT:
                o = o + torch.from_numpy(self.tok).double()[torch.from_numpy(self.S).long()]
            outs.append(o)
        return h, outs

    def run(self, G, nproj, pre, B_out=1, B_src=1, X=None, S=None, rows=None):
        """namp_node_linear on the first G rows (or on X / S given); returns (h or None, [nproj outputs]) as numpy."""
        L, d = hip.lib(), self.d
        X = d["X"] if X is None else X
        S = d["S"] if S is None else S
        rows = B_out * G if rows is None else rows
        outs = [torch.full((rows, H), float("nan"), device=self.dev) for _ in range(nproj)]
        hout = torch.full((rows, H), float("nan"), device=self.dev) if pre else None
        proj = (hip.NampProj * nproj)(*[
            hip.NampProj(self.img[1 + q].data_ptr(), None if q == NOBIAS_AT else d["b"][q].data_ptr(),
                         d["tok"].data_ptr() if q == TOK_AT else None, outs[q].data_ptr()) for q in range(nproj)])
        p = hip.NampProj(self.img[0].data_ptr(), d["bpre"].data_ptr(), None, hout.data_ptr()) if pre else None
        hip.check(L.namp_node_linear(X.data_ptr(), S.data_ptr(), B_out, B_src, G, proj, nproj, C.byref(p) if pre else None, stream()))
        torch.cuda.synchronize()
        return (hout.cpu().numpy() if pre else None), [o.cpu().numpy() for o in outs]


@pytest.fixture(scope="module")
def case():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return Case(torch.device("cuda:0"))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("pre", [False, True], ids=["nopre", "pre"])
@pytest.mark.parametrize("G", SIZES)
def test_small_g_bitwise_against_the_host_formulation(case, G, pre):
    """Every output element equals the host evaluation of node_linear_kernel's order bit for bit, and torch fp64 within 2e-4."""
    hh, ho = case.host(pre)
    h64, o64 = case.f64(pre)
    for nproj in (1, 2, 8):
        h, outs = case.run(G, nproj, pre)
        if pre:
            nbad = int((bits(h) != bits(hh[:G])).sum())
            print(f"node_linear G={G} nproj={nproj} pre: h differs from the host formulation in {nbad} of {h.size} elements")
            assert nbad == 0
            assert np.abs(h - h64[:G].numpy()).max() <= REL_F64 * float(h64.abs().max())
        for q in range(nproj):
            nbad = int((bits(outs[q]) != bits(ho[q][:G])).sum())
            err = float(np.abs(outs[q] - o64[q][:G].numpy()).max())
            print(f"node_linear G={G} nproj={nproj} pre={pre} block {q}: {nbad} of {outs[q].size} elements differ from the host "
                  f"formulation; max |out - fp64| = {err:.3e} (bar {REL_F64 * float(o64[q].abs().max()):.3e})")
            assert nbad == 0
            assert err <= REL_F64 * float(o64[q].abs().max())


@pytest.mark.parametrize("pre", [False, True], ids=["nopre", "pre"])
def test_small_g_bitwise_against_the_wave_per_unit_kernel(case, pre):
    """The 250 rows inside a launch of more tiles than compute units (node_linear_kernel) and alone (node_linear_tile_kernel): equal bits."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Gbig = 16 * (cus + 1)
    reps = (Gbig + GMAX - 1) // GMAX
    Xb = case.d["X"].repeat(reps, 1)[:Gbig].contiguous()
    Sb = case.d["S"].repeat(reps)[:Gbig].contiguous()
    hb, ob = case.run(Gbig, 2, pre, X=Xb, S=Sb)
    h, o = case.run(GMAX, 2, pre)
    if pre:
        assert np.array_equal(bits(h), bits(hb[:GMAX]))
    for q in range(2):
        assert np.array_equal(bits(o[q]), bits(ob[q][:GMAX])), q


def test_broadcast_source_rows(case):
    """B_src = 1 feeding B_out = 2 (the decoder's tables of a batch of sequences on one structure): output row n reads source row n % N."""
    G = 17
    _, o1 = case.run(G, 2, False)
    _, o2 = case.run(G, 2, False, B_out=2, B_src=1)                 # tokens of the second copy: S[G : 2G]
    second = host_products(case.W[TOK_AT], case.X[:G], case.bias(TOK_AT)) + case.tok[case.S[G:2 * G]]
    assert np.array_equal(bits(o2[TOK_AT][:G]), bits(o1[TOK_AT])) and np.array_equal(bits(o2[TOK_AT][G:]), bits(second))
    assert np.array_equal(bits(o2[NOBIAS_AT][:G]), bits(o1[NOBIAS_AT])) and np.array_equal(bits(o2[NOBIAS_AT][G:]), bits(o1[NOBIAS_AT]))


@pytest.mark.parametrize("prec", [1, 2], ids=["x3", "bf16"])
@pytest.mark.parametrize("G", SIZES)
def test_small_g_split_bf16_and_bf16_products(case, G, prec):
    """namp_node_linear_prec on x3 images: split-bf16 products within 2e-4 of fp64, plain bf16 products within the format's bound; the
    rows do not depend on how many rows or blocks the launch has (G rows against the first G of 250; 8 blocks against 1 and 2)."""
    L, d = hip.lib(), case.d

    def run(g, nproj):
        outs = [torch.full((g, H), float("nan"), device=case.dev) for _ in range(nproj)]
        proj = (hip.NampProj * nproj)(*[
            hip.NampProj(case.ximg[1 + q].data_ptr(), None if q == NOBIAS_AT else d["b"][q].data_ptr(), None, outs[q].data_ptr())
            for q in range(nproj)])
        hip.check(L.namp_node_linear_prec(d["X"].data_ptr(), g, proj, nproj, prec, stream()))
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    full = run(GMAX, 8)
    X64, absX = torch.from_numpy(case.X).double(), np.abs(case.X).astype(np.float64)
    for nproj in (1, 2, 8):
        outs = run(G, nproj)
        for q in range(nproj):
            assert np.array_equal(bits(outs[q]), bits(full[q][:G])), (nproj, q)
            ref = X64 @ torch.from_numpy(case.W[q]).double().T
            if case.bias(q) is not None:
                ref = ref + torch.from_numpy(case.b[q]).double()
            err = np.abs(outs[q] - ref[:G].numpy())
            if prec == 1:
                print(f"node_linear x3 G={G} nproj={nproj} block {q}: max |out - fp64| = {err.max():.3e} (bar {REL_F64 * float(ref.abs().max()):.3e})")
                assert err.max() <= REL_F64 * float(ref.abs().max())
            else:
                bound = 2.0 ** -7 * (absX[:G] @ np.abs(case.W[q]).astype(np.float64).T) + 1e-6
                print(f"node_linear bf16 G={G} nproj={nproj} block {q}: max err / bound = {(err / bound).max():.3f}")
                assert (err <= bound).all()
