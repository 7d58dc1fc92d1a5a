"""The memory contract of namp_train_feat_wgrad with a coordinate gradient attached (namp_train_feat_xgrad)
under the guarded buffers of tests/guarded.py, for both atom forms of the carrier: nothing outside the declared buffers is written, the
input section (the weight) is found unchanged, the output section does not depend on what the workspace held, neighbour indices out of
range give the bits of the call with the clamped indices, and dW_part has the bits of the unattached call."""
import pytest
import torch

from na_mpnn_amd import hip
import xgrad_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
H, COLS = 128, 5200


@pytest.mark.parametrize("form", ["x18_m18", "packed"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 17)])
def test_attached_carrier_under_guarded_buffers(shape, form):
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    Lb, dev = hip.lib(), torch.device("cuda:0")
    B, L, K = shape
    E, G = B * L * K, B * L
    prec = 0 if form == "x18_m18" else 1                          # the exact-fp32 launch takes X18 + M18, the split-bf16 launch the packed atoms
    g = mc.gen(61)
    X18 = mc.rn(g, G, 18, 3, sc=3.0)
    M18 = (torch.rand(G, 18, generator=g) > 0.2).float()
    M18[0, 1] = 1.0
    idx0 = mc.rand_idx(g, B, L, K)
    E_pos, g_pre, W = mc.rn(g, E, 16), mc.rn(g, E, H), mc.rn(g, H, COLS, sc=0.05)
    dims = (E, B, L, K)
    need, o_in, o_out = (getattr(Lb, "namp_train_feat_xgrad_" + n)(*dims) for n in ("ws_ints", "in_offset", "out_offset"))
    plain = Lb.namp_train_feat_wgrad_ws_ints(E)
    assert need > 0 and plain <= o_in and o_in + H * COLS <= o_out and o_out + 54 * G <= need
    Wd = W.to(dev)

    def arena(idx, attach):
        ar = Arena(dev)
        if prec:
            Xb, Mb = ar.inp("X18", torch.cat((X18, M18.unsqueeze(-1)), -1)), None
        else:
            Xb, Mb = ar.inp("X18", X18), ar.inp("M18", M18)
        ib, pb, gb = ar.inp("E_idx", idx), ar.inp("E_pos", E_pos), ar.inp("g_pre", g_pre)
        dW = ar.out("dW_part", mc.f32, (Lb.namp_train_feat_wgrad_chunks(E), H, COLS))
        tws = ar.ws("tile_ws", 4 * (need if attach else plain))
        seen = []

        def call(_ar=None):
            sec = tws.t[4 * o_in:4 * (o_in + H * COLS)].view(torch.float32).view(H, COLS) if attach else None
            if attach:
                sec.copy_(Wd)
                assert Lb.namp_train_feat_xgrad(need) == 0
            rc = Lb.namp_train_feat_wgrad(Xb.ptr, Mb.ptr if Mb else None, ib.ptr, pb.ptr, gb.ptr, None, dW.ptr, tws.ptr, prec, B, L, K,
                                          hip.current_stream())
            torch.cuda.synchronize()
            if attach:
                assert torch.equal(sec, Wd), "the call wrote into its input section"
                seen.append(tws.t[4 * o_out:4 * (o_out + 54 * G)].view(torch.float32).view(G, 18, 3).cpu().clone())
            return rc
        return ar, call, seen

    def run(idx, attach=True):
        ar, call, seen = arena(idx, attach)
        outs, reproducible = run_contract(call, ar)
        assert reproducible
        assert all(torch.equal(s.view(torch.int32), seen[0].view(torch.int32)) for s in seen)     # whatever the workspace held before
        return outs["dW_part"].cpu(), (seen[0] if attach else None)

    dW_a, dX = run(idx0)
    dW_p, _ = run(idx0, attach=False)
    assert torch.equal(dW_a.view(torch.int32), dW_p.view(torch.int32))                              # dW_part: the unattached call's bits
    ref = xgrad_ref.dX18_closed_form(W, X18.view(B, L, 18, 3), M18.view(B, L, 18), idx0, g_pre.view(B, L, K, H))
    e = xgrad_ref.rel(dX.view(B, L, 18, 3), torch.from_numpy(ref))
    print(f"contract {shape} {form}: dX18 rel {e:.2e}")
    assert torch.isfinite(dX).all() and e < 1e-4 and bool((dX[M18 == 0] == 0).all())

    # neighbour indices out of range: the bits of the clamped call.  (The carrier's own launches read the rows such an index names — a few
    # rows beside X18 / M18, inside the arena's guard bands here —, so dW_part is not defined for them and run_contract's checks of it do
    # not apply: guards and inputs are checked, and dX18 compared.)
    bad, ok = idx0.clone(), idx0.clone()
    bad[0, 0, 0], ok[0, 0, 0] = L + 3, L - 1
    bad[0, L - 1, K - 1], ok[0, L - 1, K - 1] = -2, 0
    got = []
    for t in (bad, ok):
        ar, call, seen = arena(t, True)
        ar.build("A")
        assert call() == 0
        ar.check()
        got.append(seen[0])
    assert torch.isfinite(got[0]).all() and torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
