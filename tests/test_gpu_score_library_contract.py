"""The memory contract of namp_decoder_fwd with a library attached (namp_library) under the guarded buffers of
tests/guarded.py: a correct call, and malformed sections — positions out of range, duplicate positions, tokens outside [0, vocab).
These are inputs the kernels are specified to clamp, with a defined result: the result of the call with the clamped values; the
input section is found unchanged, the outputs do not depend on what the workspace held, and nothing outside the declared buffers is
touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def plan_rows(env, t, N, K, pos):
    """The list sizes |U_1..3| of a library on the case's graph: one attached call with n_chunk = 0, read back."""
    dev = env.dev
    dims = (N, K, 3, len(pos), 0, 0, 0, 0)
    need, ioff, ooff = (f(*dims) for f in (env.L.namp_library_workspace_bytes, env.L.namp_library_in_offset, env.L.namp_library_out_offset))
    assert need > 0 and ioff % 256 == 0 and ooff % 256 == 0 and ioff + 4 * len(pos) <= ooff and ooff + 256 <= need
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ws[ioff:ioff + 4 * len(pos)].view(torch.int32).copy_(torch.tensor(pos, dtype=torch.int32))
    hV, hE, idx, S, msk, rank = (t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank"))
    lp = torch.zeros(1, N, 33, device=dev)
    assert env.L.namp_library(len(pos), 0, 0, 0, 0) == 0
    rc = env.L.namp_decoder_fwd(env.packed.model(), hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), S.data_ptr(), msk.data_ptr(), rank.data_ptr(),
                                lp.data_ptr(), None, None, ws.data_ptr(), need, 1, 1, N, K, env.s())
    assert rc == 0
    counts = ws[ooff:ooff + 36].view(torch.int32).tolist()
    assert counts[6:9] == [0, 0, 0] and all(a <= u for a, u in zip(counts[:3], counts[3:6]))
    return counts[3:6], counts[:3]


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_library_under_guarded_buffers(weights_np, shape, prec):
    """namp_decoder_fwd with a library of three sequences attached, under guarded buffers.  The correct call against the same three
    sequences as streams of the unattached decoder (< 2e-4, two summation orders) and its base rows against the unattached call;
    positions out of range, duplicate positions (the last listed column is the residue's) and tokens outside [0, vocab) give the
    bits of the call with the clamped values; a row capacity below the plan's counts gives a defined, reproducible result.
    Measured (MI355X) at (1, 17, 48): against the decoder's streams x3 5.2e-6, fp32 9.5e-7; the base rows are the unattached call's
    bits; 13 active and 14 evaluated rows per layer."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t = mc.graph_case(B, N, K)
    K = t["K"]
    n = 3

    def run(pos, tok, rows=None, plan_pos=None):
        rows = plan_rows(env, t, N, K, pos if plan_pos is None else plan_pos)[0] if rows is None else rows
        n_var = len(pos)
        dims = (N, K, 3, n_var, n) + tuple(rows)
        need, ioff, ooff = (f(*dims) for f in (env.L.namp_library_workspace_bytes, env.L.namp_library_in_offset, env.L.namp_library_out_offset))
        assert need > 0 and ioff + 4 * (n_var + n * n_var) <= ooff and ooff + 256 + 4 * n * N <= need
        section = torch.cat((torch.tensor(pos, dtype=torch.int32), torch.tensor(tok, dtype=torch.int32).reshape(-1))).to(env.dev)
        ar = Arena(env.dev)
        hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
        S, msk, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
        lp = ar.out("log_probs", mc.f32, (1, N, mc.V33))
        ws = ar.ws("ws", need)
        seen = []

        def call():
            ws.t[ioff:ioff + 4 * section.numel()].view(torch.int32).copy_(section)
            assert env.L.namp_library(n_var, n, *rows) == 0
            rc = env.L.namp_decoder_fwd(env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, msk.ptr, rank.ptr, lp.ptr, None, None, ws.ptr,
                                        ws.nbytes, 1, 1, N, K, env.s())
            torch.cuda.synchronize()
            assert torch.equal(ws.t[ioff:ioff + 4 * section.numel()].view(torch.int32), section), "the call wrote into its input section"
            out = ws.t[ooff:ooff + 256 + 4 * n * N]
            seen.append((out[:36].view(torch.int32).cpu().clone(), out[256:].view(torch.float32).view(n, N).cpu().clone()))
            return rc
        outs, reproducible = run_contract(lambda a: mc.with_precision(env, prec, call)(), ar)
        assert reproducible
        assert torch.equal(env.packed.flat, env.snapshot)
        assert all(torch.equal(c, seen[0][0]) and torch.equal(x, seen[0][1]) for c, x in seen)   # (the output section does not depend on what the workspace held)
        assert bool(torch.isfinite(seen[0][1]).all())
        return outs["log_probs"].cpu(), seen[0][1], seen[0][0].tolist()

    def streams(S_rows):
        """The same sequences as streams of the unattached decoder -> log_probs [len, N, 33]."""
        dev, b = env.dev, len(S_rows)
        hV, hE, idx, msk, rank = (t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "mask", "rank"))
        Sd = torch.tensor(S_rows, dtype=torch.int32, device=dev)
        msk_b, rank_b = msk.repeat(b, 1).contiguous(), rank.repeat(b, 1).contiguous()      # (held until the call's work is done)
        lp = torch.zeros(b, N, 33, device=dev)
        ws = torch.zeros(env.L.namp_workspace_bytes(1, b, N, K), dtype=torch.uint8, device=dev)
        rc = mc.with_precision(env, prec, lambda: env.L.namp_decoder_fwd(
            env.packed.model(), hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), Sd.data_ptr(), msk_b.data_ptr(), rank_b.data_ptr(),
            lp.data_ptr(), None, None, ws.data_ptr(), ws.numel(), b, 1, N, K, env.s()))()
        torch.cuda.synchronize()
        assert rc == 0
        return lp.cpu()

    S0 = t["S"][0].tolist()
    if N < 17:                                               # N = 1: the one residue; a position out of range is that residue
        tok = [[3], [30], [11]]
        lp, tlp, counts = run([0], tok)
        assert counts[:3] == [0, 0, 0] and counts[3:9] == [1] * 6
        ref = streams([[a[0]] for a in tok])
        assert float((tlp - torch.stack([ref[k, 0, tok[k][0]] for k in range(n)])[:, None]).abs().max()) < 2e-4
        lp_b, tlp_b, counts_b = run([7], tok)
        assert torch.equal(tlp_b, tlp) and torch.equal(lp_b, lp) and counts_b == counts
        lp_c, tlp_c, _ = run([0], [[-4], [77], [11]])
        lp_e, tlp_e, _ = run([0], [[0], [32], [11]])
        assert torch.equal(tlp_c, tlp_e) and torch.equal(lp_c, lp_e)
        return
    pos = [2, 5, 9, 11]
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(0, 33, (n, len(pos)), generator=g).tolist()
    lp, tlp, counts = run(pos, tok)
    assert counts[3:6] == counts[6:9] and counts[5] >= len(pos)
    full = [list(S0) for _ in range(n)]
    for k in range(n):
        for p, a in zip(pos, tok[k]):
            full[k][p] = a
    ref = streams(full + [S0])
    want = torch.stack([ref[k].gather(1, torch.tensor(full[k])[:, None])[:, 0] for k in range(n)])
    d, d_base = float((tlp - want).abs().max()), float((lp[0] - ref[n]).abs().max())
    print(f"library contract {shape} {prec}: max|d| vs the decoder's streams {d:.3e}, base rows {d_base:.3e}; counts {counts}")
    assert d < 2e-4 and d_base < 2e-4
    assert float((want[0] - want[1]).abs().max()) > 1e-2                                   # (the sequences do differ)
    # positions out of range: the call with the clamped values
    lp_b, tlp_b, counts_b = run([-3, 5, 99, 11], tok, plan_pos=[0, 5, N - 1, 11])
    lp_e, tlp_e, counts_e = run([0, 5, N - 1, 11], tok)
    assert torch.equal(tlp_b, tlp_e) and torch.equal(lp_b, lp_e) and counts_b == counts_e
    assert not torch.equal(tlp_b, tlp)
    # duplicate positions: the last listed column is the residue's
    lp_d, tlp_d, counts_d = run([2, 5, 5, 11], tok, plan_pos=[2, 5, 11])
    lp_e, tlp_e, counts_e = run([2, 5, 11], [[a[0], a[2], a[3]] for a in tok])
    assert torch.equal(tlp_d, tlp_e) and torch.equal(lp_d, lp_e) and counts_d == counts_e
    # tokens outside [0, vocab): clamped to the first / the last token
    bad = [list(a) for a in tok]
    clamped = [list(a) for a in tok]
    bad[0][1], bad[1][0], bad[2][3] = -4, 77, 33
    clamped[0][1], clamped[1][0], clamped[2][3] = 0, 32, 32
    lp_c, tlp_c, _ = run(pos, bad)
    lp_e, tlp_e, _ = run(pos, clamped)
    assert torch.equal(tlp_c, tlp_e) and torch.equal(lp_c, lp_e)
    # a row capacity below the plan's counts: rows beyond it are base rows — defined, reproducible, in bounds
    rows = plan_rows(env, t, N, K, pos)[0]
    lp_s, tlp_s, counts_s = run(pos, tok, rows=[max(1, r // 2) for r in rows])
    assert torch.equal(lp_s, lp) and counts_s[3:6] == rows and counts_s[6:9] == [max(1, r // 2) for r in rows]


def test_a_too_small_workspace_is_refused_and_clears_the_attachment(weights_np):
    """ws_bytes one byte short of namp_library_workspace_bytes: NAMP_EINVAL before any launch, and the attachment is gone — the NEXT
    plain namp_decoder_fwd call is the unattached one, bit for bit.  Bad arguments of namp_library attach nothing, and the sizes are
    0 where the route is not supported."""
    import test_gpu_memory_contract as mc
    env = mc.Env(weights_np)
    B, N, K = 1, 17, 16
    t = mc.graph_case(B, N, K)
    K = t["K"]
    dev = env.dev
    hV, hE, idx, S, msk, rank = (t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank"))

    def call(ws, nbytes):
        lp = torch.zeros(B, N, mc.V33, device=dev)
        rc = env.L.namp_decoder_fwd(env.packed.model(), hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), S.data_ptr(), msk.data_ptr(),
                                    rank.data_ptr(), lp.data_ptr(), None, None, ws.data_ptr(), nbytes, 1, 1, N, K, env.s())
        torch.cuda.synchronize()
        return rc, lp.cpu()
    plain_bytes = env.L.namp_workspace_bytes(1, 1, N, K)
    plain_ws = torch.zeros(plain_bytes, dtype=torch.uint8, device=dev)
    rc, lp_plain = call(plain_ws, plain_bytes)
    assert rc == 0 and float(lp_plain.abs().max()) > 0
    pos = [2, 5, 9, 11]
    rows = plan_rows(env, t, N, K, pos)[0]
    dims = (N, K, 3, len(pos), 3) + tuple(rows)
    need = env.L.namp_library_workspace_bytes(*dims)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ioff = env.L.namp_library_in_offset(*dims)
    ws[ioff:ioff + 16].view(torch.int32).copy_(torch.tensor(pos, dtype=torch.int32))
    assert env.L.namp_library(len(pos), 3, *rows) == 0
    rc, lp = call(ws, need - 1)
    assert rc == -1 and b"workspace too small" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)                     # plain: the attachment was cleared by the refused call
    assert rc == 0 and torch.equal(lp, lp_plain)
    # an attached call that succeeds clears it as well
    assert env.L.namp_library(len(pos), 3, *rows) == 0
    rc, lp = call(ws, need)
    assert rc == 0 and float((lp - lp_plain).abs().max()) < 2e-4
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    # bad arguments attach nothing
    assert env.L.namp_library(-1, 3, *rows) == -1
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    # sizes are 0 where unsupported: another number of decoder layers, K > N, n_var > N, a capacity above N
    for bad in ((N, K, 4, 4, 3, 4, 4, 4), (N, N + 1, 3, 4, 3, 4, 4, 4), (N, K, 3, N + 1, 3, 4, 4, 4), (N, K, 3, 4, 3, 4, 4, N + 1)):
        assert env.L.namp_library_workspace_bytes(*bad) == 0 and env.L.namp_library_in_offset(*bad) == 0
        assert env.L.namp_library_out_offset(*bad) == 0
