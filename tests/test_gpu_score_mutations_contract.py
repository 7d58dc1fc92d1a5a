"""The memory contract of namp_decoder_fwd with a mutational scan attached (namp_mutations) under the guarded buffers
of tests/guarded.py: a correct call, and malformed sections — residues, site indices and tokens out of range, duplicate edits,
capacities below the counts.  These are inputs the kernels are specified to clamp, with a defined result: the result of the call
with the clamped values; the input section is found unchanged, the outputs do not depend on what the workspace held, and nothing
outside the declared buffers is touched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

E = 8                                                        # NAMP_MUT_MAX_EDITS


def pad(elems):
    """Bytes of one array of the output section (include/namp.h): one extra element, rounded up to 256."""
    return (4 * (elems + 1) + 255) & ~255


def section(sites, variants, w):
    s8 = np.full((len(sites), E), -1, np.int32)
    for q, row in enumerate(sites):
        s8[q, :len(row)] = row
    v9 = np.zeros((len(variants), 1 + E), np.int32)
    for q, row in enumerate(variants):
        v9[q, :len(row)] = row
    return torch.from_numpy(np.concatenate((s8.reshape(-1), v9.reshape(-1), np.asarray(w, np.float32).view(np.int32))))


def plan_sizes(env, t, N, K, sites):
    """|U_1..3(site)| of every site on the case's graph: one attached call with no variants, read back."""
    dev = env.dev
    dims = (N, K, 3, len(sites), 0, 0, 0, 0, 0, 0, 0)
    need, ioff, ooff = (f(*dims) for f in (env.L.namp_mutations_workspace_bytes, env.L.namp_mutations_in_offset, env.L.namp_mutations_out_offset))
    sec = section(sites, [], np.ones(N))
    assert need > 0 and ioff % 256 == 0 and ooff % 256 == 0 and ioff + 4 * sec.numel() <= ooff and ooff + 12 * len(sites) <= need
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    hV, hE, idx, S, msk, rank = (t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank"))
    lp = torch.zeros(1, N, 33, device=dev)
    assert env.L.namp_mutations(*dims[3:]) == 0
    rc = env.L.namp_decoder_fwd(env.packed.model(), hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), S.data_ptr(), msk.data_ptr(), rank.data_ptr(),
                                lp.data_ptr(), None, None, ws.data_ptr(), need, 1, 1, N, K, env.s())
    torch.cuda.synchronize()
    assert rc == 0
    return ws[ooff:ooff + 12 * len(sites)].view(torch.int32).view(len(sites), 3).tolist()


def capacities(sizes, variants, n_sites):
    lcap = [sum(s[l] for s in sizes) for l in range(3)]
    icap = [sum(sizes[min(max(v[0], 0), n_sites - 1)][l] for v in variants) for l in range(3)]
    return lcap, icap


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_mutations_under_guarded_buffers(weights_np, shape, prec):
    """namp_decoder_fwd with a scan attached, under guarded buffers.  The correct call against the same variants as streams of the
    unattached decoder (< 2e-4, two summation orders); residues >= N, site indices and tokens out of range, and duplicate edits
    (the last listed is the residue's) give the bits of the call with the clamped values; capacities below the counts give a
    defined, reproducible result; the input section is unchanged; nothing outside the declared buffers is written.
    Measured (MI355X) at (1, 17, 48): against the decoder's streams x3 5.7e-6, fp32 9.5e-7; the base rows are the unattached call's
    bits; sizes [6, 6, 6], [14, 14, 14], [14, 14, 14]."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t = mc.graph_case(B, N, K)
    K = t["K"]
    w = (np.arange(N) % 3 != 0).astype(np.float32) if N > 1 else np.ones(1, np.float32)

    def run(sites, variants, caps=None, plan_sites=None):
        sizes = plan_sizes(env, t, N, K, sites if plan_sites is None else plan_sites)
        lcap, icap = capacities(sizes, variants, len(sites)) if caps is None else caps
        ns, nv = len(sites), len(variants)
        dims = (N, K, 3, ns, nv) + tuple(lcap) + tuple(icap)
        need, ioff, ooff = (f(*dims) for f in (env.L.namp_mutations_workspace_bytes, env.L.namp_mutations_in_offset, env.L.namp_mutations_out_offset))
        sec = section(sites, variants, w).to(env.dev)
        out_bytes = pad(3 * ns) + pad(nv) + 2 * pad(icap[2])
        assert need > 0 and ioff + 4 * sec.numel() <= ooff and ooff + out_bytes <= need
        ar = Arena(env.dev)
        hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
        S, msk, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
        lp = ar.out("log_probs", mc.f32, (1, N, mc.V33))
        ws = ar.ws("ws", need)
        seen = []

        def call():
            ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
            assert env.L.namp_mutations(*dims[3:]) == 0
            rc = env.L.namp_decoder_fwd(env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, msk.ptr, rank.ptr, lp.ptr, None, None, ws.ptr,
                                        ws.nbytes, 1, 1, N, K, env.s())
            torch.cuda.synchronize()
            assert torch.equal(ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32), sec), "the call wrote into its input section"
            o = ws.t[ooff:ooff + out_bytes]
            a, b, c = pad(3 * ns), pad(3 * ns) + pad(nv), pad(3 * ns) + pad(nv) + pad(icap[2])
            seen.append((o[:12 * ns].view(torch.int32).cpu().clone(), o[a:a + 4 * nv].view(torch.float32).cpu().clone(),
                         o[b:b + 4 * icap[2]].view(torch.int32).cpu().clone(), o[c:c + 4 * icap[2]].view(torch.float32).cpu().clone()))
            return rc
        outs, reproducible = run_contract(lambda a: mc.with_precision(env, prec, call)(), ar)
        assert reproducible
        assert torch.equal(env.packed.flat, env.snapshot)
        assert all(all(torch.equal(x, y) for x, y in zip(s, seen[0])) for s in seen)   # (the output section does not depend on what the workspace held)
        assert bool(torch.isfinite(seen[0][1]).all()) and bool(torch.isfinite(seen[0][3]).all())
        return (outs["log_probs"].cpu(),) + seen[0]

    def streams(S_rows):
        """Sequences as streams of the unattached decoder -> log_probs [len, N, 33]."""
        dev, b = env.dev, len(S_rows)
        hV, hE, idx, msk, rank = (t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "mask", "rank"))
        Sd = torch.tensor(S_rows, dtype=torch.int32, device=dev)
        msk_b, rank_b = msk.repeat(b, 1).contiguous(), rank.repeat(b, 1).contiguous()
        lp = torch.zeros(b, N, 33, device=dev)
        ws = torch.zeros(env.L.namp_workspace_bytes(1, b, N, K), dtype=torch.uint8, device=dev)
        rc = mc.with_precision(env, prec, lambda: env.L.namp_decoder_fwd(
            env.packed.model(), hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), Sd.data_ptr(), msk_b.data_ptr(), rank_b.data_ptr(),
            lp.data_ptr(), None, None, ws.data_ptr(), ws.numel(), b, 1, N, K, env.s()))()
        torch.cuda.synchronize()
        assert rc == 0
        return lp.cpu()

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    S0 = t["S"][0].tolist()
    if N < 17:                                               # N = 1: the one residue; a residue out of range is that residue
        variants = [[0, 3], [0, 30], [0, 11]]
        got = run([[0]], variants)
        lp, sizes, delta, res, rlp = got
        assert sizes.tolist() == [1, 1, 1] and res.tolist() == [0, 0, 0]
        ref = streams([[v[1]] for v in variants] + [S0])
        want = torch.stack([ref[k, 0, variants[k][1]] for k in range(3)])
        assert float((rlp - want).abs().max()) < 2e-4
        assert float((delta - (want - ref[3, 0, S0[0]])).abs().max()) < 4e-4
        assert same(run([[7]], variants, plan_sites=[[0]]), got)
        assert same(run([[0]], [[5, 3], [-2, 30], [0, 11]]), got)                         # site indices: clamped
        assert same(run([[0]], [[0, -4], [0, 77], [0, 11]]), run([[0]], [[0, 0], [0, 32], [0, 11]]))
        return
    sites = [[2], [5, 9], [11, 3, 7, 0, 16, 1, 4, 8]]
    g = torch.Generator().manual_seed(5)
    variants = [[s] + torch.randint(0, 33, (len(sites[s]),), generator=g).tolist() for s in (0, 1, 1, 2, 0, 2)]
    got = run(sites, variants)
    lp, sizes, delta, res, rlp = got
    sizes = sizes.view(3, 3).tolist()
    full = [list(S0) for _ in variants]
    for k, v in enumerate(variants):
        for r, a in zip(sites[v[0]], v[1:]):
            full[k][r] = a
    ref = streams(full + [S0])
    offs = np.concatenate(([0], np.cumsum([sizes[v[0]][2] for v in variants])))
    assert len(res) == offs[-1] and int(res.min()) >= 0
    worst = 0.0
    for k in range(len(variants)):
        rows = res[offs[k]:offs[k + 1]].long()
        assert rows.tolist() == sorted(set(rows.tolist())) and set(sites[variants[k][0]]) <= set(rows.tolist())
        want = ref[k][rows, torch.tensor(full[k])[rows]]
        worst = max(worst, float((rlp[offs[k]:offs[k + 1]] - want).abs().max()))
        others = torch.ones(N, dtype=torch.bool); others[rows] = False                   # outside U_3 nothing differs from the base stream
        assert float((ref[k][others] - ref[-1][others]).abs().max()) < 2e-4 if bool(others.any()) else True
        base = ref[-1][rows, torch.tensor(S0)[rows]]
        d = float((torch.from_numpy(w)[rows] * (want - base)).sum())
        assert abs(float(delta[k]) - d) < 2e-4 * len(rows)
    d_base = float((lp[0] - ref[-1]).abs().max())
    print(f"mutations contract {shape} {prec}: max|d| vs the decoder's streams {worst:.3e}, base rows {d_base:.3e}; sizes {sizes}")
    assert worst < 2e-4 and d_base < 2e-4
    # residues out of range: the call with the clamped values (a negative word is no edit)
    bad_sites = [[2], [5, 99], [11, 3, 7, 0, 16, 1, 4, 8]]
    assert same(run(bad_sites, variants, plan_sites=[[2], [5, N - 1], sites[2]]), run([[2], [5, N - 1], sites[2]], variants))
    assert not same(run(bad_sites, variants, plan_sites=[[2], [5, N - 1], sites[2]]), got)
    v_short = [[v[0]] + (v[1:2] if v[0] == 1 else v[1:]) for v in variants]
    assert same(run([[2], [5, -1], sites[2]], variants, plan_sites=[[2], [5], sites[2]]), run([[2], [5], sites[2]], v_short))
    # site indices and tokens out of range: clamped
    bad = [list(v) for v in variants]; ok = [list(v) for v in variants]
    bad[0][0], bad[3][0], bad[1][1], bad[2][2], bad[5][8] = -3, 9, -4, 77, 33
    ok[0][0], ok[3][0], ok[1][1], ok[2][2], ok[5][8] = 0, 2, 0, 32, 32
    assert same(run(sites, bad), run(sites, ok))
    # duplicate edits: the last listed is the residue's
    dup_sites = [[2], [5, 9, 5], sites[2]]
    dup = [[v[0]] + (v[1:3] + [(v[1] + 7) % 33] if v[0] == 1 else v[1:]) for v in variants]
    und = [[v[0]] + ([v[2], (v[1] + 7) % 33] if v[0] == 1 else v[1:]) for v in variants]
    a, b = run(dup_sites, dup, plan_sites=[[2], [9, 5], sites[2]]), run([[2], [9, 5], sites[2]], und)
    assert same(a, b)
    # capacities below the counts: what lies beyond is dropped — defined, reproducible, in bounds
    lcap, icap = capacities(sizes, variants, len(sites))
    cut = run(sites, variants, caps=([max(1, c // 2) for c in lcap], [max(1, c // 2) for c in icap]))
    assert torch.equal(cut[0], lp) and cut[1].view(3, 3).tolist() == sizes
    cut2 = run(sites, variants, caps=([max(1, c // 2) for c in lcap], icap))
    assert int(cut2[3].min()) == -1 and torch.equal(cut2[0], lp)                      # (rows no variant owns: residue -1, entry 0)


def test_a_too_small_workspace_is_refused_and_clears_the_attachment(weights_np):
    """ws_bytes one byte short of namp_mutations_workspace_bytes: NAMP_EINVAL before any launch, and the attachment is gone — the
    NEXT plain namp_decoder_fwd call is the unattached one, bit for bit.  Bad arguments of namp_mutations attach nothing, a library
    and a scan attached together run neither, and the sizes are 0 where the route is not supported."""
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
    sites, variants = [[2], [5, 9]], [[0, 4], [1, 7, 8], [1, 1, 2]]
    sizes = plan_sizes(env, t, N, K, sites)
    lcap, icap = capacities(sizes, variants, 2)
    dims = (N, K, 3, 2, 3) + tuple(lcap) + tuple(icap)
    need = env.L.namp_mutations_workspace_bytes(*dims)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sec = section(sites, variants, np.ones(N))
    ioff = env.L.namp_mutations_in_offset(*dims)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    assert env.L.namp_mutations(*dims[3:]) == 0
    rc, lp = call(ws, need - 1)
    assert rc == -1 and b"workspace too small" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)                     # plain: the attachment was cleared by the refused call
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_mutations(*dims[3:]) == 0              # an attached call that succeeds clears it as well
    rc, lp = call(ws, need)
    assert rc == 0 and float((lp - lp_plain).abs().max()) < 2e-4
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_mutations(-1, *dims[4:]) == -1         # bad arguments attach nothing
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_mutations(*dims[3:]) == 0 and env.L.namp_library(1, 0, 0, 0, 0) == 0      # both attached: neither runs, both are gone
    rc, lp = call(ws, need)
    assert rc == -1 and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    # sizes are 0 where unsupported: another number of decoder layers, K > N, variants without a site, a negative capacity
    for bad in ((N, K, 4, 2, 3, 4, 4, 4, 4, 4, 4), (N, N + 1, 3, 2, 3, 4, 4, 4, 4, 4, 4), (N, K, 3, 0, 3, 4, 4, 4, 4, 4, 4),
                (N, K, 3, 2, 3, 4, 4, 4, 4, 4, -1)):
        assert env.L.namp_mutations_workspace_bytes(*bad) == 0 and env.L.namp_mutations_in_offset(*bad) == 0
        assert env.L.namp_mutations_out_offset(*bad) == 0
