"""The memory contract of namp_decoder_fwd with a specificity scan attached (namp_state_mutations) under the guarded
buffers of tests/guarded.py, at (M, L, K) = (1, 1, 1) and (2, 17, 48): a correct call, and malformed sections — residues and site indices
out of range, tokens out of range, a repeated copy.  These are inputs the kernels are specified to clamp, with a defined result: the
result of the call with the clamped values; the input section is found unchanged, the outputs do not depend on what the workspace held,
and nothing outside the declared buffers is touched."""
import numpy as np
import pytest
import torch

from test_gpu_score_mutations_contract import capacities, pad, section

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def flat_case(mc, M, L, K):
    """M synthetic graphs of L residues as ONE complex of M * L: block-diagonal E_idx, state 0's rank repeated per block; the states
    after the first have a masked tail of their own length (absent copies)."""
    t = mc.graph_case(M, L, K)
    K = t["K"]
    N = M * L
    shift = (torch.arange(M, dtype=torch.int32) * L)[:, None, None]
    flat = {"V": t["V"].reshape(1, N, -1), "E": t["E"].reshape(1, N, K, -1), "E_idx": (t["E_idx"] + shift).reshape(1, N, K).contiguous(),
            "S": t["S"][:1].repeat(1, M).contiguous(), "mask": t["mask"].reshape(1, N), "rank": t["rank"][:1].repeat(1, M).contiguous(), "K": K}
    counted = (np.arange(L) % 3 != 0) if L > 1 else np.ones(1, bool)
    present = t["mask"].numpy().reshape(M, L) != 0
    flat["w"] = (counted[None] & present).reshape(N).astype(np.float32)
    sw = np.array([1.0, -0.5, 0.75, 0.25][:M], np.float32)
    flat["unit_w"] = (sw[:, None] * present).reshape(N).astype(np.float32)
    return flat


def state_section(sites, variants, t):
    return torch.cat((section(sites, variants, t["w"]), torch.from_numpy(t["unit_w"].view(np.int32))))


def attached_call(env, t, M, L, sites, variants, lcap, icap, ptrs, ws_ptr, ws_bytes, lp_ptr):
    N, K = M * L, t["K"]
    assert env.L.namp_state_mutations(M, L, len(sites), len(variants), *lcap, *icap) == 0
    return env.L.namp_decoder_fwd(env.packed.model(), *ptrs, lp_ptr, None, None, ws_ptr, ws_bytes, 1, 1, N, K, env.s())


def plan_sizes(env, t, M, L, sites):
    """|U_1..3(site)| of every site: one attached call with no variants, read back."""
    N, K, dev = M * L, t["K"], env.dev
    dims = (N, K, 3, M, len(sites), 0, 0, 0, 0, 0, 0, 0)
    need, ioff, ooff = (getattr(env.L, "namp_state_mutations" + f)(*dims) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
    sec = state_section(sites, [], t)
    assert need > 0 and ioff + 4 * sec.numel() <= ooff
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    dv = [t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank")]
    lp = torch.zeros(1, N, 33, device=dev)
    rc = attached_call(env, t, M, L, sites, [], (0, 0, 0), (0, 0, 0), [x.data_ptr() for x in dv], ws.data_ptr(), need, lp.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return ws[ooff:ooff + 12 * len(sites)].view(torch.int32).view(len(sites), 3).tolist()


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 17, 48)])
def test_state_scan_under_guarded_buffers(weights_np, shape, prec):
    """Measured (MI355X) at (2, 17, 48): see the printed line (deltas and units against the unattached decoder's streams, 2e-4 x rows
    and 2e-4: two summation orders of one model)."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    M, L, K = shape
    t = flat_case(mc, M, L, K)
    N, K = M * L, t["K"]

    def run(sites, variants, plan_sites=None):
        sizes = plan_sizes(env, t, M, L, sites if plan_sites is None else plan_sites)
        lcap, icap = capacities(sizes, variants, len(sites))
        ns, nv = len(sites), len(variants)
        dims = (N, K, 3, M, ns, nv) + tuple(lcap) + tuple(icap)
        need, ioff, ooff = (getattr(env.L, "namp_state_mutations" + f)(*dims) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
        sec = state_section(sites, variants, t).to(env.dev)
        parts = [(3 * ns, torch.int32), (nv, torch.float32), (nv * M, torch.float32), (icap[2], torch.int32), (icap[2], torch.float32),
                 (icap[2], torch.int32), (icap[2], torch.float32), (L, torch.float32)]
        out_bytes = sum(pad(e) for e, _ in parts)
        assert need > 0 and ioff + 4 * sec.numel() <= ooff and ooff + out_bytes == need
        ar = Arena(env.dev)
        bufs = [ar.inp(name, t[k]) for name, k in (("h_V_enc", "V"), ("h_E", "E"), ("E_idx", "E_idx"), ("S", "S"), ("mask", "mask"),
                                                   ("rank", "rank"))]
        lp = ar.out("log_probs", mc.f32, (1, N, mc.V33))
        ws = ar.ws("ws", need)
        seen = []

        def call():
            ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
            rc = attached_call(env, t, M, L, sites, variants, lcap, icap, [x.ptr for x in bufs], ws.ptr, ws.nbytes, lp.ptr)
            torch.cuda.synchronize()
            assert torch.equal(ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32), sec), "the call wrote into its input section"
            got, o = [], ooff
            for elems, dt in parts:
                got.append(ws.t[o:o + 4 * elems].view(dt).cpu().clone())
                o += pad(elems)
            seen.append(got)
            return rc
        outs, reproducible = run_contract(lambda a: mc.with_precision(env, prec, call)(), ar)
        assert reproducible
        assert torch.equal(env.packed.flat, env.snapshot)
        assert all(all(torch.equal(x, y) for x, y in zip(s, seen[0])) for s in seen)   # (the output section does not depend on what the workspace held)
        assert all(bool(torch.isfinite(x).all()) for x in seen[0] if x.dtype == torch.float32)
        return [outs["log_probs"].cpu()] + seen[0]

    def streams(S_rows):
        """Sequences as streams of the unattached decoder on the flat graph -> log_probs [len, N, 33]."""
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
    present = (t["mask"][0] != 0).view(M, L)
    w, uw = torch.from_numpy(t["w"]).view(M, L), torch.from_numpy(t["unit_w"]).view(M, L)

    def units_of(rows, S_row):
        """rows [N, 33] of one stream, its tokens -> unit [L] at the first present copy's token (none present: copy 0 alone)."""
        rows, tok = rows.view(M, L, 33), torch.tensor(S_row).view(M, L)
        solo = ~present.any(0)
        wt = torch.where(solo[None], (torch.arange(M) == 0).float()[:, None].expand(M, L), uw * present)
        z = (wt[:, :, None] * rows).sum(0)
        seat = present.float().argmax(0)
        return torch.log_softmax(z, -1).gather(1, tok.gather(0, seat[None])[0][:, None])[:, 0]

    def check(sites, variants, got):
        """The call against the same variants as streams of the unattached decoder."""
        lp, sizes, delta, sdelta, res, rlp, ures, ulp, bunit = got
        sizes = sizes.view(len(sites), 3).tolist()
        full = [list(S0) for _ in variants]
        for k, v in enumerate(variants):
            for r, a in zip(sites[v[0]], v[1:]):
                full[k][r] = a
        ref = streams(full + [S0])
        base_units = units_of(ref[-1], S0)
        offs = np.concatenate(([0], np.cumsum([sizes[v[0]][2] for v in variants])))
        assert len(res) == offs[-1] and int(res.min()) >= 0
        worst_e = worst_d = 0.0
        for k, v in enumerate(variants):
            rows = res[offs[k]:offs[k + 1]].long()
            assert rows.tolist() == sorted(set(rows.tolist())) and set(sites[v[0]]) <= set(rows.tolist())
            want = ref[k][rows, torch.tensor(full[k])[rows]]
            worst_e = max(worst_e, float((rlp[offs[k]:offs[k + 1]] - want).abs().max()))
            units = units_of(ref[k], full[k])
            counted = (w.sum(0) != 0).float()
            worst_d = max(worst_d, abs(float(delta[k]) - float((counted * (units - base_units)).sum())) / len(rows))
            own = ref[k].view(M, L, 33).gather(2, torch.tensor(full[k]).view(M, L, 1))[..., 0]
            own0 = ref[-1].view(M, L, 33).gather(2, torch.tensor(S0).view(M, L, 1))[..., 0]
            worst_d = max(worst_d, float(((w * (own - own0)).sum(1) - sdelta.view(len(variants), M)[k]).abs().max()) / len(rows))
            lead = ures[offs[k]:offs[k + 1]]
            led = lead[lead >= 0].long()
            assert sorted(led.tolist()) == sorted({int(r) % L for r in rows.tolist() if present.view(N)[r]})
            worst_e = max(worst_e, float((ulp[offs[k]:offs[k + 1]][lead >= 0] - units[led]).abs().max()))
        d_base = max(float((lp[0] - ref[-1]).abs().max()), float((bunit - base_units).abs().max()))
        print(f"state scan contract {shape} {prec}: entries and units vs the decoder's streams {worst_e:.3e}, deltas / rows {worst_d:.3e}, "
              f"base rows and units {d_base:.3e}; sizes {sizes}")
        assert worst_e < 2e-4 and worst_d < 2e-4 and d_base < 2e-4

    if N == 1:                                                   # the one residue in the one state; a residue out of range is that residue
        variants = [[0, 3], [0, 30], [0, 11]]
        got = run([[0]], variants)
        assert got[1].tolist() == [1, 1, 1] and got[4].tolist() == [0, 0, 0] and got[6].tolist() == [0, 0, 0]
        check([[0]], variants, got)
        assert same(run([[7]], variants, plan_sites=[[0]]), got)
        assert same(run([[0]], [[5, 3], [-2, 30], [0, 11]]), got)                         # site indices: clamped
        assert same(run([[0]], [[0, -4], [0, 77], [0, 11]]), run([[0]], [[0, 0], [0, 32], [0, 11]]))
        return
    # sites of the copies of shared residues 2 | 5 and 9 | 14, 15, 16 (16 and 15 are absent in state 1) and 0
    sites = [[2, L + 2], [5, L + 5, 9, L + 9], [14, L + 14, 15, L + 15, 16, L + 16, 0, L + 0]]
    assert not present[1, 16] and not present[1, 15] and present[0, 16]
    g = torch.Generator().manual_seed(5)
    variants = []
    for s in (0, 1, 1, 2, 0, 2):
        tok = torch.randint(0, 33, (len(sites[s]) // 2,), generator=g).tolist()
        variants.append([s] + [a for a in tok for _ in range(2)])                         # (both copies of a residue hold its token)
    got = run(sites, variants)
    check(sites, variants, got)
    # residues out of range: the call with the clamped values (a negative word is no edit)
    bad_sites = [sites[0], [5, L + 5, 9, 99], sites[2]]
    ok_sites = [sites[0], [5, L + 5, 9, N - 1], sites[2]]
    assert same(run(bad_sites, variants, plan_sites=ok_sites), run(ok_sites, variants))
    assert not same(run(bad_sites, variants, plan_sites=ok_sites), got)
    # site indices and tokens out of range: clamped
    bad = [list(v) for v in variants]; ok = [list(v) for v in variants]
    bad[0][0], bad[3][0], bad[1][1], bad[2][2], bad[5][8] = -3, 9, -4, 77, 33
    ok[0][0], ok[3][0], ok[1][1], ok[2][2], ok[5][8] = 0, 2, 0, 32, 32
    assert same(run(sites, bad), run(sites, ok))
    # a repeated copy: the last listed is the residue's
    dup_sites = [sites[0], [5, L + 5, 9, L + 9, 5], sites[2]]
    dup = [v + [(v[1] + 7) % 33] if v[0] == 1 else v for v in variants]
    und_sites = [sites[0], [L + 5, 9, L + 9, 5], sites[2]]
    und = [[v[0], v[2], v[3], v[4], (v[1] + 7) % 33] if v[0] == 1 else v for v in variants]
    assert same(run(dup_sites, dup, plan_sites=und_sites), run(und_sites, und))


def test_a_too_small_workspace_is_refused_and_a_double_attachment_runs_neither(weights_np):
    """ws_bytes one byte short of namp_state_mutations_workspace_bytes: NAMP_EINVAL before any launch, and the attachment is gone — the
    NEXT plain namp_decoder_fwd call is the unattached one, bit for bit.  Attached together with namp_mutations neither runs; a call
    whose N is not n_states * L is refused."""
    import test_gpu_memory_contract as mc
    env = mc.Env(weights_np)
    M, L = 2, 17
    t = flat_case(mc, M, L, 16)
    N, K, dev = M * L, t["K"], env.dev
    dv = [t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank")]
    ptrs = [x.data_ptr() for x in dv]

    def call(ws, nbytes):
        lp = torch.zeros(1, N, mc.V33, device=dev)
        rc = env.L.namp_decoder_fwd(env.packed.model(), *ptrs, lp.data_ptr(), None, None, ws.data_ptr(), nbytes, 1, 1, N, K, env.s())
        torch.cuda.synchronize()
        return rc, lp.cpu()
    plain_bytes = env.L.namp_workspace_bytes(1, 1, N, K)
    plain_ws = torch.zeros(plain_bytes, dtype=torch.uint8, device=dev)
    rc, lp_plain = call(plain_ws, plain_bytes)
    assert rc == 0 and float(lp_plain.abs().max()) > 0
    sites, variants = [[2, L + 2], [5, L + 5]], [[0, 4, 4], [1, 7, 7], [1, 1, 1]]
    sizes = plan_sizes(env, t, M, L, sites)
    lcap, icap = capacities(sizes, variants, 2)
    dims = (N, K, 3, M, 2, 3) + tuple(lcap) + tuple(icap)
    need = env.L.namp_state_mutations_workspace_bytes(*dims)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sec = state_section(sites, variants, t)
    ioff = env.L.namp_state_mutations_in_offset(*dims)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    attach = lambda: env.L.namp_state_mutations(M, L, *dims[4:])
    assert attach() == 0
    rc, lp = call(ws, need - 1)
    assert rc == -1 and b"workspace too small" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)                     # plain: the attachment was cleared by the refused call
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert attach() == 0                                     # an attached call that succeeds clears it as well
    rc, lp = call(ws, need)
    assert rc == 0 and float((lp - lp_plain).abs().max()) < 2e-4
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert attach() == 0 and env.L.namp_mutations(*dims[4:]) == 0       # both kinds attached: neither runs, both are gone
    rc, lp = call(ws, need)
    assert rc == -1 and b"attached together" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_state_mutations(M, L + 1, *dims[4:]) == 0         # N != n_states * L: refused by the carrier, nothing launched
    rc, lp = call(ws, need)
    assert rc == -1 and b"bad dims" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
