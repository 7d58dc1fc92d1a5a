"""The memory contract of namp_decoder_fwd with a group scan attached (namp_group_mutations) under the guarded buffers
of tests/guarded.py, at (L, K) = (1, 1) and (17, 48): a correct call without groups against the unattached decoder's streams, and
malformed sections — successors out of range, no `first`, a tail that leads into a cycle, a masked member, tokens and site indices out
of range, capacities below the counts.  These are inputs the kernels are specified to clamp or to read as "not tied", with a defined
result: the result of the call with the clamped values (a group that does not validate: the call without it); the input section is
found unchanged, the outputs do not depend on what the workspace held, and nothing outside the declared buffers is touched."""
import numpy as np
import pytest
import torch

from test_gpu_score_mutations_contract import capacities, pad, section

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def no_groups(N):
    return np.full(N, -1, np.int32), np.zeros(N, np.int32), np.ones(N, np.float32)


def with_groups(N, groups, weights):
    nxt, first, wt = no_groups(N)
    for g, gw in zip(groups, weights):
        for q, r in enumerate(g):
            nxt[r], wt[r] = g[(q + 1) % len(g)], gw[q]
        first[g[0]] = 1
    return nxt, first, wt


def group_section(sites, variants, w, grp):
    nxt, first, wt = grp
    return torch.cat((section(sites, variants, w), torch.from_numpy(np.concatenate((nxt, first, wt.view(np.int32))))))


def attached_call(env, N, K, sites, variants, lcap, icap, ptrs, ws_ptr, ws_bytes, lp_ptr):
    assert env.L.namp_group_mutations(len(sites), len(variants), *lcap, *icap) == 0
    return env.L.namp_decoder_fwd(env.packed.model(), *ptrs, lp_ptr, None, None, ws_ptr, ws_bytes, 1, 1, N, K, env.s())


def plan_sizes(env, t, N, K, sites, w, grp):
    """|U_1..3(site)| of every site: one attached call with no variants, read back."""
    dev = env.dev
    dims = (N, K, 3, len(sites), 0, 0, 0, 0, 0, 0, 0)
    need, ioff, ooff = (getattr(env.L, "namp_group_mutations" + f)(*dims) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
    sec = group_section(sites, [], w, grp)
    assert need > 0 and ioff % 256 == 0 and ooff % 256 == 0 and ioff + 4 * sec.numel() <= ooff
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    dv = [t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank")]
    lp = torch.zeros(1, N, 33, device=dev)
    rc = attached_call(env, N, K, sites, [], (0, 0, 0), (0, 0, 0), [x.data_ptr() for x in dv], ws.data_ptr(), need, lp.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return ws[ooff:ooff + 12 * len(sites)].view(torch.int32).view(len(sites), 3).tolist()


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_group_scan_under_guarded_buffers(weights_np, shape, prec):
    """Measured (MI355X): see the printed line (entries, units and deltas of the call without groups against the unattached decoder's
    streams, 2e-4 and 2e-4 x rows: two summation orders of one model)."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t0 = mc.graph_case(B, N, K)
    K = t0["K"]
    w = (np.arange(N) % 3 != 0).astype(np.float32) if N > 1 else np.ones(1, np.float32)

    def run(sites, variants, grp, caps=None, plan_sites=None, t=t0):
        sizes = plan_sizes(env, t, N, K, sites if plan_sites is None else plan_sites, w, grp)
        lcap, icap = capacities(sizes, variants, len(sites)) if caps is None else caps
        ns, nv = len(sites), len(variants)
        dims = (N, K, 3, ns, nv) + tuple(lcap) + tuple(icap)
        need, ioff, ooff = (getattr(env.L, "namp_group_mutations" + f)(*dims) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
        sec = group_section(sites, variants, w, grp).to(env.dev)
        parts = [(3 * ns, torch.int32), (nv, torch.float32), (icap[2], torch.int32), (icap[2], torch.float32), (icap[2], torch.int32),
                 (icap[2], torch.float32), (N, torch.float32), (63, torch.int32)]
        assert need > 0 and ioff + 4 * sec.numel() <= ooff and ooff + sum(pad(e) for e, _ in parts) == need
        ar = Arena(env.dev)
        bufs = [ar.inp(name, t[k]) for name, k in (("h_V_enc", "V"), ("h_E", "E"), ("E_idx", "E_idx"), ("S", "S"), ("mask", "mask"),
                                                   ("rank", "rank"))]
        lp = ar.out("log_probs", mc.f32, (1, N, mc.V33))
        ws = ar.ws("ws", need)
        seen = []

        def call():
            ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
            rc = attached_call(env, N, K, sites, variants, lcap, icap, [x.ptr for x in bufs], ws.ptr, ws.nbytes, lp.ptr)
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
        """Sequences as streams of the unattached decoder -> log_probs [len, N, 33]."""
        dev, b = env.dev, len(S_rows)
        hV, hE, idx, msk, rank = (t0[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "mask", "rank"))
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

    S0 = t0["S"][0].tolist()
    unmasked = t0["mask"][0] != 0

    def check(sites, variants, got):
        """The call WITHOUT groups against the same variants as streams of the unattached decoder: every unit is an own entry."""
        lp, sizes, delta, res, rlp, ures, ulp, bunit, header = got
        sizes = sizes.view(len(sites), 3).tolist()
        assert header[:2].tolist() == [0, 0]
        full = [list(S0) for _ in variants]
        for k, v in enumerate(variants):
            for r, a in zip(sites[v[0]], v[1:]):
                full[k][r] = a
        ref = streams(full + [S0])
        own0 = ref[-1][torch.arange(N), torch.tensor(S0)]
        offs = np.concatenate(([0], np.cumsum([sizes[v[0]][2] for v in variants])))
        assert len(res) == offs[-1] and int(res.min()) >= 0
        worst_e = worst_d = 0.0
        for k, v in enumerate(variants):
            rows = res[offs[k]:offs[k + 1]].long()
            assert rows.tolist() == sorted(set(rows.tolist())) and set(sites[v[0]]) <= set(rows.tolist())
            want = ref[k][rows, torch.tensor(full[k])[rows]]
            worst_e = max(worst_e, float((rlp[offs[k]:offs[k + 1]] - want).abs().max()))
            lead = ures[offs[k]:offs[k + 1]]
            assert torch.equal(lead[lead >= 0].long(), rows[unmasked[rows]]) and torch.equal(lead < 0, ~unmasked[rows])
            assert torch.equal(ulp[offs[k]:offs[k + 1]][lead >= 0], rlp[offs[k]:offs[k + 1]][lead >= 0])
            wt = torch.from_numpy(w)[rows] * unmasked[rows]
            worst_d = max(worst_d, abs(float(delta[k]) - float((wt * (want - own0[rows])).sum())) / len(rows))
        d_base = max(float((lp[0] - ref[-1])[unmasked].abs().max()), float((bunit - own0)[unmasked].abs().max()))
        print(f"group scan contract {shape} {prec}: entries vs the decoder's streams {worst_e:.3e}, deltas / rows {worst_d:.3e}, "
              f"base rows and units {d_base:.3e}; sizes {sizes}")
        assert worst_e < 2e-4 and worst_d < 2e-4 and d_base < 2e-4

    none = no_groups(N)
    if N == 1:                                                   # the one residue; a residue out of range is that residue
        variants = [[0, 3], [0, 30], [0, 11]]
        got = run([[0]], variants, none)
        assert got[1].tolist() == [1, 1, 1] and got[3].tolist() == [0, 0, 0] and got[5].tolist() == [0, 0, 0]
        check([[0]], variants, got)
        assert same(run([[7]], variants, none, plan_sites=[[0]]), got)
        assert same(run([[0]], [[5, 3], [-2, 30], [0, 11]], none), got)                    # site indices: clamped
        assert same(run([[0]], [[0, -4], [0, 77], [0, 11]], none), run([[0]], [[0, 0], [0, 32], [0, 11]], none))
        # a self-loop with `first`, a successor out of range: no group
        assert same(run([[0]], variants, (np.array([0], np.int32), np.array([1], np.int32), np.array([0.5], np.float32))), got)
        assert same(run([[0]], variants, (np.array([9], np.int32), np.array([1], np.int32), np.array([0.5], np.float32))), got)
        return
    um = [int(i) for i in np.nonzero(unmasked.numpy())[0]]
    g1, g2 = [um[1], um[5], um[8]], [um[10], um[3]]                  # (listed order is not index order)
    x, y = um[6], um[0]
    sites = [g1, g2 + [x], [y]]
    g = torch.Generator().manual_seed(5)
    variants = []
    for s in (0, 1, 1, 2, 0, 2):
        a, b = torch.randint(0, 33, (2,), generator=g).tolist()
        variants.append([s] + ([a] * 3 if s == 0 else [a, a, b] if s == 1 else [a]))
    got0 = run(sites, variants, none)
    check(sites, variants, got0)
    both = with_groups(N, [g1, g2], [[1.0, 0.5, 0.25], [1.0, 1.0]])
    only1, only2 = with_groups(N, [g1], [[1.0, 0.5, 0.25]]), with_groups(N, [g2], [[1.0, 1.0]])
    got = run(sites, variants, both)
    assert got[8][0].item() == 5 and got[8][1].item() > 0 and not same(got, got0)          # (K = N: the members are neighbours)
    lead = got[5]
    assert sorted(set(lead[lead >= 0].tolist())) == sorted(set(r if r not in g1 + g2 else (g1[0] if r in g1 else g2[0])
                                                              for r in got[3].tolist() if unmasked[r]))

    def edited(grp, **at):
        nxt, first, wt = (a.copy() for a in grp)
        for r, v in at.get("next", {}).items():
            nxt[r] = v
        for r, v in at.get("first", {}).items():
            first[r] = v
        return nxt, first, wt
    # a successor out of range: the group does not validate, its residues are units of one
    assert same(run(sites, variants, edited(both, next={g2[1]: 99})), run(sites, variants, only1))
    assert same(run(sites, variants, edited(both, next={g2[0]: -5})), run(sites, variants, only1))
    # no `first`, two of them
    assert same(run(sites, variants, edited(both, first={g1[0]: 0})), run(sites, variants, only2))
    assert same(run(sites, variants, edited(both, first={g1[2]: 1})), run(sites, variants, only2))
    # a tail that leads into a cycle: the tail is ungrouped, the cycle stands
    assert same(run(sites, variants, edited(both, next={x: g2[0]})), got)
    # a masked member: the group is not tied
    t1 = dict(t0, mask=t0["mask"].clone())
    t1["mask"][0, g1[1]] = 0
    assert same(run(sites, variants, both, t=t1), run(sites, variants, only2, t=t1))
    # site indices and tokens out of range: clamped
    bad = [list(v) for v in variants]; ok = [list(v) for v in variants]
    bad[0][0], bad[3][0], bad[1][1], bad[2][2] = -3, 9, -4, 77
    ok[0][0], ok[3][0], ok[1][1], ok[2][2] = 0, 2, 0, 32
    assert same(run(sites, bad, both), run(sites, ok, both))
    # residues out of range: the call with the clamped values
    bad_sites, ok_sites = [g1, g2 + [99], [y]], [g1, g2 + [N - 1], [y]]
    assert same(run(bad_sites, variants, both, plan_sites=ok_sites), run(ok_sites, variants, both))
    # capacities below the counts: a defined, reproducible result inside the declared buffers
    sizes = plan_sizes(env, t0, N, K, sites, w, both)
    lcap, icap = capacities(sizes, variants, len(sites))
    for caps in (([c // 2 for c in lcap], icap), (lcap, [c // 2 for c in icap]), ([1, 1, 1], [1, 1, 1]), (lcap, [icap[0], 3, icap[2] - 1])):
        cut = run(sites, variants, both, caps=caps)
        assert same(cut, run(sites, variants, both, caps=caps)) and torch.equal(cut[7], got[7])      # (the base units do not depend on them)


def test_a_too_small_workspace_is_refused_and_a_double_attachment_runs_neither(weights_np):
    """ws_bytes one byte short of namp_group_mutations_workspace_bytes: NAMP_EINVAL before any launch, and the attachment is gone — the
    NEXT plain namp_decoder_fwd call is the unattached one, bit for bit.  Attached together with another kind (a tied score) neither
    runs; the group scan shares the attach kind of namp_mutations, so of those two the later call holds."""
    import test_gpu_memory_contract as mc
    env = mc.Env(weights_np)
    N = 17
    t = mc.graph_case(1, N, 16)
    K, dev = t["K"], env.dev
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
    w, grp = np.ones(N, np.float32), no_groups(N)
    sites, variants = [[2], [5]], [[0, 4], [1, 7], [1, 1]]
    sizes = plan_sizes(env, t, N, K, sites, w, grp)
    lcap, icap = capacities(sizes, variants, 2)
    dims = (N, K, 3, 2, 3) + tuple(lcap) + tuple(icap)
    need = env.L.namp_group_mutations_workspace_bytes(*dims)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sec = group_section(sites, variants, w, grp)
    ioff = env.L.namp_group_mutations_in_offset(*dims)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    attach = lambda: env.L.namp_group_mutations(*dims[3:])
    unmasked = t["mask"][0] != 0
    assert attach() == 0
    rc, lp = call(ws, need - 1)
    assert rc == -1 and b"workspace too small for a group scan" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)                     # plain: the attachment was cleared by the refused call
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert attach() == 0                                     # an attached call that succeeds clears it as well
    rc, lp_group = call(ws, need)
    assert rc == 0 and float((lp_group - lp_plain)[0][unmasked].abs().max()) < 2e-4
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert attach() == 0 and env.L.namp_tied_score(1, mc.V33, 0) == 0   # two kinds attached: neither runs, both are gone
    rc, lp = call(ws, need)
    assert rc == -1 and b"attached together" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_mutations(*dims[3:]) == 0 and attach() == 0       # the kind of namp_mutations is shared: the later call holds
    rc, lp = call(ws, need)
    assert rc == 0 and torch.equal(lp, lp_group)             # (the base rows of the group scan's item pass)
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
