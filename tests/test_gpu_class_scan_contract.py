"""The memory contract of namp_decoder_fwd with a class scan attached (namp_class_mutations) under the guarded buffers
of tests/guarded.py, at (B, L, K) = (1, 2, 2) — one pair whose members are each other's only neighbour — and (1, 17, 48): a well-formed
section (identity tables and a zero bias: the bits of namp_group_mutations; a wobble pair beside a mapped group: the wild type has delta
0), and malformed sections — table indices and entries out of range, negative entries, a cycle that does not close, capacities smaller
than the plan.  These are inputs the kernels are specified to clamp or to read as "absent" / "not tied", with a defined result: that of
the call with the clamped values; the input section is found unchanged, the outputs do not depend on what the workspace held, and
nothing outside the declared buffers is touched."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import spec
from test_gpu_score_mutations_contract import capacities, pad, section
from test_gpu_group_scan_contract import group_section, with_groups

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

RTI = spec.restype_to_int()
IDENT = list(range(33)) + [-1] * 31
G, C, A, U = RTI["G"], RTI["C"], RTI["A"], RTI["U"]


def class_section(sites, variants, w, grp, table_idx, tables, bias):
    nxt, first, wt = grp
    words = np.concatenate((nxt, first, np.asarray(table_idx, np.int32), wt.view(np.int32), np.asarray(tables, np.int32).reshape(-1),
                            np.asarray(bias, np.float32).reshape(-1).view(np.int32)))
    return torch.cat((section(sites, variants, w), torch.from_numpy(words)))


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 2, 2), (1, 17, 48)])
def test_class_scan_under_guarded_buffers(weights_np, shape, prec):
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t0 = mc.graph_case(B, N, K)
    K = t0["K"]
    w = (np.arange(N) % 3 != 0).astype(np.float32) if N > 2 else np.ones(N, np.float32)

    def run(sites, variants, grp, cls=None, caps=None, t=t0, n_classes=35):
        """cls: None — namp_group_mutations; else (table_idx, tables, bias) — namp_class_mutations.  The plan call first (no variants),
        then the call under guarded buffers -> [log_probs, the arrays of the output section]."""
        fam = "namp_group_mutations" if cls is None else "namp_class_mutations"
        head = () if cls is None else (len(cls[1]), n_classes)
        make = (lambda v: group_section(sites, v, w, grp)) if cls is None else (lambda v: class_section(sites, v, w, grp, *cls))
        sizes_of = lambda tail: tuple(getattr(env.L, fam + f)(N, K, 3, *head, *tail) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))

        def attached(tail, ptrs, ws_ptr, ws_bytes, lp_ptr):
            assert getattr(env.L, fam)(*head, *tail) == 0
            return env.L.namp_decoder_fwd(env.packed.model(), *ptrs, lp_ptr, None, None, ws_ptr, ws_bytes, 1, 1, N, K, env.s())
        ns, nv = len(sites), len(variants)
        # ---- the sizes
        tail = (ns, 0, 0, 0, 0, 0, 0, 0)
        need, ioff, ooff = sizes_of(tail)
        sec = make([])
        assert need > 0 and ioff % 256 == 0 and ooff % 256 == 0 and ioff + 4 * sec.numel() <= ooff
        ws0 = torch.zeros(need, dtype=torch.uint8, device=env.dev)
        ws0[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
        dv = [t[k].to(env.dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank")]
        lp0 = torch.zeros(1, N, 33, device=env.dev)
        rc = mc.with_precision(env, prec, lambda: attached(tail, [x.data_ptr() for x in dv], ws0.data_ptr(), need, lp0.data_ptr()))()
        torch.cuda.synchronize()
        assert rc == 0
        sizes = ws0[ooff:ooff + 12 * ns].view(torch.int32).view(ns, 3).tolist()
        lcap, icap = capacities(sizes, variants, ns) if caps is None else caps(*capacities(sizes, variants, ns))
        # ---- the call
        tail = (ns, nv) + tuple(lcap) + tuple(icap)
        need, ioff, ooff = sizes_of(tail)
        sec = make(variants).to(env.dev)
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
            rc = attached(tail, [x.ptr for x in bufs], ws.ptr, ws.nbytes, lp.ptr)
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
        assert all(same(s, seen[0]) for s in seen)                 # (the output section does not depend on what the workspace held)
        return [outs["log_probs"].cpu()] + seen[0]

    first_t, second_t = spec.class_table(RTI, "rna-rna", True, True), spec.class_table(RTI, "rna-rna", True, False)
    wob_bias = [0.0] * 64
    wob_bias[spec.CLASS_GU] = wob_bias[spec.CLASS_UG] = 0.75
    tables, bias = [IDENT, first_t, second_t], [[0.0] * 64, wob_bias, wob_bias]
    ident3 = [IDENT] * 3, [[0.0] * 64] * 3
    if N == 2:
        t1 = dict(t0, S=torch.tensor([[G, C]], dtype=t0["S"].dtype))
        pair = with_groups(N, [[0, 1]], [[1.0, 0.5]])
        sites = [[0, 1]]
        variants = [[0, G, C], [0, G, U], [0, U, G], [0, A, U], [0, C, G]]
        # identity tables and a zero bias: the bits of the group scan (tokens that are one group token)
        same_tok = [[0, 3, 3], [0, 30, 30], [0, int(t0["S"][0, 0]), int(t0["S"][0, 0])]]
        t2 = dict(t0, S=t0["S"][:, :1].repeat(1, 2))
        assert same(run(sites, same_tok, pair, cls=([0, 0], [IDENT], [[0.0] * 64]), t=t2), run(sites, same_tok, pair, t=t2))
        assert same(run(sites, same_tok, pair, cls=([2, 1], *ident3), t=t2), run(sites, same_tok, pair, t=t2))
        got = run(sites, variants, pair, cls=([1, 2], tables, bias), t=t1)
        lp, sizes, delta, res, rlp, ures, ulp, bunit, header = got
        assert sizes.tolist() == [2, 2, 2] and header[0].item() == 2 and header[1].item() >= 1 and res.tolist() == [0, 1] * 5
        assert ures.tolist() == [0, -1] * 5 and bool(torch.isfinite(delta).all()) and bool(torch.isfinite(bunit).all())
        assert abs(float(delta[0])) < 2e-4 and float(bunit[0]) == float(bunit[1]) and float(ulp[0]) < 0
        # without the bias the wobble classes lose weight: the units of the wobble variants fall, by less than the bias
        nob = run(sites, variants, pair, cls=([1, 2], tables, [[0.0] * 64] * 3), t=t1)
        assert 0 < float(ulp[2] - nob[6][2]) < 0.75 and 0 < float(ulp[4] - nob[6][4]) < 0.75 and float(ulp[0]) < float(nob[6][0])
        # a table index out of range is the clamped one; an entry out of range the clamped token; any negative entry is "absent"
        assert same(run(sites, variants, pair, cls=([1, 77], tables, bias), t=t1), got)
        assert same(run(sites, variants, pair, cls=([-3, 2], tables, bias), t=t1), run(sites, variants, pair, cls=([0, 2], tables, bias), t=t1))
        hi, cl = [list(r) for r in tables], [list(r) for r in tables]
        hi[2][A], cl[2][A] = 99, 32
        hi[1][3], cl[1][3] = -7, -1
        assert same(run(sites, variants, pair, cls=([1, 2], hi, bias), t=t1), run(sites, variants, pair, cls=([1, 2], cl, bias), t=t1))
        # a cycle that does not close: units of one, the same for every table
        open_ = (np.array([1, 9], np.int32), pair[1], pair[2])
        solo = run(sites, variants, open_, cls=([1, 2], tables, bias), t=t1)
        assert same(solo, run(sites, variants, open_, cls=([0, 0], [IDENT], [[0.0] * 64]), t=t1)) and solo[8][:2].tolist() == [0, 0]
        assert solo[5].tolist() == [0, 1] * 5
        # n_classes = the vocabulary: the wobble lanes are no classes, a wobble variant breaks the tie (-inf), the others are defined
        low = run(sites, variants, pair, cls=([1, 2], tables, bias), t=t1, n_classes=33)
        assert float(low[6][2]) == float("-inf") and bool(torch.isfinite(low[6][[0, 6, 8]]).all())
        # capacities below the plan: a defined, reproducible result inside the declared buffers
        for caps in ((lambda lc, ic: ([1, 1, 1], ic)), (lambda lc, ic: (lc, [3, 3, 3])), (lambda lc, ic: ([1, 1, 1], [1, 1, 1]))):
            cut = run(sites, variants, pair, cls=([1, 2], tables, bias), t=t1, caps=caps)
            assert same(cut, run(sites, variants, pair, cls=([1, 2], tables, bias), t=t1, caps=caps)) and torch.equal(bits(cut[7]), bits(got[7]))
        return
    unmasked = t0["mask"][0] != 0
    um = [int(i) for i in np.nonzero(unmasked.numpy())[0]]
    g1, p1, p2 = [um[1], um[5], um[8]], [um[10], um[3]], [um[2], um[7]]      # (listed order is not index order)
    x, y = um[6], um[0]
    S1 = t0["S"].clone()
    S1[0, g1] = 4
    S1[0, p1[0]], S1[0, p1[1]], S1[0, p2[0]], S1[0, p2[1]] = G, U, A, U
    t1 = dict(t0, S=S1)
    grp = with_groups(N, [g1, p1, p2], [[1.0, 0.5, 0.25], [1.0, 1.0], [0.5, 1.0]])
    tidx = np.zeros(N, np.int32)
    tidx[[p1[0], p2[0]]], tidx[[p1[1], p2[1]]] = 1, 2
    sites = [g1, p1 + [x], [y], p1 + p2 + g1]
    variants = [[0, 7, 7, 7], [0, 4, 4, 4], [1, G, U, 5], [1, G, C, 5], [1, C, G, 9], [2, 3], [3, U, G, G, C, 2, 2, 2], [3, G, U, A, U, 4, 4, 4]]
    # identity tables, zero bias, the same groups: the bits of namp_group_mutations (a group token per unit)
    S2 = t0["S"].clone()
    for g in (g1, p1, p2):
        S2[0, g] = int(S2[0, g[0]])
    t2 = dict(t0, S=S2)
    wild = [3] + [int(S2[0, r]) for r in sites[3]]
    ident_variants = [[0, 7, 7, 7], [1, 3, 3, 5], [2, 3], [3, 30, 30, 1, 1, 2, 2, 2], wild]
    want = run(sites, ident_variants, grp, t=t2)
    assert same(run(sites, ident_variants, grp, cls=(np.zeros(N, np.int32), [IDENT], [[0.0] * 64]), t=t2), want)
    assert same(run(sites, ident_variants, grp, cls=(tidx, *ident3), t=t2), want)
    assert abs(float(want[2][-1])) < 2e-4 * 17
    got = run(sites, variants, grp, cls=(tidx, tables, bias), t=t1)
    lp, sizes, delta, res, rlp, ures, ulp, bunit, header = got
    assert header[0].item() == 7 and header[1].item() > 0 and bool(torch.isfinite(delta).all()) and bool(torch.isfinite(bunit).all())
    assert abs(float(delta[1])) < 2e-4 * 17 and abs(float(delta[-1])) < 2e-4 * 17           # the wild types
    lead = ures[ures >= 0].tolist()
    members = {r: g[0] for g in (g1, p1, p2) for r in g}
    assert sorted(set(lead)) == sorted(set(members.get(r, r) for r in res.tolist() if unmasked[r]))
    print(f"class scan contract {shape} {prec}: sizes {sizes.view(-1, 3).tolist()} delta {[round(float(d), 4) for d in delta]}")
    # table indices and entries out of range, negative entries
    bad_idx, ok_idx = tidx.copy(), tidx.copy()
    bad_idx[p1[1]], ok_idx[p1[1]] = 400, 2
    bad_idx[p2[0]], ok_idx[p2[0]] = -2, 0
    assert same(run(sites, variants, grp, cls=(bad_idx, tables, bias), t=t1), run(sites, variants, grp, cls=(ok_idx, tables, bias), t=t1))
    hi, cl = [list(r) for r in tables], [list(r) for r in tables]
    hi[2][A], cl[2][A] = 1 << 20, 32
    hi[1][7], cl[1][7] = -(1 << 30), -1
    assert same(run(sites, variants, grp, cls=(tidx, hi, bias), t=t1), run(sites, variants, grp, cls=(tidx, cl, bias), t=t1))
    # a cycle that does not close: that group is not tied, the others stand
    broken = (grp[0].copy(), grp[1], grp[2])
    broken[0][p2[1]] = 99
    without = with_groups(N, [g1, p1], [[1.0, 0.5, 0.25], [1.0, 1.0]])
    v_ok = variants[:6]
    assert same(run(sites[:3], v_ok, broken, cls=(tidx, tables, bias), t=t1), run(sites[:3], v_ok, without, cls=(tidx, tables, bias), t=t1))
    # site indices and tokens out of range: clamped
    bad = [list(v) for v in variants]; ok = [list(v) for v in variants]
    bad[0][0], bad[5][0], bad[3][3], bad[2][3] = -3, 9, -4, 77
    ok[0][0], ok[5][0], ok[3][3], ok[2][3] = 0, 3, 0, 32
    assert same(run(sites, bad, grp, cls=(tidx, tables, bias), t=t1), run(sites, ok, grp, cls=(tidx, tables, bias), t=t1))
    # capacities below the plan: a defined, reproducible result inside the declared buffers
    for caps in ((lambda lc, ic: ([c // 2 for c in lc], ic)), (lambda lc, ic: (lc, [c // 2 for c in ic])), (lambda lc, ic: ([1, 1, 1], [1, 1, 1])),
                 (lambda lc, ic: (lc, [ic[0], 3, ic[2] - 1]))):
        cut = run(sites, variants, grp, cls=(tidx, tables, bias), t=t1, caps=caps)
        assert same(cut, run(sites, variants, grp, cls=(tidx, tables, bias), t=t1, caps=caps)) and torch.equal(bits(cut[7]), bits(got[7]))


def test_a_too_small_workspace_is_refused_and_the_later_of_the_three_holds(weights_np):
    """ws_bytes one byte short: NAMP_EINVAL before any launch and the attachment is gone.  The class scan shares the attach kind of
    namp_mutations and namp_group_mutations: of the three the later call holds, a refused one leaves none; beside a tied score none runs."""
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
    assert rc == 0
    w, grp = np.ones(N, np.float32), with_groups(N, [], [])
    sites = [[2], [5]]
    tail = (2, 0, 0, 0, 0, 0, 0, 0)
    dims = (N, K, 3, 1, 35) + tail
    need, ioff = env.L.namp_class_mutations_workspace_bytes(*dims), env.L.namp_class_mutations_in_offset(*dims)
    assert need > env.L.namp_group_mutations_workspace_bytes(N, K, 3, *tail)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sec = class_section(sites, [], w, grp, np.zeros(N, np.int32), [IDENT], [[0.0] * 64])
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    attach = lambda: env.L.namp_class_mutations(1, 35, *tail)
    unmasked = t["mask"][0] != 0
    assert attach() == 0
    rc, lp = call(ws, need - 1)
    assert rc == -1 and b"workspace too small for a class scan" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)                     # plain: the attachment was cleared by the refused call
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert attach() == 0
    rc, lp_class = call(ws, need)
    assert rc == 0 and float((lp_class - lp_plain)[0][unmasked].abs().max()) < 2e-4
    assert env.L.namp_class_mutations(1, 32, *tail) == 0     # n_classes below the vocabulary: the attached call is refused
    rc, lp = call(ws, need)
    assert rc == -1 and b"bad dims for the attached class scan" in env.L.namp_last_error()
    assert attach() == 0 and env.L.namp_tied_score(1, mc.V33, 0) == 0
    rc, lp = call(ws, need)
    assert rc == -1 and b"attached together" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    assert env.L.namp_mutations(*tail) == 0 and env.L.namp_group_mutations(*tail) == 0 and attach() == 0
    rc, lp = call(ws, need)
    assert rc == 0 and torch.equal(lp, lp_class)
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
