"""The memory contract of namp_decoder_loo with a pair-class attachment (namp_loo_classes) under the guarded buffers of
tests/guarded.py: correct calls for pairs and for groups, and malformed class tables — a table index out of range, entries outside
[-1, vocab), a member that lacks a class its closing member has, bad next / first.  These are inputs the kernel is specified to clamp,
with a defined result: what stays valid is tied, the rest get leave-one-out rows and class rows of -inf, and nothing outside the
declared buffers is touched."""
import pytest
import torch

from na_mpnn_amd import spec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NEG = -float("inf")
GU, UG = spec.CLASS_GU, spec.CLASS_UG


def class_tables():
    """Eight tables [64] and their biases: 0 the identity, 1 the Watson-Crick map (no class beyond the vocabulary), 2 / 3 the first /
    second member of an RNA-RNA wobble pair (bias 0.7 on the two wobble lanes), 4 = 3 with an entry above the vocabulary (class 5)
    and one below -1 (class GU), 5 = what 4 is clamped to (token 32; no class GU), 6 = 2 without the class UG, 7 = 3 without it."""
    rti = spec.restype_to_int()
    pad = [-1] * (64 - 33)
    t = [list(range(33)) + pad, spec.token_map(rti, "same") + pad, spec.class_table(rti, "rna-rna", True, True),
         spec.class_table(rti, "rna-rna", True, False)]
    t.append(list(t[3])); t[4][5], t[4][GU] = 1000, -7
    t.append(list(t[3])); t[5][5], t[5][GU] = 32, -1
    for src in (2, 3):
        t.append(list(t[src])); t[-1][UG] = -1
    bias = [[0.0] * 64 for _ in t]
    for k in range(2, len(t)):
        bias[k][GU] = bias[k][UG] = 0.7
    return t, bias


def section_of(N, groups, tables, bias, weights=(1.0, 0.5, 0.25)):
    """The input section of include/namp.h for one complex: next (for groups of two: the partner), first, table_idx, weight bits,
    tables, bias bits.  groups: [(members in listed order, their table indices)]."""
    nxt, first, tidx, w = [-1] * N, [0] * N, [0] * N, [1.0] * N
    for g, ti in groups:
        for t, r in enumerate(g):
            nxt[r], tidx[r], w[r] = g[(t + 1) % len(g)], ti[t], weights[t % len(weights)]
        first[g[0]] = 1
    return torch.cat((torch.tensor(nxt + first + tidx, dtype=torch.int32), torch.tensor(w).view(torch.int32),
                      torch.tensor(tables, dtype=torch.int32).reshape(-1), torch.tensor(bias).view(torch.int32).reshape(-1)))


def marginal(clp, table):
    """row[t] = logsumexp of clp[c] over {c : table[c] == t}, in fp64."""
    T = torch.tensor(table)
    sel = (T[:, None] == torch.arange(33)[None, :]) & torch.isfinite(clp)[:, None]
    return torch.logsumexp(torch.where(sel, clp.double()[:, None], torch.full((64, 33), NEG, dtype=torch.float64)), 0)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_class_tables_under_guarded_buffers(weights_np, shape, prec):
    """namp_decoder_loo with class tables attached, under the guarded buffers of the contract table's row.  N = 17: a correct call for
    groups (a group of three without wobble lanes: the canonical call's bits; a wobble pair: live lanes 33 / 34, every member's row the
    marginal of its class row) and for pairs (the same bits through either section); malformed tables give the rows of the call whose
    tables hold the clamped values; bad next / first and a partner that does not name the residue back untie exactly that pair or
    group.  N = 1: a self-loop and a successor out of range.  The input section is found unchanged, the class rows do not depend on what
    the workspace held, and nothing is written outside the declared buffers."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t = mc.graph_case(B, N, K)
    K = t["K"]
    tables, bias = class_tables()
    n_tab = len(tables)
    off = env.L.namp_loo_groups_offset(B, N, K, 3)

    def run(section, groups, mask=None, canonical=None):
        """One guarded call: section None = no attachment; canonical = (section, n_maps) attaches token maps (namp_loo_groups) instead."""
        ar = Arena(env.dev)
        hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
        S, msk, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"] if mask is None else mask), ar.inp("rank", t["rank"])
        lp, counts = ar.out("log_probs", mc.f32, (B, N, mc.V33)), ar.out("counts", mc.i32, (2,))
        if canonical is not None:
            section, n_maps = canonical
            nbytes = env.L.namp_loo_groups_workspace_bytes(B, N, K, 3, n_maps)
        elif section is not None:
            nbytes = env.L.namp_loo_classes_workspace_bytes(B, N, K, 3, n_tab, groups)
            c_off = env.L.namp_loo_classes_out_offset(B, N, K, 3, n_tab, groups)
            assert c_off + 256 * B * N == nbytes and off + 4 * section.numel() <= c_off
        else:
            nbytes = env.L.namp_loo_workspace_bytes(B, N, K, 3)
        ws = ar.ws("ws", nbytes)
        sec_dev = section.to(env.dev) if section is not None else None
        seen = []

        def call():
            if section is not None:
                ws.t[off:off + 4 * section.numel()].view(torch.int32).copy_(sec_dev)
                assert (env.L.namp_loo_groups(n_maps) if canonical is not None else env.L.namp_loo_classes(n_tab, spec.N_CLASSES, groups)) == 0
            rc = env.L.namp_decoder_loo(env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, msk.ptr, rank.ptr, lp.ptr, counts.ptr, ws.ptr,
                                        ws.nbytes, B, N, K, env.s())
            if section is not None:
                torch.cuda.synchronize()
                assert torch.equal(ws.t[off:off + 4 * section.numel()].view(torch.int32), sec_dev), "the call wrote into its input section"
                if canonical is None:
                    seen.append(ws.t[c_off:c_off + 256 * B * N].view(torch.float32).view(B * N, 64).cpu().clone())
            return rc
        outs, reproducible = run_contract(lambda a: mc.with_precision(env, prec, call)(), ar)
        assert reproducible
        assert torch.equal(env.packed.flat, env.snapshot)
        assert all(torch.equal(s, seen[0]) for s in seen)     # (the class rows do not depend on what the workspace held)
        return outs["log_probs"].cpu(), outs["counts"].cpu(), (seen[0] if seen else None)

    lp_none, c_none, _ = run(None, 0)
    if N < 17:                                               # N = 1: a partner / successor that is the residue itself; one out of range
        for groups in (0, 1):
            for nxt in (0, 5):
                sec = section_of(N, [], tables, bias)
                sec[0], sec[N] = nxt, 1
                lp, c, cls = run(sec, groups)
                assert torch.equal(lp, lp_none) and torch.equal(c, c_none) and bool((cls == NEG).all())
        return
    free = [r for r in range(N) if t["mask"][0].tolist()[r]]
    three, two = [free[1], free[6], free[4]], [free[9], free[2]]
    good = section_of(N, [(three, [0, 1, 0]), (two, [2, 3])], tables, bias)
    lp_good, c_good, cls_good = run(good, 1)
    # the canonical call on the same cycles (token maps: the tables below the vocabulary, the identity beyond)
    maps = [tb[:33] + list(range(33, 64)) for tb in tables[:4]]
    canon = torch.cat((good[:4 * N], torch.tensor(maps, dtype=torch.int32).reshape(-1)))
    lp_canon, c_canon, _ = run(None, 1, canonical=(canon, 4))
    assert torch.equal(c_good, c_canon)
    rest = [r for r in range(N) if r not in three + two]
    assert torch.equal(lp_good[0, rest], lp_none[0, rest]) and torch.equal(lp_good[0, three], lp_canon[0, three])     # no wobble lanes: the canonical bits
    assert float((lp_good - lp_canon)[0, two].abs().amax(-1).min()) > 1e-3                   # two live wobble lanes
    assert float((lp_good - lp_none)[0, three + two].abs().amax(-1).min()) > 1e-2
    lead = [three[0], two[0]]
    assert bool((cls_good[[r for r in range(N) if r not in lead]] == NEG).all())
    assert bool(torch.isfinite(cls_good[lead][:, :33]).all()) and bool((cls_good[:, 35:] == NEG).all())
    assert bool((cls_good[three[0], 33:] == NEG).all()) and bool(torch.isfinite(cls_good[two[0], 33:35]).all())
    assert float((cls_good[lead].double().exp().sum(-1) - 1).abs().max()) < 1e-5
    for g, ti in ((three, [0, 1, 0]), (two, [2, 3])):        # every member's row is the marginal of its group's class row
        for r, k in zip(g, ti):
            assert float((lp_good[0, r].double() - marginal(cls_good[g[0]], tables[k])).abs().max()) < 1e-5, (g, r)
    # pairs through the pair section: the same bits as through the group section
    pair_sec = section_of(N, [(two, [2, 3]), ([free[1], free[6]], [0, 1])], tables, bias)
    lp_p, c_p, cls_p = run(pair_sec, 0)
    lp_pg, c_pg, cls_pg = run(pair_sec, 1)
    assert torch.equal(lp_p, lp_pg) and torch.equal(c_p, c_pg) and torch.equal(cls_p, cls_pg)
    assert torch.equal(lp_p[0, two], lp_good[0, two]) and torch.equal(cls_p[two[0]], cls_good[two[0]])
    # malformed tables: table indices out of range (clamped to the last / the first table), entries outside [-1, vocab) (clamped
    # to the last token / absent) — the rows of the call whose tables hold the clamped values
    bad, expect = good.clone(), good.clone()
    for r, b_idx, e_idx in ((three[1], 99, n_tab - 1), (three[2], -5, 0), (two[1], 4, 5)):
        bad[2 * N + r], expect[2 * N + r] = b_idx, e_idx
    lp_bad, c_bad, cls_bad = run(bad, 1)
    lp_exp, c_exp, cls_exp = run(expect, 1)
    assert torch.equal(lp_bad, lp_exp) and torch.equal(c_bad, c_exp) and torch.equal(cls_bad, cls_exp)
    assert bool(torch.isfinite(cls_bad[two[0], UG])) and bool(cls_bad[two[0], GU] == NEG) and bool((cls_bad[three[0], 33:] == NEG).all())
    assert not torch.equal(lp_bad[0, two], lp_good[0, two]) and torch.equal(lp_bad[0, rest], lp_none[0, rest])
    # a member that lacks a class its closing member has: the class is absent, as if the closing member lacked it too
    lacks, both = good.clone(), good.clone()
    lacks[2 * N + two[0]] = 6
    both[2 * N + two[0]], both[2 * N + two[1]] = 6, 7
    lp_l, c_l, cls_l = run(lacks, 1)
    lp_2, c_2, cls_2 = run(both, 1)
    assert torch.equal(lp_l, lp_2) and torch.equal(c_l, c_2) and torch.equal(cls_l, cls_2)
    assert bool(torch.isfinite(cls_l[two[0], GU])) and bool(cls_l[two[0], UG] == NEG)
    assert float((lp_l[0, two].double().exp().sum(-1) - 1).abs().max()) < 1e-5 and not torch.equal(lp_l[0, two], lp_good[0, two])
    # bad next / first: nothing stays tied
    broken = good.clone()
    broken[three[1]] = N + 5                                 # a successor out of range
    broken[N + two[1]] = 1                                   # two `first` flags
    lp_b, c_b, cls_b = run(broken, 1)
    assert torch.equal(lp_b, lp_none) and torch.equal(c_b, c_none) and bool((cls_b == NEG).all())
    # the pair section: a partner that does not name the residue back unties that pair only
    half = pair_sec.clone()
    half[free[6]] = free[4]
    only = section_of(N, [(two, [2, 3])], tables, bias)
    lp_h, c_h, cls_h = run(half, 0)
    lp_o, c_o, cls_o = run(only, 0)
    assert torch.equal(lp_h, lp_o) and torch.equal(c_h, c_o) and torch.equal(cls_h, cls_o)
    assert torch.equal(lp_h[0, [free[1], free[6]]], lp_none[0, [free[1], free[6]]]) and bool((cls_h[free[1]] == NEG).all())


def test_a_too_small_workspace_is_refused_and_clears_the_attachment(weights_np):
    """ws_bytes one byte short of namp_loo_classes_workspace_bytes: NAMP_EINVAL before any launch, and the attachment is gone — the
    next call, a plain one in a plain workspace, gives the plain bits."""
    import test_gpu_memory_contract as mc
    env = mc.Env(weights_np)
    B, N, K = 1, 17, 16
    t = mc.graph_case(B, N, K)
    K = t["K"]
    dev = env.dev
    hV, hE, idx, S, msk, rank = (t[k].to(dev).contiguous() for k in ("V", "E", "E_idx", "S", "mask", "rank"))
    tables, bias = class_tables()

    def call(ws, nbytes):
        lp, counts = torch.zeros(B, N, mc.V33, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        rc = env.L.namp_decoder_loo(env.packed.model(), hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), S.data_ptr(), msk.data_ptr(),
                                    rank.data_ptr(), lp.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, B, N, K, env.s())
        torch.cuda.synchronize()
        return rc, lp.cpu(), counts.cpu()
    plain_bytes = env.L.namp_loo_workspace_bytes(B, N, K, 3)
    rc, lp_plain, c_plain = call(torch.empty(plain_bytes, dtype=torch.uint8, device=dev), plain_bytes)
    assert rc == 0
    for groups in (0, 1):
        need = env.L.namp_loo_classes_workspace_bytes(B, N, K, 3, len(tables), groups)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        sec = section_of(N, [([1, 2], [2, 3])], tables, bias)
        off = env.L.namp_loo_groups_offset(B, N, K, 3)
        ws[off:off + 4 * sec.numel()].view(torch.int32).copy_(sec.to(dev))
        assert env.L.namp_loo_classes(len(tables), spec.N_CLASSES, groups) == 0
        rc, lp, _ = call(ws, need - 1)
        assert rc == -1 and b"workspace too small" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
        rc, lp, c = call(ws, plain_bytes)                    # plain: the attachment was cleared by the refused call
        assert rc == 0 and torch.equal(lp, lp_plain) and torch.equal(c, c_plain)
    # n_classes below the vocabulary is refused by the call itself, which clears the attachment as well
    assert env.L.namp_loo_classes(len(tables), 20, 0) == 0
    rc, _, _ = call(ws, need)
    assert rc == -1 and b"n_classes" in env.L.namp_last_error()
    rc, lp, c = call(ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain) and torch.equal(c, c_plain)
