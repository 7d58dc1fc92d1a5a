"""The memory contract of namp_decoder_fwd with a tied score attached (namp_tied_score) under the guarded buffers of
tests/guarded.py: a correct call, and malformed sections — successors and table indices out of range, broken cycles, table entries
and tokens out of range.  These are inputs the kernels are specified to clamp (a broken cycle: to ungroup), with a defined result:
the result of the call with the clamped values; the input section is found unchanged, the outputs do not depend on what the
workspace held, and nothing outside the declared buffers is touched."""
import numpy as np
import pytest
import torch

import tied_score_ref as tr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

LANES, V = 64, 33


def pad(elems):
    """Bytes of one float array of the output section (include/namp.h): one extra element, rounded up to 256."""
    return (4 * (elems + 1) + 255) & ~255


def section(N, groups, tables, seqs):
    """groups: [(members, weights, table index per member)] -> the int32 words of the input section."""
    nxt, first, tidx, w = [-1] * N, [0] * N, [0] * N, [1.0] * N
    for g, gw, gt in groups:
        for t, r in enumerate(g):
            nxt[r], tidx[r], w[r] = g[(t + 1) % len(g)], gt[t], gw[t]
        first[g[0]] = 1
    words = [np.asarray(nxt + first + tidx, np.int32), np.asarray(w, np.float32).view(np.int32), np.asarray(tables, np.int32).reshape(-1),
             np.zeros(LANES * len(tables), np.int32), np.asarray(seqs, np.int32).reshape(-1)]
    return torch.from_numpy(np.concatenate(words))


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 48)])
def test_tied_score_under_guarded_buffers(weights_np, shape, prec):
    """namp_decoder_fwd with a tied score attached, under guarded buffers.  Without groups the units are the own entries of the same
    sequences as streams of the unattached decoder (< 2e-4, two summation orders).  With groups: the header holds the grouped
    residues and the hidden-backward edges of the numpy restatement, the members of a group carry one value, log_probs holds the
    rows of the first sequence.  Malformed sections give the bits of the clamped call; the input section is unchanged; nothing
    outside the declared buffers is written."""
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    env = mc.Env(weights_np)
    B, N, K = shape
    t = mc.graph_case(B, N, K)
    K = t["K"]
    ident = list(range(LANES))
    swap = list(range(LANES)); swap[0:4] = [3, 2, 1, 0]                # an involution below the vocabulary
    tables = [ident, swap]

    def run(groups, seqs, n_tables=2, raw=None):
        nk = len(seqs)
        dims = (N, K, 3, n_tables, V, nk)
        need, ioff, ooff = (f(*dims) for f in (env.L.namp_tied_score_workspace_bytes, env.L.namp_tied_score_in_offset,
                                               env.L.namp_tied_score_out_offset))
        sec = (section(N, groups, tables[:n_tables], seqs) if raw is None else raw).to(env.dev)
        out_bytes = 256 + 2 * pad(nk * N)
        assert need > 0 and ioff % 256 == 0 and ooff % 256 == 0 and ioff + 4 * sec.numel() <= ooff and ooff + out_bytes <= need
        ar = Arena(env.dev)
        hV, hE, idx = ar.inp("h_V_enc", t["V"]), ar.inp("h_E", t["E"]), ar.inp("E_idx", t["E_idx"])
        S, msk, rank = ar.inp("S", t["S"]), ar.inp("mask", t["mask"]), ar.inp("rank", t["rank"])
        lp = ar.out("log_probs", mc.f32, (1, N, mc.V33))
        ws = ar.ws("ws", need)
        seen = []

        def call():
            ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
            assert env.L.namp_tied_score(*dims[3:]) == 0
            rc = env.L.namp_decoder_fwd(env.packed.model(), hV.ptr, hE.ptr, idx.ptr, S.ptr, msk.ptr, rank.ptr, lp.ptr, None, None, ws.ptr,
                                        ws.nbytes, 1, 1, N, K, env.s())
            torch.cuda.synchronize()
            assert torch.equal(ws.t[ioff:ioff + 4 * sec.numel()].view(torch.int32), sec), "the call wrote into its input section"
            o = ws.t[ooff:ooff + out_bytes]
            a, b = 256, 256 + pad(nk * N)
            seen.append((o[:256].view(torch.int32).cpu().clone(), o[a:a + 4 * nk * N].view(torch.float32).view(nk, N).cpu().clone(),
                         o[b:b + 4 * nk * N].view(torch.float32).view(nk, N).cpu().clone()))
            return rc
        outs, reproducible = run_contract(lambda a: mc.with_precision(env, prec, call)(), ar)
        assert reproducible
        assert torch.equal(env.packed.flat, env.snapshot)
        assert all(all(torch.equal(x, y) for x, y in zip(s, seen[0])) for s in seen)   # (the output section does not depend on what the workspace held)
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
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

    g = torch.Generator().manual_seed(3)
    seqs = torch.randint(0, 33, (3, N), generator=g).tolist()
    plain = run([], seqs)
    lp, header, unit, member = plain
    ref = streams(seqs)
    want = ref.gather(2, torch.tensor(seqs)[:, :, None])[:, :, 0]
    d = float((unit - want).abs().max())
    print(f"tied score contract {shape} {prec}: no groups, max|d| vs the decoder's streams {d:.3e}")
    assert d < 2e-4 and header[:2].tolist() == [0, 0] and int(header[2:].abs().max()) == 0
    assert torch.equal(unit.view(torch.int32), member.view(torch.int32)) and float((lp[0] - ref[0]).abs().max()) < 2e-4
    assert torch.equal(lp[0].gather(1, torch.tensor(seqs[0])[:, None])[:, 0].view(torch.int32), member[0].view(torch.int32))
    # tokens out of range: clamped
    bad = [list(s) for s in seqs]; ok = [list(s) for s in seqs]
    bad[0][0], bad[1][N - 1], ok[0][0], ok[1][N - 1] = -4, 77, 0, 32
    assert same(run([], bad), run([], ok))
    if N < 17:                                               # N = 1: no group can close; a self-loop is ungrouped
        assert same(run([([0], [1.0], [1])], seqs), plain)
        return
    um = [i for i in range(N) if int(t["mask"][0, i])]
    masked = [i for i in range(N) if not int(t["mask"][0, i])]
    pair, triple = ([um[1], um[5]], [1.0, 0.5], [0, 1]), ([um[2], um[7], um[9]], [0.5, 0.25, 0.25], [0, 0, 0])
    seqs_c = [list(s) for s in seqs]
    for s in seqs_c[:2]:                                     # two consistent sequences, the third as drawn
        s[pair[0][1]] = swap[s[pair[0][0]]]
        s[triple[0][1]] = s[triple[0][2]] = s[triple[0][0]]
    got = run([pair, triple], seqs_c)
    lp, header, unit, member = got
    rank, E = t["rank"][0].numpy(), t["E_idx"][0].numpy()
    key, leader = tr.keys_and_leaders(rank, [pair[0], triple[0]])
    assert header[:2].tolist() == [5, int((tr.edge_kinds(E, key, leader) == tr.HID).sum())]
    for grp in (pair[0], triple[0]):
        assert all(torch.equal(unit[:, grp[0]], unit[:, r]) for r in grp) and bool(torch.isfinite(unit[:2, grp[0]]).all())
    assert bool(torch.isfinite(member).all())
    assert torch.equal(lp[0].gather(1, torch.tensor(seqs_c[0])[:, None])[:, 0].view(torch.int32), member[0].view(torch.int32))
    assert float((unit[:, pair[0][0]] - plain[2][:, pair[0][0]]).abs().max()) > 0          # (the tie is read)
    # a group with a masked member, a cycle that leaves [0, N), one without `first`, a tail into a cycle: ungrouped
    only_pair = run([pair], seqs_c)
    if masked:
        assert same(run([pair, ([masked[0], um[3]], [1.0, 1.0], [0, 0])], seqs_c), only_pair)
    raw = section(N, [pair, triple], tables, seqs_c)
    for word, value in ((triple[0][1], 99), (triple[0][2], -3), (N + triple[0][0], 0), (triple[0][2], triple[0][1])):
        broken = raw.clone()
        broken[word] = value
        a, b = run(None, seqs_c, raw=broken), only_pair
        assert a[1][:2].tolist() == b[1][:2].tolist() and a[1][0] == 2 and same((a[0], a[2], a[3]), (b[0], b[2], b[3]))
    # table indices and table entries out of range: clamped (an entry below 0 is absent: no class every member has -> -inf)
    hi = section(N, [(pair[0], pair[1], [0, 7]), triple], tables, seqs_c)
    assert same(run(None, seqs_c, raw=hi), got)
    lo = section(N, [(pair[0], pair[1], [-5, 1]), triple], tables, seqs_c)
    assert same(run(None, seqs_c, raw=lo), got)
    big = [list(ident), list(swap)]; big[1][5] = 77
    clamped = [list(ident), list(swap)]; clamped[1][5] = 32
    a = run(None, seqs_c, raw=section(N, [pair, triple], big, seqs_c))
    assert same(a, run(None, seqs_c, raw=section(N, [pair, triple], clamped, seqs_c)))


def test_a_too_small_workspace_is_refused_and_clears_the_attachment(weights_np):
    """ws_bytes one byte short of namp_tied_score_workspace_bytes: NAMP_EINVAL before any launch, and the attachment is gone — the
    NEXT plain namp_decoder_fwd call is the unattached one, bit for bit.  Bad arguments of namp_tied_score attach nothing, a tied
    score and a library attached together run neither, and the sizes are 0 where the route is not supported."""
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
    dims = (N, K, 3, 1, V, 2)
    need = env.L.namp_tied_score_workspace_bytes(*dims)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sec = section(N, [], [list(range(LANES))], [t["S"][0].tolist()] * 2)
    ioff = env.L.namp_tied_score_in_offset(*dims)
    ws[ioff:ioff + 4 * sec.numel()].view(torch.int32).copy_(sec)
    assert env.L.namp_tied_score(*dims[3:]) == 0
    rc, lp = call(ws, need - 1)
    assert rc == -1 and b"workspace too small" in env.L.namp_last_error() and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)                     # plain: the attachment was cleared by the refused call
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_tied_score(*dims[3:]) == 0             # an attached call that succeeds clears it as well
    rc, lp = call(ws, need)
    assert rc == 0 and float((lp - lp_plain).abs().max()) < 2e-4
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    for bad in ((0, V, 2), (65, V, 2), (1, 65, 2), (1, V, -1)):     # bad arguments attach nothing
        assert env.L.namp_tied_score(*bad) == -1
        rc, lp = call(plain_ws, plain_bytes)
        assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_tied_score(1, V - 1, 2) == 0           # n_classes below the vocabulary: refused by the call itself
    rc, lp = call(ws, need)
    assert rc == -1 and float(lp.abs().max()) == 0.0
    assert env.L.namp_tied_score(*dims[3:]) == 0 and env.L.namp_library(1, 0, 0, 0, 0) == 0      # both attached: neither runs, both are gone
    rc, lp = call(ws, need)
    assert rc == -1 and float(lp.abs().max()) == 0.0
    rc, lp = call(plain_ws, plain_bytes)
    assert rc == 0 and torch.equal(lp, lp_plain)
    assert env.L.namp_tied_score(*dims[3:]) == 0             # n_chunk = 0 plans only: log_probs is not written
    assert env.L.namp_tied_score(1, V, 0) == 0
    rc, lp = call(ws, need)
    assert rc == 0 and float(lp.abs().max()) == 0.0
    # sizes are 0 where unsupported: another number of decoder layers, K > N, no table, too many classes, row codes past 2^28
    for bad in ((N, K, 4, 1, V, 2), (N, N + 1, 3, 1, V, 2), (N, K, 3, 0, V, 2), (N, K, 3, 65, V, 2), (N, K, 3, 1, 65, 2),
                (N, K, 3, 1, V, (1 << 28) // N + 1)):
        assert env.L.namp_tied_score_workspace_bytes(*bad) == 0 and env.L.namp_tied_score_in_offset(*bad) == 0
        assert env.L.namp_tied_score_out_offset(*bad) == 0
