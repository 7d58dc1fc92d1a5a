"""The memory contract of the three samplers with a forbidden-motifs attachment (namp_sample_motifs, include/namp.h) under the guarded
buffers of tests/guarded.py: a correct call on each route, and malformed sections — a window index out of range, a window index that is
the residue itself, entries that ask for tokens outside the vocabulary, every window empty.  These are inputs the kernel is specified
to clamp, with a defined result: the rows of the call whose section holds the clamped values.  Nothing outside the declared buffers is
touched, the section is found unchanged, a workspace without room for the section is refused, and a bad attach leaves the next call
plain."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HW = 3
W = 2 * HW
ROUTES = ("walk", "levels", "sequential")
# 56 motifs of two tokens (a neighbour that holds one of 8 tokens takes 7 candidates away) and one of four, which sets the half width
MOTIFS = [(a, b) for a in range(8) for b in range(7)] + [(0, 1, 2, 3)]


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 24)])
def test_motifs_under_guarded_buffers(weights_np, shape):
    import test_gpu_memory_contract as mc
    from guarded import Arena, run_contract
    from na_mpnn_amd.model import level_work_lists, motif_entries, motif_windows
    env = mc.Env(weights_np)
    B, N, K = shape
    bs = 2
    t = dict(mc.graph_case(B, N, K))
    K = t["K"]
    g = mc.gen(70 + N)
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(bs)]).to(mc.i32)
    rank = torch.empty_like(order).scatter_(1, order.long(), torch.arange(N, dtype=mc.i32).expand(bs, -1).contiguous())
    chain = ((torch.rand(1, N, generator=g) > 0.2).to(mc.i32) * t["mask"]) if N > 1 else t["mask"].clone()
    uniform, bias = torch.rand(bs, N, generator=g), mc.rn(g, 1, N, mc.V33, sc=0.1)
    entries = motif_entries(MOTIFS)
    E = entries.shape[0]
    n_dec = env.packed.n_dec
    base = env.L.namp_sample_workspace_bytes_n(1, bs, N, K, n_dec)
    off = env.L.namp_sample_motifs_offset(1, bs, N, K, n_dec, 0, 0, mc.V33)
    need = env.L.namp_sample_motifs_workspace_bytes(1, bs, N, K, n_dec, 0, 0, E, HW)
    assert base <= off and off % 256 == 0 and need == off + 4 * (N * W + 6 * E)

    # the clean section: one chain with a break in the middle, every residue present
    labels = (torch.arange(N) >= (N + 1) // 2).to(mc.i32)[None]
    window = motif_windows(labels, torch.arange(N, dtype=mc.i32)[None], torch.ones(1, N, dtype=mc.i32), HW)

    def section_of(win, ent):
        return torch.cat((win.reshape(-1).to(torch.int32), ent.reshape(-1).to(torch.int32)))

    def lists(dep):
        """Levels and work lists of the plain branch with the windows as further dependencies (inputs of the calls, not under test)."""
        dv = lambda x: x.to(env.dev).contiguous()
        idx, o, r, dp = dv(t["E_idx"]), dv(order), dv(rank), dv(dep)
        level = torch.empty(bs, N, dtype=mc.i32, device=env.dev)
        env.hip.check(env.L.namp_sample_levels_dep(idx.data_ptr(), o.data_ptr(), r.data_ptr(), dp.data_ptr(), W, None, None, level.data_ptr(),
                                                   bs, 1, N, K, env.s()), "sample_levels_dep")
        torch.cuda.synchronize()
        sel, flat, _, _, _ = level_work_lists(level.cpu(), None, None, order[0], t["E_idx"][0].long(), split=False)
        work = torch.stack((sel // N, sel % N), 1).to(mc.i32).contiguous()
        hist = torch.zeros(N + 1, dtype=mc.i64).scatter_add_(0, flat, torch.ones_like(flat))
        return work, torch.cat((hist.new_zeros(1), hist.cumsum(0))).to(mc.i32).contiguous(), torch.bincount(flat).tolist()

    work_t, off_t, counts = lists(window)
    assert env.L.namp_decoder_sample_walk_grid(bs, N, K) > 0

    def run(route, section, ws_bytes=None, attach=(E, HW)):
        """One guarded call: section None = no attachment."""
        ar = Arena(env.dev)
        a = dict(h_V=ar.inp("h_V_enc", t["V"]), h_E=ar.inp("h_E", t["E"]), idx=ar.inp("E_idx", t["E_idx"]), mask=ar.inp("mask", t["mask"]),
                 mask_dec=ar.inp("mask_dec", t["mask"].repeat(bs, 1)), chain=ar.inp("chain_mask", chain), S_true=ar.inp("S_true", t["S"]),
                 bias=ar.inp("bias", bias), order=ar.inp("order", order), rank=ar.inp("rank", rank), uniform=ar.inp("uniform", uniform))
        work, loff = ar.inp("work", work_t), ar.inp("level_off", off_t)
        S_out, probs, logp = ar.out("S_out", mc.i32, (bs, N)), ar.out("probs_out", mc.f32, (bs, N, mc.V33)), ar.out("logp_out", mc.f32, (bs, N, mc.V33))
        ws = ar.ws("ws", (need if section is not None else base) if ws_bytes is None else ws_bytes)
        sec_dev = section.to(env.dev) if section is not None else None
        counts_c = (C.c_int32 * len(counts))(*counts)

        def call():
            if section is not None:
                if off + 4 * section.numel() <= ws.nbytes:
                    ws.t[off:off + 4 * section.numel()].view(torch.int32).copy_(sec_dev)
                assert (env.L.namp_sample_motifs(*attach) == 0) == (attach == (E, HW))
            common = (env.packed.model(), a["h_V"].ptr, a["h_E"].ptr, a["idx"].ptr, a["mask"].ptr, a["mask_dec"].ptr, a["chain"].ptr,
                      a["S_true"].ptr, a["bias"].ptr, a["order"].ptr, a["rank"].ptr, a["uniform"].ptr, None, None, None, None, None)
            tail = (0.7, mc.SPECIAL, S_out.ptr, probs.ptr, logp.ptr, ws.ptr, ws.nbytes, bs, 1, N, K, env.s())
            if route == "walk":
                rc = env.L.namp_decoder_sample_walk(*common, work.ptr, None, bs * N, loff.ptr, None, None, None, *tail)
            elif route == "levels":
                rc = env.L.namp_decoder_sample_levels(*common, work.ptr, None, counts_c, len(counts), *tail)
            else:
                rc = env.L.namp_decoder_sample(*common, *tail)
            if section is not None and rc == 0:
                torch.cuda.synchronize()
                assert torch.equal(ws.t[off:off + 4 * section.numel()].view(torch.int32), sec_dev), "the call wrote into its input section"
            return rc
        if ws_bytes is not None:                                  # a refused call: nothing runs, nothing is written
            ar.build("A")
            rc = call()
            ar.check()
            return rc
        outs, reproducible = run_contract(lambda _a: call(), ar)
        assert reproducible and torch.equal(env.packed.flat, env.snapshot)
        return {k: v.cpu() for k, v in outs.items()}

    def same(x, y, what):
        for k in ("S_out", "probs_out", "logp_out"):
            assert torch.equal(x[k], y[k]), (what, k)

    clean = section_of(window, entries)
    ref = {route: run(route, clean) for route in ROUTES}
    plain = {route: run(route, None) for route in ROUTES}
    for route in ROUTES[:2]:
        same(ref[route], ref["sequential"], route)
        same(plain[route], plain["sequential"], route + " without an attachment")
    if N > 1:
        assert not torch.equal(ref["walk"]["probs_out"], plain["walk"]["probs_out"])       # (the section reaches the draw)

    # malformed sections give the rows of the call they are specified to clamp to
    i0 = N // 2
    d0 = HW if N > 1 and int(window[0, i0, HW]) >= 0 else HW - 1                         # a slot of residue i0 that holds a neighbour (N > 1)
    for route in ROUTES:
        absent = window.clone(); absent[0, i0, d0] = -1
        want = run(route, section_of(absent, entries))
        for what, v in (("window index >= N", N + 1000), ("window index < -1", -7), ("window index == residue", i0)):
            bad = window.clone(); bad[0, i0, d0] = v
            same(run(route, section_of(bad, entries)), want, (route, what))
        # entries that ask for a token outside the vocabulary never match: the rows of the section that repeats entry 0 in their place
        over, dup = entries.clone(), entries.clone()
        for e in (1, E - 1):
            over[e, 1] = (over[e, 1] & ~(0x3f << 12)) | ((40 + 1) << 12)                  # slot 7 (the member itself) asks for token 40 >= vocab
            dup[e] = entries[0]
        same(run(route, section_of(window, over)), run(route, section_of(window, dup)), (route, "entry tokens out of range"))
        same(run(route, section_of(torch.full_like(window, -1), entries)), plain[route], (route, "every window empty"))

    # too small a workspace for the section: NAMP_EINVAL, and the attachment is gone (the next call is a plain one and succeeds)
    for route in ROUTES:
        assert run(route, clean, ws_bytes=need - 1) == -1 and b"motif section" in env.L.namp_last_error()
        assert run(route, clean, ws_bytes=base) == -1
    same(run("walk", None), plain["walk"], "after a refused call")
    # a bad attach leaves nothing attached: the call behind it is the plain call (its workspace holds the section all the same)
    same(run("walk", clean, attach=(E, 8)), plain["walk"], "after a bad attach")
    same(run("walk", clean, attach=(505, HW)), plain["walk"], "after a bad attach")
