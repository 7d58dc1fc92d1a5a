"""numpy restatement of the index grids of the leave-one-out cone (na_mpnn_amd/csrc/namp_loo.h: loo_prepare_kernel /
loo_edges_kernel) and brute-force set definitions of the same cone, for one complex.  Helper module of
test_conditional_host.py / test_gpu_conditional.py (not a test)."""
import numpy as np


def loo_grids(E_idx, rank, mask):
    """E_idx [L, K], rank [L], mask [L] -> rev [L, K] (edge (a, k) -> b: position of a in E_idx[b], or -1), act1 [L, K] (layer-1 item
    (m, k), i = E_idx[m, k]: m used to see i as decoded), act2 [L, K] (layer-2 item (i, kq), q = E_idx[i, kq]: a layer-1 override feeds q)."""
    E_idx = np.asarray(E_idx, np.int64); rank = np.asarray(rank, np.int64); mask = np.asarray(mask)
    L, K = E_idx.shape
    ar = np.arange(L)
    eq = E_idx[E_idx] == ar[:, None, None]                                   # [a, k, p]: E_idx[E_idx[a, k], p] == a
    rev = np.where(eq.any(-1), eq.argmax(-1), -1)
    act1 = (E_idx != ar[:, None]) & (rank[E_idx] < rank[:, None]) & (mask[:, None] != 0)
    in_a1 = np.zeros((L, L), bool)                                           # [i, m]: m in A1(i)
    mm, kk = np.nonzero(act1)
    in_a1[E_idx[mm, kk], mm] = True
    q = E_idx                                                                # [i, kq]
    cen_ov = in_a1[ar[:, None], q]
    nb = E_idx[q]                                                            # [i, kq, k']: neighbours of q
    bw = (nb != ar[:, None, None]) & (rank[nb] < rank[q][..., None])
    ov = bw & in_a1[ar[:, None, None], nb]
    act2 = (q != ar[:, None]) & (mask[q] != 0) & (cen_ov | ov.any(-1))
    return rev, act1, act2


def cone_sets(E_idx, rank, mask):
    """Brute force, straight from the definition: per stream i the sets A1(i) (residues whose layer-1 output differs from the base
    stream), need2(i) (neighbours of i whose layer-2 output differs) and need1(i) (the members of A1(i) that i's layers actually
    read: its own neighbours and the decoded neighbours of need2(i))."""
    L, K = E_idx.shape
    radj = [[] for _ in range(L)]
    for j in range(L):
        for q in E_idx[j]:
            radj[int(q)].append(j)
    A1, N1, N2 = [], [], []
    for i in range(L):
        a1 = {j for j in radj[i] if j != i and rank[i] < rank[j] and mask[j]}
        a2 = set(a1)
        for q in a1:
            a2.update(j for j in radj[q] if j != i and rank[q] < rank[j] and mask[j])
        nb = set(int(q) for q in E_idx[i]) - {i}
        need2 = nb & a2
        need1 = set(nb & a1)
        for q in need2:
            need1.update(int(m) for m in E_idx[q] if m != i and rank[m] < rank[q] and int(m) in a1)
            if q in a1:
                need1.add(q)
        A1.append(a1); N1.append(need1); N2.append(need2)
    return A1, N1, N2


def oracle_conditional(w, fd, top_k, chunk=32):
    """Leave-one-out conditionals on the CPU oracle (oracle/cpu_ref.py), straight from the definition: encode once, then the parallel
    decoder with the order of score() in which i is moved to the end, row i of stream i — `chunk` streams per decoder call.
    w: torch weights, fd: CPU feature_dict with a batch dimension.  Returns log_probs [B, L, vocab], the base order [B, L], E_idx."""
    import torch
    from oracle import cpu_ref as R
    h_V, h_E, E_idx = R.encode(w, fd, top_k)
    S, mask = fd["S"].long(), fd["mask"]
    B, L = S.shape
    order = R.decoding_order_of(mask * fd["chain_mask"], fd["randn"])
    out = None
    for b in range(B):
        ob = order[b]
        rep = lambda t, n: t[b:b + 1].expand(n, *t.shape[1:])
        for i0 in range(0, L, chunk):
            ids = list(range(i0, min(L, i0 + chunk)))
            n = len(ids)
            orders = torch.stack([torch.cat([ob[ob != i], ob.new_tensor([i])]) for i in ids])
            E_rep = rep(E_idx, n).contiguous()
            lp, _ = R.decode_parallel(w, rep(h_V, n), rep(h_E, n), E_rep, rep(S, n), rep(mask, n), R.backward_mask(orders, E_rep))
            if out is None:
                out = torch.empty(B, L, lp.shape[-1])
            out[b, i0:i0 + n] = lp[torch.arange(n), torch.tensor(ids)]
    return out, order[:B], E_idx


def near_tie_rows(ref_log_probs, mask, gap=2e-3):
    """Rows whose arg-max is compared: mask == 1 and the oracle's top-two gap is at least `gap`.  Returns (compared [.., L] bool, left out)."""
    import torch
    top2 = torch.topk(ref_log_probs, 2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) >= gap
    valid = mask.bool()
    return valid & clear, int((valid & ~clear).sum())
