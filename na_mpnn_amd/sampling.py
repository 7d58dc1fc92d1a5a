"""The host side of ProteinMPNN.sample() in three stages: the PLAN of a design call (SamplePlan: visit order, groups, levels, level-sorted work
lists) from one of four builders — plain_plan, pairs_plan and states_plan on the device, host_plan through symmetry_visits and level_work_lists —,
the per-residue arrays (SamplerArrays; model.py's callers form them: they differ) and the one launch() of the three sampler entry points."""
from __future__ import annotations

import collections
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip


def _i32(t):
    return t.to(torch.int32).contiguous()


class SamplePlan(NamedTuple):
    """What a sampler launch reads beside the per-residue arrays; n = the residues the decoder sees (L, or M * L with tied states), everything int32
    on the device unless noted.  Without groups the three group arrays are None; the sequential walk (namp_decoder_sample) needs the first six only."""
    E: torch.Tensor                                        # the neighbour lists the decoder sees: E_idx [B, n, K], or flattened [n * K]
    order: torch.Tensor                                    # [B_dec, n] the residues in visit order
    rank: torch.Tensor                                     # [B_dec, n] its inverse
    group_first: Optional[torch.Tensor] = None             # [B_dec, n] by visit: the first visit of the visit's group
    group_last: Optional[torch.Tensor] = None              # [B_dec, n] by visit: 1 on a group's last visit
    sym_w: Optional[torch.Tensor] = None                   # [n] float32: the weight of every residue in its group's sum
    level: Optional[torch.Tensor] = None                   # [B_dec, n] by visit (namp_sample_levels_dep)
    work: Optional[torch.Tensor] = None                    # [>= nwork, 2] (stream, first visit) of every work item, sorted by level
    work_n: Optional[torch.Tensor] = None                  # [>= nwork] visits per item (None: one each)
    nwork: int = 0
    level_off: Optional[torch.Tensor] = None               # [n + 2] where every level's items start (the walk)
    levels: Optional[torch.Tensor] = None                  # the number of levels: a device scalar (the walk)
    close: Optional[torch.Tensor] = None                   # the deferred draws of split groups, sorted by level, and
    close_off: Optional[torch.Tensor] = None               # where every level's draws start
    step_of: Optional[torch.Tensor] = None                 # [n] int64, host route on request: visit -> the step of its group
    item_level: Optional[torch.Tensor] = None              # [nwork] int64, host route: the level of every item (per-level launches count them)


# the per-residue arrays of a sampler launch as the kernels read them (contiguous; int32 / float32), [B_dec or B_enc, n, ...]
SamplerArrays = collections.namedtuple("SamplerArrays", "h_V h_E mask mask_dec chain_mask S bias uniform forced pair_bias", defaults=(None, None))


def level_work_lists(level, group_first, group_last, order0, E_idx0, split):
    """Work lists of the level-parallel sampler (include/namp.h: namp_decoder_sample_levels / _walk) from the per-visit levels.

    level [B_dec, L] int32 by visit (namp_sample_levels_dep); group_first / group_last [B_dec, L] int32 by visit, or None without
    symmetry groups (every stream has the same groups); order0 [L] the residues in visit order, E_idx0 [L, K] the neighbour lists.
    Returns (sel, flat, work_n, close, close_off): sel = stream * L + first visit of every work item, sorted by level (flat = those
    levels); work_n = visits per item (None without groups); close / close_off = the deferred-draw lists when `split`, else None.
    split: a group none of whose members has another member among its graph neighbours becomes single-member items (decoded in
    parallel, one deferred draw per group); a group with internal edges stays ONE item whose members run one after the other."""
    B_dec, L = level.shape
    dev = level.device
    if group_first is None:
        flat = level.reshape(-1).long()
        perm = torch.argsort(flat, stable=True)
        return perm, flat[perm], None, None, None
    ar = torch.arange(L, dtype=torch.int32, device=dev)
    gf0 = group_first[0].to(torch.int32)
    gsize = torch.bincount(gf0.long(), minlength=L).to(torch.int32)                       # by first visit
    whole = torch.ones(L, dtype=torch.bool, device=dev)                                    # visit v belongs to a group run as ONE item
    close = close_off = None
    if split:
        ord0 = order0.long()
        gid_res = torch.empty(L, dtype=torch.int32, device=dev).scatter_(0, ord0, gf0)    # residue -> its group's first visit
        nb = E_idx0.long()
        intra = ((gid_res[nb] == gid_res[:, None]) & (nb != ar[:, None].long())).any(1)   # residue has a neighbour in its own group
        gdep = torch.zeros(L, dtype=torch.int32, device=dev).scatter_reduce_(0, gf0.long(), intra[ord0].to(torch.int32), "amax")
        whole = gdep[gf0.long()] > 0
        lastv = (group_last[0] != 0).nonzero().view(-1)                                    # one closing entry per group and stream
        cl_v = lastv.repeat(B_dec)
        cl_b = torch.arange(B_dec, device=dev).repeat_interleave(lastv.numel())
        cl_lv = level[cl_b, cl_v].long()
        cperm = torch.argsort(cl_lv, stable=True)
        close = torch.stack((cl_b[cperm], cl_v[cperm]), 1).to(torch.int32).contiguous()
        chist = torch.zeros(L + 1, dtype=torch.int64, device=dev).scatter_add_(0, cl_lv, torch.ones_like(cl_lv))
        close_off = torch.cat((chist.new_zeros(1), chist.cumsum(0))).to(torch.int32).contiguous()
    heads0 = (~whole) | (gf0 == ar)                                                        # an item starts at this visit
    n0 = torch.where(whole, gsize[gf0.long()], torch.ones_like(gsize))
    head_pos0 = heads0.nonzero().view(-1)
    head_pos = (torch.arange(B_dec, device=dev)[:, None] * L + head_pos0[None, :]).view(-1)   # stream-major
    sizes = n0[head_pos0].repeat(B_dec)
    flat = level.reshape(-1)[head_pos].long()
    perm = torch.argsort(flat, stable=True)
    return head_pos[perm], flat[perm], sizes[perm].contiguous(), close, close_off


def symmetry_visits(groups, weights, order0, L):
    """Visit plan of symmetry-tied sampling (model_utils.py:220-235): tied residues are visited together, in the order stream 0's
    decoding order `order0` (a list of the L residues) reaches their first member; every stream then uses that one order.  A residue
    listed in several groups belongs to the FIRST listed one (as in the reference).  groups / weights: the feature_dict's
    symmetry_residues / symmetry_weights.  Returns lists of L: (visits, group_first, group_last, w) = the residues in visit order, the
    first visit of each visit's group, 1 on a group's last visit (else 0), and the weight of each residue (1 outside the groups)."""
    w = [1.0] * L
    for i1, group in enumerate(groups):
        for i2, item in enumerate(group):
            w[item] = float(weights[i1][i2])
    group_of = {}
    for g in groups:
        for item in g:
            group_of.setdefault(int(item), g)
    seen, visit_groups = set(), []
    for t in order0:
        if t in seen:
            continue
        visit_groups.append(list(group_of.get(t, (t,))))
        seen.update(visit_groups[-1])
    visits = [t for g in visit_groups for t in g]
    if sorted(visits) != list(range(L)):
        raise ValueError("symmetry_residues groups must be disjoint")
    gf, gl, v = [], [], 0
    for g in visit_groups:
        gf += [v] * len(g); gl += [0] * (len(g) - 1) + [1]; v += len(g)
    return visits, gf, gl, w


def carve_i32(sizes, dev):
    """16-byte aligned pieces of ONE int32 allocation -> (the allocation, its pieces in the order of `sizes`)."""
    offs = np.concatenate(([0], np.cumsum([(q + 3) & ~3 for q in sizes]))).tolist()
    buf = torch.empty(offs[-1], dtype=torch.int32, device=dev)
    return buf, [buf[a:a + q] for a, q in zip(offs, sizes)]


def side_stream_work(model, o, tensors, enqueue):
    """Plan launches run on the model's side stream, beside the encoder.  Records an event in the calling stream NOW — what the launches read
    is out and what they write is allocated: the side stream writes behind the event only, and a block the allocator hands out later could
    still be a temporary of the encoder launches enqueued in between — and returns start(): the side stream waits for the event, enqueue(side
    stream) enqueues, o.wait() orders the decoder behind it, and none of `tensors` (all the side stream touches) is recycled before it is done."""
    dev = tensors[0].device
    ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(dev))
    def start():
        side = model._side_stream(dev)
        side.wait_event(ev)
        enqueue(side.cuda_stream)
        o.event = torch.cuda.Event(); o.event.record(side)
        for t in tensors:
            t.record_stream(side)
    return start


def plain_plan(model, E, order32, rank, deps, dims, o=None):
    """The plan without groups on the device: the dependency levels (namp_sample_levels_dep; deps = (dep_idx, n_dep) beside the graph's, or
    (None, 0)) and the walk's level-sorted work lists (namp_sample_work_lists: one launch instead of a stable argsort, gathers, divisions, a
    histogram and its prefix sums).  E, order32, rank: int32, contiguous.  o (the call's _DecodingOrder) given: on the side stream, beside the
    encoder launches enqueued next (the levels are a serial walk of one wave per stream: 62 us at 97 residues); None: in the calling stream."""
    (B_dec, B_enc, L, K), Lb, dev = dims, hip.lib(), E.device
    level, work, level_off, n_levels = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((B_dec, L), (B_dec * L, 2), L + 2, 1))
    dep, n_dep = deps
    def enqueue(stream):
        hip.check(Lb.namp_sample_levels_dep(E.data_ptr(), order32.data_ptr(), rank.data_ptr(), hip.ptr(dep), n_dep, None, None, level.data_ptr(),
                                            B_dec, B_enc, L, K, stream), "sample_levels")
        hip.check(Lb.namp_sample_work_lists(level.data_ptr(), work.data_ptr(), level_off.data_ptr(), n_levels.data_ptr(), B_dec, L, stream),
                  "sample_work_lists")
    if o is None:
        enqueue(hip.current_stream())
    else:       # (dep is a piece of the pair terms' workspace, uploaded and sorted in the calling stream in front of the event)
        side_stream_work(model, o, (E, order32, rank, level, work, level_off, n_levels) + (() if dep is None else (dep,)), enqueue)()
    return SamplePlan(E, order32, rank, level=level, work=work, nwork=B_dec * L, level_off=level_off, levels=n_levels[0])


def pairs_plan(model, pair_list, o, E_idx, dims):
    """The plan of a base-paired design (every group a pair, one complex) on the device, nothing read back: the host's part uploaded (partner,
    listed-first flag, weights), the device's part ONE allocation.  -> (plan, start); start() enqueues on the side stream the visit order of every
    stream (namp_pairs_plan), the groups' levels (namp_sample_levels_dep) and the level-sorted work lists, pairs as whole items (namp_pairs_work_lists)."""
    (B_dec, _, L, K), Lb, dev = dims, hip.lib(), E_idx.device
    partner, first, w = [-1] * L, [0] * L, [1.0] * L
    for i, j, wi, wj, _ in pair_list:
        partner[i], partner[j], first[i], w[i], w[j] = j, i, 1, wi, wj
    pf = torch.tensor([partner, first], dtype=torch.int32).to(dev)
    sym_w = torch.tensor(w, dtype=torch.float32).to(dev)
    n = B_dec * L
    buf, (order, rank, group_first, group_last, level, work, work_n, level_off, n_levels) = carve_i32((n, n, n, n, n, 2 * n, n, L + 2, 1), dev)
    order, rank, group_first, group_last, level = (t.view(B_dec, L) for t in (order, rank, group_first, group_last, level))
    def enqueue(s_):
        hip.check(Lb.namp_pairs_plan(pf[0].data_ptr(), pf[1].data_ptr(), o.order32.data_ptr(), o.rank.data_ptr(), order.data_ptr(),
                                     rank.data_ptr(), group_first.data_ptr(), group_last.data_ptr(), B_dec, L, s_), "pairs_plan")
        hip.check(Lb.namp_sample_levels_dep(E_idx.data_ptr(), order.data_ptr(), rank.data_ptr(), None, 0, group_first.data_ptr(),
                                            group_last.data_ptr(), level.data_ptr(), B_dec, 1, L, K, s_), "sample_levels")
        hip.check(Lb.namp_pairs_work_lists(level.data_ptr(), group_first.data_ptr(), work.data_ptr(), work_n.data_ptr(),
                                           level_off.data_ptr(), n_levels.data_ptr(), B_dec, L, s_), "pairs_work_lists")
    plan = SamplePlan(E_idx, order, rank, group_first, group_last, sym_w, level, work.view(n, 2), work_n, n - B_dec * len(pair_list), level_off, n_levels[0])
    return plan, side_stream_work(model, o, (E_idx, o.order32, o.rank, pf, buf), enqueue)


def states_plan(model, w, o, E_idx, dims):
    """The plan of one sequence tied across M states (weights w) on the flattened graph of N = M * L residues in ONE launch
    (namp_states_plan): the flattened neighbour lists, the visit plan of every stream, the levels, the level-sorted lists and the
    deferred draws; its walk over the L steps is serial.  dims = (bs, M, L, K).  -> (plan, start) as pairs_plan."""
    (bs, M, L, K), Lb, dev = dims, hip.lib(), E_idx.device
    N = M * L
    buf, (E_f, sym_w, work_n, level, order_f, rank_f, group_first, group_last, work, level_off, n_levels, close, close_off) = carve_i32(
        (N * K, N, bs * N, L, bs * N, bs * N, bs * N, bs * N, 2 * bs * N, N + 2, 1, 2 * bs * L, N + 2), dev)
    sym_w, wt = sym_w.view(torch.float32), torch.tensor(w, dtype=torch.float32).to(dev)
    def enqueue(s_):
        hip.check(Lb.namp_states_plan(E_idx.data_ptr(), o.order32.data_ptr(), o.rank.data_ptr(), wt.data_ptr(), E_f.data_ptr(),
                                      order_f.data_ptr(), rank_f.data_ptr(), group_first.data_ptr(), group_last.data_ptr(),
                                      sym_w.data_ptr(), work_n.data_ptr(), level.data_ptr(), work.data_ptr(), level_off.data_ptr(),
                                      n_levels.data_ptr(), close.data_ptr(), close_off.data_ptr(), bs, M, L, K, s_), "states_plan")
    plan = SamplePlan(E_f, order_f, rank_f, group_first, group_last, sym_w, level, work, work_n, bs * N, level_off, n_levels[0], close, close_off)
    return plan, side_stream_work(model, o, (E_idx, o.order32, o.rank, wt, buf), enqueue)


def host_plan(model, groups, weights, order, rank, E, dims, deps, walk, split, steps=False):
    """The plan through the host, in the calling stream: the visits of the groups (symmetry_visits along order[0], read back: ONE order for every
    stream; groups None: no ties, order / rank [B_dec, n] as given), the levels (namp_sample_levels_dep; deps = (dep_idx, n_dep) or (None, 0);
    deps None: the sequential walk reads neither levels nor work lists), the level-sorted work lists (level_work_lists with `split`) and, for the
    walk, where every level starts.  E: the neighbour lists the decoder sees, int32, contiguous, [.., n, K]; dims = (B_dec, B_enc, n, K)."""
    (B_dec, B_enc, n, K), dev = dims, E.device
    group_first = group_last = sym_w = step_of = None
    if groups is not None:
        visits, gf, gl, wl = symmetry_visits(groups, weights, order[0].tolist(), n)
        order = torch.tensor(visits, device=dev).repeat(B_dec, 1)
        group_first = torch.tensor(gf, dtype=torch.int32, device=dev).repeat(B_dec, 1).contiguous()
        group_last = torch.tensor(gl, dtype=torch.int32, device=dev).repeat(B_dec, 1).contiguous()
        sym_w = torch.tensor(wl, dtype=torch.float32).to(dev)
        rank = model.ranks_of(order)
        if steps:
            step_of = torch.tensor(np.cumsum([int(v == f) for v, f in enumerate(gf)]) - 1, device=dev)
    order, rank = _i32(order), _i32(rank)
    if deps is None:
        return SamplePlan(E, order, rank, group_first, group_last, sym_w)
    # residue i depends only on the neighbours decoded before it -> decode by dependency level (one launch per level over all
    # streams, ~64 levels at L = 1000 instead of 1000 sequential steps).  Symmetry-tied: the unit of work is a GROUP (its members
    # run one after the other in the group's workgroup slot and share one draw); its level follows its members' dependencies
    level = torch.empty(B_dec, n, dtype=torch.int32, device=dev)
    hip.check(hip.lib().namp_sample_levels_dep(E.data_ptr(), order.data_ptr(), rank.data_ptr(), hip.ptr(deps[0]), deps[1], hip.ptr(group_first),
                                               hip.ptr(group_last), level.data_ptr(), B_dec, B_enc, n, K, hip.current_stream()), "sample_levels")
    sel, flat, work_n, close, close_off = level_work_lists(level, group_first, group_last, order[0], E.view(-1, n, K)[0].long(), split=split)
    work = torch.stack((sel // n, sel % n), 1).to(torch.int32).contiguous()
    level_off = levels = None
    if walk:    # the level histogram stays on the device (levels < n, so n + 2 offsets; everything behind the last level equals nwork)
        hist = torch.zeros(n + 1, dtype=torch.int64, device=dev).scatter_add_(0, flat, torch.ones_like(flat))
        level_off = torch.cat((hist.new_zeros(1), hist.cumsum(0))).to(torch.int32).contiguous()
        levels = (hist > 0).sum()
    return SamplePlan(E, order, rank, group_first, group_last, sym_w, level, work, work_n, int(sel.numel()), level_off, levels, close, close_off, step_of, flat)


def launch(model, plan, arrays, maps, pterms, temperature, dims, walk):
    """One sampler call: namp_decoder_sample (a plan without work lists: the sequential walk), namp_decoder_sample_walk (`walk`: one persistent
    launch walking the levels, nothing read back, the call returns with the whole design enqueued) or namp_decoder_sample_levels (one launch per
    level; counting them is its one host sync).  maps = (tok_maps, n_maps, classes) as _attach_maps takes them and pterms (the dict of
    _pair_terms_section — pair terms, forbidden motifs or both —, whose workspace the call then uses; or None) are attached to THIS call of the thread.  dims = (B_dec, B_enc, n, K).
    -> (S int32 [B_dec, n], sampling_probs, log_probs [B_dec, n, V], levels: None, the plan's device scalar or the count of launches), code: the
    walk's barrier status (its words are left in model._walk_sync) if model.sample_check_walk, else 0; non-zero: decode again with walk=False."""
    (B_dec, B_enc, n, K), Lb, dev, V, a = dims, hip.lib(), plan.E.device, model.num_letters, arrays
    special = 0
    for name in ("UNK", "DX", "RX", "MAS", "PAD"):                        # never drawn (model_utils.py:199-203)
        special |= 1 << int(model.restype_to_int[name])
    W = model._weights()
    S_out, probs = torch.empty(B_dec, n, dtype=torch.int32, device=dev), torch.empty(B_dec, n, V, device=dev)
    logp = torch.empty_like(probs)
    ws_bytes = Lb.namp_sample_workspace_bytes_n(B_enc, B_dec, n, K, len(model.decoder_layers))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if pterms is None else pterms["ws"]      # (the section behind the carve)
    common = (W.model(), a.h_V.data_ptr(), a.h_E.data_ptr(), plan.E.data_ptr(), a.mask.data_ptr(), a.mask_dec.data_ptr(),
              a.chain_mask.data_ptr(), a.S.data_ptr(), a.bias.data_ptr(), plan.order.data_ptr(), plan.rank.data_ptr(), a.uniform.data_ptr(),
              hip.ptr(a.forced), hip.ptr(plan.group_first), hip.ptr(plan.group_last), hip.ptr(plan.sym_w), hip.ptr(a.pair_bias))
    tail = (float(temperature), special, S_out.data_ptr(), probs.data_ptr(), logp.data_ptr(), ws.data_ptr(), ws.numel(),
            B_dec, B_enc, n, K, hip.current_stream())
    model._attach_maps(*maps)
    if pterms is not None and pterms["D"]:
        hip.check(Lb.namp_sample_pair_terms(pterms["D"], pterms["n_tables"], pterms["members"]), "sample_pair_terms")
    if pterms is not None and pterms["motifs"] is not None:
        hip.check(Lb.namp_sample_motifs(*pterms["motifs"]), "sample_motifs")
    levels, code = plan.levels, 0
    if plan.work is None:
        hip.check(Lb.namp_decoder_sample(*common, *tail), "decoder_sample")     # (no host sync: temporaries are stream-ordered, see _featurize_hip)
    elif not walk:
        counts = torch.bincount(plan.item_level).cpu().tolist()
        hip.check(Lb.namp_decoder_sample_levels(*common, plan.work.data_ptr(), hip.ptr(plan.work_n), (C.c_int32 * len(counts))(*counts),
                                                len(counts), *tail), "decoder_sample_levels")
        levels = len(counts)
    else:
        zbuf = torch.empty(B_dec, n, V, device=dev) if plan.close is not None else None
        hip.check(Lb.namp_decoder_sample_walk(*common, plan.work.data_ptr(), hip.ptr(plan.work_n), plan.nwork, plan.level_off.data_ptr(),
                                              hip.ptr(plan.close), hip.ptr(plan.close_off), hip.ptr(zbuf), *tail), "decoder_sample_walk")
        # the 64 barrier words, copied out of the per-call workspace (a view would keep the whole workspace alive on the model)
        model._walk_sync = ws[ws_bytes - 4096:][:256].view(torch.int32).clone()
        code = model.sample_walk_status() if model.sample_check_walk else 0
    return (S_out, probs, logp, levels), code
