"""Drop-in ``ProteinMPNN`` for NA-MPNN on MI355X.

Mirrors the reference module surface — constructor keywords, ``state_dict`` key set and the
``feature_dict`` methods ``encode / score / unconditional_probs / sample / forward``
(/root/reference/inference/model_utils.py:8-424 and /root/reference/na_model_utils.py:519-646) —
while every encoder/decoder op runs in hand-written HIP kernels reached through the C ABI of
``libnamp_hip.so`` (include/namp.h).  The ``nn.Linear`` / ``nn.LayerNorm`` / ``nn.Embedding``
children are parameter containers only (they give the reference's key names and initialisers);
their ``forward`` is never called on the hot path.

There is no CPU path: tensors must live on a HIP device and the extension must be built,
otherwise a RuntimeError is raised.
"""
from __future__ import annotations

import collections
import sys
import warnings
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import hip, sampling, spec
from .pack import PackedWeights
from .sampling import _i32, level_work_lists, symmetry_visits          # (the two host routines: imported from here by tests and tools)

H = spec.H


# --------------------------------------------------------------------------------------------
# parameter containers (names = reference state_dict keys)
# --------------------------------------------------------------------------------------------
class _FFN(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.W_in = nn.Linear(h, 4 * h, bias=True)
        self.W_out = nn.Linear(4 * h, h, bias=True)


class _EncLayerParams(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(h), nn.LayerNorm(h), nn.LayerNorm(h)
        self.W1, self.W2, self.W3 = nn.Linear(3 * h, h), nn.Linear(h, h), nn.Linear(h, h)
        self.W11, self.W12, self.W13 = nn.Linear(3 * h, h), nn.Linear(h, h), nn.Linear(h, h)
        self.dense = _FFN(h)


class _DecLayerParams(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(h), nn.LayerNorm(h)
        self.W1, self.W2, self.W3 = nn.Linear(4 * h, h), nn.Linear(h, h), nn.Linear(h, h)
        self.dense = _FFN(h)


class _PosEmb(nn.Module):
    def __init__(self, n_emb, max_rel):
        super().__init__()
        self.linear = nn.Linear(2 * max_rel + 2, n_emb)


class _FeatureParams(nn.Module):
    def __init__(self, edge_features, node_features, n_polytypes, n_atoms_aug):
        super().__init__()
        self.embeddings = _PosEmb(spec.NUM_POS, spec.MAX_REL)
        self.node_embedding = nn.Linear(n_polytypes, node_features, bias=False)
        self.norm_nodes = nn.LayerNorm(node_features)
        self.edge_embedding = nn.Linear(spec.NUM_POS + spec.NUM_RBF * n_atoms_aug * n_atoms_aug, edge_features, bias=False)
        self.norm_edges = nn.LayerNorm(edge_features)


def _require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"na_mpnn_amd: '{what}' is on {t.device}; this implementation runs only on a HIP device "
                           "(no CPU fallback — use the reference or oracle/cpu_ref.py for CPU checks)")


def _section_bytes(elems):
    """The bytes one array of elems (+ 1) four-byte entries takes in a workspace section: rounded to 256 (include/namp.h)."""
    return (4 * (elems + 1) + 255) & ~255


def output_section_layout(family, dims):
    """The arrays of the OUTPUT SECTION of an attached namp_decoder_fwd call, in the order include/namp.h lists (and the library
    carves) them -> [(name, elems, dtype), ...]; needs no device.  family: "library", "mutations", "state_mutations", "group_mutations", "class_mutations" or "tied_score";
    dims: the ints of the family's size functions.  The 64-word header of "library" / "tied_score" is carved as it stands: 63 (+ 1)."""
    i32, f32 = torch.int32, torch.float32
    if family == "library":
        N, n_chunk = dims[0], dims[4]
        return [("counts", 63, i32), ("token_log_probs", n_chunk * N, f32)]
    if family == "tied_score":
        N, n_chunk = dims[0], dims[5]
        return [("header", 63, i32), ("unit_log_probs", n_chunk * N, f32), ("member_log_probs", n_chunk * N, f32)]
    at = {"mutations": 3, "state_mutations": 4, "group_mutations": 3, "class_mutations": 5}     # where n_sites stands (behind n_dec and the family's own ints)
    if family in at:                                                # one scan: a base list, and the tails of the family
        q, N, M = at[family], dims[0], dims[3] if family == "state_mutations" else 1
        ns, nv, rows3 = dims[q], dims[q + 1], dims[q + 7]
        head = [("site_rows", 3 * ns, i32), ("delta", nv, f32)]
        rows = [("row_residue", rows3, i32), ("row_token_log_prob", rows3, f32)]
        units = [("unit_residue", rows3, i32), ("unit_log_prob", rows3, f32), ("base_units", N // M, f32)]
        if family == "mutations":
            return head + rows
        if family == "state_mutations":
            return head + [("state_delta", nv * M, f32)] + rows + units
        return head + rows + units + [("header", 63, i32)]
    raise ValueError(f"no output section is described for {family!r}")


def _read_sections(ws, out_offset, layout):
    """The arrays of output_section_layout as views of the workspace -> {name: view [elems]} (clone what must outlive the workspace's
    next use)."""
    views = {}
    for name, elems, dtype in layout:
        views[name] = ws[out_offset:out_offset + 4 * elems].view(dtype)
        out_offset += _section_bytes(elems)
    return views


def _positions_argument(positions, L):
    """The `positions` of score_sequences() / score_mutations(), checked -> a host list of ints."""
    p = torch.as_tensor(positions)
    if p.dim() != 1 or p.dtype.is_floating_point or p.dtype == torch.bool:
        raise ValueError("positions must be a one-dimensional integer tensor")
    pos = [int(v) for v in p.tolist()]
    if any(v < 0 or v >= L for v in pos):
        raise ValueError(f"positions must lie in [0, {L})")
    if any(b <= a for a, b in zip(pos, pos[1:])):
        raise ValueError("positions must be ascending and unique")
    return pos


def _require_one_complex(fd, who, states_note):
    """One input complex; states_note: what state_weights would mean for `who`, where it does not take them (else None)."""
    S = fd["S"]
    if S.dim() != 2 or S.shape[0] != 1:
        raise ValueError(f"{who} expects one input complex (B == 1); got S of shape {tuple(S.shape)}")
    if states_note is not None and fd.get("state_weights") is not None:
        raise NotImplementedError(f"{who} does not take state_weights ({states_note})")


def _listed(v):
    """Whether a tie list of a feature_dict names anything (None, [] and [[]] do not)."""
    return v is not None and len(v) > 0 and not (len(v) == 1 and hasattr(v[0], "__len__") and len(v[0]) == 0)


def _counted_weights(fd):
    """w = mask * chain_mask of the one complex as a host list [L]."""
    return [a * b for a, b in zip(fd["mask"][0].reshape(-1).tolist(), fd["chain_mask"][0].reshape(-1).tolist())]


def _require_counted(st, w):
    """Every residue the sites st name is counted (w != 0): the tied scans are differences of score_tied(), which edits no other."""
    for r in sorted({int(r) for r in st.reshape(-1) if r >= 0}):
        if w[r] == 0:
            raise ValueError(f"residue {r} has mask * chain_mask == 0: score_tied would not apply an edit there")


def _variant_library(S_true, st, tk, base_row=None):
    """The explicit library of a scan's dense route -> int64 [n (+ 1), L]: per variant S with the tokens tk[v, 1:] at the residues of
    its site st[tk[v, 0]] (padding -1 skipped); S itself in front of them (base_row "first"), behind them ("last") or absent (None)."""
    n, L, dev = len(tk), S_true.shape[1], S_true.device
    S_full = S_true.long().expand(n + (base_row is not None), L).clone()
    res = st[tk[:, 0]].reshape(-1)
    keep = res >= 0
    vi = torch.from_numpy((base_row == "first") + np.repeat(np.arange(n), st.shape[1])[keep]).to(dev)
    S_full[vi, torch.from_numpy(res[keep]).to(dev)] = torch.from_numpy(tk[:, 1:].reshape(-1)[keep]).to(dev)
    return S_full


def _scan_head(st, tk, dev, **own):
    """What every route of score_mutations() reports of its arguments, and the `own` keys of the route."""
    return {"site_index": torch.from_numpy(tk[:, 0].copy()).to(dev), "sites": torch.from_numpy(st).to(dev),
            "site_tokens": torch.from_numpy(tk).to(dev), "site_rows": None, **own}


def _empty_rows(dev):
    """No variants -> (delta [0], row_offsets [1], row_residue [0], row_token_log_prob [0]); the sparse units have the same shapes."""
    return (torch.zeros(0, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
            torch.zeros(0, device=dev))


def _sparse_units(got, n, L):
    """The sparse units of a cone scan: the leader rows of _cone_scan's "unit_residue" / "unit_log_prob", per variant ascending in the
    unit's residue -> (unit_offsets int64 [n + 1], unit_residue, unit_log_prob)."""
    ures, ulp = got["unit_residue"], got["unit_log_prob"]
    vid = torch.repeat_interleave(torch.arange(n), got["row_counts"]).to(ures.device)
    lead = ures >= 0
    srt = torch.argsort(vid[lead] * L + ures[lead].long(), stable=True)
    uoffs = torch.cat((torch.zeros(1, dtype=torch.int64, device=ures.device), torch.bincount(vid[lead], minlength=n).cumsum(0)))
    return uoffs, ures[lead][srt], ulp[lead][srt]


def tied_stream_keys(rank0, groups):
    """The keys of the forced tied stream (score_tied): rank0 [N] the ranks of score()'s order, groups the tied groups
    (lists of residues in LISTED order, disjoint) -> (key [N], leader [N]) as lists: key(i) = (min of rank0 over i's group) << 4 |
    listed position of i (an ungrouped residue: rank0[i] << 4), leader(i) = the listed-first member of i's group (i itself when
    ungrouped).  Sorting the residues by key gives the visits of symmetry_visits; an edge i <- j is forward when key(j) >= key(i),
    hidden-backward when key(j) < key(i) and leader(j) == leader(i), backward otherwise."""
    rank0 = [int(r) for r in rank0]
    key, leader = [r << 4 for r in rank0], list(range(len(rank0)))
    for g in groups:
        mn = min(rank0[int(r)] for r in g)
        for t, r in enumerate(g):
            key[int(r)], leader[int(r)] = (mn << 4) | t, int(g[0])
    return key, leader


def mapped_groups(L, restype_to_int, pairs=None, pair_weights=None, polymer=None, fixed=None, groups=None, weights=None, maps=None,
                  wobble=None, wobble_bias=None):
    """Groups of mapped symmetry-tied sampling — base pairs (feature_dict["paired_residues"]) and explicit token maps
    (feature_dict["symmetry_token_maps"]) — as plain lists; needs no device.

    Member j of a mapped group carries a token map P_j, an involution of the vocabulary that fixes the special tokens: for the group's
    token a the member receives P_j[a], and the group's logit sum reads its logits through P_j.  pairs [(i, j), ...] ties residue j to
    the Watson-Crick complement of residue i (spec.WC_SAME for two residues of one polymer type, spec.WC_CROSS for DNA with RNA;
    polymer [L]: 1 DNA, 2 RNA, anything else is refused); pair_weights (w_i, w_j) or one such tuple per pair, default (1, 1).  A member
    that is fixed (fixed [L] true) is listed first, so that its partner receives the complement of its token.  groups / weights / maps:
    symmetry_residues, symmetry_weights and symmetry_token_maps (per group None or a list with None or a [vocab] map per member).  A
    pair whose members sit in symmetry groups joins the two groups: the members of i's group first, the weights of each side multiplied
    by the pair's weight of that side, the maps of j's side composed with the pair's map.
    Returns (groups, weights, maps, pair_list): lists parallel to each other, every map a list of vocab ids; pair_list = the pairs as
    (first listed, second listed, w_first, w_second, kind) when the pairs are ALL there is (else None).  ValueError on a residue in two
    pairs, paired with itself, outside [0, L) or not a nucleic acid, and on a map that is not an involution or moves a special token.

    wobble (None: as above; a bool, or one per pair): the call speaks in PAIR CLASSES (spec.class_table) — a pair that asks for wobble
    and has an RNA member may also hold G-U / U-G (classes spec.CLASS_GU / CLASS_UG: the first listed member's G with the second's U / T,
    and the reverse), with wobble_bias (a float, or one per pair; default 0) added to the totals of those two classes.  Returns
    (groups, weights, tables, pair_list, class_bias) then: per member a table of spec.N_CLASS_LANES ids (-1: no such class; a pair
    without wobble and every other group: its map, -1 beyond the vocabulary), per group the N_CLASS_LANES biases of its classes.
    ValueError on a wobble pair with a member in a symmetry_residues group (tables that are no maps do not compose)."""
    V = len(spec.RESTYPES)
    ident = list(range(V))
    out, group_of = [], {}                                   # out: [members, weights, maps] or None once merged away
    plain = groups is None or (len(groups) == 1 and len(groups[0]) == 0)
    if maps is not None and (plain or len(maps) != len(groups)):
        raise ValueError("symmetry_token_maps must be parallel to symmetry_residues")
    if not plain:
        for gi, g in enumerate(groups):
            gm = maps[gi] if maps is not None else None
            if gm is not None and len(gm) != len(g):
                raise ValueError(f"symmetry_token_maps[{gi}] has {len(gm)} entries for the {len(g)} residues of its group")
            ms = []
            for k, r in enumerate(g):
                if not 0 <= int(r) < L:
                    raise ValueError(f"symmetry_residues: residue {int(r)} is outside [0, {L})")
                m = None if gm is None else gm[k]
                if m is not None:
                    m = m.tolist() if hasattr(m, "tolist") else list(m)
                    m = spec.check_token_map(restype_to_int, m, f"symmetry_token_maps[{gi}][{k}]")
                ms.append(ident if m is None else m)
                group_of.setdefault(int(r), gi)
            out.append([[int(r) for r in g], [float(v) for v in weights[gi]], ms])
    pair_list = [] if plain else None
    paired = set()
    per_pair = lambda v, n, default: default if v is None else (v[n] if hasattr(v, "__len__") else v)
    wobbling = {}                                            # (first listed, second listed) -> (kind of spec.PAIR_KINDS, bias)
    for n, pr in enumerate(pairs or []):
        i, j = int(pr[0]), int(pr[1])
        pw = (1.0, 1.0) if pair_weights is None else pair_weights
        if len(pw) and hasattr(pw[0], "__len__"):
            pw = pw[n]
        wi, wj = float(pw[0]), float(pw[1])
        for r in (i, j):
            if not 0 <= r < L:
                raise ValueError(f"paired_residues: residue {r} is outside [0, {L})")
        if i == j:
            raise ValueError(f"paired_residues: residue {i} is paired with itself")
        for r in (i, j):
            if r in paired:
                raise ValueError(f"paired_residues: residue {r} is in two pairs")
            if polymer is not None and int(polymer[r]) not in (1, 2):
                raise ValueError(f"paired_residues: residue {r} is not a nucleic acid (protein residues cannot be base-paired)")
        paired.update((i, j))
        if fixed is not None and bool(fixed[j]) and not bool(fixed[i]):
            i, j, wi, wj = j, i, wj, wi
        kind = "same" if polymer is None or int(polymer[i]) == int(polymer[j]) else "cross"
        P = spec.token_map(restype_to_int, kind)
        if pair_list is not None:
            pair_list.append((i, j, wi, wj, kind))
        if wobble is not None and bool(per_pair(wobble, n, False)):
            if polymer is None:
                raise ValueError("paired_wobble needs the polymer type of the paired residues")
            for r in (i, j):
                if r in group_of:
                    raise ValueError(f"paired_wobble: residue {r} of the wobble pair ({i}, {j}) sits in a symmetry_residues group; "
                                     "wobble pairs do not join symmetry groups")
            names = {1: "dna", 2: "rna"}
            if 2 in (int(polymer[i]), int(polymer[j])):                         # (a DNA-DNA pair never wobbles)
                wobbling[(i, j)] = (f"{names[int(polymer[i])]}-{names[int(polymer[j])]}", float(per_pair(wobble_bias, n, 0.0)))
        for r in (i, j):
            if r not in group_of:
                group_of[r] = len(out)
                out.append([[r], [1.0], [ident]])
        gi, gj = group_of[i], group_of[j]
        if gi == gj:
            raise ValueError(f"paired_residues: residues {i} and {j} are already tied to each other by symmetry_residues")
        A, Bm = out[gi], out[gj]
        Pi, Pj = A[2][A[0].index(i)], Bm[2][Bm[0].index(j)]
        A[1] = [w * wi for w in A[1]]
        for r, w, Pk in zip(*Bm):
            if group_of.get(r) != gj:                      # (listed in an earlier group as well: it belongs to that one)
                continue
            A[0].append(r); A[1].append(w * wj); A[2].append([Pk[Pj[P[Pi[a]]]] for a in ident])
            group_of[r] = gi
        out[gj] = None
    out = [g for g in out if g is not None]
    for g in out:
        for r, m in zip(g[0], g[2]):
            spec.check_token_map(restype_to_int, m, f"the token map of residue {r}")
    if wobble is None:
        return [g[0] for g in out], [g[1] for g in out], [g[2] for g in out], pair_list
    # (a design has a few distinct tables for hundreds of pairs: each is built and checked once, and shared)
    tables, class_bias, made, biases = [], [], {}, {}

    def table(key, make, r):
        t = made.get(key)
        if t is None:
            t = spec.check_class_table(restype_to_int, make(), f"the class table of residue {r}")
            t = made[key] = (t, tuple(c >= 0 for c in t))
        return t
    for g in out:
        kind, b = wobbling.get(tuple(g[0]), (None, 0.0))
        if kind is None:
            ts = [table(tuple(m), lambda m=m: list(m) + [-1] * (spec.N_CLASS_LANES - V), r) for r, m in zip(g[0], g[2])]
        else:
            ts = [table((kind, first), lambda first=first: spec.class_table(restype_to_int, kind, True, first), r)
                  for r, first in zip(g[0], (True, False))]
        if any(t[1] is not ts[0][1] and t[1] != ts[0][1] for t in ts):          # (the sampler reads a group's classes from its closing member)
            raise ValueError(f"the members of group {g[0]} do not have tokens for the same pair classes")
        if b not in biases:
            biases[b] = [0.0] * spec.N_CLASS_LANES
            if kind is not None:
                biases[b][spec.CLASS_GU] = biases[b][spec.CLASS_UG] = b
        tables.append([t[0] for t in ts]); class_bias.append(biases[b])       # (b is 0 for a group that is no wobble pair)
    return [g[0] for g in out], [g[1] for g in out], tables, pair_list, class_bias


def pair_bias_dependencies(pair_bias, max_deps=64):
    """Extra dependencies of the sampler's levels from pair_bias [B, L, A, L, A] (model_utils.py:116,169-172): the bias of residue i
    reads the token of every residue j whose block pair_bias[:, i, :, j, :] is not all zero — the sequence neighbours for run.py's
    --pair_bias_AA (data_utils.py:7-16).  A non-finite entry counts as a dependency.  Returns (dep_idx, n_dep): n_dep = the most partners
    of any residue, dep_idx [B, L, n_dep] int32 their indices padded with -1 (None when n_dep == 0); None when some residue has more than
    `max_deps` partners (namp_sample_levels_dep's limit: a dense bias keeps the sequential walk)."""
    B, L, A = pair_bias.shape[:3]
    dev = pair_bias.device
    # (row block by row block: one amax over the whole [B, L, 33, L, 33] tensor would materialise a second copy of it — 4.4 GB at L = 1000)
    nz = torch.empty(B, L, L, dtype=torch.bool, device=dev)
    step = max(1, (1 << 26) // max(1, A * L * A))
    for i0 in range(0, L, step):
        blk = pair_bias[:, i0:i0 + step]
        nz[:, i0:i0 + step] = ((blk != 0) | ~torch.isfinite(blk)).any(dim=4).any(dim=2)
    n_dep = int(nz.sum(-1).max())
    if n_dep > max_deps:
        return None
    if n_dep == 0:
        return None, 0
    cols = torch.where(nz, torch.arange(L, device=dev)[None, None, :], torch.full((), L, device=dev))
    cols = cols.sort(dim=-1).values[:, :, :n_dep]
    return torch.where(cols < L, cols, torch.full((), -1, device=dev)).to(torch.int32).contiguous(), n_dep


PAIR_TERMS_MAX_SLOTS, PAIR_TERMS_MAX_TABLES = 64, 256          # namp_sample_pair_terms' limits (D: namp_sample_levels_dep's)


def pair_terms_arguments(pair_terms, B, L, V):
    """feature_dict["pair_terms"] checked on the host -> (partner int32 [B, L, D], table int32 [B, L, D], tables float32 [n, V, V], all
    contiguous on the CPU, members: 0 "closing" / 1 "all").  The compact form of pair_bias: residue i reads partner[b, i, d] (-1: none)
    through tables[table[b, i, d]], term(i)[a] = sum_d tables[table][a][token of the partner] (include/namp.h)."""
    if not isinstance(pair_terms, dict) or not {"partner", "table", "tables"} <= set(pair_terms):
        raise ValueError("pair_terms must be a dict with 'partner', 'table', 'tables' (and 'members')")
    members = pair_terms.get("members", "closing")
    if members not in ("closing", "all"):
        raise ValueError(f"pair_terms['members'] must be 'closing' or 'all'; got {members!r}")
    partner, table, tables = (torch.as_tensor(pair_terms[k]).detach().cpu() for k in ("partner", "table", "tables"))
    if partner.dim() != 3 or tuple(partner.shape[:2]) != (B, L) or tuple(table.shape) != tuple(partner.shape):
        raise ValueError(f"pair_terms['partner'] / ['table'] must both be [{B}, {L}, D]; got {tuple(partner.shape)} / {tuple(table.shape)}")
    if partner.dtype.is_floating_point or table.dtype.is_floating_point or partner.dtype == torch.bool or table.dtype == torch.bool:
        raise ValueError("pair_terms['partner'] / ['table'] must be integer tensors")
    D = partner.shape[2]
    if not 1 <= D <= PAIR_TERMS_MAX_SLOTS:
        raise ValueError(f"pair_terms has D = {D} slots per residue; 1 <= D <= {PAIR_TERMS_MAX_SLOTS}")
    if tables.dim() != 3 or tuple(tables.shape[1:]) != (V, V):
        raise ValueError(f"pair_terms['tables'] must be [n_tables, {V}, {V}]; got {tuple(tables.shape)}")
    if not 1 <= tables.shape[0] <= PAIR_TERMS_MAX_TABLES:
        raise ValueError(f"pair_terms has {tables.shape[0]} tables; 1 <= n_tables <= {PAIR_TERMS_MAX_TABLES}")
    return (partner.to(torch.int32).contiguous(), table.to(torch.int32).contiguous(), tables.to(torch.float32).contiguous(),
            int(members == "all"))


def sort_pair_slots(partner, table):
    """The slots of every residue in the order the kernels sum them: by partner index, stable, absent slots (a partner outside [0, L) or
    the residue itself) last and set to -1.  partner / table [..., L, D] on any device -> (partner, table), new tensors."""
    L = partner.shape[-2]
    own = torch.arange(L, device=partner.device).view(L, 1)
    key = torch.where((partner < 0) | (partner >= L) | (partner == own), torch.full((), L, device=partner.device, dtype=partner.dtype), partner)
    key, perm = torch.sort(key, dim=-1, stable=True)
    return torch.where(key >= L, torch.full_like(key, -1), key), table.gather(-1, perm)


def pair_terms_dense(pair_terms, L):
    """The dense pair_bias [B, L, V, L, V] that feature_dict["pair_terms"] stands for: pair_bias[b, i, a, j, b'] = the sum over the slots d of
    residue i with partner j of tables[table[b, i, d]][a][b'] (slots of one partner summed in sorted slot order).  For tests and small L."""
    tables = torch.as_tensor(pair_terms["tables"]).detach().cpu().float()
    V = tables.shape[-1]
    partner, table = torch.as_tensor(pair_terms["partner"]).detach().cpu().long(), torch.as_tensor(pair_terms["table"]).detach().cpu().long()
    partner, table = sort_pair_slots(partner, table)
    B, _, D = partner.shape
    out = torch.zeros(B, L, V, L, V)
    for b in range(B):
        for i in range(L):
            for d in range(D):
                j = int(partner[b, i, d])
                if j >= 0:
                    out[b, i, :, j, :] += tables[max(0, min(len(tables) - 1, int(table[b, i, d])))]      # (clamped, as on the device)
    return out


MOTIF_MIN_LEN, MOTIF_MAX_LEN, MOTIF_MAX_COUNT = 2, 8, 63       # namp_sample_motifs' limits: 63 motifs x 8 alignments = 504 entries


def forbidden_motifs_arguments(motifs, V, special=(), B=1, tied=False, pair_bias=False):
    """feature_dict["forbidden_motifs"] checked on the host (needs no device) -> a list of token tuples.  `motifs`: a list of token
    sequences, or an int tensor [n, Lm] whose rows are padded with -1.  Refused: a token outside [0, V), a special token (`special`: they
    are never drawn, and PAD stands for "not decoded yet"), a length outside 2..8, more than 63 motifs, the dense pair_bias beside
    motifs, and several complexes (B != 1) with ties."""
    if pair_bias:
        raise ValueError("forbidden_motifs do not go with the dense pair_bias: give the pair bias as pair_terms")
    if tied and B != 1:
        raise ValueError(f"forbidden_motifs with ties expect one input complex (B == 1); got B = {B}")
    if torch.is_tensor(motifs):
        if motifs.dim() != 2 or motifs.dtype.is_floating_point or motifs.dtype == torch.bool:
            raise ValueError(f"forbidden_motifs as a tensor must be an integer tensor [n, Lm] padded with -1; got {motifs.dtype} {tuple(motifs.shape)}")
        rows = []
        for row in motifs.detach().cpu().tolist():
            n = len(row)
            while n and row[n - 1] == -1:
                n -= 1
            rows.append(row[:n])
        motifs = rows
    elif not isinstance(motifs, (list, tuple)):
        raise ValueError(f"forbidden_motifs must be a list of token tuples or an int tensor [n, Lm]; got {type(motifs).__name__}")
    out, bad = [], {int(t) for t in special}
    for m in motifs:
        if torch.is_tensor(m):
            m = m.detach().cpu().tolist()
        if not isinstance(m, (list, tuple)) or any(isinstance(t, (float, bool, str)) for t in m):
            raise ValueError(f"forbidden_motifs: a motif is a sequence of integer tokens; got {m!r}")
        m = tuple(int(t) for t in m)
        if not MOTIF_MIN_LEN <= len(m) <= MOTIF_MAX_LEN:
            raise ValueError(f"forbidden_motifs: a motif has {MOTIF_MIN_LEN}..{MOTIF_MAX_LEN} tokens; got {len(m)} in {m}")
        if any(not 0 <= t < min(V, 62) for t in m):
            raise ValueError(f"forbidden_motifs: tokens must lie in [0, {min(V, 62)}); got {m}")
        if any(t in bad for t in m):
            raise ValueError(f"forbidden_motifs: {m} holds a special token (never drawn; PAD stands for 'not decoded yet')")
        out.append(m)
    if len(out) > MOTIF_MAX_COUNT:
        raise ValueError(f"forbidden_motifs: {len(out)} motifs; at most {MOTIF_MAX_COUNT}")
    return out


def motif_adjacency(chain_labels, R_idx, mask):
    """[B, L - 1] bool on the inputs' device: residues i and i + 1 are consecutive on one chain (same chain_labels, R_idx one apart:
    the adjacency of cli.make_pair_terms) and both present (mask)."""
    m = mask != 0
    return ((R_idx[:, 1:] - R_idx[:, :-1]) == 1) & (chain_labels[:, 1:] == chain_labels[:, :-1]) & m[:, 1:] & m[:, :-1]


def motif_windows(chain_labels, R_idx, mask, half_width):
    """The windows of the motif section: int32 [B, L, 2 * half_width], the residue at chain offset -half_width .. -1, +1 .. +half_width of
    every residue, -1 where the run of consecutive present residues (motif_adjacency) ends before it."""
    B, L = mask.shape
    hw = int(half_width)
    adj = motif_adjacency(chain_labels, R_idx, mask)
    win = torch.full((B, L, 2 * hw), -1, dtype=torch.int32, device=mask.device)
    ar = torch.arange(L, dtype=torch.int32, device=mask.device)
    reach = torch.ones(B, L, dtype=torch.bool, device=mask.device)            # reach[i]: i .. i + k are consecutive
    for k in range(1, hw + 1):
        if k >= L:
            break
        reach = reach[:, :L - k] & adj[:, k - 1:]
        win[:, :L - k, hw + k - 1] = torch.where(reach, ar[k:], -1)            # i -> i + k
        win[:, k:, hw - k] = torch.where(reach, ar[:L - k], -1)                # i + k -> i
    return win


def motif_entries(motifs):
    """The packed entries of the motif section: int32 [n_entries, 6] = (pattern[3], mask[3]), one per motif and alignment k (the member
    at position k of the motif).  A window is 15 slots of 6 bits, slot 7 the member, slot 7 + o its chain neighbour at offset o, slot s
    at bit 6 * (s % 5) of word s // 5; token m_q sits in slot 7 - k + q as m_q + 1."""
    rows = []
    for m in motifs:
        for k in range(len(m)):
            pat, msk = [0, 0, 0], [0, 0, 0]
            for q, t in enumerate(m):
                s = 7 - k + q
                pat[s // 5] |= (int(t) + 1) << (6 * (s % 5))
                msk[s // 5] |= 0x3f << (6 * (s % 5))
            rows.append(pat + msk)
    return torch.tensor(rows, dtype=torch.int32).view(-1, 6)


def motif_hits(S, adj, motifs):
    """Occurrences of the motifs in S [R, L] (adj [R, L - 1] bool: motif_adjacency, a row per row of S) -> int64 [R], with stock torch ops
    on the device of S."""
    R, L = S.shape
    hits = torch.zeros(R, dtype=torch.int64, device=S.device)
    for m in motifs:
        n = len(m)
        if n > L:
            continue
        ok = torch.ones(R, L - n + 1, dtype=torch.bool, device=S.device)
        for q, t in enumerate(m):
            ok &= S[:, q:L - n + 1 + q] == t
        for q in range(n - 1):
            ok &= adj[:, q:L - n + 1 + q]
        hits += ok.sum(1)
    return hits


MUT_MAX_EDITS = 8     # NAMP_MUT_MAX_EDITS of include/namp.h: residues per site of score_mutations()

# A scan on the per-site cones as ProteinMPNN._cone_scan drives it: the family riding on namp_decoder_fwd; the carrier's N, K; what
# comes before (n_sites, n_variants, list1..3, items1..3) in the ints of the size functions (dims) and of the attach; the start of the
# "no workspace" message; the padded sites / variants (flat_sites_and_variants); the float tail of the input section (on the device);
# the output arrays (output_section_layout) with one entry per variant {name: trailing shape} and those with one per row of U_3.
_ConeRoute = collections.namedtuple("_ConeRoute", "family N K dims attach what sites8 tok9 weights per_variant per_row")


def mutation_chunks(site_index, site_rows, budget):
    """The chunk cutter of score_mutations(method="cone"); needs no device.  site_index [n]: the site of every variant; site_rows
    [n_sites][3]: |U_1..3(site)|; budget: item rows (all three layers) per decoder call.  -> (perm, cuts): perm the variants in a
    stable order by site (the variants of a site are neighbours and share its plan), cuts [(q0, q1), ...] the chunks as ranges of
    perm.  A chunk closes before the variant that would take its item total past the budget; a variant that exceeds the budget alone
    is a chunk of its own."""
    site_index = [int(s) for s in site_index]
    perm = sorted(range(len(site_index)), key=lambda v: site_index[v])
    cuts, q0, total = [], 0, 0
    for q, v in enumerate(perm):
        rows = sum(int(r) for r in site_rows[site_index[v]])
        if q > q0 and total + rows > budget:
            cuts.append((q0, q))
            q0, total = q, 0
        total += rows
    if len(perm) > q0:
        cuts.append((q0, len(perm)))
    return perm, cuts


def variant_row_order(perm, counts):
    """The sparse rows of score_mutations(method="cone") back into the order the variants were given in; needs no device.  perm [n]:
    the order the variants ran in (mutation_chunks), counts int64 [n]: rows per variant, in the GIVEN order.  -> (offsets int64
    [n + 1] of the given order, idx int64 [sum(counts)] with restored = ran[idx], or None where perm is the identity)."""
    offs = torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0)))
    if np.array_equal(perm, np.arange(len(perm))):
        return offs, None
    pt = torch.as_tensor(np.asarray(perm, np.int64))
    start_sorted = torch.cat((torch.zeros(1, dtype=torch.int64), counts[pt].cumsum(0)))[:-1]
    start = torch.empty(len(pt), dtype=torch.int64)
    start[pt] = start_sorted
    return offs, torch.repeat_interleave(start - offs[:-1], counts) + torch.arange(int(offs[-1]))


def flat_sites_and_variants(st, tk, M, L):
    """The sites and variants of the input section of namp_mutations / namp_state_mutations; needs no device.  st int [n_sites, s]
    padded with -1, tk int [n, 1 + s] (a site index, then one token per column of st), M states of L residues (M = 1: the plain scan)
    -> sites8 int32 [n_sites, 8], tok9 int32 [n, 9]: with e counting the residues a site lists, copy m * L + r of edit e sits at column
    e * M + m and its token at 1 + e * M + m; padded columns hold -1 / 0.  (The callers have checked that s * M <= 8 edits are listed.)"""
    sites8 = np.full((len(st), MUT_MAX_EDITS), -1, np.int32)
    tok9 = np.zeros((len(tk), 1 + MUT_MAX_EDITS), np.int32)
    tok9[:, 0] = tk[:, 0]
    s = min(st.shape[1], MUT_MAX_EDITS // M)
    first = np.argsort(st < 0, axis=1, kind="stable")                               # the listed residues first, in their order
    res = np.take_along_axis(st, first, 1)[:, :s]
    tok = np.take_along_axis(tk[:, 1:], first[tk[:, 0]], 1)[:, :s]
    sites8[:, :s * M] = np.where(res[:, :, None] >= 0, res[:, :, None] + L * np.arange(M), -1).reshape(len(st), s * M)
    tok9[:, 1:1 + s * M] = np.repeat(np.where(res[tk[:, 0]] >= 0, tok, 0), M, axis=1)
    return sites8, tok9


def expand_group_sites(st, tk, groups, L):
    """The sites of score_mutations(tied=True) on the device; needs no device.  st int [n_sites, s] padded with -1, tk
    int [n, 1 + s], groups: the tied groups (lists of residues in LISTED order, disjoint).  Every named residue stands for its whole
    unit: the edit goes to all members of its group with the same token -> (st_x int64 [n_sites, s_x], tk_x int64 [n, 1 + s_x]), the
    members in listed order, unit by unit in the order the site names them.  Two named residues of one site in one unit, or more than
    MUT_MAX_EDITS flat residues in one expanded site: ValueError."""
    unit = {}
    for g in groups:
        for r in g:
            unit[int(r)] = [int(q) for q in g]
    rows, cols = [], []
    for s, row in enumerate(st):
        flat, col, seen = [], [], set()
        for c, r in enumerate(row):
            if r < 0:
                continue
            members = unit.get(int(r), [int(r)])
            if members[0] in seen:
                raise ValueError(f"sites[{s}] names two residues of one tied unit (the unit of residue {members[0]}): a named residue "
                                 "stands for its whole unit")
            seen.add(members[0])
            flat += members
            col += [c] * len(members)
        if len(flat) > MUT_MAX_EDITS:
            raise ValueError(f"sites[{s}] expands to {len(flat)} flat residues (every member of every named unit); at most "
                             f"{MUT_MAX_EDITS} fit")
        rows.append(flat)
        cols.append(col)
    width = max([len(f) for f in rows], default=1) or 1
    st_x = np.full((len(st), width), -1, np.int64)
    src = np.zeros((len(st), width), np.int64)
    for s, (flat, col) in enumerate(zip(rows, cols)):
        st_x[s, :len(flat)] = flat
        src[s, :len(col)] = col
    tk_x = np.zeros((len(tk), 1 + width), np.int64)
    if len(tk):
        tk_x[:, 0] = tk[:, 0]
        tk_x[:, 1:] = np.where(st_x[tk[:, 0]] >= 0, np.take_along_axis(tk[:, 1:], src[tk[:, 0]], 1), 0)
    return st_x, tk_x


def class_lane(tables, named):
    """The class a variant means for one tied unit; needs no device.  tables: the members' class tables in listed
    order (spec.N_CLASS_LANES entries each, below 0: no such class), named: {listed position: token} -> the LOWEST lane below
    spec.N_CLASSES every member has an entry on and whose entry equals the token at every named member, or -1.  (The canonical classes
    lie below the wobble lanes: naming G alone means G-C, naming both members (G, U) the wobble class.)"""
    for c in range(spec.N_CLASSES):
        if all(C[c] >= 0 for C in tables) and all(tables[t][c] == tok for t, tok in named.items()):
            return c
    return -1


def expand_class_sites(st, tk, units, L):
    """The sites of score_mutations(tied=True, classes=True) on the device; needs no device.  st int [n_sites, s]
    padded with -1, tk int [n, 1 + s], units: [(members in LISTED order, their class tables)] the tied units, disjoint.  For every
    unit with a named member the variant's class is class_lane over the named members of that unit, and EVERY member, named or not,
    gets its table's token for it; a residue in no unit keeps the token it was given -> (st_x int64 [n_sites, s_x], tk_x int64
    [n, 1 + s_x]), the members in listed order, unit by unit in the order the site first names them.  No lane for the given tokens, or
    more than MUT_MAX_EDITS flat residues in one expanded site: ValueError."""
    unit = {}
    for members, tables in units:
        for t, r in enumerate(members):
            unit[int(r)] = ([int(q) for q in members], tables, t)
    plans = []
    for s, row in enumerate(st):
        order, cols = [], {}
        for c, r in enumerate(row):
            if r < 0:
                continue
            members, tables, t = unit.get(int(r), ([int(r)], None, 0))
            if members[0] not in cols:
                order.append((members, tables))
                cols[members[0]] = {}
            cols[members[0]][t] = c
        flat = sum(len(m) for m, _ in order)
        if flat > MUT_MAX_EDITS:
            raise ValueError(f"sites[{s}] expands to {flat} flat residues (every member of every named unit); at most {MUT_MAX_EDITS} fit")
        plans.append([(members, tables, cols[members[0]]) for members, tables in order])
    width = max([sum(len(m) for m, _, _ in p) for p in plans], default=1) or 1
    st_x = np.full((len(st), width), -1, np.int64)
    for s, p in enumerate(plans):
        flat = [r for members, _, _ in p for r in members]
        st_x[s, :len(flat)] = flat
    tk_x = np.zeros((len(tk), 1 + width), np.int64)
    for v, row in enumerate(tk):
        tk_x[v, 0], q = row[0], 1
        for members, tables, named in plans[int(row[0])]:
            given = {t: int(row[1 + c]) for t, c in named.items()}
            if tables is None:
                tk_x[v, q] = given[0]
            else:
                lane = class_lane(tables, given)
                if lane < 0:
                    raise ValueError(f"site_tokens[{v}]: the unit of residue {members[0]} has no class with " +
                                     ", ".join(f"token {tok} at residue {members[t]}" for t, tok in sorted(given.items())))
                tk_x[v, q:q + len(members)] = [C[lane] for C in tables]
            q += len(members)
    return st_x, tk_x


def polymer_alphabet(prot, dna, rna, s0):
    """synth.make_complex's ranges for one residue (its polymer flags and its token): the 20 amino acids, the 4 DNA and the 4 RNA letters."""
    if dna or (not prot and not rna and 21 <= s0 < 26):
        return range(21, 25)
    if rna or (not prot and 26 <= s0 < 31):
        return range(26, 30)
    return range(0, 20)


def mutations_dense(out, L):
    """The result of score_mutations() as dense token log-probs [n, L]: the base entries, overwritten by the sparse rows (for tests
    and small cases: n * L floats)."""
    base = out["base_token_log_probs"]
    n = out["row_offsets"].numel() - 1
    dense = base[None].expand(n, L).clone()
    counts = out["row_offsets"][1:] - out["row_offsets"][:-1]
    variant = torch.repeat_interleave(torch.arange(n, device=counts.device), counts)
    dense[variant, out["row_residue"].long()] = out["row_token_log_prob"]
    return dense


def leave_one_out_ranks(rank, start=0, stop=None):
    """Decoding ranks of the leave-one-out streams of conditional_probs(): stream i is the order of `rank` [B, L] (the inverse of a
    decoding order) with residue i taken out and appended at the end — rank_i[j] = rank[j] - (rank[j] > rank[i]) for j != i,
    rank_i[i] = L - 1.  Returns [B, stop - start, L] (streams start .. stop-1; all L by default) in rank's dtype; works on CPU tensors."""
    B, L = rank.shape
    stop = L if stop is None else stop
    i = torch.arange(start, stop, device=rank.device)
    ri = rank[:, start:stop, None]
    out = rank[:, None, :] - (rank[:, None, :] > ri).to(rank.dtype)
    out[:, i - start, i] = L - 1
    return out


class _DecodingOrder:
    """The decoding order of ONE score / forward / sample call: order int64, order32 / rank int32 [B', L].  With the HIP sort
    (namp_decoding_order) the three tensors are allocated but not yet written while `pending`: the call's featuriser launch takes the
    sort along as the first workgroups of its edge-feature launch (`_featurize_hip(order=...)`, namp_featurize_ordered), and `wait()`
    launches it in the calling stream if none did.  The call holds this object, so nothing pending outlives it."""

    def __init__(self, order, rank, order32=None, inputs=None):
        self.order, self.order32, self.rank = order, order32, rank
        self.inputs = inputs                    # (mask, chain_mask or None, randn) as the sort reads them
        self.pending = inputs is not None
        self.event = None                       # side-stream work the decoder must wait for (sample()'s early levels)

    def sort_args(self):
        m, cm, r = self.inputs
        return (m.data_ptr(), hip.ptr(cm), r.data_ptr(), self.order.data_ptr(), self.order32.data_ptr(), self.rank.data_ptr(),
                self.order.shape[0])

    def wait(self):
        """Order the calling stream behind the sort — launching it here if no featuriser launch took it — and behind `event`
        (no host synchronisation)."""
        if self.pending:
            self.pending = False
            Bm, L = self.inputs[0].shape
            hip.check(hip.lib().namp_decoding_order(*self.sort_args(), Bm, L, hip.current_stream()), "decoding_order")
        if self.event is not None:
            torch.cuda.current_stream().wait_event(self.event)
            self.event = None


class ProteinMPNN(nn.Module):
    """Same constructor keywords as the inference copy (model_utils.py:9-23); the training copy's
    extra keywords (na_model_utils.py:520-539) are accepted as well."""

    def __init__(self, num_letters=21, node_features=128, edge_features=128, hidden_dim=128,
                 num_encoder_layers=3, num_decoder_layers=3, vocab=21, k_neighbors=48,
                 augment_eps=0.0, dropout=0.0, model_type="na_mpnn",
                 atom_dict=None, restype_to_int=None, polytype_to_int=None,
                 protein_augment_eps=None, dna_augment_eps=None, rna_augment_eps=None,
                 decode_protein_first=0, na_ref_atom="C1'", include_pred_na_N=1, device=None):
        super().__init__()
        if model_type != "na_mpnn":
            # reference behaviour (model_utils.py:44-46)
            print("Choose --model_type flag from currently available models")
            sys.exit()
        if atom_dict is None:
            raise Exception("atom_dict is necessary for featurization!")
        if polytype_to_int is None:
            raise Exception("polytype_to_int is necessary for featurization!")
        if (node_features, edge_features, hidden_dim) != (H, H, H):
            raise ValueError("the HIP kernels are specialised for node/edge/hidden width 128 "
                             "(the only configuration the reference instantiates)")
        # include_pred_na_N = 0 (training copy, na_model_utils.py:404-407,479-491): no virtual N_na atom; the edge embedding
        # sees 17 x 17 atom pairs ([128 x 4640]).  The kernels keep their 18-atom layout: the weight is expanded to the
        # 5200-column form with zero columns for every pair that involves atom 17, and atom 17 is marked absent on every
        # residue, so its (structurally zero) k-tiles are skipped — bit-identical to a 17-atom evaluation.
        self.include_pred_na_N = int(bool(include_pred_na_N))
        if vocab != num_letters:
            # the per-token tables (W1s . W_s, one row per letter) and the output head share one size in the kernels; the
            # reference only ever builds vocab == num_letters (run.py:184-202, na_run.py:73-92)
            raise ValueError(f"vocab ({vocab}) must equal num_letters ({num_letters})")
        if num_decoder_layers > hip.NAMP_MAX_LAYERS or num_encoder_layers > hip.NAMP_MAX_LAYERS:
            raise ValueError(f"at most {hip.NAMP_MAX_LAYERS} encoder / decoder layers are supported")
        self.model_type = model_type
        self.node_features, self.edge_features, self.hidden_dim = node_features, edge_features, hidden_dim
        self.vocab, self.num_letters = vocab, num_letters
        self.k_neighbors = k_neighbors
        self.restype_to_int = restype_to_int
        self.atom_dict = dict(atom_dict)
        self.na_ref_atom = na_ref_atom
        self.decode_protein_first = decode_protein_first
        self.mask_token = restype_to_int["MAS"] if restype_to_int else None
        eps = lambda v: augment_eps if v is None else v
        self.protein_augment_eps, self.dna_augment_eps, self.rna_augment_eps = \
            eps(protein_augment_eps), eps(dna_augment_eps), eps(rna_augment_eps)

        self.W_v = nn.Linear(node_features, hidden_dim, bias=True)
        self.features = _FeatureParams(edge_features, node_features, len(polytype_to_int),
                                       len(atom_dict) + 1 + self.include_pred_na_N)
        self.W_e = nn.Linear(edge_features, hidden_dim, bias=True)
        self.W_s = nn.Embedding(vocab, hidden_dim)
        self.dropout = nn.Dropout(dropout)
        self.encoder_layers = nn.ModuleList([_EncLayerParams(hidden_dim) for _ in range(num_encoder_layers)])
        self.decoder_layers = nn.ModuleList([_DecLayerParams(hidden_dim) for _ in range(num_decoder_layers)])
        self.W_out = nn.Linear(hidden_dim, num_letters, bias=True)
        for p in self.parameters():          # model_utils.py:67-69
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self._packed = None
        self._packed_sig = None
        self._ws = None
        self._tokens_ok = {}          # argument name -> (weakref to the validated tensor, its version)
        self._conv = {}               # (id(tensor), kind) -> (weakref, version, converted): see _as
        self._zeros = {}              # (shape, device) -> int32 zeros (the N_na masks of a model built without include_pred_na_N)
        self._v_cache = None          # (weakref to R_polymer_type, version, weights signature, V)
        self._tie_tables = {}         # (tied, classes) -> (key, host lists, tables) of the last conditional_probs of that kind
        # per-edge message / edge-update GEMMs: "x3" (default, parity mode) = three bf16 products of split operands with fp32
        # accumulation, fp32-equivalent to ~2^-16 (3e-5 on log-probs, arg-max unchanged) at 3/16 of the fp32 MFMA cost;
        # "fp32" = exact fp32 MFMA; "bf16" = plain bf16 inputs, BASELINE configs[2]'s throughput mode (~1e-2 on log-probs).
        self.message_precision = "x3"

    # ---------------------------------------------------------------------------------------
    # packed weights / workspace plumbing
    # ---------------------------------------------------------------------------------------
    def edge_weight18(self):
        """features.edge_embedding.weight in the kernels' 18-atom column layout [128 x 5200] (differentiable)."""
        W = self.features.edge_embedding.weight
        if self.include_pred_na_N:
            return W
        A = spec.N_ATOMS_AUG                                                   # 18; the model holds 17 x 17 pairs
        a, b, r = torch.meshgrid(torch.arange(A - 1), torch.arange(A - 1), torch.arange(spec.NUM_RBF), indexing="ij")
        cols = torch.cat((torch.arange(spec.NUM_POS), (spec.NUM_POS + (a * A + b) * spec.NUM_RBF + r).reshape(-1))).to(W.device)
        return torch.zeros(W.shape[0], spec.EDGE_IN, dtype=W.dtype, device=W.device).index_copy(1, cols, W)

    def _na_masks(self, fd):
        """(dna_mask, rna_mask) as the featuriser kernels see them: they only decide the presence of the virtual N_na atom."""
        if self.include_pred_na_N:
            return fd["dna_mask"], fd["rna_mask"]
        key = (tuple(fd["dna_mask"].shape), fd["dna_mask"].device)
        z = self._zeros.get(key)
        if z is None:
            if len(self._zeros) > 64:
                self._zeros.clear()
            z = self._zeros[key] = torch.zeros(key[0], dtype=torch.int32, device=key[1])
        return z, z

    def _weights_signature(self):
        """What the packed weight images are valid for: the storage address and version counter of every parameter.  A HIP launch that
        writes a parameter through its raw pointer must bump the counter (train.mark_written) to be seen here."""
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _weights(self):
        sig = self._weights_signature()
        if self._packed is None or sig != self._packed_sig:
            dev = self.W_v.weight.device
            _require_device(self.W_v.weight, "model parameters")
            sd = {k: v for k, v in self.state_dict().items()}
            sd["features.edge_embedding.weight"] = self.edge_weight18().detach()
            if self._packed is None or self._packed.flat.device != dev:
                self._packed = PackedWeights(sd, len(self.encoder_layers), len(self.decoder_layers), self.num_letters, dev)
            else:
                self._packed.repack(sd)
            self._packed_sig = sig
        if getattr(self._packed, "precision", "x3") != self.message_precision:
            self._packed.set_precision(self.message_precision)
        return self._packed

    def _check_tokens(self, S, what="S"):
        """Token ids index the per-token tables inside the kernels: anything outside [0, vocab) would read out of bounds
        where the reference's nn.Embedding raises (model_utils.py:402).  One device reduction + host read per NEW tensor
        OBJECT (identity through a weak reference + its version counter, one slot per argument name — never the address: the
        caching allocator hands a fresh `S.to(device)` the block of the previous batch), so steady-state calls on a resident
        feature_dict stay asynchronous.  An inference tensor has no version counter: it is checked on every call."""
        cached = not S.is_inference()
        slot = self._tokens_ok.get(what)
        if cached and slot is not None and slot[0]() is S and slot[1] == S._version:
            return
        lo, hi = torch.aminmax(S)
        if int(lo) < 0 or int(hi) >= self.vocab:
            raise IndexError(f"na_mpnn_amd: token ids in '{what}' must lie in [0, {self.vocab}); got [{int(lo)}, {int(hi)}]")
        if cached:
            self._tokens_ok[what] = (weakref.ref(S), S._version)

    def _host_list(self, t, what):
        """`t` (a small per-residue tensor of the feature_dict) as a Python list, read back ONCE per tensor object and version (see
        _check_tokens): the plan of a base-paired design needs the polymer types and the fixed residues on the host."""
        cached = torch.is_tensor(t) and not t.is_inference()
        slot = self._tokens_ok.get(("host", what))
        if cached and slot is not None and slot[0]() is t and slot[1] == t._version:
            return slot[2]
        out = t.detach().reshape(-1).tolist() if torch.is_tensor(t) else list(np.asarray(t).reshape(-1))
        if cached:
            self._tokens_ok[("host", what)] = (weakref.ref(t), t._version, out)
        return out

    def _mapped_arguments(self, fd, B, L):
        """Base pairs / token maps of a sample() call (feature_dict["paired_residues"], "paired_weights", "symmetry_token_maps") ->
        (groups, weights, the token maps as n_maps lists of 64 ids (map 0: the identity), the map index of every residue as a list of L,
        pair_list or None, None), see mapped_groups(); None without them.  With feature_dict["paired_wobble"] (a bool, or one per pair;
        "paired_wobble_bias": a float, or one per pair) true for some pair the maps are class tables (table 0: the identity below the
        vocabulary, -1 beyond) and the last entry holds the 64 class biases of every table: tables are told apart by (table, bias)."""
        pairs, maps = fd.get("paired_residues"), fd.get("symmetry_token_maps")
        wobble, wobble_bias, asked = self._wobble_arguments(fd, 0 if pairs is None else len(pairs))
        if not asked:
            wobble = None                                                        # no pair asks for wobble: the token maps, as without the key
        if (pairs is None or len(pairs) == 0) and maps is None:
            return None
        if self.restype_to_int is None:
            raise ValueError("paired_residues / symmetry_token_maps need the model's restype_to_int")
        if B != 1:
            raise ValueError("paired_residues / symmetry_token_maps expect one input complex (B == 1)")
        if "pair_bias" in fd:
            raise ValueError("pair_bias is not supported together with paired_residues / symmetry_token_maps")
        polymer = fixed = None
        if pairs is not None and len(pairs):
            dna, rna = self._host_list(fd["dna_mask"], "dna_mask"), self._host_list(fd["rna_mask"], "rna_mask")
            m, cm = self._host_list(fd["mask"], "mask"), self._host_list(fd["chain_mask"], "chain_mask")
            fixed = [not (a and b) for a, b in zip(m, cm)]                       # (a masked residue keeps its token as a fixed one does)
            # (a masked residue without a polymer flag is fixed, so all the map does is hand the complement of its token to its partner)
            polymer = self._pair_polymer(fd, pairs, L, dna, rna, m)
        groups, weights, gmaps, pair_list, *gbias = mapped_groups(L, self.restype_to_int, pairs, fd.get("paired_weights"), polymer, fixed,
                                                                  fd.get("symmetry_residues"), fd.get("symmetry_weights"), maps,
                                                                  wobble, wobble_bias)
        idx, seen = [None] * L, {}
        if wobble is None:
            table, index, bias = [list(range(64))], {tuple(range(self.num_letters)): 0}, None
            gbias = [None] * len(groups)
        else:
            V = len(spec.RESTYPES)
            table, bias = [list(range(V)) + [-1] * (spec.N_CLASS_LANES - V)], [[0.0] * spec.N_CLASS_LANES]
            index, gbias = {(tuple(table[0]), tuple(bias[0])): 0}, gbias[0]
        for g, ms, gb in zip(groups, gmaps, gbias):
            for r, m in zip(g, ms):
                if idx[r] is not None:                                            # (listed in an earlier group: it belongs to that one)
                    continue
                k = seen.get((id(m), id(gb)))                                   # (shared list objects: hundreds of pairs, a few tables)
                if k is not None:
                    idx[r] = k
                    continue
                key = tuple(m) if gb is None else (tuple(m), tuple(gb))
                k = index.get(key)
                seen[(id(m), id(gb))] = len(table) if k is None else k
                if k is None:
                    k = index[key] = len(table)
                    table.append(list(m) + list(range(len(m), 64)))
                    if gb is not None:
                        bias.append(list(gb))
                idx[r] = k
        if not groups:
            groups, weights = [[]], [[]]
        return groups, weights, table, [k or 0 for k in idx], pair_list, bias

    @staticmethod
    def _token_map_array(table, idx, device, bias=None):
        """What namp_sample_token_maps takes: ONE int32 array, the maps [n_maps][64] and behind them the map index of every residue; with
        `bias` what namp_sample_class_tables takes: behind those the class biases [n_maps][64] as float32 (their bits, in the one array)."""
        ints = torch.tensor([t for m in table for t in m] + list(idx), dtype=torch.int32)
        if bias is not None:
            ints = torch.cat((ints, torch.tensor([b for row in bias for b in row], dtype=torch.float32).view(torch.int32)))
        return ints.to(device)

    def _attach_maps(self, tok_maps, n_maps, classes):
        """The token maps (class tables: `classes`) go to the NEXT sampler call of this thread."""
        Lb = hip.lib()
        if tok_maps is not None and classes:
            hip.check(Lb.namp_sample_class_tables(tok_maps.data_ptr(), n_maps, spec.N_CLASSES), "sample_class_tables")
        elif tok_maps is not None:
            hip.check(Lb.namp_sample_token_maps(tok_maps.data_ptr(), n_maps), "sample_token_maps")

    def _pair_terms_of(self, fd, B, L):
        """feature_dict["pair_terms"] checked (pair_terms_arguments), or None without the key."""
        if fd.get("pair_terms") is None:
            return None
        if "pair_bias" in fd:
            raise ValueError("pair_terms and pair_bias are two forms of one quantity: give one of them")
        return pair_terms_arguments(fd["pair_terms"], B, L, self.num_letters)

    def _motifs_of(self, fd, B, L, tied):
        """feature_dict["forbidden_motifs"] checked (forbidden_motifs_arguments) with what the section needs, built on the CPU (one
        read of chain_labels / R_idx / mask): {"motifs", "hw": the windows' half width, "window" int32 [B, L, 2 hw], "entries" int32
        [n, 6], "adj": motif_adjacency on the device, for motif_hits}; None without the key or with no motif."""
        if fd.get("forbidden_motifs") is None:
            return None
        special = [int(self.restype_to_int[name]) for name in ("UNK", "DX", "RX", "MAS", "PAD")]
        motifs = forbidden_motifs_arguments(fd["forbidden_motifs"], self.num_letters, special, B, tied, "pair_bias" in fd)
        if not motifs:
            return None
        if min(self.k_neighbors, L) > 128:
            raise ValueError(f"forbidden_motifs need k_neighbors <= 128 (the sampler's form for K = {min(self.k_neighbors, L)} carries no motif code)")
        hw = max(len(m) for m in motifs) - 1
        cl, ri, mk = fd["chain_labels"], fd["R_idx"], fd["mask"]
        return {"motifs": motifs, "hw": hw, "window": motif_windows(cl.detach().cpu(), ri.detach().cpu(), mk.detach().cpu(), hw),
                "entries": motif_entries(motifs), "adj": motif_adjacency(cl, ri, mk)}

    def _pair_terms_section(self, pt, B, B_dec, N, K, dev, counted=None, motifs=None):
        """The sampler's workspace with the INPUT SECTION of the pair terms and / or the forbidden motifs (include/namp.h) filled: ONE
        pinned copy — to be enqueued before the encoder's launches, a host-to-device copy waits for the stream —, then the slots of every
        residue sorted by partner on the device.  pt: pair_terms_arguments' tuple or None; motifs: _motifs_of's dict or None.
        N > L (tied states: the flattened graph of N = M * L residues): the rows go to state 0's copies, every other copy has no slot
        and an empty window.
        counted (bool per residue, optional): residues whose terms count; the others lose their slots.
        -> {"ws", "dep": [B * N * n_dep] int32 — namp_sample_levels_dep's dep_idx: the partners and the window of every residue side by
        side —, "n_dep", "D", "n_tables", "members", "motifs": (n_entries, half_width) or None}."""
        Lb, n_dec, V, G = hip.lib(), len(self.decoder_layers), self.num_letters, B * N
        D = n_tab = members = n_pt = 0
        if pt is not None:
            partner, table, tables, members = pt
            L, D, n_tab = partner.shape[1], partner.shape[2], tables.shape[0]
            n_pt = 2 * G * D + tables.numel()
        off = Lb.namp_sample_pair_terms_offset(B, B_dec, N, K, n_dec)
        if motifs is None:
            need, words = Lb.namp_sample_pair_terms_workspace_bytes(B, B_dec, N, K, n_dec, D, n_tab), n_pt
        else:
            hw, W, E = motifs["hw"], 2 * motifs["hw"], motifs["entries"].shape[0]
            need = Lb.namp_sample_motifs_workspace_bytes(B, B_dec, N, K, n_dec, D, n_tab, E, hw)
            w0 = (Lb.namp_sample_motifs_offset(B, B_dec, N, K, n_dec, D, n_tab, V) - off) // 4
            e0 = w0 + G * W
            words = e0 + 6 * E
        if need == 0:
            raise ValueError(f"pair_terms / forbidden_motifs: no sampler workspace for B={B} batch={B_dec} N={N} K={K} D={D} n_tables={n_tab}")
        host = torch.empty(words, dtype=torch.int32, pin_memory=True)
        if pt is not None:
            p, t = host[:G * D].view(B, N, D), host[G * D:2 * G * D].view(B, N, D)
            p.fill_(-1); t.zero_()
            p[:, :L], t[:, :L] = torch.where(partner < L, partner, torch.full_like(partner, -1)), table
            if counted is not None:
                p[:, :L][:, ~torch.as_tensor(counted, dtype=torch.bool)] = -1
            host[2 * G * D:n_pt] = tables.view(-1).view(torch.int32)
        if motifs is not None:
            host[w0:e0] = -1
            host[w0:e0].view(B, N, W)[:, :motifs["window"].shape[1]] = motifs["window"]
            host[e0:] = motifs["entries"].reshape(-1)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sec = ws[off:off + 4 * host.numel()].view(torch.int32)
        sec.copy_(host, non_blocking=True)
        dep, n_dep = sec[:G * D], D
        if pt is not None:
            pd, td = sec[:G * D].view(B, N, D), sec[G * D:2 * G * D].view(B, N, D)
            ps, ts = sort_pair_slots(pd, td)
            pd.copy_(ps); td.copy_(ts)
        if motifs is not None:
            wd = sec[w0:e0]
            dep, n_dep = (wd if pt is None else torch.cat((pd, wd.view(B, N, W)), 2).reshape(-1)), D + W
        return {"ws": ws, "dep": dep, "n_dep": n_dep, "D": D, "n_tables": n_tab, "members": members,
                "motifs": None if motifs is None else (E, hw)}

    def _as(self, t, kind):
        """`t` in the dtype / layout the kernels read ("i32": int32, "f32": float32; contiguous), converted ONCE per tensor object: a
        feature_dict that stays resident (run.py scores / samples the same parsed complex many times; bench.py's shards) costs its ~12
        cast launches on the first call only.  Keyed on the tensor's identity through a weak reference and on its version counter — never on
        its address (the caching allocator hands a new tensor the block of a freed one) — so an in-place edit or a new tensor converts afresh;
        the converted copy lives as long as its source.  An inference tensor has no version counter: it is converted on every call."""
        dt = torch.int32 if kind == "i32" else torch.float32
        if t.dtype == dt and t.is_contiguous():
            return t
        if t.is_inference():
            return t.to(dt).contiguous()
        key = (id(t), kind)
        e = self._conv.get(key)
        if e is not None and e[0]() is t and e[1] == t._version:
            return e[2]
        c = t.to(dt).contiguous()
        if len(self._conv) > 8192:                            # (dead entries normally leave through their weak references' callbacks)
            self._conv.clear()
        conv = self._conv
        self._conv[key] = (weakref.ref(t, lambda _r, k=key: conv.pop(k, None)), t._version, c)
        return c

    def _decoding_order(self, mask, chain_mask, randn):
        """The decoding order of one call (see _DecodingOrder): the HIP sort still pending, or — for shapes the kernel does not take
        (L > 8192, mismatched rows) and off the device — the stock ops' result."""
        Bm, L = mask.shape
        Br = randn.shape[0]
        if mask.is_cuda and L <= 8192 and Br % Bm == 0 and tuple(randn.shape) == (Br, L) and (chain_mask is None or chain_mask.shape == mask.shape):
            m, r = self._as(mask, "f32"), self._as(randn, "f32")
            cm = self._as(chain_mask, "f32") if chain_mask is not None else None
            order = torch.empty(Br, L, dtype=torch.int64, device=mask.device)
            order32 = torch.empty(Br, L, dtype=torch.int32, device=mask.device)        # (what the sampler's launches read: no cast launch)
            rank = torch.empty(Br, L, dtype=torch.int32, device=mask.device)
            return _DecodingOrder(order, rank, order32, (m, cm, r))
        order = self.decoding_order(mask if chain_mask is None else mask * chain_mask, randn)
        return _DecodingOrder(order, self.ranks_of(order).to(torch.int32))

    def order_and_rank(self, mask, chain_mask, randn):
        """Decoding order argsort((mask * chain_mask + 1e-4) * |randn|) (model_utils.py:389; na_model_utils.py:623) and its inverse permutation
        in one HIP launch in the calling stream (namp_decoding_order): order int64 [B', L], rank int32 [B', L], B' = rows of randn; mask /
        chain_mask [B, L] with B' % B == 0 (chain_mask None = ones).  Shapes the kernel does not take (L > 8192, mismatched rows) run the stock ops."""
        o = self._decoding_order(mask, chain_mask, randn)
        o.wait()
        return o.order, o.rank

    def _side_stream(self, device):
        st = getattr(self, "_side", None)
        if st is None or st.device != device:
            st = self._side = torch.cuda.Stream(device=device)
        return st

    def _workspace(self, B_enc, B_dec, N, K, device):
        need = hip.lib().namp_workspace_bytes(B_enc, B_dec, N, K)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    # ---------------------------------------------------------------------------------------
    # a11: featurisation (ProteinFeaturesNA.forward, model_utils.py:528-593).  The product path is the fused HIP
    # featuriser (`_featurize_hip`: prep_atoms / knn_select / edge_features kernels) and nothing else: a non-standard atom
    # order raises.  (A stock-ops restatement used as an on-device cross-check lives in tests/featurize_torch.py.)
    # ---------------------------------------------------------------------------------------
    def _virtual(self, p0, p1, p2, wa, wb, wc):
        b, c = p1 - p0, p2 - p1
        return wa * torch.cross(b, c, dim=-1) + wb * b + wc * c + p1

    def _require_reference_atom_order(self):
        """The HIP featuriser hard-codes the reference's atom order (run.py:15-19); there is no other featuriser."""
        if [self.atom_dict.get(a) for a in spec.ATOM_TYPES] != list(range(spec.N_ATOMS)) or \
                self.na_ref_atom not in self.atom_dict:
            raise NotImplementedError("na_mpnn_amd's featuriser needs the reference's atom order (inference/run.py:15-19): "
                                      f"atom_dict must map {list(spec.ATOM_TYPES)} to 0..{spec.N_ATOMS - 1}")

    def _noised_X(self, fd):
        X = fd["X"]
        if self.training and max(self.protein_augment_eps, self.dna_augment_eps, self.rna_augment_eps) > 0:   # :539-546
            eps = fd["protein_mask"] * self.protein_augment_eps + fd["dna_mask"] * self.dna_augment_eps + \
                fd["rna_mask"] * self.rna_augment_eps
            X = X + fd["X_m"][:, :, :, None] * eps[:, :, None, None] * torch.randn_like(X)
        return X

    def _node_features(self, fd):
        fp = self.features
        rp = fd["R_polymer_type"]
        # inference: V depends on the polymer types and three small parameters only (an inference tensor has no version counter: no cache)
        cached = not torch.is_grad_enabled() and not rp.is_inference()
        if cached:
            c = self._v_cache
            sig = tuple((p.data_ptr(), p._version) for p in (fp.node_embedding.weight, fp.norm_nodes.weight, fp.norm_nodes.bias))
            if c is not None and c[0]() is rp and c[1] == rp._version and c[2] == sig:
                return c[3]
        V = fp.node_embedding.weight.t()[rp.long()]      # one-hot @ W^T == row select (6 rows)
        V = nn.functional.layer_norm(V, (self.node_features,), fp.norm_nodes.weight, fp.norm_nodes.bias, 1e-5)
        if cached:
            self._v_cache = (weakref.ref(rp), rp._version, sig, V)
        return V

    @torch.no_grad()
    def _featurize_hip(self, fd, want_E=True, want_hE=False, order=None):
        """a11 on the HIP kernels (prep_atoms, knn, edge_features): returns V, E (or None), h_E0 (or None), E_idx.  A pending
        decoding-order sort of the same (B, L) (`order`, a _DecodingOrder) rides in the edge-feature launch."""
        self._require_reference_atom_order()
        X = self._noised_X(fd)
        X = self._as(X, "f32") if X is fd["X"] else X.float().contiguous()
        _require_device(X, "X")
        W = self._weights()
        Lb = hip.lib()
        B, L = X.shape[:2]
        K = int(min(self.k_neighbors, L))
        dev = X.device
        E_idx = torch.empty(B, L, K, dtype=torch.int32, device=dev)
        E = torch.empty(B, L, K, self.edge_features, device=dev) if want_E else None
        hE = torch.empty(B, L, K, self.hidden_dim, device=dev) if want_hE else None
        ws = torch.empty(Lb.namp_featurize_workspace_bytes(B, L) + Lb.namp_featurize_split_bytes(B, L, int(self.k_neighbors)),
                         dtype=torch.uint8, device=dev)
        dna_m, rna_m = self._na_masks(fd)
        t = [self._as(fd[k], "i32") for k in ("X_m", "mask", "R_idx", "chain_labels", "protein_mask")] + [self._as(dna_m, "i32"), self._as(rna_m, "i32")]
        if order is not None and order.pending and order.inputs[0].shape == (B, L) and order.inputs[0].device == dev:
            order.pending = False
            hip.check(Lb.namp_featurize_ordered(W.model(), X.data_ptr(), *[x.data_ptr() for x in t], int(self.k_neighbors),
                                                int(self.atom_dict[self.na_ref_atom]), E_idx.data_ptr(), hip.ptr(E), hip.ptr(hE),
                                                ws.data_ptr(), ws.numel(), B, L, *order.sort_args(), hip.current_stream()), "featurize_ordered")
        else:
            hip.check(Lb.namp_featurize(W.model(), X.data_ptr(), *[x.data_ptr() for x in t], int(self.k_neighbors),
                                        int(self.atom_dict[self.na_ref_atom]), E_idx.data_ptr(), hip.ptr(E), hip.ptr(hE),
                                        ws.data_ptr(), ws.numel(), B, L, hip.current_stream()), "featurize")
        # no host sync: the int32 temporaries and the workspace come from torch's stream-ordered caching allocator, so
        # their blocks are only reused by work enqueued AFTER these launches on the same stream
        return self._node_features(fd), E, hE, E_idx

    @torch.no_grad()
    def featurize(self, fd):
        """ProteinFeaturesNA.forward (model_utils.py:528-593) -> V, E, E_idx (int64 like the reference).  V is the caller's own
        copy, not the model's cached one."""
        V, E, _, E_idx = self._featurize_hip(fd, want_E=True, want_hE=False)
        return V.clone(), E, E_idx.long()

    # ---------------------------------------------------------------------------------------
    # a7: encoder
    # ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_graph(self, V, E, E_idx, mask, h_E_embedded=None):
        """(V [B,N,128], E [B,N,K,128], E_idx [B,N,K], mask [B,N]) -> h_V, h_E  (model_utils.py:88-94).
        ``h_E_embedded`` (= W_e.E + b, updated in place) may be given instead of E."""
        _require_device(V, "V")
        W = self._weights()
        B, N, K = E_idx.shape
        V = V.float().contiguous()
        E = E.float().contiguous() if E is not None else None
        E_idx32, mask32 = _i32(E_idx), _i32(mask)
        h_V = torch.empty(B, N, H, device=V.device)
        h_E = h_E_embedded if h_E_embedded is not None else torch.empty(B, N, K, H, device=V.device)
        ws = self._workspace(B, B, N, K, V.device)
        hip.check(hip.lib().namp_encoder_fwd(W.model(), V.data_ptr(), hip.ptr(E), E_idx32.data_ptr(), mask32.data_ptr(),
                                             h_V.data_ptr(), h_E.data_ptr(), ws.data_ptr(), ws.numel(), B, N, K,
                                             hip.current_stream()), "encoder_fwd")
        return h_V, h_E

    @torch.no_grad()
    def encode(self, feature_dict, order=None):
        """ProteinMPNN.encode (model_utils.py:71-99).  With the HIP featuriser W_e is applied inside the feature
        kernel, so E itself is never written.  `order`: a pending decoding-order sort for the featuriser to take along."""
        V, _, h_E, E_idx = self._featurize_hip(feature_dict, want_E=False, want_hE=True, order=order)
        h_V, h_E = self.encode_graph(V, None, E_idx, feature_dict["mask"], h_E_embedded=h_E)
        return h_V, h_E, E_idx.long()

    # ---------------------------------------------------------------------------------------
    # a8 / a10: parallel decoder
    # ---------------------------------------------------------------------------------------
    @staticmethod
    def decoding_order(chain_mask, randn):
        """argsort((chain_mask + 1e-4) * |randn|)  (model_utils.py:389; na_model_utils.py:623)."""
        return torch.argsort((chain_mask + 0.0001) * torch.abs(randn))

    @staticmethod
    def ranks_of(order):
        rank = torch.empty_like(order)
        rank.scatter_(1, order, torch.arange(order.shape[1], device=order.device).expand_as(order))
        return rank

    @torch.no_grad()
    def decode_graph(self, h_V, h_E, E_idx, S, mask, rank, want_logits=False):
        """Teacher-forced decoder (model_utils.py:406-421).  S / mask / rank: [B_dec, N];
        h_V / h_E / E_idx carry B_enc batches with B_dec % B_enc == 0."""
        _require_device(h_V, "h_V")
        W = self._weights()
        B_enc, N, K = E_idx.shape
        B_dec = S.shape[0]
        self._check_tokens(S)
        h_V, h_E = h_V.float().contiguous(), h_E.float().contiguous()
        E32, S32, m32, r32 = _i32(E_idx), _i32(S), _i32(mask), _i32(rank)
        log_probs = torch.empty(B_dec, N, self.num_letters, device=h_V.device)
        logits = torch.empty_like(log_probs) if want_logits else None
        ws = self._workspace(B_enc, B_dec, N, K, h_V.device)
        hip.check(hip.lib().namp_decoder_fwd(W.model(), h_V.data_ptr(), h_E.data_ptr(), E32.data_ptr(), S32.data_ptr(),
                                             m32.data_ptr(), r32.data_ptr(), log_probs.data_ptr(), hip.ptr(logits), None,
                                             ws.data_ptr(), ws.numel(), B_dec, B_enc, N, K, hip.current_stream()),
                  "decoder_fwd")
        return (log_probs, logits) if want_logits else log_probs

    @torch.no_grad()
    def encode_decode(self, feature_dict, S, rank, want_logits=False, idx_long=True, order=None):
        """encode() + decode_graph() for one decoder batch per complex, as ONE library call (namp_encdec_fwd): lets the
        kernels fuse across the encoder/decoder boundary.  Returns h_V, h_E, E_idx, log_probs(, logits); E_idx is int64 like the
        reference's unless idx_long=False (score() does not return it: no cast launch).  `order`: the _DecodingOrder that `rank`
        comes from, while its sort may still be pending."""
        mask = feature_dict["mask"]
        self._check_tokens(S)
        V, E, h_E, E_idx = self._featurize_hip(feature_dict, want_E=False, want_hE=True, order=order)
        W = self._weights()
        B, N, K = E_idx.shape
        V = V.float().contiguous()
        E32, S32, m32, r32 = E_idx, self._as(S, "i32"), self._as(mask, "i32"), self._as(rank, "i32")
        h_V = torch.empty(B, N, H, device=V.device)
        log_probs = torch.empty(B, N, self.num_letters, device=V.device)
        logits = torch.empty_like(log_probs) if want_logits else None
        need = 2 * hip.lib().namp_workspace_bytes(B, B, N, K)
        if self._ws is None or self._ws.numel() < need or self._ws.device != V.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=V.device)
        if order is not None:
            order.wait()
        hip.check(hip.lib().namp_encdec_fwd(W.model(), V.data_ptr(), hip.ptr(E.float().contiguous() if E is not None else None),
                                            E32.data_ptr(), m32.data_ptr(), S32.data_ptr(), r32.data_ptr(), h_V.data_ptr(),
                                            h_E.data_ptr(), log_probs.data_ptr(), hip.ptr(logits), self._ws.data_ptr(),
                                            self._ws.numel(), B, N, K, hip.current_stream()), "encdec_fwd")
        return h_V, h_E, (E_idx.long() if idx_long else E_idx), log_probs, logits

    @torch.no_grad()
    def score(self, feature_dict):
        """ProteinMPNN.score (model_utils.py:366-424)."""
        bs = feature_dict["batch_size"]
        S_true, mask = feature_dict["S"], feature_dict["mask"]
        B, L = S_true.shape
        o = self._decoding_order(mask, feature_dict["chain_mask"], feature_dict["randn"])
        rank = o.rank[:B]                        # the reference's gather keeps only E_idx's batch rows (:393)
        if bs == 1:
            log_probs = self.encode_decode(feature_dict, S_true, rank, idx_long=False, order=o)[3]
            return {"S": S_true, "log_probs": log_probs, "decoding_order": o.order[0]}
        h_V, h_E, E_idx = self.encode(feature_dict, order=o)
        o.wait()
        rep = lambda t: t.repeat(bs, *([1] * (t.dim() - 1)))
        log_probs = self.decode_graph(h_V, h_E, E_idx, rep(S_true), rep(mask), rep(rank))
        return {"S": rep(S_true), "log_probs": log_probs, "decoding_order": o.order[0]}

    def coordinate_gradients(self, feature_dict, decoding_randn=None, weights=None):
        """dL/dX of L = sum_i w_i (-log p(S_i)) under score()'s decoding order (sorted on mask * chain_mask: fixed residues first), through
        the differentiable training forward (train.forward_train) and the featuriser's coordinate gradient.  decoding_randn
        [B, L] (default: feature_dict["randn"], else drawn); weights [B, L] (default mask * chain_mask).  The neighbour lists are constants.
        -> {"loss" scalar, "dX" [B, L, 16, 3] (virtual Cb / N_na folded back onto their parents by autograd), "residue_norm" [B, L] =
        the Euclidean norm of a residue's 16 x 3 block}.  The model's mode decides dropout and coordinate noise: call it in eval().
        Parameter gradients are not touched."""
        from . import train
        fd = dict(feature_dict)
        mask = fd["mask"]
        B, L = mask.shape
        X = fd["X"].detach().float().clone().requires_grad_(True)
        fd["X"] = X
        order_mask = mask * fd["chain_mask"] if fd.get("chain_mask") is not None else mask
        if decoding_randn is None:
            decoding_randn = fd["randn"][:B] if fd.get("randn") is not None else torch.randn(B, L, device=mask.device)
        w = (order_mask if weights is None else weights).to(torch.float32)
        with torch.enable_grad():
            log_probs, _ = train.forward_train(self, fd, decoding_randn, order_mask=order_mask)
            loss = -(w * torch.gather(log_probs, -1, fd["S"].long().unsqueeze(-1)).squeeze(-1)).sum()
            dX, = torch.autograd.grad(loss, X)
        return {"loss": loss.detach(), "dX": dX, "residue_norm": dX.reshape(B, L, -1).norm(dim=-1)}

    @torch.no_grad()
    def unconditional_probs(self, feature_dict):
        """ProteinMPNN.unconditional_probs (model_utils.py:329-364): nothing is decoded 'before'."""
        bs = feature_dict["batch_size"]
        mask = feature_dict["mask"]
        h_V, h_E, E_idx = self.encode(feature_dict)
        rep = lambda t: t.repeat(bs, *([1] * (t.dim() - 1)))
        m = rep(mask)
        zeros = torch.zeros_like(m, dtype=torch.int32)
        return {"log_probs": self.decode_graph(h_V, h_E, E_idx, zeros, m, zeros)}

    # ---- shared by the calls that ride on a decoder call (conditional_probs, score_sequences, score_mutations, score_tied) ----------

    def _item_routes_ok(self, who, method, fallback):
        """What the item kernel of the cone conditionals evaluates: three decoder layers, split-bf16 or exact fp32 -> whether this
        model has them; `who` asked for an item route by name (method "cone", "active" or "items") without them: NotImplementedError."""
        ok = len(self.decoder_layers) == 3 and self.message_precision in ("x3", "fp32")
        if method in ("cone", "active", "items") and not ok:
            raise NotImplementedError(f"{who}(method='{method}') needs three decoder layers and message_precision 'x3' or 'fp32'; "
                                      f"use method='{fallback}'")
        return ok

    def _state_arguments_of(self, fd):
        """fd["state_weights"] checked as sample() checks them, for a call that draws nothing -> (state weights, M, L, the context
        states of _state_contexts or None)."""
        fd_chk = dict(fd, batch_size=int(fd["randn"].shape[0]))
        fd_chk.setdefault("bias", torch.zeros(1, 1, self.num_letters))
        fd_chk.pop("S_forced", None)
        got = self._states_arguments(fd_chk)
        return got[:3] + got[5:]

    def _encode_side_by_side(self, fd, order, state_w, M, L, ctx=None):
        """The states (one without state_weights) side by side as the encoder batch, as _sample_states featurises them -> h_V, h_E, E_idx.
        ctx: the context states (every state with its own tokens and presence) or None."""
        fd_enc = fd
        if state_w is not None:
            fd_enc = dict(fd)
            for k in self._STATE_SHARED:
                fd_enc[k] = fd[k].expand(M, L)
            if ctx is not None:
                fd_enc["S"], fd_enc["mask"] = ctx[:2]
        V, _, h_E, E_idx = self._featurize_hip(fd_enc, want_E=False, want_hE=True, order=order)
        h_V, h_E = self.encode_graph(V, None, E_idx, fd_enc["mask"], h_E_embedded=h_E)
        return h_V, h_E, E_idx

    def _item_decoder_inputs(self, h_V, h_E, E_idx, S, mask, rank, M, L, ctx=None):
        """What the ABI calls with item launches read -> (packed weights, h_V, h_E float32 contiguous, E_idx, S, mask, rank int32).  The M
        states are ONE complex of M * L residues: the block-diagonal flattened graph; S, mask and rank repeat per block
        (with context states, ctx, S and mask are the states' own rows)."""
        W = self._weights()
        E_f = E_idx if M == 1 else (E_idx + (torch.arange(M, dtype=torch.int32, device=h_V.device) * L)[:, None, None]).contiguous()
        rep = (lambda t: t) if M == 1 else (lambda t: t.repeat(1, M))
        E32, S32, m32, r32 = _i32(E_f), _i32(rep(self._as(S, "i32"))), _i32(rep(self._as(mask, "i32"))), _i32(rep(_i32(rank)))
        if ctx is not None:
            S32, m32 = _i32(ctx[0].reshape(1, M * L)), _i32(ctx[1].reshape(1, M * L))
        return W, h_V.float().contiguous(), h_E.float().contiguous(), E32, S32, m32, r32

    def _attached_decoder_call(self, family, dims, attach_args, fill, inputs, log_probs, N, K, what):
        """One namp_decoder_fwd call that carries what namp_<family>(*attach_args) attaches: the workspace is sized
        for dims (a size of 0: ValueError(what)), fill(section) writes the input section (a uint8 view from its offset on), then the
        attach and the call -> the arrays of its output section by name (output_section_layout: views of the call's workspace).
        inputs: _item_decoder_inputs."""
        Lb = hip.lib()
        W, h_V, h_E, E32, S32, m32, r32 = inputs
        need = getattr(Lb, f"namp_{family}_workspace_bytes")(*dims)
        if need == 0:
            raise ValueError(what)
        ws = torch.empty(need, dtype=torch.uint8, device=h_V.device)
        fill(ws[getattr(Lb, f"namp_{family}_in_offset")(*dims):])
        hip.check(getattr(Lb, "namp_" + family)(*attach_args), family)
        hip.check(Lb.namp_decoder_fwd(W.model(), h_V.data_ptr(), h_E.data_ptr(), E32.data_ptr(), S32.data_ptr(), m32.data_ptr(),
                                      r32.data_ptr(), log_probs.data_ptr(), None, None, ws.data_ptr(), ws.numel(), 1, 1, N, K,
                                      hip.current_stream()), f"decoder_fwd ({family})")
        return _read_sections(ws, getattr(Lb, f"namp_{family}_out_offset")(*dims), output_section_layout(family, dims))

    # streams of the L-stream form of conditional_probs() per decoder call: chunk * L stays within the 64 x 1000 tokens of the B = 64 batches
    loo_dense_tokens = 65536

    @torch.no_grad()
    def conditional_probs(self, feature_dict, method="auto", tied=False, classes=False):
        """Leave-one-out conditionals of every residue in one call: out["log_probs"][b, i, :] = log p(s_i | X, S_-i), row i of score()'s
        parallel decoder (model_utils.py:391-421) run with score()'s decoding order (:388-389) in which residue i is moved to the end,
        the true S teacher-forced everywhere (leave_one_out_ranks).  Returns {"S", "log_probs" [B, L, vocab], "decoding_order"};
        `batch_size` is ignored (nothing is random once `randn` is given).  Rows of masked residues are what the reference computes
        for them (a zero context).
        method: "dense" — L streams through the ordinary decoder (namp_decoder_fwd), chunked over streams; "cone" — only the dependency
        cone of every stream (namp_decoder_loo: about K + 3 layer evaluations per residue instead of 3 L), for three decoder layers in
        the split-bf16 ("x3") and exact fp32 evaluations; it also returns "cone_items", the int32 [2] device tensor of active layer-1 /
        layer-2 items; "auto" — the cone where it is implemented, the dense form otherwise (another number of decoder layers, the
        bf16 throughput mode).
        Pair conditionals.  With feature_dict["paired_residues"] [(i, j), ...] (optional "paired_weights" as in sample()) the rows of
        a pair's two residues hold the PAIR's conditional instead, the exact distribution paired sample() would draw the pair from if
        it were decoded last with everything else teacher-forced: the stream is score()'s order with i and j taken out and appended
        as ..., i, j (listed order; chain_mask does not reorder members), i's token hidden, and with z_i, z_j the members' logits
        there total[a] = w_i z_i[P_i[a]] + w_j z_j[P_j[a]], lp = log_softmax(total), row_m[P_m[a]] = lp[a] (P: the Watson-Crick maps
        of mapped_groups; T = 1, no bias, special tokens kept).  A pair with a masked member is dropped: both residues keep their
        leave-one-out rows.  Also returned: "pairs" int64 [n, 2], the pairs actually tied in listed order, and "pair_log_probs"
        [n, vocab], the rows of their listed-first members.  The cone evaluates all pairs in the one call (namp_loo_pairs); "dense",
        and "auto" where the cone does not apply, is the SLOW route: the unpaired rows through the L streams, and ONE teacher-forced
        design call of the sampler per pair (the pair decoded last), whose two log_probs rows are combined as above.
        paired_wobble (pair classes are the follow-up), pairs together with symmetry_residues or state_weights: NotImplementedError;
        pairs with more than one input complex: ValueError.
        Group conditionals (tied=True).  Every tie sample() knows except pair classes is honoured: symmetry_residues /
        symmetry_weights / symmetry_token_maps, state_weights (X [M, L, A, 3], the shared entries [1, L]; the result is [1, L, vocab]),
        and paired_residues alone or joined with either.  A group (m_1, ..., m_n) is in the LISTED order of mapped_groups(fixed=None),
        with states the union across the states on the flattened graph (flat residue m * L + i, state-major, weights w_m * w_member).
        Its stream is score()'s order with all members taken out and appended as ..., m_1, ..., m_n, EVERY member's token hidden;
        total[a] = sum_t w_t z_t[P_t[a]], lp = log_softmax(total), row_{m_t}[P_t[a]] = lp[a].  A group with a masked member is dropped
        whole and a group of one is the ordinary leave-one-out row; a group of more than hip.loo_group_max() = 16 members, a residue in
        two groups: ValueError; paired_wobble: NotImplementedError.  Also returned: "groups" int64 [n, max_size] padded with -1, the
        groups actually tied (flat indices with states), and "group_log_probs" [n, vocab], the rows of their listed-first members.
        The cone evaluates all groups in the one call (namp_loo_groups); "dense", and "auto" where the cone does not apply, is the
        slow route: one teacher-forced design call of the sampler per group.  With tied=False (the default) nothing above applies:
        symmetry_residues alone are not read, and the refusals of the pair conditionals stand.
        Pair classes (classes=True).  paired_wobble / paired_wobble_bias (a bool / float, or one per pair, as in
        sample()) are honoured: the members of a pair or group speak through the class tables C_t and the group class bias b of
        mapped_groups(..., wobble, wobble_bias), and on the SAME stream as above total[c] = sum_t w_t z_t[C_t[c]] + b[c] over the
        classes c < spec.N_CLASSES every member has a token for (listed order, the bias added last; absent classes -inf),
        clp = log_softmax(total), and a member's row is the log-marginal in its own alphabet, row_m[t] = logsumexp of clp[c] over
        {c : C_m[c] == t} (T = 1, no `bias`, special tokens kept: the sampler removes the classes that close on a special token, the
        conditional does not).  With tied=False: pairs only, the refusals above stand, and "pair_class_log_probs" [n, 64] (clp of every
        tied pair, -inf on absent lanes) is returned beside "pair_log_probs", the marginal rows of the listed-first members.  With
        tied=True: every tie above with class tables — wobble pairs joined with state_weights are groups of 2 M members, a wobble pair
        with a member in a symmetry_residues group is mapped_groups' ValueError — and "group_class_log_probs" [n, 64] is returned.
        Without paired_wobble, or with no pair that can wobble (DNA with DNA), the rows are the bits of the classes=False call and the
        class rows hold -inf on lanes 33 / 34.  The cone combines in one launch (namp_loo_classes); the slow route is the per-group
        design call above with the class combine applied in torch.  With classes=False (the default) paired_wobble stays refused."""
        if method not in ("auto", "dense", "cone"):
            raise ValueError(f"method must be 'auto', 'dense' or 'cone'; got {method!r}")
        fd, tied, classes = feature_dict, bool(tied), bool(classes)
        if fd.get("state_S") is not None or fd.get("state_mask") is not None:
            raise NotImplementedError("conditional_probs does not take context states (state_S / state_mask): score_tied() scores them")
        S_true, mask = fd["S"], fd["mask"]
        B, L = S_true.shape
        state_w, M = None, 1
        if tied and fd.get("state_weights") is not None:
            state_w, M, L = self._state_arguments_of(fd)[:3]
        ties = self._conditional_arguments(fd, B, L, state_w, tied, classes)
        cone_ok = self._item_routes_ok("conditional_probs", method, "dense")
        use_cone = method == "cone" or (method == "auto" and cone_ok)
        Lb, n_dec, N = hip.lib(), len(self.decoder_layers), M * L
        K = int(min(self.k_neighbors, L))
        ws = None
        if ties is not None:
            # The tables go up BEFORE the encoder is enqueued (a host-to-device copy waits for the stream), page-locked once with the
            # cached tables: with the cone into the input section of the call's workspace — ONE copy —, and the index of the ties for the result.
            _require_device(fd["X"], "X")
            dev, n_tab = S_true.device, ties["n_tables"]
            for key in ("section", "index"):
                if not ties[key].is_pinned():
                    ties[key] = ties[key].pin_memory()
            if use_cone:
                section = ties["section"]
                nbytes = Lb.namp_loo_classes_workspace_bytes(1, N, K, n_dec, n_tab, int(tied)) if classes else \
                    (Lb.namp_loo_groups_workspace_bytes if tied else Lb.namp_loo_pairs_workspace_bytes)(1, N, K, n_dec, n_tab)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                off = (Lb.namp_loo_groups_offset if tied else Lb.namp_loo_pairs_offset)(1, N, K, n_dec)
                ws[off:off + 4 * section.numel()].view(torch.int32).copy_(section, non_blocking=True)
            index = ties["index"].to(dev, non_blocking=True)
            lead = index[:, 0] if index.numel() else index.reshape(-1)
        o = self._decoding_order(mask, fd["chain_mask"], fd["randn"][:1] if state_w is not None else fd["randn"])
        if tied and ties is not None:
            h_V, h_E, E_idx = self._encode_side_by_side(fd, o, state_w, M, L)
        else:
            h_V, h_E, E_idx = self.encode(fd, order=o)
        self._check_tokens(S_true)
        o.wait()
        rank = o.rank[:B]
        out = {"S": S_true, "decoding_order": o.order[0]}
        dev = h_V.device
        if use_cone:
            W, h_V, h_E, E32, S32, m32, r32 = self._item_decoder_inputs(h_V, h_E, E_idx, S_true, mask, rank, M, L)
            if ties is None:
                ws = torch.empty(Lb.namp_loo_workspace_bytes(B, N, K, n_dec), dtype=torch.uint8, device=dev)
            elif classes:                                  # the NEXT namp_decoder_loo call reads the section
                hip.check(Lb.namp_loo_classes(n_tab, spec.N_CLASSES, int(tied)), "loo_classes")
            else:
                hip.check((Lb.namp_loo_groups if tied else Lb.namp_loo_pairs)(n_tab), "loo_groups" if tied else "loo_pairs")
            counts = torch.empty(2, dtype=torch.int32, device=dev)
            log_probs = torch.empty(B, N, self.num_letters, device=dev)
            hip.check(Lb.namp_decoder_loo(W.model(), h_V.data_ptr(), h_E.data_ptr(), E32.data_ptr(), S32.data_ptr(), m32.data_ptr(),
                                          r32.data_ptr(), log_probs.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), B, N, K,
                                          hip.current_stream()), "decoder_loo")
            out["cone_items"] = counts
            if classes and ties is not None:
                c_off = Lb.namp_loo_classes_out_offset(1, N, K, n_dec, n_tab, int(tied))
                class_rows = ws[c_off:c_off + 4 * spec.N_CLASS_LANES * N].view(torch.float32).view(N, spec.N_CLASS_LANES)[lead]
        else:
            log_probs = self._loo_dense(h_V, h_E, E_idx, S_true, mask, rank)
            if ties is not None:
                log_probs = log_probs.view(1, N, self.num_letters)
                rows = self._tied_conditionals_by_sampling(fd, o.order[0], ties, log_probs, tied, classes)
                if classes:
                    class_rows = torch.stack(rows) if rows else torch.zeros(0, spec.N_CLASS_LANES, device=dev)
        if ties is None:
            out["log_probs"] = log_probs
            return out
        what = "group" if tied else "pair"
        out.update({"log_probs": log_probs[:, :L], what + "s": index, what + "_log_probs": log_probs[0, lead]})
        if classes:
            out[what + "_class_log_probs"] = class_rows
        return out

    def _loo_dense(self, h_V, h_E, E_idx, S, mask, rank):
        """The L-stream form: per encoded block (a complex of the batch, or a state under the one S / mask / rank) L streams through the
        ordinary decoder, chunked over streams -> the leave-one-out rows [blocks, L, vocab]."""
        nb, L = h_V.shape[:2]
        log_probs = torch.empty(nb, L, self.num_letters, device=h_V.device)
        chunk = max(1, self.loo_dense_tokens // L)
        for b in range(nb):
            S_b, m_b, r_b = (t[b:b + 1] if t.shape[0] == nb else t[:1] for t in (S, mask, rank))
            for i0 in range(0, L, chunk):
                i1 = min(L, i0 + chunk)
                n = i1 - i0
                ranks = leave_one_out_ranks(r_b, i0, i1)[0]
                lp = self.decode_graph(h_V[b:b + 1], h_E[b:b + 1], E_idx[b:b + 1], S_b.expand(n, L), m_b.expand(n, L), ranks)
                ar = torch.arange(n, device=lp.device)
                log_probs[b, i0:i1] = lp[ar, i0 + ar]
        return log_probs

    # tokens (sequences x L) per decoder call of the dense route of score_sequences(); the active route spends the same budget on the
    # rows it evaluates: 3 * score_library_tokens layer evaluations per call
    score_library_tokens = 65536

    def _library_arguments(self, fd, S_lib, positions):
        """The checked arguments of score_sequences() (no device needed): -> positions int64 [n_var] as a host list, the tokens at the
        positions [n, n_var] and the full sequences [n, L] (int64, on S_lib's device)."""
        _require_one_complex(fd, "score_sequences", "a library over several backbone states")
        S_true, mask = fd["S"], fd["mask"]
        L = S_true.shape[1]
        if positions is None:
            pos = torch.nonzero((mask[0] * fd["chain_mask"][0]) != 0).reshape(-1).tolist()
        else:
            pos = _positions_argument(positions, L)
        S_lib = torch.as_tensor(S_lib)
        n_var = len(pos)
        if S_lib.dim() != 2 or S_lib.dtype.is_floating_point or S_lib.shape[1] not in (L, n_var):
            raise ValueError(f"S_lib must be an integer tensor [n, {L}] (full sequences) or [n, {n_var}] (tokens at the positions); "
                             f"got {tuple(S_lib.shape)}")
        idx = torch.tensor(pos, dtype=torch.long, device=S_lib.device)
        tokens = (S_lib[:, idx] if S_lib.shape[1] == L else S_lib).long().contiguous()
        if tokens.numel():
            self._check_tokens(tokens, "S_lib")
        S_full = S_true.to(S_lib.device).long().expand(S_lib.shape[0], L).clone()
        S_full[:, idx] = tokens
        return pos, tokens, S_full

    def _library_auto(self, n_var, L, n):
        """The rule of score_sequences(method="auto") where the active route applies — from what the host knows without a read-back:
        at most half of the residues are library positions (see the docstring of score_sequences)."""
        return 2 * n_var <= L

    @torch.no_grad()
    def score_sequences(self, feature_dict, S_lib, positions=None, method="auto"):
        """The log-likelihoods of a LIBRARY of candidate sequences on one complex: for sequence k exactly what score() returns when
        feature_dict["S"] is replaced by sequence k — the same randn, batch_size = 1, hence the same decoding order — reduced to the
        token's own entry.  One input complex (B != 1: ValueError); state_weights: NotImplementedError; ties are not read (a given
        sequence is scored as it stands).
        positions: the library positions, an int tensor [n_var], ascending and unique, inside [0, L) (ValueError otherwise); default:
        the residues with mask * chain_mask != 0.  S_lib: int [n, L] (full sequences: everything outside `positions` is IGNORED and
        taken from feature_dict["S"]) or [n, n_var] (the tokens at `positions`); ids outside [0, vocab) raise IndexError, special
        tokens are legal.
        Returns "token_log_probs" float32 [n, L] (log_probs_k[i, S_k[i]], for masked residues what the reference computes for them),
        "loss" [n] (get_score's mean of -token_log_probs over mask * chain_mask, data_utils.py:36-52), "S" the full sequences [n, L],
        "decoding_order", "base_log_probs" [1, L, vocab] (the rows of feature_dict["S"]), "chunks" (decoder calls the library took) and,
        on the active route, "active_rows": an int32 [3] device tensor (|act_1|, |act_2|, |act_3|).
        method: "dense" — every sequence is a stream of the ordinary decoder (namp_decoder_fwd), score_library_tokens // L sequences
        per call, the entry gathered in torch: every number of decoder layers and every precision mode.  "active" — with chain_mask
        the fixed residues decode first, so only the rows a varying token reaches need a per-sequence evaluation: with var the
        library positions and act_0 = 0, act_l[i] = mask[i] and (act_{l-1}[i] or some earlier-decoded neighbour j of i has var[j]
        or act_{l-1}[j]); one pass over feature_dict["S"] gives the base tables and base_log_probs, and per layer the items
        (sequence, row of act_l or var) run through the item kernel of the cone conditionals with the rows a varying token changed
        overridden (namp_library, include/namp.h), 3 * score_library_tokens // sum_l |act_l + var| sequences per
        call.  The host reads the three row counts back ONCE per call, to size the chunks (never per chunk).  Three decoder layers
        and message_precision "x3" or "fp32" (NotImplementedError otherwise).  "auto" — the active route where it applies (three
        decoder layers, "x3" / "fp32") and 2 * n_var <= L, the dense route otherwise.  The rule reads n_var and L only (no read-back):
        with every residue designed the active route evaluates as many rows as the dense one and is measured 1.46x ("x3") / 1.14x
        ("fp32") slower per row (390 residues, K = 32, n = 1,000: 25.6 / 40.7 ms against 17.5 / 35.7 ms,
        profiles/score_library_time.log — item tables and 16-row item tiles against the decoder's fused launches), so it pays
        while fewer than about two thirds of the rows are evaluated; a layer usually holds about n_var rows (the designed residues
        decode last), and n_var <= L / 2 leaves room for fixed rows that a designed residue decoded early reaches."""
        if method not in ("auto", "dense", "active"):
            raise ValueError(f"method must be 'auto', 'dense' or 'active'; got {method!r}")
        fd = feature_dict
        pos, tokens, S_full = self._library_arguments(fd, S_lib, positions)
        S_true, mask = fd["S"], fd["mask"]
        L, n, n_var = S_true.shape[1], S_full.shape[0], len(pos)
        active_ok = self._item_routes_ok("score_sequences", method, "dense")
        use_active = method == "active" or (method == "auto" and active_ok and self._library_auto(n_var, L, n))
        _require_device(fd["X"], "X")
        dev = fd["X"].device
        tokens, S_full = tokens.to(dev), S_full.to(dev)
        o = self._decoding_order(mask, fd["chain_mask"], fd["randn"])
        h_V, h_E, E_idx = self.encode(fd, order=o)
        self._check_tokens(S_true)
        o.wait()
        rank = o.rank[:1]
        out = {"S": S_full, "decoding_order": o.order[0]}
        tlp = torch.empty(n, L, device=dev)
        chunks = 0
        if use_active:
            K = E_idx.shape[2]
            inputs = self._item_decoder_inputs(h_V, h_E, E_idx, S_true, mask, rank, 1, L)
            pos32 = torch.tensor(pos, dtype=torch.int32).to(dev)
            tok32 = tokens.to(torch.int32)
            base = torch.empty(1, L, self.num_letters, device=dev)

            def call(k0, k1, rows):
                """One attached decoder call over sequences k0 .. k1 - 1 -> the arrays of its output section."""
                def fill(section):
                    sec = section[:4 * (n_var + (k1 - k0) * n_var)].view(torch.int32)
                    sec[:n_var] = pos32
                    sec[n_var:] = tok32[k0:k1].reshape(-1)
                return self._attached_decoder_call(
                    "library", (L, K, 3, n_var, k1 - k0) + tuple(rows), (n_var, k1 - k0) + tuple(rows), fill, inputs, base, L, K,
                    f"score_sequences: no library workspace for L={L} K={K} n_var={n_var} sequences={k1 - k0}")

            counts = call(0, 0, (0, 0, 0))["counts"][:6].clone()    # the plan alone: the counts, and base_log_probs
            out["active_rows"] = counts[:3]
            rows = [int(v) for v in counts[3:6].tolist()]        # the call's ONE read-back: the chunks are sized by it
            chunk = max(1, min(3 * self.score_library_tokens // max(1, sum(rows)), ((1 << 28) - 1) // L))
            for k0 in range(0, n, chunk):
                k1 = min(n, k0 + chunk)
                tlp[k0:k1] = call(k0, k1, rows)["token_log_probs"].view(k1 - k0, L)
                chunks += 1
        else:
            base = self.decode_graph(h_V, h_E, E_idx, S_true, mask, rank)
            chunk = max(1, self.score_library_tokens // L)
            for k0 in range(0, n, chunk):
                k1 = min(n, k0 + chunk)
                S_k = S_full[k0:k1]
                lp = self.decode_graph(h_V, h_E, E_idx, S_k, mask.expand(k1 - k0, L), rank.expand(k1 - k0, L))
                tlp[k0:k1] = lp.gather(2, S_k[:, :, None])[:, :, 0]
                chunks += 1
        cm = (mask * fd["chain_mask"])[0].to(tlp.dtype)
        out.update({"token_log_probs": tlp, "loss": (-tlp * cm).sum(-1) / (cm.sum() + 1e-8), "base_log_probs": base, "chunks": chunks})
        return out

    def _mutation_arguments(self, fd, positions, tokens, sites, site_tokens, pairs):
        """The checked arguments of score_mutations() (no device needed) -> (sites int64 [n_sites, M] padded with -1, site_tokens int64
        [n, 1 + M] (0 in the padded columns), scan): both numpy; scan is None in the general form, else {"positions": the scanned
        residues (of a pair its first listed member), "tokens": the token axis, "valid": bool [P, T]}."""
        _require_one_complex(fd, "score_mutations", "several state weights need X [M, L, atoms, 3], one backbone per state")
        L = fd["S"].shape[1]
        general = sites is not None or site_tokens is not None
        if general and (positions is not None or tokens is not None):
            raise ValueError("score_mutations takes positions / tokens (the scan form) or sites / site_tokens (the general form), not both")
        if general:
            if sites is None or site_tokens is None:
                raise ValueError("the general form of score_mutations needs both sites and site_tokens")
            if pairs:
                raise ValueError("pairs=True belongs to the scan form: a general site lists its residues itself")
            st, tk = torch.as_tensor(sites), torch.as_tensor(site_tokens)
            if st.dim() != 2 or st.dtype.is_floating_point or st.dtype == torch.bool or st.shape[1] < 1:
                raise ValueError("sites must be an integer tensor [n_sites, M]")
            M = st.shape[1]
            if M > MUT_MAX_EDITS:
                raise ValueError(f"a site holds at most {MUT_MAX_EDITS} residues; got M = {M}")
            if tk.dim() != 2 or tk.dtype.is_floating_point or tk.shape[1] != 1 + M:
                raise ValueError(f"site_tokens must be an integer tensor [n, {1 + M}] (a site index, then one token per column of sites)")
            st, tk = st.cpu().numpy().astype(np.int64), tk.cpu().numpy().astype(np.int64).copy()
            for s, row in enumerate(st):
                res = [int(r) for r in row if r >= 0]
                if not res or any(r >= L for r in res) or any(r < -1 for r in row):
                    raise ValueError(f"sites[{s}] must hold 1 to {M} residues of [0, {L}) (padding: -1)")
                if len(set(res)) != len(res):
                    raise ValueError(f"sites[{s}] repeats a residue")
            if len(tk) and (tk[:, 0].min() < 0 or tk[:, 0].max() >= len(st)):
                raise ValueError(f"site_tokens: a site index is outside [0, {len(st)})")
            if len(tk):
                tk[:, 1:][st[tk[:, 0]] < 0] = 0
                self._check_tokens(torch.from_numpy(tk[:, 1:]), "site_tokens")
            return st, tk, None
        host = lambda key: [int(v) for v in fd[key][0].reshape(-1).tolist()]
        w = _counted_weights(fd)
        if positions is None:
            pos = [i for i in range(L) if w[i] != 0]
        else:
            pos = _positions_argument(positions, L)
        S0, prot, dna, rna = host("S"), host("protein_mask"), host("dna_mask"), host("rna_mask")
        partner = {}
        if pairs:
            if fd.get("paired_wobble") is not None and self._wobble_arguments(fd)[2]:
                raise NotImplementedError("score_mutations(pairs=True) walks canonical duplexes: paired_wobble is not supported")
            pr = fd.get("paired_residues")
            if pr is None or self.restype_to_int is None:
                raise ValueError("pairs=True needs feature_dict['paired_residues'] and the model's restype_to_int")
            polymer = self._pair_polymer(fd, pr, L, dna, rna, host("mask"))
            for i, j, _, _, kind in mapped_groups(L, self.restype_to_int, pr, None, polymer, None)[3]:
                partner[i] = partner[j] = (i, j, spec.token_map(self.restype_to_int, kind))

        def alphabet(i):
            return polymer_alphabet(prot[i], dna[i], rna[i], S0[i])
        site_list, seen = [], set()
        for p in pos:                                            # a pair is one site, scanned once from its first listed member
            members = partner[p][:2] if p in partner else (p,)
            if members[0] not in seen:
                seen.add(members[0])
                site_list.append(members)
        if tokens is None:
            T = sorted({t for m in site_list for t in alphabet(m[0])})
            valid = np.array([[t in alphabet(m[0]) for t in T] for m in site_list], bool).reshape(len(site_list), len(T))
        else:
            t = torch.as_tensor(tokens)
            if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError("tokens must be a one-dimensional integer tensor")
            if t.numel():
                self._check_tokens(t, "tokens")
            T = [int(v) for v in t.tolist()]
            valid = np.ones((len(site_list), len(T)), bool)
        M = 2 if partner else 1
        st = np.full((len(site_list), M), -1, np.int64)
        rows = []
        for s, members in enumerate(site_list):
            st[s, :len(members)] = members
            for q, t in enumerate(T):
                if valid[s, q]:
                    rows.append([s, t] + ([partner[members[0]][2][t]] if len(members) == 2 else [0] * (M - 1)))
        tk = np.array(rows, np.int64).reshape(len(rows), 1 + M)
        return st, tk, {"positions": [m[0] for m in site_list], "tokens": T, "valid": valid}

    @torch.no_grad()
    def score_mutations(self, feature_dict, positions=None, tokens=None, sites=None, site_tokens=None, pairs=False, method="auto", tied=False,
                        classes=False):
        """A mutational scan: for every VARIANT — a SITE of 1 to 8 distinct residues with one token per residue, every other residue
        keeping feature_dict["S"] — the change of the joint log-likelihood score() reports, delta = sum_i w_i (log p_v(S_v[i]) -
        log p(S[i])) with w = mask * chain_mask, under score()'s own decoding order (the same randn, batch_size = 1: the definition
        of score_sequences()).  One input complex (B != 1: ValueError); with state_weights and X [M, L, atoms, 3] the call is the
        specificity scan of _score_state_mutations (several weights beside one backbone: NotImplementedError); ties
        other than paired_residues with pairs=True are not read.
        The scan form: positions int [P], ascending and unique (default: mask * chain_mask != 0) x tokens int [T] (default: every
        letter of the residue's own polymer alphabet — 0..19, 21..24, 26..29 — and the token axis is their union; a given `tokens`
        is applied to every position as it stands).  pairs=True with feature_dict["paired_residues"]: scanning a paired residue
        edits its partner too, with the token of the involution paired sample() uses (mapped_groups: spec.WC_SAME / WC_CROSS) — the
        site is the pair, scanned once, from its first listed member; paired_wobble: NotImplementedError.  The general form:
        sites int [n_sites, M <= 8] padded with -1 and site_tokens int [n, 1 + M] (a site index, then the tokens; padded columns
        are ignored).  Both forms at once, positions out of range or not ascending, M > 8, a repeated residue: ValueError; token ids
        outside [0, vocab): IndexError.
        Returns "delta_log_likelihood" float32 [n], "loss" [n] (get_score's mean for the variant: base_loss - delta / sum(w)),
        "base_loss", "base_token_log_probs" [L], "base_log_probs" [1, L, vocab], "decoding_order", "site_index" [n], "sites",
        "site_tokens", the sparse rows "row_offsets" int64 [n + 1], "row_residue" int32 [nnz], "row_token_log_prob" float32 [nnz]
        (the variant's own entry on every row of U_3(site), ascending; mutations_dense(out, L) spreads them over [n, L]),
        "site_rows" int32 [n_sites, 3] (|U_1..3(site)|, read back once; None where the cone route does not apply or "dense" was
        asked for), "chunks", "method" (the route taken) and, in the scan form, "positions", "tokens" and "delta" [P, T] (NaN where
        a token lies outside the residue's alphabet).
        method: "cone" — per site the rows a variant can differ on, U_l(site) = act_l(site) + site (the sets of score_sequences with
        var = the site), are planned on the device; the items (variant, row of U_l(site)) run through the item kernel of the cone
        conditionals, laid out by prefix sums, the override rows found by binary search in the site's sorted list (namp_mutations,
        include/namp.h).  One attached call with zero variants gives the sizes; the host reads them back ONCE and
        cuts the variants, grouped by site, into calls of at most 3 * score_library_tokens item rows.  Three decoder layers and
        message_precision "x3" or "fp32" (NotImplementedError otherwise).  "dense" — the explicit library through
        score_sequences(method="dense"), reduced in torch (every row is listed): every layer count and precision mode.  "auto" —
        decided after the read-back: the cone where it applies and the mean of sum_l |U_l(site)| over the variants is at most 2 L
        (two thirds of the dense route's 3 L rows: the break-even measured for the item route, score_sequences()), else dense.
        tied=True: the symmetric scan of _score_group_mutations — feature_dict["symmetry_residues"] are read as
        score_tied() reads them, a named residue stands for its whole unit and the deltas are differences of score_tied()'s
        log_likelihood; with state_weights and no listed group the call is the specificity scan as it stands (with both:
        NotImplementedError).  tied=False reads no symmetry group.
        tied=True, classes=True: the paired scan — every tie score_tied() reads on one backbone (base pairs, wobble,
        symmetry groups with or without token maps, pairs joined with groups) through class tables: a variant names the class of
        every unit it touches (class_lane: the lowest matching lane) and every member gets its token; pairs=True scans the class axis
        of every pair.  classes=True without tied=True: ValueError; with state_weights or pair_terms: NotImplementedError."""
        if method not in ("auto", "cone", "dense"):
            raise ValueError(f"method must be 'auto', 'cone' or 'dense'; got {method!r}")
        fd = feature_dict
        sw = fd.get("state_weights")
        if classes:
            if not tied:
                raise ValueError("score_mutations(classes=True) needs tied=True: class tables belong to the tied scan")
            return self._score_group_mutations(fd, positions, tokens, sites, site_tokens, pairs, method, True)
        if tied:
            if sw is not None and _listed(fd.get("symmetry_residues")):
                raise NotImplementedError("score_mutations(tied=True): symmetry_residues joined with state_weights are not supported")
            if sw is None:
                return self._score_group_mutations(fd, positions, tokens, sites, site_tokens, pairs, method)
        if sw is not None:
            # (several weights beside ONE backbone stay the refusal they were: _mutation_arguments raises NotImplementedError)
            if not (fd["X"].dim() == 4 and fd["X"].shape[0] == 1 and (sw.numel() if torch.is_tensor(sw) else len(sw)) != 1):
                return self._score_state_mutations(fd, positions, tokens, sites, site_tokens, pairs, method)
        st, tk, scan = self._mutation_arguments(fd, positions, tokens, sites, site_tokens, pairs)
        S_true, mask = fd["S"], fd["mask"]
        L, n, n_sites = S_true.shape[1], len(tk), st.shape[0]
        cone_ok = self._item_routes_ok("score_mutations", method, "dense")
        _require_device(fd["X"], "X")
        dev = fd["X"].device
        w = (mask * fd["chain_mask"])[0].float()
        out = _scan_head(st, tk, dev)
        use_cone, base = False, None
        if cone_ok and method != "dense" and n_sites:
            o = self._decoding_order(mask, fd["chain_mask"], fd["randn"])
            h_V, h_E, E_idx = self.encode(fd, order=o)
            self._check_tokens(S_true)
            o.wait()
            K = E_idx.shape[2]
            inputs = self._item_decoder_inputs(h_V, h_E, E_idx, S_true, mask, o.rank[:1], 1, L)
            base = torch.empty(1, L, self.num_letters, device=dev)
            route = _ConeRoute("mutations", L, K, (L, K, 3), (), f"score_mutations: no workspace for L={L} K={K}",
                               *flat_sites_and_variants(st, tk, 1, L), w, {"delta": ()}, ("row_residue", "row_token_log_prob"))
            got = self._cone_scan(route, inputs, base, tk[:, 0], method)
            out["site_rows"], use_cone = got["site_rows"], got["use_cone"]
        if n == 0:
            sc = self.score(dict(fd, batch_size=1))
            base, order = sc["log_probs"], sc["decoding_order"]
            (delta, offs, rres, rlp), chunks = _empty_rows(dev), 0
        elif use_cone:
            order = o.order[0]
            delta, offs, rres, rlp, chunks = (got[k] for k in ("delta", "row_offsets", "row_residue", "row_token_log_prob", "chunks"))
        else:
            union = torch.tensor(sorted({int(r) for r in st[tk[:, 0]].reshape(-1) if r >= 0}), dtype=torch.long)
            lib = self.score_sequences(fd, _variant_library(S_true, st, tk), union, method="dense")
            base, order = lib["base_log_probs"], lib["decoding_order"]
            tlp = lib["token_log_probs"]
            btlp = base[0].gather(1, S_true[0].long()[:, None])[:, 0]
            delta = ((tlp - btlp[None]) * w[None]).sum(-1)
            offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
            rres = torch.arange(L, dtype=torch.int32, device=dev).repeat(n)
            rlp = tlp.reshape(-1)
            chunks = lib["chunks"]
        btlp = base[0].gather(1, S_true[0].long()[:, None])[:, 0]
        denom = w.sum() + 1e-8
        base_loss = (-btlp * w).sum() / denom
        return self._scan_result(out, scan, delta, base_loss, denom, btlp, base, order, (offs, rres, rlp), {}, chunks, use_cone)

    @staticmethod
    def _scan_result(out, scan, delta, base_loss, denom, btlp, base, order, rows, extra, chunks, use_cone):
        """What both forms of score_mutations() return alike, added to out: the deltas and losses, the sparse rows (offsets, residues,
        entries), `extra` (the form's own keys), "chunks", "method" and, in the scan form, the [P, T] grid."""
        dev = delta.device
        out.update({"delta_log_likelihood": delta, "loss": base_loss - delta / denom, "base_loss": base_loss, "base_token_log_probs": btlp,
                    "base_log_probs": base, "decoding_order": order, "row_offsets": rows[0], "row_residue": rows[1],
                    "row_token_log_prob": rows[2], **extra, "chunks": chunks, "method": "cone" if use_cone else "dense"})
        if scan is not None:
            grid = torch.full((len(scan["positions"]), len(scan["tokens"])), float("nan"), device=dev)
            grid[torch.from_numpy(scan["valid"]).to(dev)] = delta
            out.update({"positions": torch.tensor(scan["positions"], dtype=torch.long, device=dev),
                        "tokens": torch.tensor(scan["tokens"], dtype=torch.long, device=dev), "delta": grid})
        return out

    def _cone_scan(self, route, inputs, base, site_index, method):
        """The cone route of both forms of score_mutations().  route: a _ConeRoute; inputs: _item_decoder_inputs;
        base: the carrier's log_probs; site_index int64 [n] (numpy): the site of every variant.  One attached call with zero variants
        gives the sizes (and base); they are read back ONCE, "auto" is decided, the variants are cut by mutation_chunks and every chunk
        is one attached call with its own sites, renumbered.  -> {"site_rows" int32 [n_sites, 3], "use_cone", "chunks", the plan call's
        arrays that are neither per variant nor per row} and, where the cone is taken and there are variants, the route's per-variant and
        per-row arrays by name in the order the variants were GIVEN in, "row_offsets" int64 [n + 1] and "row_counts" (on the host).
        Every array is a clone: the next call reuses the workspace."""
        r, n_sites, n, dev = route, len(route.sites8), len(site_index), base.device

        def call(site_ids, variant_ids, lcap, icap):
            """One attached decoder call over the listed sites and variants -> the arrays of its output section."""
            ns, nv = len(site_ids), len(variant_ids)
            tail = (ns, nv) + tuple(lcap) + tuple(icap)

            def fill(section):
                local = np.zeros(n_sites, np.int32)
                local[site_ids] = np.arange(ns, dtype=np.int32)
                var = r.tok9[variant_ids].copy()
                var[:, 0] = local[var[:, 0]]
                sec = torch.from_numpy(np.concatenate((r.sites8[site_ids].reshape(-1), var.reshape(-1))))
                section[:4 * sec.numel()].view(torch.int32).copy_(sec)
                section[4 * sec.numel():4 * (sec.numel() + r.weights.numel())].view(torch.float32).copy_(r.weights)   # (they never leave the device)
            return self._attached_decoder_call(r.family, r.dims + tail, r.attach + tail, fill, inputs, base, r.N, r.K,
                                               f"{r.what} sites={ns} variants={nv}")

        first = call(np.arange(n_sites), np.zeros(0, np.int64), (0, 0, 0), (0, 0, 0))         # the plan alone: the sizes, and base_log_probs
        got = {"site_rows": first.pop("site_rows").view(n_sites, 3).clone(), "chunks": 0}
        got.update({k: v.clone() for k, v in first.items() if k not in r.per_variant and k not in r.per_row})
        rows_host = got["site_rows"].cpu().numpy().astype(np.int64)               # the call's ONE read-back: route and chunks hang on it
        got["use_cone"] = method == "cone" or int(rows_host[site_index].sum()) <= 2 * r.N * n
        if not (got["use_cone"] and n):
            return got
        perm, cuts = mutation_chunks(site_index.tolist(), rows_host.tolist(), 3 * self.score_library_tokens)
        perm = np.asarray(perm, np.int64)
        names = tuple(r.per_variant) + tuple(r.per_row)
        parts = {k: [] for k in names}
        for q0, q1 in cuts:
            vids = perm[q0:q1]
            sids = np.unique(site_index[vids])                                    # (perm is ordered by site: the order of appearance)
            lcap = rows_host[sids].sum(0).tolist()
            icap = rows_host[site_index[vids]].sum(0).tolist()
            sec = call(sids, vids, lcap, icap)
            for k in names:
                parts[k].append(sec[k].clone())
        counts = torch.from_numpy(rows_host[site_index, 2])
        offs, idx = variant_row_order(perm, counts)
        pt = torch.from_numpy(perm).to(dev)
        for k, shape in r.per_variant.items():
            ran = torch.cat(parts[k]).view((n,) + shape)
            got[k] = torch.empty_like(ran)
            got[k][pt] = ran
        idx = None if idx is None else idx.to(dev)
        for k in r.per_row:
            got[k] = torch.cat(parts[k]) if idx is None else torch.cat(parts[k])[idx]
        got.update({"row_offsets": offs.to(dev), "row_counts": counts, "chunks": len(cuts)})
        return got

    def _state_scan_arguments(self, fd, positions, tokens, sites, site_tokens, pairs):
        """The checked arguments of the specificity scan (no device needed) -> (state weights, M, L, ctx, sites [n_sites, s], site_tokens
        [n, 1 + s], scan: _mutation_arguments over SHARED residues; flat sites int32 [n_sites, 8] and flat variants int32 [n, 9]: the
        edit of shared residue r goes to all M copies m * L + r, absent ones too)."""
        if pairs or any(_listed(fd.get(k)) for k in ("symmetry_residues", "paired_residues")) or fd.get("pair_terms") is not None \
                or self._wobble_arguments(fd)[2]:
            raise NotImplementedError("score_mutations with state_weights scans backbone states alone: pairs=True, symmetry_residues, "
                                      "paired_residues, paired_wobble and pair_terms are not supported beside them")
        _require_one_complex(fd, "score_mutations", None)
        state_w, M, L, ctx = self._state_arguments_of(fd)
        shared = {k: v for k, v in fd.items() if k != "state_weights"}
        st, tk, scan = self._mutation_arguments(shared, positions, tokens, sites, site_tokens, False)
        s = int((st >= 0).sum(1).max()) if len(st) else 1
        if s * M > MUT_MAX_EDITS:
            raise ValueError(f"a site of {s} residues in {M} states is {s * M} edits on the flattened graph; at most {MUT_MAX_EDITS} fit")
        w = _counted_weights(fd)
        _require_counted(st, w)
        return (state_w, M, L, ctx, st, tk, scan) + flat_sites_and_variants(st, tk, M, L)

    def _score_state_mutations(self, fd, positions, tokens, sites, site_tokens, pairs, method):
        """score_mutations() with feature_dict["state_weights"] — the specificity scan: which point mutations widen the
        gap between backbone states.  The states arguments and conventions are score_tied()'s (state_weights of M entries, optionally
        state_S / state_mask, shared [1, L] rows, X [M, L, A, 3]; T = 1, no bias, special tokens kept, score()'s order from the shared
        mask * chain_mask and row 0 of randn).  positions / sites are SHARED residue indices with mask * chain_mask != 0 (else ValueError);
        the edit goes to all M copies, so a site of s residues is s * M <= 8 edits on the flattened graph (else ValueError).
        delta_log_likelihood[v] = score_tied(fd, S_v)["log_likelihood"] - score_tied(fd, S)["log_likelihood"], the sum over the counted
        residues of unit_v[i] - unit[i], unit[i] = log_softmax(sum over the states in which i is present of w_m lp_m[i])[S[i]] (M = 1:
        the own entry, as score_tied has it); "state_delta" [n, M] the difference of score_tied's state_log_likelihood.  Returns what
        score_mutations returns, "loss" / "base_loss" / "base_token_log_probs" [L] on units (-inf where the present copies of a fixed
        residue hold different tokens, as in score_tied), "base_log_probs" [1, M * L, vocab] and the sparse rows in FLAT residues, and
        adds "state_delta", "base_state_log_likelihood" [M], "state_weights" [M] and the sparse units "unit_offsets" int64 [n + 1],
        "unit_residue" int32 (shared, ascending per variant), "unit_log_prob" float32: one entry per shared residue with a copy in
        U_3(site).  method: "cone" — namp_state_mutations (include/namp.h) carried by one decoder call per chunk on the flattened
        graph; "dense" — the explicit library through score_tied(method="stream"); "auto" — the cone where it applies and the mean of
        sum_l |U_l(site)| over the variants is at most 2 * M * L."""
        state_w, M, L, ctx, st, tk, scan, sites8, tok9 = self._state_scan_arguments(fd, positions, tokens, sites, site_tokens, pairs)
        S_true, mask = fd["S"], fd["mask"]
        n, n_sites, N, Vn = len(tk), len(st), M * L, self.num_letters
        cone_ok = self._item_routes_ok("score_mutations", method, "dense")
        _require_device(fd["X"], "X")
        dev = fd["X"].device
        counted = (mask * fd["chain_mask"])[0] != 0                                        # [L]
        present = (mask.expand(M, L) if ctx is None else ctx[1]) != 0                       # [M, L]
        sw = torch.tensor(state_w if M > 1 else [1.0], dtype=torch.float32, device=dev)     # (M = 1: the own entry, as score_tied has it)
        w_flat = (counted[None] & present).reshape(N).float()
        unit_w = (sw[:, None] * present).reshape(N).float()
        out = _scan_head(st, tk, dev, state_weights=torch.tensor(state_w, dtype=torch.float32, device=dev))
        o = self._decoding_order(mask, fd["chain_mask"], fd["randn"][:1])
        h_V, h_E, E_idx = self._encode_side_by_side(fd, o, state_w, M, L, ctx)
        self._check_tokens(S_true)
        o.wait()
        K = E_idx.shape[2]
        inputs = self._item_decoder_inputs(h_V, h_E, E_idx, S_true, mask, o.rank[:1], M, L, ctx)
        S_flat = inputs[4][0].long()
        use_cone, base, btlp = False, None, None
        if cone_ok and method != "dense" and n_sites:
            base = torch.empty(1, N, Vn, device=dev)
            route = _ConeRoute("state_mutations", N, K, (N, K, 3, M), (M, L), f"score_mutations: no workspace for {M} states x L={L} K={K}",
                               sites8, tok9, torch.cat((w_flat, unit_w)), {"delta": (), "state_delta": (M,)},
                               ("row_residue", "row_token_log_prob", "unit_residue", "unit_log_prob"))
            got = self._cone_scan(route, inputs, base, tk[:, 0], method)         # (the plan call: sizes, base rows, base units)
            out["site_rows"], btlp, use_cone = got["site_rows"], got["base_units"], got["use_cone"] and n > 0
        if use_cone:
            delta, sdelta, offs, rres, rlp, chunks = (got[k] for k in (
                "delta", "state_delta", "row_offsets", "row_residue", "row_token_log_prob", "chunks"))
            uoffs, ures, ulp = _sparse_units(got, n, L)                          # (ascending in the shared residue)
        elif n == 0:
            (delta, offs, rres, rlp), (_, uoffs, ures, ulp) = _empty_rows(dev), _empty_rows(dev)
            sdelta, chunks = torch.zeros(0, M, device=dev), 0
        else:
            lib = self.score_tied(fd, _variant_library(S_true, st, tk, "last"), method="stream")
            own = lib["member_log_probs"]                                          # [n + 1, M, L]
            state_ll = torch.where((counted[None] & present)[None], own, torch.zeros_like(own)).sum(-1)
            delta = lib["log_likelihood"][:n] - lib["log_likelihood"][n]
            sdelta = state_ll[:n] - state_ll[n:]
            offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * N
            rres = torch.arange(N, dtype=torch.int32, device=dev).repeat(n)
            rlp = own[:n].reshape(-1)
            uoffs = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
            ures = torch.arange(L, dtype=torch.int32, device=dev).repeat(n)
            ulp = lib["token_log_probs"][:n].reshape(-1)
            btlp = lib["token_log_probs"][n].clone()
            chunks = lib["chunks"]
        if base is None:                                                           # the flat base rows of the routes that ran no attached call
            rows = S_flat.view(M, L)
            base = self.decode_graph(h_V, h_E, E_idx.long(), rows, present.to(mask.dtype), o.rank[:1].expand(M, L)).reshape(1, N, Vn)
        if btlp is None:
            btlp = self.score_tied(fd, method="stream")["token_log_probs"][0]
        else:
            # (the device reports every unit at its first present copy's token; where the present copies of a fixed residue hold
            #  different tokens score_tied has -inf)
            tok = S_flat.view(M, L)
            seat = torch.where(present.any(0), present.float().argmax(0), torch.zeros(L, dtype=torch.long, device=dev))
            same = ((tok == tok.gather(0, seat[None])) | ~present).all(0)
            btlp = torch.where(same, btlp, torch.full_like(btlp, float("-inf")))
        own0 = base[0].gather(1, S_flat[:, None])[:, 0]
        wl = counted.float()
        denom = wl.sum() + 1e-8
        base_loss = -torch.where(counted, btlp, torch.zeros_like(btlp)).sum() / denom
        extra = {"state_delta": sdelta, "base_state_log_likelihood": (own0 * w_flat).view(M, L).sum(-1),
                 "unit_offsets": uoffs, "unit_residue": ures, "unit_log_prob": ulp}
        return self._scan_result(out, scan, delta, base_loss, denom, btlp, base, o.order[0], (offs, rres, rlp), extra, chunks, use_cone)

    def _group_scan_arguments(self, fd, positions, tokens, sites, site_tokens, pairs):
        """The checked arguments of the symmetric scan (no device needed) -> (ties: _conditional_arguments(tied=True) or None, groups:
        the validly tied groups in listed order, leader [L] as a list, st [n_sites, s] and tk [n, 1 + s] as NAMED, scan, st_x / tk_x:
        expand_group_sites, sites8 int32 [n_sites, 8], tok9 int32 [n, 9])."""
        if pairs or fd.get("symmetry_token_maps") is not None or _listed(fd.get("paired_residues")) or fd.get("pair_terms") is not None \
                or self._wobble_arguments(fd)[2]:
            raise NotImplementedError("score_mutations(tied=True) scans symmetry groups with identity token maps: symmetry_token_maps, "
                                      "paired_residues, pairs=True, paired_wobble and pair_terms are not supported")
        _require_one_complex(fd, "score_mutations", None)
        L = fd["S"].shape[1]
        ties = self._conditional_arguments(fd, 1, L, None, True, False)
        groups = [list(flat) for flat, *_ in (ties["tied"] if ties is not None else ())]
        S0 = [int(v) for v in fd["S"][0].reshape(-1).tolist()]
        leader = list(range(L))
        for g in groups:
            if len({S0[r] for r in g}) != 1:
                raise ValueError(f"feature_dict['S'] is not tie-consistent on the group of residue {g[0]}: a tied scan has no base there")
            for r in g:
                leader[r] = g[0]
        w = _counted_weights(fd)
        if positions is None and sites is None and site_tokens is None:
            positions = torch.tensor([i for i in range(L) if leader[i] == i and w[i] != 0], dtype=torch.long)
        plain = {k: v for k, v in fd.items() if k not in ("symmetry_residues", "symmetry_weights")}
        st, tk, scan = self._mutation_arguments(plain, positions, tokens, sites, site_tokens, False)
        _require_counted(st, w)
        st_x, tk_x = expand_group_sites(st, tk, groups, L)
        return (ties, groups, leader, st, tk, scan, st_x, tk_x) + flat_sites_and_variants(st_x, tk_x, 1, L)

    def _class_scan_arguments(self, fd, positions, tokens, sites, site_tokens, pairs):
        """The checked arguments of the paired scan (no device needed) -> what _group_scan_arguments returns — the ties
        read with class tables, st / tk as NAMED, st_x / tk_x from expand_class_sites — and the scan form's own result keys.  pairs=True
        (scan form only, no `tokens`): every scanned unit once from its listed-first member over the class axis, one variant per class
        every member has and whose first-member token lies in that member's polymer alphabet; a unit of one: lanes = tokens."""
        if fd.get("state_weights") is not None:
            raise NotImplementedError("score_mutations(tied=True, classes=True): state_weights are not supported (states joined with "
                                      "pairs: a pair over M states is 2 M edits of a site's 8)")
        if fd.get("pair_terms") is not None:
            raise NotImplementedError("score_mutations(tied=True, classes=True): pair_terms are not supported (score_tied reads none)")
        _require_one_complex(fd, "score_mutations", None)
        L = fd["S"].shape[1]
        ties = self._conditional_arguments(fd, 1, L, None, True, True)
        units = [([int(r) for r in flat], [list(C) for C in ft]) for flat, _, ft, _, _ in (ties["tied"] if ties is not None else ())]
        host = lambda key: [int(v) for v in fd[key][0].reshape(-1).tolist()]
        S0 = host("S")
        leader, unit_of = list(range(L)), {}
        for members, tables in units:
            if class_lane(tables, {t: S0[r] for t, r in enumerate(members)}) < 0:
                raise ValueError(f"feature_dict['S'] matches no class of the unit of residue {members[0]}: a tied scan has no base there")
            for r in members:
                leader[r], unit_of[r] = members[0], (members, tables)
        w = _counted_weights(fd)
        general = sites is not None or site_tokens is not None
        if positions is None and not general:
            positions = torch.tensor([i for i in range(L) if leader[i] == i and w[i] != 0], dtype=torch.long)
        extra = {}
        if pairs:
            if general:
                raise ValueError("pairs=True belongs to the scan form: a general site lists its residues itself")
            if tokens is not None:
                raise ValueError("score_mutations(tied=True, classes=True, pairs=True) scans the class axis: it takes no tokens")
            prot, dna, rna = host("protein_mask"), host("dna_mask"), host("rna_mask")
            firsts, seen = [], set()
            for p in _positions_argument(positions, L):
                if leader[p] not in seen:
                    seen.add(leader[p])
                    firsts.append(leader[p])
            lanes = []
            for f in firsts:
                members, tables = unit_of.get(f, ([f], [list(range(spec.N_CLASS_LANES))]))
                alpha = polymer_alphabet(prot[f], dna[f], rna[f], S0[f])
                lanes.append([c for c in range(spec.N_CLASSES if f in unit_of else len(spec.RESTYPES))
                              if all(C[c] >= 0 for C in tables) and tables[0][c] in alpha])
            T = sorted({c for ls in lanes for c in ls})
            valid = np.array([[c in ls for c in T] for ls in lanes], bool).reshape(len(firsts), len(T))
            st = np.full((len(firsts), 2), -1, np.int64)
            ctok = np.full((len(firsts), len(T), 2), -1, np.int64)
            rows = []
            for q, f in enumerate(firsts):
                members, tables = unit_of.get(f, ([f], [list(range(spec.N_CLASS_LANES))]))
                st[q, :min(2, len(members))] = members[:2]
                for k, c in enumerate(T):
                    if valid[q, k]:
                        ctok[q, k, :min(2, len(members))] = [C[c] for C in tables[:2]]
                        rows.append([q] + [max(int(t), 0) for t in ctok[q, k]])
            tk = np.array(rows, np.int64).reshape(len(rows), 3)
            scan = {"positions": firsts, "tokens": T, "valid": valid}
            extra = {"classes": torch.tensor(T, dtype=torch.long), "class_tokens": torch.from_numpy(ctok)}
        else:
            plain = {k: v for k, v in fd.items() if k not in ("symmetry_residues", "symmetry_weights", "symmetry_token_maps", "paired_residues",
                                                              "paired_weights", "paired_wobble", "paired_wobble_bias")}
            st, tk, scan = self._mutation_arguments(plain, positions, tokens, sites, site_tokens, False)
        _require_counted(st, w)
        st_x, tk_x = expand_class_sites(st, tk, units, L)
        return (ties, [m for m, _ in units], leader, st, tk, scan, st_x, tk_x) + flat_sites_and_variants(st_x, tk_x, 1, L) + (extra,)

    def _score_group_mutations(self, fd, positions, tokens, sites, site_tokens, pairs, method, classes=False):
        """score_mutations(tied=True) — the symmetric scan: which point mutations of a tied design change its likelihood
        under the distribution tied sample() draws from.  One complex; feature_dict["symmetry_residues"] / ["symmetry_weights"] are read
        as score_tied() reads them (listed order, a group with a masked member is not tied, the caps of conditional_probs(tied=True));
        T = 1, no bias, special tokens kept, score()'s order as rank0.  A site names 1 to s residues and every named residue stands for
        its whole unit: the edit goes to ALL members of its group with the same token (identity maps), so the device site is the
        expanded list of flat residues (more than 8: ValueError; two named residues of one unit in a site: ValueError; a named residue
        with mask * chain_mask == 0: ValueError; feature_dict["S"] not tie-consistent on a tied group: ValueError).  The scan form's
        default positions are the listed-first members of the units whose leader has mask * chain_mask != 0.  symmetry_token_maps,
        paired_residues, pairs=True, paired_wobble, pair_terms: NotImplementedError.  Without any tie every unit is a unit of one.
        delta_log_likelihood[v] = score_tied(fd, S_v)["log_likelihood"] - score_tied(fd, S)["log_likelihood"] = the sum over the counted
        units u of w_u (unit_v[u] - unit[u]), unit[u] = log_softmax(sum over the members t of u, listed order, of weight_t row_t)[token],
        row_t the member's log-softmax row of the tied stream (keys; forward / backward / hidden-backward edges).  Returns what
        score_mutations returns — "sites" / "site_tokens" as named, "loss" / "base_loss" / "base_token_log_probs" [L] on units (the
        unit's value at every member), the sparse own-entry rows as today ("base_log_probs" is None where no attached call ran) — and adds
        "leader" int64 [L] and the sparse units "unit_offsets" int64 [n + 1], "unit_residue" int32 (the unit's listed-first member,
        ascending per variant), "unit_log_prob" float32: one entry per unit with a member in U_3(site).
        method: "cone" — namp_group_mutations (include/namp.h) carried by one decoder call per chunk; "dense" — the explicit library
        [S; S_v ...] through score_tied(method="auto"): every layer count and precision mode; "auto" — the cone where it applies and
        the mean of sum_l |U_l(site)| over the variants is at most 2 L.
        classes=True — the paired scan: the ties are every tie score_tied() reads on one backbone, read with class
        tables (_class_scan_arguments); the units are total[c] = sum_t weight_t row_t[C_t[c]] + b_u[c] over the classes every member
        has, clp = log_softmax(total), unit = logsumexp of clp over the classes that match the members' tokens; a variant's class per
        touched unit is class_lane's and every member gets its token (expand_class_sites).  The cone is namp_class_mutations; the result
        adds "sites_flat" / "site_tokens_flat" (the expanded sites and the tokens every member received) and, with pairs=True,
        "classes" int64 [T] and "class_tokens" int64 [P, T, 2] (-1: no such class) beside "delta" [P, T]."""
        class_keys = {}
        if classes:
            *args, class_keys = self._class_scan_arguments(fd, positions, tokens, sites, site_tokens, pairs)
        else:
            args = self._group_scan_arguments(fd, positions, tokens, sites, site_tokens, pairs)
        ties, groups, leader_l, st, tk, scan, st_x, tk_x, sites8, tok9 = args
        S_true, mask = fd["S"], fd["mask"]
        L, n, n_sites, Vn = S_true.shape[1], len(tk), len(st), self.num_letters
        cone_ok = self._item_routes_ok("score_mutations", method, "dense")
        _require_device(fd["X"], "X")
        dev = fd["X"].device
        cm = (mask * fd["chain_mask"])[0] != 0
        leader = torch.tensor(leader_l, dtype=torch.long, device=dev)
        counted = torch.zeros(L, dtype=torch.bool, device=dev)
        counted[leader] = True
        counted &= cm
        out = _scan_head(st, tk, dev, leader=leader)
        use_cone, base, btlp, order = False, None, None, None
        if cone_ok and method != "dense" and n_sites:
            o = self._decoding_order(mask, fd["chain_mask"], fd["randn"])
            h_V, h_E, E_idx = self.encode(fd, order=o)
            self._check_tokens(S_true)
            o.wait()
            order = o.order[0]
            K = E_idx.shape[2]
            inputs = self._item_decoder_inputs(h_V, h_E, E_idx, S_true, mask, o.rank[:1], 1, L)
            if ties is None:
                nxt = torch.full((L,), -1, dtype=torch.int32)
                first, gw = torch.zeros(L, dtype=torch.int32), torch.ones(L, dtype=torch.float32)
                sec = torch.cat((nxt, first, first, gw.view(torch.int32), torch.arange(Vn, dtype=torch.int32),
                                 torch.full((spec.N_CLASS_LANES - Vn,), -1, dtype=torch.int32), torch.zeros(spec.N_CLASS_LANES, dtype=torch.int32)))
            else:
                sec = ties["section"]
                nxt, first, gw = sec[:L], sec[L:2 * L], sec[3 * L:4 * L].view(torch.float32)
            base = torch.empty(1, L, Vn, device=dev)
            per_row = ("row_residue", "row_token_log_prob", "unit_residue", "unit_log_prob")
            if classes:                                    # (the group section of namp_tied_score as it stands, behind w)
                n_tab = 1 if ties is None else ties["n_tables"]
                tail = torch.cat((cm.float(), sec.view(torch.float32).to(dev)))
                route = _ConeRoute("class_mutations", L, K, (L, K, 3, n_tab, spec.N_CLASSES), (n_tab, spec.N_CLASSES),
                                   f"score_mutations: no workspace for the class scan L={L} K={K} tables={n_tab}", sites8, tok9, tail,
                                   {"delta": ()}, per_row)
            else:
                tail = torch.cat((cm.float(), torch.cat((nxt, first)).view(torch.float32).to(dev), gw.to(dev)))
                route = _ConeRoute("group_mutations", L, K, (L, K, 3), (), f"score_mutations: no workspace for the group scan L={L} K={K}",
                                   sites8, tok9, tail, {"delta": ()}, per_row)
            got = self._cone_scan(route, inputs, base, tk[:, 0], method)         # (the plan call: sizes, base rows, base units)
            out["site_rows"], btlp, use_cone = got["site_rows"], got["base_units"], got["use_cone"] and n > 0
        if use_cone:
            delta, offs, rres, rlp, chunks = (got[k] for k in ("delta", "row_offsets", "row_residue", "row_token_log_prob", "chunks"))
            uoffs, ures, ulp = _sparse_units(got, n, L)                          # (ascending in the unit's listed-first member)
        else:
            lib = self.score_tied(fd, _variant_library(S_true, st_x, tk_x, "first"), method="auto")
            tlp, own = lib["token_log_probs"], lib["member_log_probs"][:, 0]
            if not torch.equal(lib["leader"], leader):
                raise RuntimeError("score_mutations(tied=True): score_tied reads other units than the scan")
            delta = lib["log_likelihood"][1:] - lib["log_likelihood"][0]
            btlp, order = tlp[0].clone(), lib["decoding_order"]
            units = torch.nonzero(leader == torch.arange(L, device=dev))[:, 0]
            offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
            rres = torch.arange(L, dtype=torch.int32, device=dev).repeat(n)
            rlp = own[1:].reshape(-1)
            uoffs = torch.arange(n + 1, dtype=torch.int64, device=dev) * units.numel()
            ures = units.to(torch.int32).repeat(n)
            ulp = tlp[1:][:, units].reshape(-1)
            chunks = lib["chunks"]
        denom = counted.float().sum() + 1e-8
        base_loss = -torch.where(counted, btlp, torch.zeros_like(btlp)).sum() / denom
        extra = {"unit_offsets": uoffs, "unit_residue": ures, "unit_log_prob": ulp}
        if classes:
            extra.update({"sites_flat": torch.from_numpy(st_x).to(dev), "site_tokens_flat": torch.from_numpy(tk_x).to(dev),
                          **{k: v.to(dev) for k, v in class_keys.items()}})
        return self._scan_result(out, scan, delta, base_loss, denom, btlp, base, order, (offs, rres, rlp), extra, chunks, use_cone)

    @staticmethod
    def _tied_combine_plan(ties, classes, dev):
        """The tied groups of a score_tied() call, bucketed by their size, as device tensors -> [(members [G, m], tables [G, m, W],
        weights [G, m], have [G, W]: the classes every member has, class bias [G, W] or None)]; W = vocab (token maps) or 64."""
        buckets = {}
        for flat, fw, ft, gb, _ in (ties["tied"] if ties is not None else ()):
            buckets.setdefault(len(flat), []).append((flat, fw, ft, gb))
        plan = []
        for m_, groups in sorted(buckets.items()):
            idx = torch.tensor([g[0] for g in groups], device=dev)
            w = torch.tensor([g[1] for g in groups], dtype=torch.float32, device=dev)
            T = torch.tensor([g[2] for g in groups], device=dev)
            have = (T >= 0).all(1)
            bias = None
            if classes:
                have = have & (torch.arange(T.shape[2], device=dev) < spec.N_CLASSES)[None, :]
                bias = torch.tensor([g[3] for g in groups], dtype=torch.float32, device=dev)
            plan.append((idx, T, w, have, bias))
        return plan

    @staticmethod
    def _tied_combine(rows, S_flat, plan):
        """The combine of score_tied()'s torch routes: rows [n, N, vocab] the members' logits or log-softmax rows (one constant per
        member cancels), S_flat [n, N] the sequences on the flattened graph, plan: _tied_combine_plan -> (unit log-probs [n, N], every
        member of a group carrying the group's value, -inf where the sequence breaks the tie; the own entries of the own log-softmax
        [n, N]).  Per group the members are summed in listed order; the bias is added last."""
        own = torch.log_softmax(rows, -1).gather(2, S_flat[:, :, None])[:, :, 0]
        unit = own.clone()
        n, ninf = rows.shape[0], float("-inf")
        for idx, T, w, have, bias in plan:
            G, m_, W = T.shape
            s = S_flat[:, idx]                                                 # [n, G, m]
            z = rows[:, idx].gather(3, T.clamp(min=0)[None].expand(n, G, m_, W))     # [n, G, m, W]: z_t[C_t[c]]
            total = w[None, :, 0, None] * z[:, :, 0]
            for t in range(1, m_):
                total = total + w[None, :, t, None] * z[:, :, t]
            if bias is not None:
                total = total + bias[None]
            clp = torch.log_softmax(torch.where(have[None], total, torch.full_like(total, ninf)), -1)
            match = have[None] & (T[None] == s[..., None]).all(2)
            hit = torch.where(match, clp, torch.full_like(clp, ninf))
            mx = hit.max(-1).values
            val = mx + torch.log(torch.exp(hit - torch.where(mx > ninf, mx, torch.zeros_like(mx))[..., None]).sum(-1))
            unit[:, idx.reshape(-1)] = torch.where(mx > ninf, val, mx)[:, :, None].expand(n, G, m_).reshape(n, G * m_)
        return unit, own

    @torch.no_grad()
    def score_tied(self, feature_dict, S_lib=None, method="auto"):
        """The joint log-likelihood of one or many tie-consistent sequences under exactly the distribution tied sample() draws from
        (DESIGN.md 5.15): what the tied branch of the sampler computes when every token is forced — T = 1, no `bias`, no omit, no pair
        terms, special tokens kept: the conventions of conditional_probs().  One input complex (B != 1: ValueError); with state_weights
        X is [M, L, A, 3] and the shared entries [1, L], as in sample().  S_lib: int [n, L], None = feature_dict["S"] as the one
        sequence; ids outside [0, vocab) raise IndexError; n = 0 is legal.
        Context states (state_S / state_mask beside state_weights): the tokens of S_lib at fixed positions are replaced
        per state by state_S, a unit is the set of PRESENT copies, residue i reports through its first present copy, member_log_probs is
        zero at absent copies, and "state_log_likelihood" [n, M] is added: the untied own-entry log-likelihood of the counted positions
        present in state m.  A unit of one present copy whose state weight is not 1: stream and sampler only ("items":
        NotImplementedError).
        Ties are read as conditional_probs(tied=True, classes=<paired_wobble asked>) reads them (mapped_groups(fixed=None), LISTED
        order; with states the union across the states in flat indices m * L + i, state-major, weights w_m * w_member; a group with a
        masked member is not tied: its residues are units of one; more than hip.loo_group_max() members, more than 64 distinct tables,
        a residue in two groups: ValueError).
        The stream.  With order0 score()'s order on the flattened graph, groups are visited when order0 reaches their first member and
        the members follow each other in listed order: key(i) = (min of rank0 over i's group, listed position of i).  An edge i <- j
        is forward when key(j) >= key(i) (the encoder state, no token), hidden-backward when key(j) < key(i) and j is in i's group (j's
        decoder state of the layer WITHOUT j's token) and backward otherwise (the decoder state plus the token S_k[j]).  Per group with
        member logits z_t, without classes total[a] = sum_t w_t z_t[P_t[a]] in listed order, lp = log_softmax(total), the group token is
        a = P_1[S_k[m_1]], the unit's log-prob lp[a] if P_t[a] == S_k[m_t] for every t; with classes total[c] = sum_t w_t z_t[C_t[c]] +
        b[c] over the classes every member has, clp = log_softmax(total), the unit's log-prob the logsumexp of clp[c] over {c : C_t[c] ==
        S_k[m_t] for all t}.  A sequence that breaks the tie of a group has -inf there.  A unit of one is the own entry of log_softmax(z).
        Returns "S" [n, L]; "token_log_probs" float32 [n, L] (the log-prob of the unit residue i belongs to: every member of a group
        carries the group's value); "leader" int64 [L] (the listed-first member of each residue's unit, in state 0's block);
        "log_likelihood" [n] (the sum of token_log_probs[:, leader] over the distinct units whose leader has mask * chain_mask != 0);
        "member_log_probs" [n, M, L] (the own-entry untied log-prob of every state's copy, from the same stream; M = 1 without states);
        "consistent" bool [n] (every counted unit finite); "decoding_order"; "chunks" (decoder calls made); "method" (the route taken).
        method: "items" — every (sequence, flat residue) of a chunk is an item of every layer of the item kernel of the cone
        conditionals (namp_tied_score, include/namp.h), score_library_tokens // (M L) sequences per call, nothing read back: three
        decoder layers and message_precision "x3" or "fp32" (NotImplementedError otherwise).  "stream" — the ordinary decoder with the
        M states as the encoder batch and the sequences times M as streams, combined in torch; hidden-backward edges are the one
        difference from the ordinary decoder run with `key` as its rank and exist only where two members of a group are graph
        neighbours, so the route is defined with state_weights alone or no tie at all (ValueError otherwise).  "sampler" — the slow
        route and on-device check: teacher-forced design calls (chain_mask all ones, a randn whose sort reproduces order0, T = 1, zero
        bias, S_forced = the sequences as batch_size streams, the groups without a masked member as symmetry groups), the log_probs rows
        combined in torch: every number of decoder layers and every precision mode.  "auto" — stream where defined, else items where
        it applies, else sampler; decided from what the host knows, with no read-back."""
        if method not in ("auto", "items", "stream", "sampler"):
            raise ValueError(f"method must be 'auto', 'items', 'stream' or 'sampler'; got {method!r}")
        fd = feature_dict
        _require_one_complex(fd, "score_tied", None)
        S_true, mask = fd["S"], fd["mask"]
        L = S_true.shape[1]
        state_w, M, ctx, present = None, 1, None, None
        if fd.get("state_weights") is not None:
            state_w, M, L, ctx = self._state_arguments_of(fd)
        elif fd.get("state_S") is not None or fd.get("state_mask") is not None:
            raise ValueError("score_tied: state_S / state_mask need state_weights")
        if ctx is not None:
            if "present" not in ctx[2]:                    # (one read-back per checked set of tensors)
                ctx[2]["present"] = tuple(tuple(bool(v) for v in row) for row in ctx[1].tolist())
            present = ctx[2]["present"]
        classes = self._wobble_arguments(fd)[2]
        ties = self._conditional_arguments(fd, 1, L, state_w, True, classes, present)
        if S_lib is None:
            S_lib = S_true
        S_lib = torch.as_tensor(S_lib)
        if S_lib.dim() != 2 or S_lib.dtype.is_floating_point or S_lib.dtype == torch.bool or S_lib.shape[1] != L:
            raise ValueError(f"S_lib must be an integer tensor [n, {L}]; got {tuple(S_lib.shape)}")
        n = S_lib.shape[0]
        if n:
            self._check_tokens(S_lib, "S_lib")
        pairs, sym = fd.get("paired_residues"), fd.get("symmetry_residues")
        listed = not (pairs is None or len(pairs) == 0) or not (sym is None or len(sym) == 0 or (len(sym) == 1 and len(sym[0]) == 0))
        if method == "stream" and listed:
            raise ValueError("score_tied(method='stream') is defined with state_weights alone or no tie at all: two members of a listed "
                             "group can be graph neighbours; use method='items' or 'sampler'")
        items_ok = self._item_routes_ok("score_tied", method, "sampler")
        # (context states: a unit of ONE present copy still draws from softmax(w_m logits_m); the item kernel's unit of one is the own
        #  entry of log_softmax(logits_m), so that route serves such units with weight 1 only)
        weighted_singles = ctx is not None and any(wr != 1.0 for _, wr in ties["singles"])
        if method == "items" and weighted_singles:
            raise NotImplementedError("score_tied(method='items'): a residue present in one state only whose state weight is not 1; "
                                      "use method='stream' or 'sampler'")
        if method == "auto":
            method = "stream" if not listed else ("items" if items_ok and not weighted_singles else "sampler")
        _require_device(fd["X"], "X")
        dev, N, Vn = fd["X"].device, M * L, self.num_letters
        S_lib = S_lib.to(dev).long().contiguous()
        leader = list(range(L))
        for flat, *_ in (ties["tied"] if ties is not None else ()):
            for r in flat:
                if r < L:
                    leader[r] = flat[0]
        seat = None
        if ctx is not None:
            # Context states: every state's copy holds the sequence's token where the design draws one and its own state_S elsewhere;
            # residue i speaks through its first present copy (its seat), and its leader is the residue of the unit's listed-first member
            state_S, state_mask = ctx[:2]
            designable = ((mask * fd["chain_mask"])[0] != 0)
            pres_t = state_mask != 0                                             # [M, L]
            absent = ((mask != 0) & ~pres_t).reshape(N)
            rows_of = lambda S_k: torch.where(designable[None, None, :], S_k[:, None, :], state_S[None])      # [n, M, L]
            seat = [next((s_ * L + i for s_ in range(M) if present[s_][i]), i) for i in range(L)]
            leader = list(range(L))
            for flat, *_ in ties["tied"]:
                for r in flat:
                    if seat[r % L] == r:
                        leader[r % L] = flat[0] % L
            seat = torch.tensor(seat, dtype=torch.long, device=dev)
        leader = torch.tensor(leader, dtype=torch.long, device=dev)
        unit_lp, member_lp = torch.empty(n, N, device=dev), torch.empty(n, N, device=dev)
        chunk = max(1, min(self.score_library_tokens // N, ((1 << 28) - 1) // N))
        chunks = 0
        if method == "sampler":
            o = self._decoding_order(mask, fd["chain_mask"], fd["randn"][:1])
            o.wait()
            order0 = o.order[0]
            keep = {k: v for k, v in fd.items() if k not in ("paired_residues", "paired_weights", "paired_wobble", "paired_wobble_bias",
                                                              "symmetry_residues", "symmetry_weights", "symmetry_token_maps", "pair_bias",
                                                              "pair_terms", "S_forced")}
            randn = torch.empty(L, device=dev)
            randn[order0] = torch.arange(1, L + 1, dtype=torch.float32, device=dev)
            randn = torch.where(mask[0] != 0, randn, randn * 1e4)              # (a masked residue's sort key is 1e-4 |randn|: its place again)
            ident = list(range(Vn))
            groups = [(flat[:len(gw)], gw, ft[:len(gw)]) for flat, _, ft, _, gw in (ties["tied"] if ties is not None else ()) if len(gw) > 1]
            if ctx is not None:                            # (a state-0 copy may be absent: the groups in residue terms)
                groups = ties["listed"]
            one = dict(keep, chain_mask=torch.ones_like(fd["chain_mask"]), temperature=1.0, bias=torch.zeros(1, L, Vn, device=dev))
            if groups:
                one.update(symmetry_residues=[g for g, _, _ in groups], symmetry_weights=[gw for _, gw, _ in groups])
                if not classes and any(list(P) != ident for _, _, gm in groups for P in gm):    # (the members' own rows do not depend on the maps)
                    one["symmetry_token_maps"] = [gm for _, _, gm in groups]
            else:
                one.update(symmetry_residues=[[]], symmetry_weights=[[]])
            plan = self._tied_combine_plan(ties, classes, dev)
            # what the design call must report: with states score()'s order (the states of a residue side by side are implied), else
            # the residues sorted by their keys — the groups visited when order0 reaches their first member, in listed order
            visits = order0
            if groups and state_w is None and n:
                rank0 = [0] * L
                for t, r in enumerate(order0.tolist()):
                    rank0[r] = t
                key = tied_stream_keys(rank0, [g for g, _, _ in groups])[0]
                visits = torch.tensor(sorted(range(L), key=key.__getitem__), device=dev)
            for k0 in range(0, n, chunk):
                k1 = min(n, k0 + chunk)
                S_k = S_lib[k0:k1]
                call = dict(one, randn=randn[None].expand(k1 - k0, L).contiguous(), batch_size=k1 - k0, S_forced=S_k)
                if ctx is not None:
                    call["S_forced_states"] = rows_of(S_k)
                got = self._sample(call, self.sample_level_walk)
                if not torch.equal(got["decoding_order"][0], visits):
                    raise RuntimeError("score_tied: the design call did not visit the residues in the order of the tied stream")
                lp_rows = got["log_probs"].reshape(k1 - k0, N, Vn)
                if ctx is None:
                    u, own = self._tied_combine(lp_rows, S_k.repeat(1, M), plan)
                else:
                    S_flat = rows_of(S_k).reshape(k1 - k0, N)
                    u, own = self._tied_combine(lp_rows, S_flat, plan)
                    for r, wr in ties["singles"]:                              # a unit of one present copy: softmax(w_m logits_m)
                        u[:, r] = torch.log_softmax(wr * lp_rows[:, r], -1).gather(1, S_flat[:, r, None])[:, 0]
                unit_lp[k0:k1], member_lp[k0:k1] = u, own
                chunks += 1
        else:
            o = self._decoding_order(mask, fd["chain_mask"], fd["randn"][:1] if state_w is not None else fd["randn"])
            h_V, h_E, E_idx = self._encode_side_by_side(fd, o, state_w, M, L, ctx)
            self._check_tokens(S_true)
            o.wait()
            order0, rank = o.order[0], o.rank[:1]
        if method == "stream":
            # no group has two members in one state's block: the ordinary decoder with key = the rank of score() is the tied stream
            sw = torch.tensor([1.0] if state_w is None else state_w, dtype=torch.float32, device=dev)
            tied_res = (mask[0] != 0) if (state_w is not None and M > 1) else torch.zeros(L, dtype=torch.bool, device=dev)
            E_long = E_idx.long()
            for k0 in range(0, n, max(1, chunk)):
                k1 = min(n, k0 + chunk)
                nk = k1 - k0
                S_k = S_lib[k0:k1]
                if ctx is not None:
                    # every state decodes its own token row under its own presence; the unit of a residue sums its present copies in
                    # state order and has a value where they all hold one token (they can differ at fixed positions only)
                    rows = rows_of(S_k)
                    lp, lg = self.decode_graph(h_V, h_E, E_long, rows.reshape(nk * M, L), state_mask.repeat(nk, 1), rank.expand(nk * M, L),
                                               want_logits=True)
                    lp, lg = lp.view(nk, M, L, Vn), lg.view(nk, M, L, Vn)
                    own = lp.gather(3, rows[..., None])[..., 0]                                # [nk, M, L]
                    total = None
                    for m_ in range(M):
                        term = torch.where(pres_t[m_][None, :, None], sw[m_] * lg[:, m_], torch.zeros_like(lg[:, m_]))
                        total = term if total is None else total + term
                    tok = rows.reshape(nk, N)[:, seat]                                         # [nk, L]
                    same = ((rows == tok[:, None, :]) | ~pres_t[None]).all(1)
                    tied_lp = torch.log_softmax(total, -1).gather(2, tok[:, :, None])[:, :, 0]
                    tied_lp = torch.where(same, tied_lp, torch.full_like(tied_lp, float("-inf")))
                    u = torch.where((tied_res[None, :] & pres_t)[None], tied_lp[:, None, :].expand(nk, M, L), own)
                    unit_lp[k0:k1], member_lp[k0:k1] = u.reshape(nk, N), own.reshape(nk, N)
                    chunks += 1
                    continue
                S_dec = S_k[:, None, :].expand(nk, M, L).reshape(nk * M, L)
                lp, lg = self.decode_graph(h_V, h_E, E_long, S_dec, mask.expand(nk * M, L), rank.expand(nk * M, L), want_logits=True)
                lp, lg = lp.view(nk, M, L, Vn), lg.view(nk, M, L, Vn)
                own = lp.gather(3, S_k[:, None, :, None].expand(nk, M, L, 1))[..., 0]          # [nk, M, L]
                total = None
                for m_ in range(M):                                                            # (listed order: state-major)
                    term = sw[m_] * lg[:, m_]
                    total = term if total is None else total + term
                tied_lp = torch.log_softmax(total, -1).gather(2, S_k[:, :, None])[:, :, 0]     # [nk, L]
                u = torch.where(tied_res[None, None, :], tied_lp[:, None, :].expand(nk, M, L), own)
                unit_lp[k0:k1], member_lp[k0:k1] = u.reshape(nk, N), own.reshape(nk, N)
                chunks += 1
        elif method == "items":
            K = E_idx.shape[2]
            n_cls = spec.N_CLASSES if classes else Vn
            if ties is None:                               # no tie at all: every residue a unit of one under the identity table
                ident = list(range(Vn)) + list(range(Vn, spec.N_CLASS_LANES))
                section = torch.tensor([-1] * N + [0] * N + [0] * N, dtype=torch.int32)
                section = torch.cat((section, torch.ones(N, dtype=torch.float32).view(torch.int32), torch.tensor(ident, dtype=torch.int32),
                                     torch.zeros(spec.N_CLASS_LANES, dtype=torch.int32)))
                n_tab = 1
            else:
                section, n_tab = ties["section"], ties["n_tables"]
                if not classes:                            # (token maps come without a bias block: zeros)
                    section = torch.cat((section, torch.zeros(n_tab * spec.N_CLASS_LANES, dtype=torch.int32)))
            section = section.to(dev)
            inputs = self._item_decoder_inputs(h_V, h_E, E_idx, S_true, mask, rank, M, L, ctx)
            seq32 = (S_lib if M == 1 else S_lib.repeat(1, M)).to(torch.int32)
            if ctx is not None and n:
                seq32 = rows_of(S_lib).reshape(n, N).to(torch.int32)
            rows0 = torch.empty(1, N, Vn, device=dev)             # the carrier's log_probs (the first sequence's own rows): the call requires it
            for k0 in range(0, n, chunk):
                k1 = min(n, k0 + chunk)
                nk = k1 - k0

                def fill(sec):
                    sec = sec[:4 * (section.numel() + nk * N)].view(torch.int32)
                    sec[:section.numel()] = section
                    sec[section.numel():] = seq32[k0:k1].reshape(-1)
                got = self._attached_decoder_call("tied_score", (N, K, 3, n_tab, n_cls, nk), (n_tab, n_cls, nk), fill, inputs, rows0, N, K,
                                                  f"score_tied: no workspace for N={N} K={K} tables={n_tab} sequences={nk}")
                unit_lp[k0:k1] = got["unit_log_probs"].view(nk, N)
                member_lp[k0:k1] = got["member_log_probs"].view(nk, N)
                chunks += 1
        tlp = (unit_lp[:, :L] if seat is None else unit_lp[:, seat]).contiguous()
        cm = (mask * fd["chain_mask"])[0] != 0
        counted = torch.zeros(L, dtype=torch.bool, device=dev)
        counted[leader] = True                                                 # one slot per distinct unit: its leader's
        counted &= cm
        picked = tlp[:, counted]
        out = {"S": S_lib, "token_log_probs": tlp, "leader": leader, "log_likelihood": picked.sum(-1), "units": counted.sum(),
               "member_log_probs": member_lp.view(n, M, L), "consistent": torch.isfinite(picked).all(-1), "decoding_order": order0,
               "chunks": chunks, "method": method}
        if ctx is not None:
            # an absent copy scores nothing; per state the untied own-entry log-likelihood of the designed positions present there:
            # what ranks designs by their on-target / off-target gap
            own = member_lp.masked_fill(absent[None, :], 0.0).view(n, M, L)
            out["member_log_probs"] = own
            out["state_log_likelihood"] = torch.where((cm[None, :] & pres_t)[None], own, torch.zeros_like(own)).sum(-1)
        return out

    def _wobble_arguments(self, fd, n_pairs=None):
        """feature_dict["paired_wobble"] / ["paired_wobble_bias"] in one normal form -> (wobble, wobble_bias, asked): each None, a scalar
        or a list with one entry per pair; asked: some pair asks for wobble.  With n_pairs the lists are checked against the pairs."""
        to_list = lambda v: v.detach().reshape(-1).tolist() if torch.is_tensor(v) else (list(v) if hasattr(v, "__len__") else v)
        wobble, wobble_bias = to_list(fd.get("paired_wobble")), to_list(fd.get("paired_wobble_bias"))
        asked = any(wobble) if isinstance(wobble, list) else bool(wobble)
        if n_pairs is not None:
            for v, what in ((wobble, "paired_wobble"), (wobble_bias, "paired_wobble_bias")):
                if isinstance(v, list) and len(v) != n_pairs:
                    raise ValueError(f"{what} has {len(v)} entries for {n_pairs} pairs")
            if asked and n_pairs == 0:
                raise ValueError("paired_wobble needs paired_residues")
        return wobble, wobble_bias, asked

    def _pair_polymer(self, fd, pairs, L, dna, rna, m):
        """The polymer type of every residue for mapped_groups (1 DNA, 2 RNA, else 0).  A residue the parser masks (a 5' nucleotide
        without its phosphate) comes without a polymer flag: its pair partner's type stands in for its own."""
        polymer = [1 if d else (2 if r else 0) for d, r in zip(dna, rna)]
        for pr in pairs:
            for r, q in ((int(pr[0]), int(pr[1])), (int(pr[1]), int(pr[0]))):
                if 0 <= r < L and 0 <= q < L and not m[r] and polymer[r] == 0 and polymer[q] in (1, 2) \
                        and not self._host_list(fd["protein_mask"], "protein_mask")[r]:
                    polymer[r] = polymer[q]
        return polymer

    def _conditional_arguments(self, fd, B, L, state_w=None, tied=False, classes=False, present=None):
        """The ties of a conditional_probs(tied, classes) call — base pairs alone with tied=False, every tie with tied=True; spoken in
        token maps, with classes=True in class tables — -> None with nothing to tie, else
        {"tied": [(members, weights, tables, class bias or None, listed weights)] what the device ties (no masked member): flat indices
        (state-major with states), the weights with the state weight, a map [vocab] or class table [64] per member; listed weights: those
        of the members in [0, L) without the state weight, for the slow route's design call,
        "index": int64 [n, width] the members padded with -1 (tied=False: [n, 2]),
        "section": the int32 input section of the workspace (include/namp.h: next, first, table_idx, weight bits, tables [n_tables][64],
        with classes the bias bits [n_tables][64]; table 0 is the identity; tables are told apart by (table, bias)), "n_tables"}.
        state_w: None or the M state weights.  present: None, or with context states a tuple of M tuples of L bools —
        a group without a masked residue is tied over its PRESENT copies only; "singles": [(flat index, weight)] the groups one present
        copy is left of (a unit of one whose logits still carry their weight), "listed": [(residues, weights, tables)] the tied groups in
        residue terms, for the slow route's design call."""
        pairs, sym = fd.get("paired_residues"), fd.get("symmetry_residues")
        pairs = None if pairs is None or len(pairs) == 0 else pairs
        sym = None if sym is None or len(sym) == 0 or (len(sym) == 1 and len(sym[0]) == 0) else sym
        wobble, wobble_bias, asked = self._wobble_arguments(fd)
        if not tied:
            if pairs is None:
                return None
            if asked and not classes:
                raise NotImplementedError("conditional_probs: paired_wobble is not supported; pair classes (DESIGN.md 5.8) are the follow-up")
            if sym is not None:
                raise NotImplementedError("conditional_probs: paired_residues together with symmetry_residues is not supported")
            if fd.get("state_weights") is not None:
                raise NotImplementedError("conditional_probs: paired_residues together with state_weights is not supported")
        else:
            if asked and not classes:
                raise NotImplementedError("conditional_probs: paired_wobble is not supported; pair classes (DESIGN.md 5.8) change the combine")
            if pairs is None and sym is None and state_w is None:
                return None
        who = "tied groups" if tied else "paired_residues"
        if B != 1:
            raise ValueError(f"{who} expect one input complex (B == 1)")
        if self.restype_to_int is None:
            raise ValueError(("paired_residues / tied groups need" if classes else who + " need") + " the model's restype_to_int")
        if classes:
            self._wobble_arguments(fd, 0 if pairs is None else len(pairs))
        m = self._host_list(fd["mask"], "mask")
        dna = rna = None
        if pairs is not None:
            dna, rna = self._host_list(fd["dna_mask"], "dna_mask"), self._host_list(fd["rna_mask"], "rna_mask")
        # The tables of the last call of every kind (tied, classes) are kept: a resident feature_dict is scored many times, and a
        # specificity profile alternates the kinds on it — in one slot each would rebuild and page-lock its tables on every call.  The
        # host lists above are the SAME objects while their tensors are unchanged; the ties are compared by value in one normal form; a
        # call with symmetry_token_maps is never served from the cache, and its own entry, whose key says so, serves no later call.
        as_list = lambda v: v.tolist() if hasattr(v, "tolist") else v
        listed = lambda v: None if v is None else [[as_list(x) for x in g] if hasattr(g, "__len__") else g for g in v]
        key = (None if pairs is None else [(int(a), int(b)) for a, b in pairs], as_list(fd.get("paired_weights")),
               None if sym is None else [[int(r) for r in g] for g in sym], listed(fd.get("symmetry_weights")) if sym is not None else None,
               state_w, wobble if classes else None, wobble_bias if classes else None, present, fd.get("symmetry_token_maps") is None)
        last = self._tie_tables.get((tied, classes))
        if last is not None and key[-1] and last[0] == key and all(x is y for x, y in zip(last[1], (dna, rna, m))):
            return last[2]
        polymer = None if pairs is None else self._pair_polymer(fd, pairs, L, dna, rna, m)
        groups, weights, gtabs, _, *gbias = mapped_groups(L, self.restype_to_int, pairs, fd.get("paired_weights"), polymer, None, sym,
                                                          fd.get("symmetry_weights") if sym is not None else None,
                                                          fd.get("symmetry_token_maps"),            # (maps without groups: refused there)
                                                          (False if wobble is None else wobble) if classes else None, wobble_bias)
        members = [r for g in groups for r in g]
        if len(set(members)) != len(members):
            raise ValueError("conditional_probs: the tied groups must be disjoint")
        M, sw = (1, [1.0]) if state_w is None else (len(state_w), state_w)
        V, lanes = len(spec.RESTYPES), spec.N_CLASS_LANES
        # a token map goes into the section with the identity beyond the vocabulary, a class table with no class there
        ident, zero = list(range(V)) + ([-1] * (lanes - V) if classes else list(range(V, lanes))), [0.0] * lanes
        gbias = gbias[0] if classes else [zero] * len(groups)
        if state_w is not None:                            # every residue is a group across the states
            tied_res = set(members)
            for i in range(L):
                if i not in tied_res:
                    groups.append([i]); weights.append([1.0]); gtabs.append([ident[:lanes if classes else V]]); gbias.append(zero)
        N = M * L
        nxt, first, tidx, w = [-1] * N, [0] * N, [0] * N, [1.0] * N
        table, bias, index = [ident], [zero], {(tuple(ident), tuple(zero)): 0}
        tied_specs, singles, listed_groups = [], [], []
        for g, gw, gt, gb in zip(groups, weights, gtabs, gbias):
            if len(g) * M > hip.loo_group_max():
                raise ValueError(f"conditional_probs: the group of residue {g[0]} has {len(g) * M} members; at most {hip.loo_group_max()} are tied")
            if len(g) * M < 2:
                continue
            # (context states: the present copies; a group with a masked residue stays whole — the device's rule unties it below)
            here = lambda s_, r: present is None or present[s_][r] or not all(m[q] for q in g)
            flat = [r + s_ * L for s_ in range(M) for r in g if here(s_, r)]    # state-major, as _sample_states lists them
            fw = [sw[s_] * float(v) for s_ in range(M) for r, v in zip(g, gw) if here(s_, r)]
            ft = [C for s_ in range(M) for r, C in zip(g, gt) if here(s_, r)]
            if len(g) > 1 and all(m[r] for r in g):
                listed_groups.append(([int(r) for r in g], [float(v) for v in gw], [list(C) for C in gt]))
            if len(flat) < 2:
                singles += [(r, wr) for r, wr in zip(flat, fw)]
                continue
            for t, (r, wr, C) in enumerate(zip(flat, fw, ft)):
                row = (tuple(C) + tuple(range(len(C), lanes)), tuple(gb))
                k = index.get(row)
                if k is None:
                    k = index[row] = len(table)
                    table.append(list(row[0])); bias.append([float(v) for v in gb])
                nxt[r], tidx[r], w[r] = flat[(t + 1) % len(flat)], k, wr
            first[flat[0]] = 1
            if all(m[r] for r in g):                       # the device's rule: a pair / group with a masked member is not tied
                tied_specs.append((flat, fw, [list(C) for C in ft], [float(v) for v in gb] if classes else None, [float(v) for v in gw]))
        if len(table) > 64:
            raise ValueError(f"conditional_probs: {len(table)} distinct {'class tables' if classes else 'token maps'}; at most 64")
        width = 2 if not tied else max([len(t[0]) for t in tied_specs], default=0)
        words = [torch.tensor(nxt + first + tidx, dtype=torch.int32), torch.tensor(w, dtype=torch.float32).view(torch.int32),
                 torch.tensor([t for C in table for t in C], dtype=torch.int32)]
        if classes:
            words.append(torch.tensor([v for row in bias for v in row], dtype=torch.float32).view(torch.int32))
        out = {"tied": tied_specs, "singles": singles, "listed": listed_groups, "section": torch.cat(words), "n_tables": len(table),
               "index": torch.tensor([t[0] + [-1] * (width - len(t[0])) for t in tied_specs], dtype=torch.int64).reshape(len(tied_specs), width)}
        self._tie_tables[(tied, classes)] = (key, (dna, rna, m), out)
        return out

    def _tied_conditionals_by_sampling(self, fd, order0, ties, log_probs, tied, classes):
        """The slow route of the tied conditionals: per tie ONE teacher-forced design call — chain_mask all ones, a randn whose sort is
        score()'s order with the tie's residues moved to the end in listed order, T = 1, zero bias; a base pair of a tied=False call as
        the call's only pair, anything else as its only symmetry group (with its maps) — whose member rows are combined into the tie's
        rows of log_probs [1, M * L, vocab] (in place).  Returns the class rows with classes, else []."""
        S_true, mask = fd["S"], fd["mask"]
        L = S_true.shape[1]
        dev = log_probs.device
        keep = {k: v for k, v in fd.items() if k not in ("paired_residues", "paired_weights", "paired_wobble", "paired_wobble_bias",
                                                          "symmetry_residues", "symmetry_weights", "symmetry_token_maps", "pair_bias", "pair_terms",
                                                          "S_forced")}
        ones = torch.ones_like(fd["chain_mask"])
        bias = torch.zeros(1, L, self.num_letters, device=dev)
        pos = torch.arange(1, L + 1, dtype=torch.float32, device=dev)
        ident = list(range(self.num_letters))
        class_rows = []
        for flat, fw, ft, gb, gw in ties["tied"]:
            g, gm = flat[:len(gw)], ft[:len(gw)]               # the members in [0, L): state 0's
            g_t = torch.tensor(g, device=dev)
            rest = order0[~torch.isin(order0, g_t)]
            order = torch.cat((rest, g_t))
            randn = torch.empty(L, device=dev)
            randn[order] = pos
            randn = torch.where(mask[0] != 0, randn, randn * 1e4)          # (a masked residue's sort key is 1e-4 |randn|: its place again)
            one = dict(keep, chain_mask=ones, randn=randn[None], batch_size=1, temperature=1.0, bias=bias, S_forced=S_true)
            if not tied and not classes:
                one.update(paired_residues=[tuple(g)], paired_weights=tuple(gw))
            elif len(g) > 1:
                one.update(symmetry_residues=[g], symmetry_weights=[gw])
                if not classes and any(list(P) != ident for P in gm):    # (the members' own rows do not depend on the maps)
                    one["symmetry_token_maps"] = [gm]
            else:
                one.update(symmetry_residues=[[]], symmetry_weights=[[]])
            got = self._sample(one, self.sample_level_walk)
            if not torch.equal(got["decoding_order"][0], order):
                raise RuntimeError(f"conditional_probs: the design call of group {g} did not decode it last")
            lp = got["log_probs"].reshape(-1, self.num_letters)             # [M * L, vocab]
            if classes:
                rows, clp = self._class_combine(lp[flat], fw, ft, gb)
                log_probs[0, flat] = rows
                class_rows.append(clp)
                continue
            maps_t = [torch.tensor(P, device=dev) for P in ft]
            total = None
            for r, wr, P in zip(flat, fw, maps_t):
                total = wr * lp[r][P] if total is None else total + wr * lp[r][P]
            row = torch.log_softmax(total, -1)
            for r, P in zip(flat, maps_t):
                log_probs[0, r, P] = row
        return class_rows

    @staticmethod
    def _class_combine(z, ws, tables, class_bias):
        """The class combine of the slow route in torch: z [n, vocab] the members' rows in listed order, ws their weights, tables their
        class tables [n][64], class_bias [64] -> (rows [n, vocab] the members' log-marginals, clp [64] with -inf on absent classes)."""
        dev, vocab = z.device, z.shape[-1]
        T = torch.tensor(tables, device=dev)
        have = (T >= 0).all(0) & (torch.arange(T.shape[1], device=dev) < spec.N_CLASSES)
        Tc = T.clamp(min=0)
        total = None
        for zt, wt, t in zip(z, ws, Tc):
            total = float(wt) * zt[t] if total is None else total + float(wt) * zt[t]
        total = total + torch.tensor(class_bias, dtype=z.dtype, device=dev)
        neg = torch.full_like(total, -float("inf"))
        clp = torch.log_softmax(torch.where(have, total, neg), -1)
        tok = torch.arange(vocab, device=dev)
        rows = [torch.logsumexp(torch.where((t[:, None] == tok[None, :]) & have[:, None], clp[:, None], neg[:, None]), 0) for t in T]
        return torch.stack(rows), torch.where(have, clp, neg)

    def forward(self, feature_dict, decoding_randn=None):
        """Training-copy surface (na_model_utils.py:589-646): feature_dict -> (log_probs, probs).
        ``decoding_randn`` replaces the internal torch.randn (:623) when reproducibility is needed."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from . import train                      # differentiable path: HIP per-edge forward/backward + torch autograd
            self._require_reference_atom_order()
            return train.forward_train(self, feature_dict, decoding_randn)
        with torch.no_grad():
            mask = feature_dict["mask"]
            chain_M = mask
            if self.decode_protein_first:
                chain_M = chain_M.masked_fill(feature_dict["protein_mask"].to(torch.bool), 0.0)
            if decoding_randn is None:
                decoding_randn = torch.randn(chain_M.shape, device=mask.device)
            o = self._decoding_order(chain_M, None, decoding_randn)
            _, _, _, log_probs, logits = self.encode_decode(feature_dict, feature_dict["S"], o.rank, want_logits=True, idx_long=False,
                                                            order=o)
            return log_probs, torch.softmax(logits, dim=-1)

    # reference quirk (model_utils.py:186): DecLayer receives mask_t of shape [B], which broadcasts so that
    # every stream is masked with STREAM 0's mask at that step.  True reproduces it; it only matters when
    # batch_size > 1 and masked residues coexist with fixed (chain_mask = 0) ones.
    reference_sample_mask_quirk = True
    # decode the plain sampling branch by dependency level (False: the one-launch sequential walk; same results)
    sample_level_parallel = True
    # ... as ONE persistent launch walking the levels (no host read-back, warm L2); False: one launch per level
    sample_level_walk = True
    # Read the walk's barrier status back after every sample() (one small host sync per design call) and re-run with per-level launches
    # if a grid barrier gave up — on by default in cli.py (the walk needs all its workgroups co-resident; on a shared or
    # partitioned device the kernel only poisons log_probs and S would be garbage); off by default here (sample() then returns with the
    # whole design merely enqueued; call sample_walk_status() yourself).
    sample_check_walk = False
    # symmetry-tied groups whose members are not graph neighbours of each other: members decoded in parallel, one deferred draw per group
    sample_split_groups = True

    @torch.no_grad()
    def sample(self, feature_dict):
        """ProteinMPNN.sample (model_utils.py:101-327; both the plain and the symmetry-tied branch, optional
        ``pair_bias``) as one persistent HIP launch.  ``feature_dict["pair_terms"]`` is the compact form of ``pair_bias`` —
        {"partner", "table": int [B, L, D], "tables": float [n, V, V], "members": "closing" | "all"}, see pair_terms_arguments — and,
        unlike the dense tensor, goes with every tie (symmetry_residues, paired_residues, paired_wobble, state_weights).
        ``feature_dict["forbidden_motifs"]`` — a list of token tuples, or an int tensor [n, Lm] padded with -1; lengths 2..8, at most 63 —
        are motifs no draw may complete on consecutive present residues of one chain (with every tie and with
        ``pair_terms``, not with the dense ``pair_bias`` and not with k_neighbors > 128): a candidate that would complete one on any
        member of the drawing group gets p = 0 in ``sampling_probs``, a ban that would leave nothing is skipped, and ``motif_hits``
        int64 [batch] — returned with the key — counts the occurrences left in ``S``.
        With ``state_weights`` one sequence is tied across backbone states, with ``state_S`` / ``state_mask`` beside it the states also
        differ in their fixed tokens and in which residues they have (_sample_states).
        The categorical draw uses torch.rand on the device (seed with torch.manual_seed) through an inverse
        CDF instead of torch.multinomial; ``feature_dict["S_forced"]`` (optional, [batch,L]) teacher-forces."""
        return self._sample(feature_dict, self.sample_level_walk)

    def _sample(self, fd, walk, uniform=None, plan_out=None):
        """sample() with the persistent level walk on or off (`walk`) and the uniforms of the draws given (None: torch.rand).
        plan_out: a dict that receives the plan arrays of a symmetry-tied call (tests compare the routes array for array).  The plan and the
        launch are sampling.py's."""
        if fd.get("state_weights") is not None:
            return self._sample_states(fd, walk, uniform)
        bs = fd["batch_size"]
        S_true, mask, bias = fd["S"], fd["mask"], fd["bias"]
        sym, sym_weights = fd.get("symmetry_residues", [[]]), fd.get("symmetry_weights", [[]])
        B, L = S_true.shape
        dev = S_true.device
        tok_maps = pair_list = cls_bias = None
        n_maps = 0
        pterms = self._pair_terms_of(fd, B, L)
        mapped = self._mapped_arguments(fd, B, L)                                 # base pairs / token maps: mapped symmetry groups
        if mapped is not None:
            sym, sym_weights, table, idx, pair_list, cls_bias = mapped
            tok_maps, n_maps = self._token_map_array(table, idx, dev, cls_bias), len(table)
        symmetric = not (len(sym) == 1 and len(sym[0]) == 0)
        self._check_tokens(S_true)
        if fd.get("S_forced") is not None:
            self._check_tokens(fd["S_forced"], "S_forced")
        motifs = self._motifs_of(fd, B, L, symmetric)
        if pterms is not None or motifs is not None:                              # (its one copy goes up before anything is enqueued)
            _require_device(fd["X"], "X")
            pterms = self._pair_terms_section(pterms, B, B * bs, L, int(min(self.k_neighbors, L)), dev, motifs=motifs)
        o = self._decoding_order(mask, fd["chain_mask"], fd["randn"])               # [max(B, bs), L]; sorted by the featuriser launch
        order, rank = o.order, o.rank
        V, _, h_E, E_idx = self._featurize_hip(fd, want_E=False, want_hE=True, order=o)   # (E_idx stays int32: the kernels' dtype)
        K = E_idx.shape[-1]
        B_dec = B * bs
        dims, Lb = (B_dec, B, L, K), hip.lib()
        # (dep_idx, n_dep) of the levels beside the graph's — the pair terms section's partner block IS one; None: the sequential walk
        deps = (None, 0) if pterms is None else (pterms["dep"], pterms["n_dep"])
        on_device = (self.sample_level_parallel and walk and o.order32 is not None and order.shape[0] == B_dec
                     and E_idx.dtype == torch.int32 and E_idx.is_contiguous())
        plan = start = None
        # Plain branch: the dependency levels and the walk's work lists need the neighbour lists and the decoding order only — enqueued on
        # the side stream behind the featuriser launch, beside the encoder launches (with pair terms too: the pairs' device plan stands aside)
        if (not symmetric and "pair_bias" not in fd and on_device and not o.pending and L <= 16000
                and Lb.namp_decoder_sample_walk_grid(B_dec, L, K) > 0):
            plan = sampling.plain_plan(self, E_idx, o.order32, rank, deps, dims, o)
        # Base pairs only: the visit plan, the levels and the work lists are built on the device, beside the encoder, with nothing read
        # back — buffers and uploads in front of the encoder's launches, the plan's own launches behind them: they are running by then
        if (pair_list and pterms is None and self.sample_pairs_device_plan and on_device and L <= 8192
                and Lb.namp_decoder_sample_walk_grid(B_dec, L, K) > 0):
            o.wait()                                                                 # (the sort, if the featuriser launch did not take it)
            plan, start = sampling.pairs_plan(self, pair_list, o, E_idx, dims)
        h_V, h_E = self.encode_graph(V, None, E_idx, mask, h_E_embedded=h_E)
        if start is not None:
            start()
        o.wait()
        if symmetric and plan is None and B != 1:
            raise ValueError("symmetry-tied sampling expects one input complex (B == 1)")
        if not symmetric and order.shape[0] != B_dec:
            raise ValueError(f"randn has {fd['randn'].shape[0]} rows; expected batch_size*B = {B_dec}")
        pair_bias = fd["pair_bias"].float().contiguous() if "pair_bias" in fd else None
        if pair_bias is not None and self.sample_level_parallel:
            if tuple(pair_bias.shape) != (B, L, self.num_letters, L, self.num_letters):
                raise ValueError(f"pair_bias must be [B, L, {self.num_letters}, L, {self.num_letters}]; got {tuple(pair_bias.shape)}")
            deps = pair_bias_dependencies(pair_bias)
        if not self.sample_level_parallel:
            deps = None
        walk = bool(walk and deps is not None and Lb.namp_decoder_sample_walk_grid(B_dec, L, K) > 0)
        if plan is None and walk and not symmetric and L <= 16000:
            plan = sampling.plain_plan(self, _i32(E_idx), _i32(order), _i32(rank), deps, dims)
        elif plan is None:
            plan = sampling.host_plan(self, sym if symmetric else None, sym_weights, order, rank, _i32(E_idx), dims, deps, walk,
                                      split=bool(symmetric and walk and self.sample_split_groups))
        chain_mask = mask * fd["chain_mask"]
        mask_dec = mask if bs == 1 else mask.repeat(bs, 1)
        if self.reference_sample_mask_quirk and B == 1 and bs > 1 and not symmetric:   # :186 vs :292
            m0 = mask[0][order[0]]                                             # stream 0's mask along the steps
            mask_dec = torch.empty_like(mask_dec).scatter_(1, order, m0.expand(B_dec, L).contiguous())
        if uniform is None:
            uniform = torch.rand(B_dec, L, device=dev)
        m32 = self._as(mask, "i32")
        arrays = sampling.SamplerArrays(
            h_V.float().contiguous(), h_E.float().contiguous(), m32, m32 if mask_dec is mask else _i32(mask_dec), _i32(chain_mask),
            self._as(S_true, "i32"), bias.float().expand(B, L, self.num_letters).contiguous(), uniform,
            _i32(fd["S_forced"]) if fd.get("S_forced") is not None else None, pair_bias)
        if plan_out is not None and symmetric and walk:
            plan_out.update(order=plan.order, rank=plan.rank, group_first=plan.group_first, group_last=plan.group_last, sym_w=plan.sym_w,
                            map_idx=tok_maps, work=plan.work[:plan.nwork], work_n=plan.work_n[:plan.nwork], level_off=plan.level_off,
                            n_levels=plan.levels)
        maps = (tok_maps, n_maps, cls_bias is not None)
        (S_out, probs, logp, levels), code = sampling.launch(self, plan, arrays, maps, pterms, fd["temperature"], dims, walk)
        if code != 0:
            # the walk's grid barriers gave up (its workgroups were not all resident: a shared or partitioned device) — that call's
            # outputs are poisoned; decode again with one launch per level, which needs no co-residency
            warnings.warn(f"persistent level walk timed out (code {code:#x}); re-running with per-level launches")
            return self._sample(fd, walk=False, uniform=uniform)
        out = {"S": S_out.long(), "sampling_probs": probs, "log_probs": logp, "uniform": uniform,
               "decoding_order": plan.order.long() if symmetric else order}       # (int64 on every route)
        if levels is not None:                                                 # (an int of the per-level launches; the walk's: a device scalar)
            out["levels"] = levels
        if walk:
            out["work_items"] = plan.nwork
        if motifs is not None:                                                 # (stream r samples complex r % B)
            out["motif_hits"] = motif_hits(out["S"], motifs["adj"].repeat(bs, 1), motifs["motifs"])
        return out

    # build the plan of a design whose groups are all base pairs on the device (sampling.pairs_plan: namp_pairs_plan,
    # namp_sample_levels_dep, namp_pairs_work_lists, nothing is read back); False: the host route (sampling.host_plan: symmetry_visits and
    # level_work_lists; same results; also what symmetry_residues or states beside the pairs and walk=False take)
    sample_pairs_device_plan = True

    # ---------------------------------------------------------------------------------------
    # tied states: one sequence over M backbone states of the same molecule
    # ---------------------------------------------------------------------------------------
    # build the plan of the flattened problem in one HIP launch (sampling.states_plan: namp_states_plan); False: the host route
    # (sampling.host_plan; same results; also what `symmetry_residues` with states and walk=False take)
    sample_states_device_plan = True
    _STATE_SHARED = ("S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")

    def _states_arguments(self, fd):
        """The checks of the tied-states path (they need no device) -> (state weights as floats, M, L, batch_size, symmetric, the context
        states of _state_contexts or None)."""
        w = fd["state_weights"]
        w = [float(v) for v in (w.detach().reshape(-1).tolist() if torch.is_tensor(w) else list(w))]
        M, bs = len(w), int(fd["batch_size"])
        X, X_m = fd["X"], fd["X_m"]
        if M < 1 or X.dim() != 4 or X.shape[0] != M or X.shape[-1] != 3:
            raise ValueError(f"state_weights has {M} entries: X must be [{M}, L, atoms, 3]; got {tuple(X.shape)}")
        L = X.shape[1]
        if tuple(X_m.shape) != tuple(X.shape[:3]):
            raise ValueError(f"X_m must be {tuple(X.shape[:3])} with states; got {tuple(X_m.shape)}")
        for k in self._STATE_SHARED:
            if tuple(fd[k].shape) != (1, L):
                raise ValueError(f"'{k}' is shared by the states and must be [1, {L}]; got {tuple(fd[k].shape)}")
        bias = fd["bias"]
        if bias.dim() != 3 or bias.shape[0] != 1 or bias.shape[1] not in (1, L) or bias.shape[2] != self.num_letters:
            raise ValueError(f"bias must be [1, {L}, {self.num_letters}] with states; got {tuple(bias.shape)}")
        if tuple(fd["randn"].shape) != (bs, L):
            raise ValueError(f"randn must be [batch_size, L] = [{bs}, {L}] with states (row 0 orders every sample); got {tuple(fd['randn'].shape)}")
        if fd.get("S_forced") is not None and tuple(fd["S_forced"].shape) != (bs, L):
            raise ValueError(f"S_forced must be [{bs}, {L}] with states; got {tuple(fd['S_forced'].shape)}")
        if "pair_bias" in fd:
            raise NotImplementedError("pair_bias is not supported together with state_weights")
        if M * L > 16000:
            raise ValueError(f"states x residues = {M * L} exceeds the level lists' limit of 16000")
        ctx = self._state_contexts(fd, M, L)
        sym = fd.get("symmetry_residues", [[]])
        return w, M, L, bs, not (len(sym) == 1 and len(sym[0]) == 0), ctx

    def _state_contexts(self, fd, M, L):
        """Context states: feature_dict["state_S"] int [M, L], the token of every residue in every state, and
        feature_dict["state_mask"] [M, L] in {0, 1}, its presence there; either alone, the other is the shared row repeated.  Checked
        here — the tokens' range, the masks' values, mask == OR of state_mask over the states: ONE host read per new set of tensor
        objects, as _check_tokens keeps it — -> None without the keys, else (state_S int64 [M, L], state_mask [M, L] in the dtype of
        mask, a dict for what callers derive from the two and keep with them), on the device of S."""
        sS, sm = fd.get("state_S"), fd.get("state_mask")
        if sS is None and sm is None:
            return None
        S, mask = fd["S"], fd["mask"]
        for k, t in (("state_S", sS), ("state_mask", sm)):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (M, L)):
                raise ValueError(f"'{k}' is given per state and must be a tensor [{M}, {L}]; got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if sS is not None and (sS.dtype.is_floating_point or sS.dtype == torch.bool):
            raise ValueError(f"'state_S' must be an integer tensor; got {sS.dtype}")
        given = tuple(t for t in (sS, sm, S, mask) if t is not None)
        cached = not any(t.is_inference() for t in given)
        slot = self._tokens_ok.get("state_contexts")
        if cached and slot is not None and len(slot[0]) == len(given) and all(r() is t and v == t._version for (r, v), t in zip(slot[0], given)) \
                and slot[1] == (sS is None, sm is None):
            return slot[2]
        sS = (S.expand(M, L) if sS is None else sS.to(S.device)).long().contiguous()
        sm = (mask.expand(M, L) if sm is None else sm.to(device=mask.device)).to(mask.dtype).contiguous()
        lo, hi = torch.aminmax(sS)
        lo, hi, bad_value, bad_or = torch.stack((lo, hi, ((sm != 0) & (sm != 1)).any().long().to(lo.device),
                                                 ((sm != 0).any(0) != (mask[0] != 0)).any().long().to(lo.device))).tolist()
        if lo < 0 or hi >= self.vocab:
            raise IndexError(f"na_mpnn_amd: token ids in 'state_S' must lie in [0, {self.vocab}); got [{lo}, {hi}]")
        if bad_value:
            raise ValueError("'state_mask' must hold 0 (absent) or 1 (present)")
        if bad_or:
            raise ValueError("'mask' must equal the OR of 'state_mask' over the states: a residue is there iff some state has it")
        if cached:
            self._tokens_ok["state_contexts"] = ([(weakref.ref(t), t._version) for t in given], (fd.get("state_S") is None, fd.get("state_mask") is None),
                                                 (sS, sm, {}))
            return self._tokens_ok["state_contexts"][2]
        return sS, sm, {}

    def _sample_states(self, fd, walk, uniform=None):
        """sample() of ONE sequence tied across M backbone states (feature_dict["state_weights"], X [M, L, A, 3]): at every step of the one
        decoding order each state runs what a plain sample() stream on that state would run given the tokens drawn so far, one token is
        drawn from softmax((sum_m w_m logits_m + bias_i) / T) and written to all states.  The states are encoded as a batch and decoded as
        a symmetric design on the block-diagonal flattened graph of M * L residues (flat residue m * L + i, neighbours E_idx[m] + m * L,
        groups {i, L + i, ...} with the state weights): the decoder sees the graph through E_idx only.  Returns S [bs, L], sampling_probs
        [bs, L, V], log_probs [bs, M, L, V], decoding_order [bs, L], uniform [bs, L] (by step), levels, work_items.
        Context states (feature_dict["state_S"] / ["state_mask"] [M, L]): every state's copy of a fixed residue holds its
        own state_S[m, i]; a residue absent in a state (state_mask 0) has a zero context there, adds nothing to the sum and still takes
        the drawn token.  Then also S_states int64 [bs, M, L], the token every copy holds; the log_probs rows of absent copies are zeros."""
        w, M, L, bs, symmetric, ctx = self._states_arguments(fd)
        sym_groups, sym_weights = fd.get("symmetry_residues", [[]]), fd.get("symmetry_weights", [[]])
        tok_maps, n_maps, cls_bias = None, 0, None
        mapped = self._mapped_arguments(fd, 1, L)                                   # base pairs beside the states: the host route
        if mapped is not None:
            sym_groups, sym_weights, table, idx, _, cls_bias = mapped
            symmetric = not (len(sym_groups) == 1 and len(sym_groups[0]) == 0)
            tok_maps, n_maps = self._token_map_array(table, idx * M, fd["S"].device, cls_bias), len(table)   # flat residue m * L + i speaks as residue i does
        S_true, mask = fd["S"], fd["mask"]
        dev, N, Vn = S_true.device, M * L, self.num_letters
        pterms = self._pair_terms_of(fd, 1, L)
        # (the windows sit on state 0's copies only, as the pair terms' rows do: a residue counts once)
        motifs = self._motifs_of(fd, 1, L, True)
        _require_device(fd["X"], "X")
        counted = None
        if pterms is not None:
            # The rows sit on state 0's copies only — a residue counts once, not M times —, so the kernel counts EVERY member of a group
            # (its closing member is a copy of the last state, which has no slots); under "closing" the residues that do not close their
            # group lose their slots instead.  One copy, before anything is enqueued.
            if pterms[3] == 0 and symmetric:
                counted = [True] * L
                for g in sym_groups:
                    for r in list(g)[:-1]:
                        counted[int(r)] = False
            pterms = pterms[:3] + (1,)
        if pterms is not None or motifs is not None:
            pterms = self._pair_terms_section(pterms, 1, bs, N, int(min(self.k_neighbors, L)), dev, counted, motifs=motifs)
        self._check_tokens(S_true)
        if fd.get("S_forced") is not None:
            self._check_tokens(fd["S_forced"], "S_forced")
        o = self._decoding_order(mask, fd["chain_mask"], fd["randn"][:1])           # row 0: the one order of every sample (model_utils.py:220)
        fd_enc = dict(fd)
        for k in self._STATE_SHARED:
            fd_enc[k] = fd[k].expand(M, L)
        if ctx is not None:                                                         # every state is encoded with its own tokens and presence
            fd_enc["S"], fd_enc["mask"] = ctx[:2]
        V, _, h_E, E_idx = self._featurize_hip(fd_enc, want_E=False, want_hE=True, order=o)
        K = E_idx.shape[-1]
        dims = (bs, 1, N, K)
        walk = bool(walk and self.sample_level_parallel and hip.lib().namp_decoder_sample_walk_grid(bs, N, K) > 0)
        plan = start = None
        if (self.sample_states_device_plan and walk and self.sample_split_groups and not symmetric and o.order32 is not None
                and L <= 8192 and pterms is None):                                 # (pair terms add dependencies: the host route)
            # (needs the neighbour lists and the decoding order only: on the side stream, beside the encoder, as the plain branch's levels)
            o.wait()                                                                   # (the sort, if the featuriser launch did not take it)
            plan, start = sampling.states_plan(self, w, o, E_idx, (bs, M, L, K))
        h_V, h_E = self.encode_graph(V, None, E_idx, fd_enc["mask"], h_E_embedded=h_E)
        if start is not None:                                                          # (enqueued behind the encoder's launches: they are running by now)
            start()
        o.wait()
        if plan is None:
            groups = [[int(i) + m * L for m in range(M) for i in g] for g in sym_groups] if symmetric else []
            weights = [[w[m] * float(ws) for m in range(M) for ws in gw] for gw in sym_weights] if symmetric else []
            tied = {int(i) for g in (sym_groups if symmetric else []) for i in g}
            for i in range(L):
                if i not in tied:
                    groups.append([i + m * L for m in range(M)]); weights.append(list(w))
            E_f = _i32(E_idx + (torch.arange(M, dtype=torch.int32, device=dev) * L)[:, None, None]).view(N, K)
            plan = sampling.host_plan(self, groups, weights, o.order, o.rank, E_f, dims, (None, 0) if pterms is None else (pterms["dep"], pterms["n_dep"]),
                                      walk, split=bool(walk and self.sample_split_groups), steps=True)
        if uniform is None:
            uniform = torch.rand(bs, L, device=dev)
        # the walk reads a group's uniform at its LAST visit; `uniform` is by step (group)
        u_f = (uniform.repeat_interleave(M, dim=1) if plan.step_of is None else uniform[:, plan.step_of]).contiguous()
        flat_i32 = lambda t: _i32(t.repeat(1, M))
        m_f, cm_f, S_f = flat_i32(mask), flat_i32(mask * fd["chain_mask"]), flat_i32(S_true)
        forced = flat_i32(fd["S_forced"]) if fd.get("S_forced") is not None else None
        if ctx is not None:
            # Context states: the flat arrays are the kernel's interface, and here their rows differ.  Presence gates a copy's context
            # (mask_true, the residue tail's mask) and its tokens are its own; cm_f stays the SHARED mask * chain_mask — a fixed member
            # passes its own token on to the members behind it, so an absent copy of a designable residue must not be one: it takes
            # the group's token as every free member does, and its logits enter the group's sum with weight zero.
            state_S, state_mask, kept = ctx
            if "flat" not in kept:                                             # (kept with the checked tensors: a resident feature_dict)
                kept["flat"] = (((mask != 0) & (state_mask == 0)).reshape(N), _i32(state_mask.reshape(1, N)), _i32(state_S.reshape(1, N)))
            absent, m_f, S_f = kept["flat"]
            plan = plan._replace(sym_w=torch.where(absent, torch.zeros_like(plan.sym_w), plan.sym_w))
            if fd.get("S_forced_states") is not None:                          # (score_tied's slow route: the forced tokens per state)
                if tuple(fd["S_forced_states"].shape) != (bs, M, L):
                    raise ValueError(f"S_forced_states must be [{bs}, {M}, {L}]; got {tuple(fd['S_forced_states'].shape)}")
                forced = _i32(fd["S_forced_states"].reshape(bs, N))
        arrays = sampling.SamplerArrays(
            h_V.float().contiguous(), h_E.float().contiguous(), m_f, m_f if bs == 1 else m_f.repeat(bs, 1), cm_f, S_f,
            fd["bias"].float().expand(1, L, Vn).repeat(1, M, 1).contiguous(), u_f, forced)
        maps = (tok_maps, n_maps, cls_bias is not None)
        (S_out, probs, logp, levels), code = sampling.launch(self, plan, arrays, maps, pterms, fd["temperature"], dims, walk)
        if code != 0:
            warnings.warn(f"persistent level walk timed out (code {code:#x}); re-running with per-level launches")
            return self._sample_states(fd, walk=False, uniform=uniform)
        out = {"S": S_out[:, :L].long(), "sampling_probs": probs[:, :L], "log_probs": logp.view(bs, M, L, Vn),
               "decoding_order": o.order[0].expand(bs, L), "uniform": uniform, "levels": levels, "work_items": plan.nwork}
        if ctx is not None:                                                    # (an absent copy scores nothing: its rows are zeros)
            out["log_probs"] = logp.view(bs, N, Vn).masked_fill(absent[None, :, None], 0.0).view(bs, M, L, Vn)
            out["S_states"] = S_out.view(bs, M, L).long()
        if motifs is not None:
            out["motif_hits"] = motif_hits(out["S"], motifs["adj"].expand(bs, -1), motifs["motifs"])
        return out

    def sample_walk_status(self):
        """Barrier state of the last persistent level walk (synchronises): 0 = every grid barrier completed; otherwise the code of the barrier
        that gave up (the device was shared with other work and the walk's workgroups were not all resident: that call's log_probs are NaN)."""
        w = getattr(self, "_walk_sync", None)
        return 0 if w is None else int(w[32].item())          # NAMP_SYNC_TIMEOUT

    # positional convenience wrapper in the upstream ProteinMPNN argument order
    def forward_positional(self, X, S, mask, chain_M, residue_idx, chain_encoding_all, randn, *, X_m,
                           protein_mask, dna_mask, rna_mask, R_polymer_type):
        fd = {"X": X, "S": S, "mask": mask, "chain_mask": chain_M, "R_idx": residue_idx,
              "chain_labels": chain_encoding_all, "randn": randn, "X_m": X_m, "protein_mask": protein_mask,
              "dna_mask": dna_mask, "rna_mask": rna_mask, "R_polymer_type": R_polymer_type, "batch_size": 1}
        return self.score(fd)["log_probs"]
