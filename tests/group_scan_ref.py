"""Reference of the symmetric scan — ProteinMPNN.score_mutations(tied=True) (namp_group_mutations) — built from the
unchanged CPU oracle: tied_score_ref.parallel_logits + unit_values on the explicit sequences [S; S_v ...], the combine in fp64 and
differences of log_likelihood; the numpy restatement of what the device plans (mutation_ref's per-site sets with the KEYS of the tied
stream for ranks and the EXPANDED sites; the leader rule) and the cases and sites the CPU and GPU tests share.

Helper module of test_group_scan_host.py / test_gpu_group_scan*.py (not a test)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref
import group_loo_ref
import mutation_ref as MR
import tied_score_ref as TR

CASES = ("trimer_l24", "trimer_l24_k48", "dimer_l48", "mixed_l12", "plain_l17", "plain_l1")
GROUPED = CASES[:4]
N_RANDOM = 3            # variants per site beside the wild type


def expand(sites, groups):
    """sites: lists of NAMED residues -> int64 [n_sites, 8] padded with -1: every named residue replaced by the members of its unit in
    listed order."""
    unit = {r: list(g) for g in groups for r in g}
    out = np.full((len(sites), 8), -1, np.int64)
    for s, named in enumerate(sites):
        flat = [m for r in named for m in unit.get(int(r), [int(r)])]
        assert len(flat) <= 8 and len(set(flat)) == len(flat)
        out[s, :len(flat)] = flat
    return out


def lead_rows(u3, leader, gpos, mask):
    """The leader rule of group_unit_kernel<Combine> on one variant's ascending layer-3 list: row r leads if it is unmasked and no earlier-listed
    member of its unit is in the list -> bool [len(u3)]."""
    here = set(int(r) for r in u3)
    out = []
    for r in u3:
        earlier = [q for q in np.nonzero(leader == leader[r])[0] if gpos[q] < gpos[r] and int(q) in here]
        out.append(bool(mask[r] != 0) and not earlier)
    return np.array(out, bool)


def unit_list(u3, leader, mask):
    """The brute force: the listed-first members of the units with an unmasked member in the list, ascending."""
    return np.unique(leader[[int(r) for r in u3 if mask[r] != 0]]).astype(np.int64)


def parallel_states(w, enc, S, mask, kinds):
    """tied_score_ref.parallel_logits that also keeps the decoder states -> ([h_V after layer 1..3] each [n, N, 128], logits)."""
    n = S.shape[0]
    rep = lambda t: t.expand(n, *t.shape[1:])
    h_V, h_E, E_idx = (rep(t) for t in enc)
    kinds = torch.as_tensor(kinds)
    m1 = rep(mask).float().view(n, -1, 1, 1)
    sel = lambda b: m1 * b.float()[None, :, :, None]
    h_S = F.embedding(S.long(), w["W_s.weight"])
    h_ES = cpu_ref.cat_neighbors_nodes(h_S, h_E, E_idx)
    h_EX = cpu_ref.cat_neighbors_nodes(torch.zeros_like(h_S), h_E, E_idx)
    ctx_fw = sel(kinds == TR.FW) * cpu_ref.cat_neighbors_nodes(h_V, h_EX, E_idx)
    states = []
    for l in range(cpu_ref.n_layers(w, "decoder")):
        h_ESV = sel(kinds == TR.BW) * cpu_ref.cat_neighbors_nodes(h_V, h_ES, E_idx) + \
            sel(kinds == TR.HID) * cpu_ref.cat_neighbors_nodes(h_V, h_EX, E_idx) + ctx_fw
        h_V = cpu_ref.dec_layer(w, f"decoder_layers.{l}.", h_V, h_ESV, rep(mask).float())
        states.append(h_V)
    return states, cpu_ref._lin(w, "W_out", h_V)


def _pick_sites(name, groups, key, leader, gpos, mask, E):
    """The NAMED sites of a case (lists of residues), with what each is for."""
    L = len(key)
    units = sorted({int(leader[i]) for i in range(L) if mask[i] != 0}, key=lambda u: key[u])
    members = lambda u: [int(r) for r in np.nonzero(leader == u)[0]]
    sites = [("first-visited unit", [units[0]])]
    if len(units) > 1:
        sites.append(("last-visited unit", [units[-1]]))
    kinds = TR.edge_kinds(E, key, leader)
    hid = sorted({int(leader[i]) for i in range(L) if (kinds[i] == TR.HID).any()}, key=lambda u: key[u])
    if hid:
        sites.append(("hidden-backward edge between two members", [hid[-1]]))
    grouped = [u for u in units if len(members(u)) > 1]
    for u in units:                                               # a cone with a later-listed member of a foreign group, not its first
        u3 = MR.site_lists(E, key, mask, expand([[u]], groups)[0])[0][2]
        here = set(int(r) for r in u3)
        if any(g not in here and g != u and any(q in here for q in members(g) if q != g) for g in grouped):
            sites.append(("a foreign group led by a later-listed member", [u]))
            break
    alone = [u for u in units if len(members(u)) == 1]
    if grouped and alone:
        sites.append(("an ungrouped residue beside groups", [alone[len(alone) // 2]]))
    if name == "dimer_l48":
        sites.append(("two units, 4 edits", [units[3], units[7]]))
        sites.append(("four units, 8 edits: the cap", [units[2] + 24, units[9], units[15], units[20] + 24]))      # (named by their second members too)
    if name == "mixed_l12":
        sites.append(("the group of four plus the pair, 6 edits", [5, 1]))
    if name == "plain_l17":
        sites.append(("two residues", [units[4], units[9]]))
    return sites


@functools.lru_cache(maxsize=None)
def case(name):
    """Computed once and shared, never modified -> dict: fd (S made tie-consistent), K, groups, key, leader, gpos, mask, E_idx, rank0,
    named (lists of residues), what, sites8 (expanded, int64 [n_sites, 8]), tk int64 [n, 1 + s] over the NAMED sites (per site the wild
    type and N_RANDOM other amino-acid assignments), site_rows int64 [n_sites, 3], lists [n_sites][3] and u3."""
    c = TR.oracle_case(name)
    fd = dict(c["fd"])
    fd["S"] = c["S_lib"][:1].clone()                             # (tied_score_ref.library's first row: S, tie-consistent)
    groups = [list(s[0]) for s in c["specs"]]
    key, leader, mask, E = c["key"], c["leader"], c["mask"].numpy(), c["E_idx"]
    gpos = np.zeros(len(key), np.int64)
    for g in groups:
        gpos[g] = np.arange(len(g))
    named = _pick_sites(name, groups, key, leader, gpos, mask, E)
    what, named = [a for a, _ in named], [b for _, b in named]
    s = max(len(b) for b in named)
    st = np.full((len(named), s), -1, np.int64)
    rng = np.random.default_rng(17)
    S0 = fd["S"][0].numpy()
    rows = []
    for q, b in enumerate(named):
        st[q, :len(b)] = b
        wild = [int(S0[r]) for r in b]
        rows.append([q] + wild + [0] * (s - len(b)))
        for _ in range(N_RANDOM):
            rows.append([q] + [int((t + 1 + rng.integers(0, 19)) % 20) if t < 20 else int(rng.integers(0, 20)) for t in wild] + [0] * (s - len(b)))
    sites8 = expand(named, groups)
    lists = [MR.site_lists(E, key, mask, row)[0] for row in sites8]
    site_rows = np.array([[len(u) for u in ls] for ls in lists], np.int64).reshape(len(lists), 3)
    return dict(fd=fd, K=TR.K_OF[name], groups=groups, weights=[list(sp[1]) for sp in c["specs"]], specs=c["specs"], key=key, leader=leader,
                gpos=gpos, mask=mask, E_idx=E, kinds=c["kinds"], rank0=TR.rank_of(c["order0"].numpy()), named=named, what=what, st=st,
                sites8=sites8, tk=np.array(rows, np.int64), site_rows=site_rows, lists=lists, u3=[ls[2] for ls in lists], w=c["w"])


def sequences(c):
    """The explicit sequences [n + 1, L]: S, then the variants (the edit at every member of every named unit)."""
    unit = {r: list(g) for g in c["groups"] for r in g}
    S = c["fd"]["S"][0].long()
    out = S[None].repeat(len(c["tk"]) + 1, 1)
    for v, row in enumerate(c["tk"]):
        for r, t in zip(c["st"][row[0]], row[1:]):
            if r >= 0:
                out[v + 1, unit.get(int(r), [int(r)])] = int(t)
    return out


def counted(c):
    L = len(c["key"])
    m = np.zeros(L, bool)
    m[c["leader"]] = True
    return torch.from_numpy(m & (c["mask"] != 0))


@functools.lru_cache(maxsize=None)
def reference(name, mistake=None):
    """-> {"delta" [n], "units" [n + 1, L], "own" [n + 1, L], "log_probs" [n + 1, L, vocab] (fp64; row 0: S), "states": the decoder
    states per layer (mistake None only)}.  mistake: None, "unhidden" (hidden-backward edges read as backward), "untied" (score()'s own
    stream and the sum of the members' own entries: the plain scan with all members edited), "weights" (symmetry_weights all 1)."""
    c = case(name)
    w = c["w"]
    enc, _, mask, _ = group_loo_ref.flat_encoding(w, c["fd"], c["K"])
    S = sequences(c)
    kinds, specs = c["kinds"], c["specs"]
    if mistake == "untied":
        kinds = TR.edge_kinds(c["E_idx"], c["rank0"] << 4, np.arange(len(c["key"])))
        specs = []
    if mistake == "weights":
        specs = [(g, [1.0] * len(g), tabs, gb) for g, _, tabs, gb in specs]
    states = None
    if mistake is None:
        states, logits = parallel_states(w, enc, S, mask, kinds)
    else:
        logits = TR.parallel_logits(w, enc, S, mask, kinds, hide=mistake != "unhidden")
    unit, own = TR.unit_values(logits, S, specs)
    cnt = counted(c) if specs or mistake != "untied" else torch.from_numpy(c["mask"] != 0)
    ll = unit[:, cnt].sum(-1)
    return dict(delta=ll[1:] - ll[0], units=unit, own=own, log_probs=torch.log_softmax(logits.double(), -1), states=states, S=S)
