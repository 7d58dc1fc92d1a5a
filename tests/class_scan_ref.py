"""Reference of the paired scan — ProteinMPNN.score_mutations(tied=True, classes=True) (namp_class_mutations) — built
from the unchanged CPU oracle: tied_score_ref.parallel_logits (group_scan_ref.parallel_states keeps the decoder states) + unit_values on
the explicit sequences [S; S_v ...], the combine in fp64 and differences of log_likelihood; the numpy restatement of the lowest-lane
rule and of the expansion of a named site into the tokens every member receives; the plan sets from mutation_ref on the KEYS of the
tied stream; the cases and sites the CPU and GPU tests share.

Helper module of test_class_scan_host.py / test_gpu_class_scan*.py (not a test)."""
import functools

import numpy as np
import torch

from na_mpnn_amd import spec, synth
from oracle import cpu_ref
import class_loo_ref as CL
import group_loo_ref
import group_scan_ref as GR
import mutation_ref as MR
import tied_score_ref as TR

CASES = ("paired_l40", "l48_k16", "l12_lt_k", "hybrid", "trimer_maps_l24", "4oqu", "joined_l32")
K_OF = dict({n: TR.K_OF[n] for n in CASES[:-1]}, joined_l32=16)
N_RANDOM = 2            # classes per site beside the wild type
V = len(spec.RESTYPES)
GU, UG = spec.CLASS_GU, spec.CLASS_UG
MISTAKES = ("untied", "unhidden", "canonical", "nobias", "weights")
# the case each mistake is meant to be caught on (test_class_scan_host.py measures every one on the scan's own variants)
CATCHES = {"untied": "l48_k16", "unhidden": "l48_k16", "canonical": "l48_k16", "nobias": "l48_k16", "weights": "joined_l32"}


def case_inputs(name):
    """tied_score_ref's cases as they stand; 4oqu with its first six pairs; joined_l32: two protein chains of 8 tied residue by residue
    at four positions (weights 1 / 0.5) beside an RNA duplex of 2 x 8 with four wobble pairs (bias 0.5, pair weights 1 / 0.75), K = 16."""
    if name == "joined_l32":
        cx, b = CL._complex(32, 41, 16, 0)
        cx["chain_labels"] = np.searchsorted([8, 16, 24], np.arange(32), side="right").astype(np.int32)
        for c in range(4):
            cx["R_idx"][cx["chain_labels"] == c] = np.arange(8, dtype=np.int32) + 100 * c
        fd = CL._fd(cx, 44, [(16 + t, 31 - t) for t in range(4)], True, 0.5)
        fd.update(symmetry_residues=[[0, 8], [1, 9], [3, 11], [5, 13]], symmetry_weights=[[1.0, 0.5]] * 4, paired_weights=(1.0, 0.75))
        L = 32
        fd.update(chain_mask=torch.ones_like(fd["chain_mask"]), bias=torch.zeros(1, L, V), temperature=1.0, batch_size=1)
        return fd
    fd = TR.case_inputs(name)
    if name == "4oqu":
        fd["paired_residues"] = list(fd["paired_residues"])[:6]
    return fd


def lowest_lane(tables, named):
    """tables: the members' class tables in listed order, named {listed position: token} -> the lowest lane below N_CLASSES every member
    has and whose entry is the token at every named member, or -1."""
    T = np.asarray(tables, np.int64)
    ok = (T >= 0).all(0) & (np.arange(T.shape[1]) < spec.N_CLASSES)
    for t, tok in named.items():
        ok &= T[t] == int(tok)
    hit = np.nonzero(ok)[0]
    return int(hit[0]) if len(hit) else -1


def expand(st, tk, units):
    """st [n_sites, s] NAMED residues padded with -1, tk [n, 1 + s], units [(members, tables)] -> (sites8 int64 [n_sites, 8] padded with
    -1, tok int64 [n, 9]): every named unit's members in listed order, unit by unit in the order of first naming, with the tokens of the
    unit's class at every member; a residue in no unit keeps its token."""
    where = {int(r): (q, t) for q, (members, _) in enumerate(units) for t, r in enumerate(members)}
    sites8 = np.full((len(st), 8), -1, np.int64)
    plans = []
    for s, row in enumerate(st):
        order, named = [], {}
        for c, r in enumerate(row):
            if r < 0:
                continue
            q, t = where.get(int(r), (-1 - int(r), 0))
            if q not in named:
                order.append(q)
                named[q] = {}
            named[q][t] = c
        flat = [r for q in order for r in (units[q][0] if q >= 0 else [-1 - q])]
        assert len(flat) <= 8 and len(set(flat)) == len(flat)
        sites8[s, :len(flat)] = flat
        plans.append([(q, named[q]) for q in order])
    tok = np.zeros((len(tk), 9), np.int64)
    for v, row in enumerate(tk):
        tok[v, 0], p = row[0], 1
        for q, cols in plans[int(row[0])]:
            if q < 0:
                tok[v, p] = row[1 + cols[0]]
                p += 1
                continue
            members, tables = units[q]
            lane = lowest_lane(tables, {t: row[1 + c] for t, c in cols.items()})
            assert lane >= 0, (v, members)
            tok[v, p:p + len(members)] = [C[lane] for C in tables]
            p += len(members)
    return sites8, tok


def _alphabet(s0):
    return range(21, 25) if 21 <= s0 < 26 else (range(26, 30) if 26 <= s0 < 31 else range(0, 20))


def _lanes(unit, S0):
    """The classes of a unit whose first-member token lies in that member's alphabet."""
    members, tables = unit
    T = np.asarray(tables)
    return [c for c in range(spec.N_CLASSES) if (T[:, c] >= 0).all() and int(T[0, c]) in _alphabet(int(S0[members[0]]))]


def _pick_sites(name, units, key, leader, mask, E, S0):
    """The sites of a case: [(what, [unit leaders ...], how)] — how: "both" names the first two listed members of every unit, "first"
    the listed-first member alone."""
    L = len(key)
    lead = sorted({int(leader[i]) for i in range(L) if mask[i] != 0}, key=lambda u: key[u])
    members = {int(m[0]): [int(r) for r in m] for m, _ in units}
    tied = [u for u in lead if u in members]
    tied_units = dict((int(m[0]), (m, t)) for m, t in units)
    sites = [("first-visited unit", [lead[0]], "both"), ("last-visited unit", [lead[-1]], "both")]
    kinds = TR.edge_kinds(E, key, leader)
    hid = sorted({int(leader[i]) for i in range(L) if (kinds[i] == TR.HID).any()}, key=lambda u: key[u])
    if hid:
        sites.append(("hidden-backward edge between two members", [hid[-1]], "both"))
    for u in tied:                                                 # a cone with a later-listed member of a foreign unit, not its first
        u3 = MR.site_lists(E, key, mask, members[u])[0][2]
        here = set(int(r) for r in u3)
        if any(g not in here and g != u and any(q in here for q in members[g] if q != g) for g in tied):
            sites.append(("a foreign unit led by a later-listed member", [u], "both"))
            break
    if len(tied) >= 2:
        sites.append(("two units", [tied[0], tied[-1]], "both"))
    if len(tied) >= 4 and all(len(members[u]) == 2 for u in tied[:4]):
        sites.append(("four pairs, 8 edits: the cap", tied[:4], "both"))
    wob = [u for u in tied if GU in _lanes(tied_units[u], S0)]
    if wob:
        sites.append(("a wobble class named by both members", [wob[len(wob) // 2]], "wobble"))
    g_tok = {21: "DG", 26: "G"}
    na = [u for u in tied if int(S0[u]) >= 21]
    if na:
        sites.append(("G named alone", [(wob or na)[0]], "first"))
    alone = [u for u in lead if u not in members]
    if alone:
        sites.append(("an untied residue beside the units", [alone[len(alone) // 2]], "both"))
    return sites, g_tok


@functools.lru_cache(maxsize=None)
def case(name):
    """Computed once and shared, never modified -> dict: fd (S made tie-consistent), K, units [(members, tables)], specs (with weights
    and biases, as tied_score_ref.unit_values takes them), key, leader, gpos, mask, E_idx, kinds, rank0, what, st / tk as NAMED, sites8 /
    tok (expanded), site_rows, lists, u3, w (the oracle's weights)."""
    fd = dict(case_inputs(name))
    rti = spec.restype_to_int()
    w = cpu_ref.to_torch(synth.make_weights(0))
    L = fd["S"].shape[1]
    specs = [tuple(s) for s in CL.class_specs(fd, rti, True)]
    fd["S"] = TR.consistent_sequence(fd["S"][0].clone().long(), specs, L, 0)[None].to(fd["S"].dtype)
    enc, _, mask_t, order0 = group_loo_ref.flat_encoding(w, fd, K_OF[name])
    E = enc[2][0].numpy()
    rank0 = TR.rank_of(order0.numpy())
    units = [([int(r) for r in g], [list(C) for C in tabs]) for g, _, tabs, _ in specs]
    key, leader = TR.keys_and_leaders(rank0, [m for m, _ in units])
    kinds = TR.edge_kinds(E, key, leader)
    mask = mask_t[0].numpy()
    gpos = np.zeros(L, np.int64)
    for m, _ in units:
        gpos[m] = np.arange(len(m))
    S0 = fd["S"][0].numpy()
    sites, g_tok = _pick_sites(name, units, key, leader, mask, E, S0)
    unit_of = {int(m[0]): (m, t) for m, t in units}
    rng = np.random.default_rng(23)
    named, rows = [], []
    for q, (_, us, how) in enumerate(sites):
        cols = []
        for u in us:
            m = unit_of.get(u, ([u], None))[0]
            cols += m[:1] if how == "first" else m[:2]
        named.append(cols)

        def tokens(lanes_of):
            out = []
            for u in us:
                m, tabs = unit_of.get(u, ([u], [list(range(64))]))
                c = lanes_of(u, (m, tabs))
                out += [int(C[c]) for C in tabs[:1 if how == "first" else 2]]
            return out
        wild = lambda u, unit: lowest_lane(unit[1], {t: S0[r] for t, r in enumerate(unit[0])})
        if how == "first":                                         # G alone: the canonical class, whatever S holds
            g = rti[g_tok[21 if int(S0[us[0]]) < 26 else 26]]
            rows.append([q, g])
            rows.append([q] + tokens(wild)[:1])
            continue
        if how == "wobble":
            rows.append([q] + tokens(lambda u, unit: GU))
            rows.append([q] + tokens(lambda u, unit: UG))
        rows.append([q] + tokens(wild))
        for _ in range(N_RANDOM):
            rows.append([q] + tokens(lambda u, unit: int(rng.choice([c for c in _lanes(unit, S0) if c != wild(u, unit)]))))
    s = max(len(b) for b in named)
    st = np.full((len(named), s), -1, np.int64)
    tk = np.zeros((len(rows), 1 + s), np.int64)
    for q, b in enumerate(named):
        st[q, :len(b)] = b
    for v, r in enumerate(rows):
        tk[v, :len(r)] = r
    sites8, tok = expand(st, tk, units)
    lists = [MR.site_lists(E, key, mask, row)[0] for row in sites8]
    site_rows = np.array([[len(u) for u in ls] for ls in lists], np.int64).reshape(len(lists), 3)
    return dict(fd=fd, K=K_OF[name], units=units, specs=specs, key=key, leader=leader, gpos=gpos, mask=mask, E_idx=E, kinds=kinds, rank0=rank0,
                what=[a for a, _, _ in sites], st=st, tk=tk, sites8=sites8, tok=tok, site_rows=site_rows, lists=lists, u3=[ls[2] for ls in lists],
                w=w, enc=enc, mask_t=mask_t)


def sequences(c):
    """The explicit sequences [n + 1, L]: S, then the variants (every member of every named unit with its class token)."""
    S = c["fd"]["S"][0].long()
    out = S[None].repeat(len(c["tok"]) + 1, 1)
    for v, row in enumerate(c["tok"]):
        for r, t in zip(c["sites8"][row[0]], row[1:]):
            if r >= 0:
                out[v + 1, int(r)] = int(t)
    return out


def counted(c):
    m = np.zeros(len(c["key"]), bool)
    m[c["leader"]] = True
    return torch.from_numpy(m & (c["mask"] != 0))


@functools.lru_cache(maxsize=None)
def reference(name, mistake=None):
    """-> {"delta" [n], "units" [n + 1, L], "own" [n + 1, L], "log_probs" [n + 1, L, vocab] (fp64; row 0: S), "states" (mistake None
    only), "S"}.  mistake: None, "untied" (score()'s own stream, the sum of the members' own entries), "unhidden" (hidden-backward edges
    read as backward), "canonical" (the wobble lanes dropped from every table: a wobble variant has no class, its delta is -inf or nan),
    "nobias" (the class bias dropped), "weights" (every member weight 1)."""
    c = case(name)
    w, enc, mask = c["w"], c["enc"], c["mask_t"]
    S = sequences(c)
    kinds, specs = c["kinds"], c["specs"]
    if mistake == "untied":
        kinds = TR.edge_kinds(c["E_idx"], c["rank0"] << 4, np.arange(len(c["key"])))
        specs = []
    if mistake == "weights":
        specs = [(g, [1.0] * len(g), tabs, gb) for g, _, tabs, gb in specs]
    if mistake == "nobias":
        specs = [(g, gw, tabs, [0.0] * len(gb)) for g, gw, tabs, gb in specs]
    if mistake == "canonical":
        specs = [(g, gw, [list(C[:GU]) + [-1, -1] + list(C[UG + 1:]) for C in tabs], gb) for g, gw, tabs, gb in specs]
    states = None
    if mistake is None:
        states, logits = GR.parallel_states(w, enc, S, mask, kinds)
    else:
        logits = TR.parallel_logits(w, enc, S, mask, kinds, hide=mistake != "unhidden")
    unit, own = TR.unit_values(logits, S, specs)
    cnt = counted(c) if mistake != "untied" else torch.from_numpy(c["mask"] != 0)
    ll = unit[:, cnt].sum(-1)
    return dict(delta=ll[1:] - ll[0], units=unit, own=own, log_probs=torch.log_softmax(logits.double(), -1), states=states, S=S)
