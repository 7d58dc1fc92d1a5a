"""numpy restatement of the per-site sets of the mutational scan (ProteinMPNN.score_mutations, na_mpnn_amd/csrc/namp_mutations.h),
the expansion of a scan into explicit sequences and the CPU oracle of the call: library_ref.oracle_library on those sequences.
Helper module of test_score_mutations_host.py / test_gpu_score_mutations*.py (not a test)."""
import numpy as np

import library_ref as LR


def site_lists(E_idx, rank, mask, site):
    """The ascending lists U_1..3(site) = act_l(site) + site (library_ref.active_sets with var = the site) and [act_1..3]."""
    site = [int(r) for r in site if int(r) >= 0]
    var, acts = LR.active_sets(E_idx, rank, mask, site)
    return [np.nonzero(a | var)[0] for a in acts], acts


def site_rows(E_idx, rank, mask, sites):
    """sites [n_sites, M] padded with -1 -> |U_1..3(site)| int [n_sites, 3] and the lists U_3(site)."""
    lists = [site_lists(E_idx, rank, mask, s)[0] for s in np.asarray(sites)]
    return np.array([[len(u) for u in ls] for ls in lists], np.int64).reshape(len(lists), 3), [ls[2] for ls in lists]


def sparse_rows(E_idx, rank, mask, sites, site_tokens):
    """What score_mutations returns as row_offsets [n + 1] and row_residue [nnz]: per variant the list U_3 of its site."""
    _, u3 = site_rows(E_idx, rank, mask, sites)
    per = [u3[int(s)] for s in np.asarray(site_tokens)[:, 0]]
    offsets = np.concatenate(([0], np.cumsum([len(u) for u in per]))).astype(np.int64)
    return offsets, (np.concatenate(per) if per else np.zeros(0)).astype(np.int32)


def expand(S, sites, site_tokens):
    """The explicit sequences [n, L] of the variants: S with the tokens of the variant at the residues of its site."""
    sites, site_tokens = np.asarray(sites, np.int64), np.asarray(site_tokens, np.int64)
    out = np.repeat(np.asarray(S, np.int64)[None], len(site_tokens), 0)
    for v, row in enumerate(site_tokens):
        for r, t in zip(sites[row[0]], row[1:]):
            if r >= 0:
                out[v, r] = t
    return out


def scan(S, positions, alphabets):
    """The scan form as the general one: positions [P], alphabets: per position its tokens -> sites [P, 1], site_tokens [n, 2]."""
    sites = np.asarray(positions, np.int64)[:, None]
    rows = [[s, t] for s, p in enumerate(positions) for t in alphabets[s]]
    return sites, np.array(rows, np.int64).reshape(len(rows), 2)


def alphabet(cx, i):
    """synth.make_complex's ranges."""
    return range(0, 20) if cx["protein_mask"][i] else (range(21, 25) if cx["dna_mask"][i] else range(26, 30))


def oracle(w, fd, top_k, S_full, key=None):
    return LR.oracle_library(w, fd, top_k, S_full, key)


def case_sites(cx, E_idx, order, seed=11):
    """The sites and variants of a GPU case on the oracle's graph and order -> (sites [n_sites, 8], site_tokens [n, 9], names):
    the first-decoded designed residue, the last-decoded residue (U_l is the site alone), a masked residue where the case has one,
    two graph neighbours, two residues with disjoint cones, one site of 8 residues.  Three random variants per site inside the
    residues' alphabets, and the wild type of the first and of the last site."""
    E_idx, order = np.asarray(E_idx), np.asarray(order)
    rank, mask = LR.ranks_of(order), np.asarray(cx["mask"])
    L = len(order)
    w = (mask * cx["chain_mask"]) != 0
    designed = [int(i) for i in order if w[i]]
    first, last = designed[0], int(order[-1])
    names, sites = ["first", "last"], [[first], [last]]
    if (mask == 0).any():
        names.append("masked"); sites.append([int(np.nonzero(mask == 0)[0][0])])
    mid = designed[len(designed) // 2]
    names.append("neighbours"); sites.append([mid, int(next(j for j in E_idx[mid] if j != mid))])
    u3 = lambda r: set(site_lists(E_idx, rank, mask, [r])[0][2].tolist())
    a = designed[-2] if designed[-1] == last else designed[-1]
    b = next((r for r in designed if r != a and len(u3(r)) > 1 and not (u3(r) & u3(a))), None)
    if b is not None:                                            # (with L <= K every residue reaches all that decode later: no such pair)
        names.append("disjoint"); sites.append([b, a])
    eight = list(dict.fromkeys(designed[::max(1, len(designed) // 8)][:8] + list(range(L))))[:8]
    names.append("eight"); sites.append(eight)
    st = np.full((len(sites), 8), -1, np.int64)
    for s, res in enumerate(sites):
        st[s, :len(res)] = res
    rng = np.random.default_rng(seed)
    rows = []
    for s, res in enumerate(sites):
        for _ in range(3):
            rows.append([s] + [int(rng.choice(list(alphabet(cx, r)))) for r in res] + [0] * (8 - len(res)))
    for s in (0, len(sites) - 1):
        rows.append([s] + [int(cx["S"][r]) for r in sites[s]] + [0] * (8 - len(sites[s])))
    return st, np.array(rows, np.int64), names
