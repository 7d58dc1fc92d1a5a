"""CPU tests of the forbidden motifs (feature_dict["forbidden_motifs"]): the window builder, the packed entries against a brute-force
search, the hit counter, the refusals, the CLI's parser, the integer-only entry points of the library, and the premises of the GPU
property tests (test_gpu_motifs.py) on the CPU oracle."""
import ctypes as C
import random

import pytest
import torch

from na_mpnn_amd import cli, hip, spec
from na_mpnn_amd.model import (ProteinMPNN, forbidden_motifs_arguments, motif_adjacency, motif_entries, motif_hits, motif_windows)
from oracle import cpu_ref
import motifs_cases
import motifs_ref

torch.set_grad_enabled(False)
V = 33
RTI = spec.restype_to_int()


def brute_windows(chain, ridx, mask, hw):
    """The windows by walking the chain one residue at a time."""
    L = len(chain)
    step = lambda i, j: 0 <= i < L and 0 <= j < L and chain[i] == chain[j] and ridx[max(i, j)] - ridx[min(i, j)] == 1 and mask[i] and mask[j]
    out = []
    for i in range(L):
        row = [-1] * (2 * hw)
        for sign in (-1, 1):
            j = i
            for k in range(1, hw + 1):
                if not step(j, j + sign):
                    break
                j += sign
                row[hw - k if sign < 0 else hw + k - 1] = j
        out.append(row)
    return out


def test_window_builder():
    """A chain break, an R_idx gap, a masked residue, a chain of one residue and a chain shorter than the motif."""
    chain = [0] * 9 + [1] * 6 + [2] + [3] * 3
    ridx = [1, 2, 3, 4, 6, 7, 8, 9, 10] + [5, 6, 7, 8, 9, 10] + [1] + [1, 2, 3]                   # a gap between residues 3 and 4
    mask = [1] * 19
    mask[11] = 0                                                                                 # absent: splits chain 1 into 2 + 3
    t = lambda v: torch.tensor([v])
    for hw in (1, 3, 7):
        win = motif_windows(t(chain), t(ridx), t(mask), hw)
        assert win.dtype == torch.int32 and tuple(win.shape) == (1, 19, 2 * hw)
        assert win[0].tolist() == brute_windows(chain, ridx, mask, hw), hw
    win = motif_windows(t(chain), t(ridx), t(mask), 3)[0].tolist()
    assert win[3] == [0, 1, 2, -1, -1, -1] and win[4] == [-1, -1, -1, 5, 6, 7]                 # the gap
    assert win[8] == [5, 6, 7, -1, -1, -1] and win[9] == [-1, -1, -1, 10, -1, -1]              # the chain break; the masked residue behind 10
    assert win[11] == [-1] * 6 and win[12] == [-1, -1, -1, 13, 14, -1]                         # a masked residue has no window and is in none
    assert win[15] == [-1] * 6 and win[16] == [-1, -1, -1, 17, 18, -1]                         # a chain of one; a chain of three
    # L = 1, and two complexes
    assert motif_windows(t([0]), t([5]), t([1]), 7)[0].tolist() == [[-1] * 14]
    two = motif_windows(torch.tensor([chain, chain]), torch.tensor([ridx, list(range(19))]), torch.tensor([mask, [1] * 19]), 2)
    assert two[0].tolist() == brute_windows(chain, ridx, mask, 2) and two[1].tolist() == brute_windows(chain, list(range(19)), [1] * 19, 2)
    adj = motif_adjacency(t(chain), t(ridx), t(mask))[0].tolist()
    assert adj == motifs_ref.next_ok({"chain_labels": t(chain), "R_idx": t(ridx), "mask": t(mask)})


def window_words(seq, i):
    """The three words the kernel packs for member i of a single all-present chain under the sequence seq (token + 1 per slot; 0: none)."""
    w = [0, 0, 0]
    for s in range(15):
        j = i + s - 7
        if 0 <= j < len(seq):
            w[s // 5] |= (seq[j] + 1) << (6 * (s % 5))
    return w


def entry_matches(e, w):
    return all(((w[q] ^ e[q]) & e[3 + q]) == 0 for q in range(3))


@pytest.mark.parametrize("n", [2, 8])
def test_entries_against_the_brute_force_search(n):
    """Every alignment of a motif of length n: entry (motif, k) matches the window of member i exactly when the motif starts at i - k;
    so some entry matches exactly when an occurrence covers the member."""
    rng = random.Random(7 + n)
    alphabet = [3, 21, 29]                                                                       # (29 + 1 = 30 fills five of a slot's six bits)
    motifs = [tuple(rng.choice(alphabet) for _ in range(n)) for _ in range(3)] + [tuple([21] * n)]
    entries = motif_entries(motifs)
    assert entries.dtype == torch.int32 and tuple(entries.shape) == (len(motifs) * n, 6)
    E = entries.tolist()
    L, seen = 30, set()
    for trial in range(300):
        seq = [rng.choice(alphabet) for _ in range(L)]
        i = rng.randrange(L)
        if trial % 3 == 0:                                                                       # plant a motif so that every alignment occurs
            mi, k = (trial // 3) % len(motifs), (trial // (3 * len(motifs))) % n
            s = rng.randrange(0, L - n + 1)
            seq[s:s + n] = motifs[mi]
            i = s + k
        w = window_words(seq, i)
        for mi, m in enumerate(motifs):
            for k in range(n):
                want = 0 <= i - k and i - k + n <= L and tuple(seq[i - k:i - k + n]) == m
                assert entry_matches(E[mi * n + k], w) == want, (seq, i, m, k)
                seen.add((mi, k, want))
        occ = motifs_ref.occurrences(seq, [True] * (L - 1), motifs)
        assert any(entry_matches(e, w) for e in E) == any(s <= i < s + ln for s, ln in occ)
    assert all((mi, k, True) in seen for mi in range(len(motifs)) for k in range(n))           # every alignment was met


def test_hit_counter_equals_the_reference():
    cx, fd, motifs = motifs_cases.plain_case()
    rng = random.Random(3)
    S = torch.tensor([[rng.choice([motifs_cases.A_, motifs_cases.R_]) for _ in range(40)] for _ in range(6)])
    adj = motif_adjacency(fd["chain_labels"], fd["R_idx"], fd["mask"])
    got = motif_hits(S, adj.expand(6, -1), motifs)
    assert got.dtype == torch.int64 and torch.equal(got, motifs_ref.hits(S, fd, motifs)) and int(got.sum()) > 0
    assert int(motif_hits(S[:, :2], adj[:, :1].expand(6, -1), motifs).sum()) == 0             # shorter than every motif


def test_argument_refusals():
    sp = [RTI[n] for n in spec.SPECIAL_RESTYPES]
    ok = forbidden_motifs_arguments([(1, 2), [3, 4, 5]], V, sp)
    assert ok == [(1, 2), (3, 4, 5)]
    assert forbidden_motifs_arguments(torch.tensor([[1, 2, -1, -1], [3, 4, 5, 6]]), V, sp) == [(1, 2), (3, 4, 5, 6)]
    assert forbidden_motifs_arguments([], V, sp) == []
    for bad, msg in (([(1,)], "2..8"), ([(1,) * 9], "2..8"), ([(1, V)], "tokens must lie"), ([(-1, 2)], "tokens must lie"),
                     ([(1, RTI["PAD"])], "special"), ([(RTI["UNK"], 2)], "special"), ([(1, 2)] * 64, "at most 63"),
                     ([(1.0, 2)], "integer tokens"), ("gg", "list of token tuples"), (torch.tensor([[1.0, 2.0]]), "integer tensor")):
        with pytest.raises(ValueError, match=msg):
            forbidden_motifs_arguments(bad, V, sp)
    assert len(forbidden_motifs_arguments([(1, 2)] * 63, V, sp)) == 63
    with pytest.raises(ValueError, match="pair_bias"):
        forbidden_motifs_arguments([(1, 2)], V, sp, pair_bias=True)
    with pytest.raises(ValueError, match="B == 1"):
        forbidden_motifs_arguments([(1, 2)], V, sp, B=2, tied=True)
    assert forbidden_motifs_arguments([(1, 2)], V, sp, B=2) == [(1, 2)]
    # the model refuses before any device work
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=12, atom_dict=spec.atom_dict(), restype_to_int=RTI, polytype_to_int=spec.polytype_to_int())
    cx, fd, motifs = motifs_cases.plain_case()
    with pytest.raises(ValueError, match="special"):
        m.sample(dict(fd, forbidden_motifs=[(1, RTI["MAS"])]))
    with pytest.raises(ValueError, match="pair_bias"):
        m.sample(dict(fd, forbidden_motifs=motifs, pair_bias=torch.zeros(1, 40, V, 40, V)))
    fds = dict(fd, state_weights=[0.5, 0.5], X=fd["X"].repeat(2, 1, 1, 1), X_m=fd["X_m"].repeat(2, 1, 1))
    with pytest.raises(ValueError, match="2..8"):
        m.sample(dict(fds, forbidden_motifs=[(1,)]))


def test_cli_parsing():
    one = {spec.RESTYPE_3TO1[k]: v for k, v in RTI.items()}
    got = cli.parse_forbidden_motifs("gggg, cccc,dna:GAATTC,rna:GGGG,KK", 0, RTI)
    assert got == [(one["g"],) * 4, (one["c"],) * 4, tuple(RTI[n] for n in ("DG", "DA", "DA", "DT", "DT", "DC")), (RTI["G"],) * 4,
                   (RTI["LYS"],) * 2]
    shared = spec.restype_to_int(True)
    assert cli.parse_forbidden_motifs("rna:GGGU,dna:GGGT", 0, shared) == [(shared["DG"],) * 3 + (shared["DT"],)]      # one motif under shared tokens
    hp = cli.parse_forbidden_motifs("", 3, RTI, ["dna"])
    assert hp == [(RTI[n],) * 4 for n in ("DA", "DC", "DG", "DT")]
    both = cli.parse_forbidden_motifs("gggg", 3, RTI, ["dna", "rna"])
    assert both[0] == (RTI["DG"],) * 4 and len(both) == 8 and len(set(both)) == 8
    assert len(cli.parse_forbidden_motifs("", 1, RTI)) == 28 and len(cli.parse_forbidden_motifs("", 7, shared, ["dna", "rna"])) == 4
    for bad in ("dna:GAZ", "xna:GG", "g?"):
        with pytest.raises(ValueError, match="forbidden_motifs"):
            cli.parse_forbidden_motifs(bad, 0, RTI)
    with pytest.raises(ValueError, match="max_homopolymer"):
        cli.parse_forbidden_motifs("", 8, RTI)
    args = cli.build_parser().parse_args(["--out_folder", "none", "--forbidden_motifs", "gggg", "--max_homopolymer", "4"])
    assert args.forbidden_motifs == "gggg" and args.max_homopolymer == 4
    for mode in (["--conditional_probs_only", "1"], ["--mutation_scan", "1"], ["--score_fasta", "x.fa"], ["--coordinate_gradients", "1"]):
        with pytest.raises(ValueError, match="constrain designs"):
            cli.main(["--pdb_path", "none.pdb", "--out_folder", "none", "--mode", "design", "--max_homopolymer", "3"] + mode)


def test_motif_entry_points_validate_without_a_gpu():
    Lb = hip.lib()
    for bad in ((0, 3), (505, 3), (-1, 3)):
        assert Lb.namp_sample_motifs(*bad) == -1 and b"n_entries" in Lb.namp_last_error()
    for bad in ((4, 0), (4, 8)):
        assert Lb.namp_sample_motifs(*bad) == -1 and b"half_width" in Lb.namp_last_error()
    dummy = (C.c_float * 4)()
    pb = C.cast(dummy, C.POINTER(C.c_float))
    nul = [None] * 16
    call = lambda pair_bias: Lb.namp_decoder_sample(*nul, pair_bias, 1.0, 0, None, None, None, None, 0, 1, 1, 10, 4, None)
    assert Lb.namp_sample_motifs(504, 7) == 0
    assert call(pb) == -1 and b"forbidden motifs and the dense pair_bias" in Lb.namp_last_error()
    assert call(pb) == -1 and b"forbidden motifs" not in Lb.namp_last_error()                  # taken and cleared by the refused call
    assert Lb.namp_sample_motifs(4, 3) == 0 and Lb.namp_sample_motifs(4, 9) == -1              # a bad attach leaves nothing attached
    assert call(pb) == -1 and b"forbidden motifs" not in Lb.namp_last_error()
    assert Lb.namp_sample_motifs(4, 3) == 0
    assert call(None) == -1 and b"null weights" in Lb.namp_last_error()
    assert call(pb) == -1 and b"forbidden motifs" not in Lb.namp_last_error()


def test_motif_workspace_arithmetic():
    Lb = hip.lib()
    for dims in ((1, 1, 1000, 48, 3), (2, 4, 80, 24, 3), (1, 1, 1, 1, 1), (1, 8, 16000, 48, 8)):
        off = Lb.namp_sample_pair_terms_offset(*dims)
        G = dims[0] * dims[2]
        assert Lb.namp_sample_motifs_offset(*dims, 0, 0, V) == off                              # motifs alone: the section starts with the window
        assert Lb.namp_sample_motifs_offset(*dims, 2, 3, V) == off + 4 * (4 * G + 3 * V * V)   # behind the pair terms' blocks
        for hw, E in ((1, 2), (3, 16), (7, 504)):
            assert Lb.namp_sample_motifs_workspace_bytes(*dims, 0, 0, E, hw) == off + 4 * (2 * hw * G + 6 * E)
            need = Lb.namp_sample_motifs_workspace_bytes(*dims, 2, 3, E, hw)
            assert need == off + 4 * (4 * G + 3 * 64 * 64 + 2 * hw * G + 6 * E)                # (tables sized for vocab = 64)
            assert need >= Lb.namp_sample_motifs_offset(*dims, 2, 3, V) + 4 * (2 * hw * G + 6 * E)
    d = (1, 1, 100, 24, 3)
    for tail in ((0, 0, 0, 3), (0, 0, 505, 3), (0, 0, 4, 0), (0, 0, 4, 8), (1, 0, 4, 3), (0, 1, 4, 3), (65, 1, 4, 3), (2, 257, 4, 3)):
        assert Lb.namp_sample_motifs_workspace_bytes(*d, *tail) == 0, tail
    assert Lb.namp_sample_motifs_workspace_bytes(0, 1, 100, 24, 3, 0, 0, 4, 3) == 0
    assert Lb.namp_sample_motifs_offset(*d, 0, 0, 65) == 0 and Lb.namp_sample_motifs_offset(*d, 1, 0, V) == 0


# ---- the premises of the GPU property tests, on the CPU oracle ------------------------------------------------------------------
def test_premise_the_unconstrained_design_holds_the_motifs(weights_np):
    """test_gpu_motifs' free-design case: under the +6 bias on the motifs' tokens the oracle's own unconstrained design holds
    occurrences (else motif_hits == 0 with the key would show nothing)."""
    cx, fd, motifs = motifs_cases.plain_case()
    w = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    torch.manual_seed(5)
    S = cpu_ref.sample(w, fd, 24)["S"]
    n = motifs_ref.hits(S, fd, motifs)
    print("occurrences in the oracle's unconstrained design per stream:", n.tolist())
    assert int(n.sum()) > 0


def test_premise_no_ban_is_ever_skipped_on_the_free_design_cases(weights_np):
    """A ban is skipped only if it leaves no candidate with p > 0.  On the free-design cases no bias is -inf-like and the oracle's
    unconstrained rows give every non-special token mass, while one draw can lose at most the distinct tokens of the motifs."""
    cx, fd, motifs = motifs_cases.plain_case()
    w = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    torch.manual_seed(5)
    P = cpu_ref.sample(w, fd, 24)["sampling_probs"]
    alive = int((P > 0).sum(-1).min())
    assert alive == V - len(spec.SPECIAL_RESTYPES) and motifs_cases.most_banned_at_once(motifs) < alive
    # the duplex cases: a nucleotide keeps the four bases of its polymer, a homopolymer ban takes one token of a residue at a time
    assert all(len(set(m)) == 1 for m in motifs_cases.NA_HOMOPOLYMERS)
