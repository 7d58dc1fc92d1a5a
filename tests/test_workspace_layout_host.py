"""CPU-side tests of the attach-and-carry protocol: every exported size / offset function of the calls that ride on
namp_decoder_fwd and namp_decoder_loo against recorded values (tests/golden/workspace_layout.json: callers and the kernels agree on
the sections only through these numbers), and the attachment state machine of namp_decoder_fwd's riders, read from the error text
of an all-null call — every path here returns before any device call."""
import json
import os

from na_mpnn_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_layout.json")
PAST = 1 << 28                                     # the first row code that no longer fits

# (N, K, n_dec, n_var, n_chunk, rows_1..3)
LIBRARY = [(1, 1, 3, 0, 0, 0, 0, 0), (1, 1, 3, 1, 1, 1, 1, 1), (17, 16, 3, 5, 3, 6, 9, 12), (17, 17, 3, 5, 3, 6, 9, 12),
           (1000, 48, 3, 40, 64, 60, 150, 400), (17, 16, 3, 5, 0, 0, 0, 0), (17, 16, 3, 0, 4, 0, 0, 0), (17, 16, 3, 5, 3, 0, 9, 12),
           # refused: n_dec, K > N, K > NAMP_MAX_K, n_var > N, a capacity > N, a negative count, a row code past 2^28
           (17, 16, 4, 5, 3, 6, 9, 12), (17, 18, 3, 5, 3, 6, 9, 12), (1000, 500, 3, 5, 3, 6, 9, 12), (17, 16, 3, 18, 3, 6, 9, 12),
           (17, 16, 3, 5, 3, 6, 9, 18), (17, 16, 3, 5, -1, 6, 9, 12), (1000, 48, 3, 40, PAST // 1000 + 1, 60, 150, 400)]
# (N, K, n_dec, n_sites, n_variants, list_1..3, items_1..3)
MUTATIONS = [(1, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1), (17, 16, 3, 2, 3, 4, 7, 9, 6, 10, 14),
             (17, 17, 3, 2, 3, 4, 7, 9, 6, 10, 14), (1000, 48, 3, 100, 2000, 300, 900, 2500, 6000, 18000, 50000),
             (17, 16, 3, 2, 0, 0, 0, 0, 0, 0, 0), (17, 16, 3, 2, 3, 4, 7, 9, 0, 10, 14),
             # refused: n_dec, K > N, variants without a site, a negative capacity, row codes past 2^28 (an item capacity, the edits)
             (17, 16, 4, 2, 3, 4, 7, 9, 6, 10, 14), (17, 18, 3, 2, 3, 4, 7, 9, 6, 10, 14), (17, 16, 3, 0, 3, 4, 7, 9, 6, 10, 14),
             (17, 16, 3, 2, 3, 4, 7, 9, 6, 10, -1), (17, 16, 3, 2, 3, 4, 7, 9, 6, 10, PAST), (17, 16, 3, 2, PAST // 8, 4, 7, 9, 6, 10, 14)]
# (N, K, n_dec, n_tables, n_classes, n_chunk)
TIED = [(1, 1, 3, 1, 1, 0), (1, 1, 3, 1, 33, 1), (17, 16, 3, 2, 35, 3), (17, 17, 3, 2, 35, 3), (1000, 48, 3, 64, 64, 65), (17, 16, 3, 1, 33, 0),
        # refused: n_dec, K > N, n_tables of 0 and 65, n_classes of 0 and 65, a negative chunk, a row code past 2^28
        (17, 16, 4, 2, 35, 3), (17, 18, 3, 2, 35, 3), (17, 16, 3, 0, 35, 3), (17, 16, 3, 65, 35, 3), (17, 16, 3, 2, 0, 3), (17, 16, 3, 2, 65, 3),
        (17, 16, 3, 2, 35, -1), (17, 16, 3, 2, 35, PAST // 17 + 1)]
# (B, N, K, n_dec); the cone sizes do not compare K with N (namp_decoder_loo does)
LOO = [(1, 1, 1, 3), (1, 17, 16, 3), (1, 17, 17, 3), (1, 1000, 48, 3), (2, 17, 16, 3), (1, 17, 18, 3),
       (1, 17, 16, 4), (0, 17, 16, 3), (1, 0, 16, 3), (1, 17, 0, 3), (1, 1000, 500, 3)]
N_MAPS = [1, 3, 64, 0, 65]
CLASSES = [(1, 0), (1, 1), (3, 0), (64, 1), (0, 0), (65, 1), (3, 2), (3, -1)]          # (n_tables, groups)

CASES = {}
for _family, _dims in (("namp_library", LIBRARY), ("namp_mutations", MUTATIONS), ("namp_tied_score", TIED)):
    for _f in ("_workspace_bytes", "_in_offset", "_out_offset"):
        CASES[_family + _f] = _dims
CASES["namp_loo_workspace_bytes"] = CASES["namp_loo_groups_offset"] = CASES["namp_loo_pairs_offset"] = LOO
CASES["namp_loo_groups_workspace_bytes"] = CASES["namp_loo_pairs_workspace_bytes"] = [d + (m,) for d in LOO for m in N_MAPS]
CASES["namp_loo_classes_workspace_bytes"] = CASES["namp_loo_classes_out_offset"] = [d + c for d in LOO for c in CLASSES]


def layout(L):
    """Every case of CASES on library L -> {function: [[args..., value], ...]}."""
    return {name: [list(args) + [int(getattr(L, name)(*args))] for args in dims] for name, dims in sorted(CASES.items())}


def test_every_size_and_offset_is_the_recorded_one():
    got, want = layout(hip.lib()), json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], name
    # the recorded cases hold what they are there for: legal shapes give sizes, every refused case gives 0 from all three functions
    for family, legal in (("namp_library", 8), ("namp_mutations", 7), ("namp_tied_score", 6)):
        rows = [want[family + f] for f in ("_workspace_bytes", "_in_offset", "_out_offset")]
        for q, (size, i_off, o_off) in enumerate(zip(*rows)):
            assert (0 < i_off[-1] < o_off[-1] < size[-1]) if q < legal else (size[-1] == i_off[-1] == o_off[-1] == 0), (family, size[:-1])


def test_attachment_state_machine_of_the_decoder_riders():
    L = hip.lib()

    def carried():
        """An all-null namp_decoder_fwd call (refused before any pointer is read, and before any device call) -> its error text."""
        assert L.namp_decoder_fwd(None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, 10, 4, None) == -1
        return L.namp_last_error()
    attach = {b"library": lambda: L.namp_library(1, 0, 0, 0, 0), b"mutational scan": lambda: L.namp_mutations(1, 0, 0, 0, 0, 0, 0, 0),
              b"tied score": lambda: L.namp_tied_score(1, 33, 2)}
    refused = {b"library": lambda: L.namp_library(-1, 0, 0, 0, 0), b"mutational scan": lambda: L.namp_mutations(1, 0, 0, 0, 0, 0, 0, -1),
               b"tied score": lambda: L.namp_tied_score(0, 33, 2)}
    plain = lambda msg: b"null weights" in msg and b"attached" not in msg
    assert plain(carried())                                                    # nothing attached: the plain decoder's refusal
    for noun in attach:
        assert attach[noun]() == 0
        msg = carried()
        assert noun + b" was attached" in msg and b"null pointer" in msg
        assert plain(carried())                                                # taken and cleared by the call that failed
        assert attach[noun]() == 0 and attach[noun]() == 0                     # the same kind again replaces it: no conflict
        assert noun + b" was attached" in carried() and plain(carried())
        assert attach[noun]() == 0 and refused[noun]() == -1                   # a refused attach of the same kind leaves it cleared
        assert plain(carried())
    for a in attach:
        for b in attach:
            if a == b:
                continue
            assert attach[a]() == 0 and attach[b]() == 0                       # two kinds: neither runs, both named, both gone
            msg = carried()
            assert a in msg and b in msg and b"null" not in msg
            assert plain(carried())
            assert attach[a]() == 0 and refused[b]() == -1                     # a refused attach of another kind leaves this one
            assert a + b" was attached" in carried() and plain(carried())
    assert all(f() == 0 for f in attach.values())                              # all three at once
    msg = carried()
    assert all(noun in msg for noun in attach) and plain(carried())
