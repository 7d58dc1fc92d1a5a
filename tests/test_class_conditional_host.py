"""CPU tests of the pair-class conditionals (ProteinMPNN.conditional_probs(classes=True)): the definition on the CPU
oracle against the sampler's class distribution (wobble_ref.class_probs), that the cases discriminate (wobble lanes, the second
member's lanes, the class bias), the invariants of the oracle's rows, the refusals and the library's sizing / attach entry points."""
import pytest
import torch

from na_mpnn_amd import hip, spec
from oracle import cpu_ref
import class_loo_ref as C
import wobble_ref
from loo_numpy import near_tie_rows

torch.set_grad_enabled(False)
V = C.V


def recombined(specs, zs, L, tables=lambda s: s[2], bias=lambda s: s[3]):
    """{residue: row} of another combine on the same streams."""
    out = {}
    for s, z in zip(specs, zs):
        rows, _ = C.class_combine(z, s[1], tables(s), bias(s))
        out.update({r: row for r, row in zip(s[0], rows) if r < L})
    return out


def moved(a, b, residues):
    """max |a - b| over the entries finite in both, over the rows of `residues`."""
    d = 0.0
    for r in residues:
        both = torch.isfinite(a[r]) & torch.isfinite(b[r])
        d = max(d, float((a[r].double() - b[r].double())[both].abs().max()))
    return d


@pytest.mark.parametrize("name", C.CASES)
def test_the_conditional_is_the_samplers_class_distribution(name):
    """Premise 1: exp(clp) of the oracle with the classes that close on a special token zeroed, renormalised, is
    wobble_ref.class_probs' unrestricted p for the teacher-forced design call with the group visited last (T = 1, zero bias; with
    states on the flattened graph, members state-major) within 1e-6."""
    fd, _, cls, _, specs, zs = C.oracle_case(name)
    N = max(max(s[0]) for s in specs) + 1
    fdN = {"temperature": 1.0, "bias": torch.zeros(1, N, V), "mask": torch.ones(1, N, dtype=torch.int32),
           "chain_mask": torch.ones(1, N, dtype=torch.int32), "S": torch.zeros(1, N, dtype=torch.int64)}
    worst = 0.0
    for (g, gw, gt, gb), z, clp in zip(specs, zs, cls):
        lp = torch.zeros(1, N, V, dtype=torch.float64)
        lp[0, g] = torch.log_softmax(z.double(), -1)
        _, draws = wobble_ref.class_probs(lp, fdN, [g], [gw], [gt], [gb])
        assert draws[0][0] == g
        p = clp.exp() * torch.tensor([int(c) not in cpu_ref.SPECIAL_TOKENS for c in gt[-1]], dtype=torch.float64)
        p = p / p.sum()
        worst = max(worst, float((p - draws[0][1][0]).abs().max()))
    print(f"premise 1 {name}: max |p - class_probs| = {worst:.2e} over {len(specs)} groups")
    assert worst < 1e-6


@pytest.mark.parametrize("name", C.CASES)
def test_the_cases_discriminate(name):
    """Premise 2: the rows of wobble-capable pairs differ from the canonical (classes=False) oracle by at least 1e-2; swapping lanes 33 /
    34 in the second member's table (every second-listed pair member of a group) moves them by more than 1e-3; ignoring the class bias
    moves the biased pairs by more than 1e-3.  Measured minima over the pairs / groups of a case (canonical, lanes swapped, bias
    ignored): l48_k16 0.375 / 0.492 / 0.727; l12_lt_k 0.200 / 0.376 / 0.184; hybrid 0.795 / 0.237 / 0.242; states_pairs 0.403 / 0.456 /
    0.0761; cap16 0.788 / 0.878 / 0.421; 4oqu 0.613 / 0.0295 / no biased pair (its bias is 0)."""
    fd, rows, _, _, specs, zs = C.oracle_case(name)
    L = fd["S"].shape[1]
    wob = [s for s in specs if C.can_wobble(s)]
    assert wob
    ref = {r: rows[0, r].double() for s in specs for r in s[0] if r < L}
    canon = C.canonical_rows(specs, zs, L)
    swap = lambda s: [C_ if t % 2 == 0 else C_[:C.GU] + [C_[C.UG], C_[C.GU]] + C_[C.UG + 1:] for t, C_ in enumerate(s[2])]
    swapped = recombined(specs, zs, L, tables=swap)
    unbiased = recombined(specs, zs, L, bias=lambda s: [0.0] * C.LANES)
    res = lambda s: [r for r in s[0] if r < L]
    d_canon = min(moved(ref, canon, res(s)) for s in wob)
    d_swap = min(moved(ref, swapped, res(s)) for s in wob)
    biased = [s for s in wob if any(v != 0 for v in s[3])]
    d_bias = min([moved(ref, unbiased, res(s)) for s in biased], default=None)
    print(f"premise 2 {name}: {len(wob)} wobble-capable of {len(specs)}; min moved: canonical {d_canon:.3g}, lanes swapped {d_swap:.3g}, "
          f"bias ignored {d_bias if d_bias is None else round(d_bias, 4)} ({len(biased)} biased)")
    assert d_canon >= 1e-2 and d_swap > 1e-3
    assert name == "4oqu" or biased
    if biased:
        assert d_bias > 1e-3
    for s in specs:                                          # a group without wobble lanes: the canonical rows
        if not C.can_wobble(s):
            assert moved(ref, canon, res(s)) < 1e-6


@pytest.mark.parametrize("name", C.CASES)
def test_invariants_of_the_oracle_rows(name):
    """logsumexp(row) = 0 on every row, exp(clp) sums to 1, absent lanes are exactly -inf (every lane from spec.N_CLASSES on; lanes
    33 / 34 of a group that cannot wobble, the DNA-DNA pairs of `hybrid` among them), and the oracle leaves NO row and no class row
    out of the arg-max comparison of the GPU tests (top-two gap at least 2e-3)."""
    fd, rows, cls, _, specs, _ = C.oracle_case(name)
    assert float(torch.logsumexp(rows.double(), -1).abs().max()) < 1e-6
    assert float((cls.exp().sum(-1) - 1).abs().max()) < 1e-12
    assert bool((cls[:, spec.N_CLASSES:] == C.NEG).all()) and bool(torch.isfinite(cls[:, :V]).all())
    for s, clp in zip(specs, cls):
        assert bool(torch.isfinite(clp[[C.GU, C.UG]]).all()) == C.can_wobble(s)
        assert C.can_wobble(s) or bool((clp[[C.GU, C.UG]] == C.NEG).all())
    assert near_tie_rows(rows, fd["mask"])[1] == 0 and C.near_tie(cls) == 0
    if name == "hybrid":
        rti = spec.restype_to_int()
        pairs = [tuple(s[0]) for s in specs]
        assert pairs == [(24, 44), (25, 45), (46, 26), (47, 27), (28, 43), (29, 42), (48, 63), (49, 62)]        # (50, 61) is dropped: 61 is masked
        assert [C.can_wobble(s) for s in specs] == [True] * 4 + [False] * 2 + [True] * 2
        t = {p: s[2] for p, s in zip(pairs, specs)}
        # "its own G / U / T": the DNA member holds DG / DT, the RNA member G / U, on either side
        assert (t[(24, 44)][0][C.GU], t[(24, 44)][1][C.GU], t[(24, 44)][0][C.UG], t[(24, 44)][1][C.UG]) == (rti["DG"], rti["U"], rti["DT"], rti["G"])
        assert (t[(46, 26)][0][C.GU], t[(46, 26)][1][C.GU], t[(46, 26)][0][C.UG], t[(46, 26)][1][C.UG]) == (rti["G"], rti["DT"], rti["U"], rti["DG"])
        assert (t[(48, 63)][0][C.GU], t[(48, 63)][1][C.GU]) == (rti["G"], rti["U"])
    if name == "cap16":
        assert max(len(s[0]) for s in specs) == 16
    if name == "states_pairs":
        assert sum(len(s[0]) == 4 for s in specs) == 6


def make_model(k=16):
    from na_mpnn_amd.model import ProteinMPNN
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int())


def test_class_arguments_are_refused_before_any_device_work():
    """Everything classes=False refuses is still refused, with classes=False word for word and with classes=True where it is no
    pair-class matter; a wobble pair inside a symmetry group is mapped_groups' ValueError."""
    m = make_model()
    fd = C.case_inputs("l48_k16")
    pairs = fd["paired_residues"]
    plain = {k: v for k, v in fd.items() if k not in ("paired_wobble", "paired_wobble_bias")}
    for tied in (False, True):
        with pytest.raises(NotImplementedError, match="pair classes"):
            m.conditional_probs(dict(plain, paired_wobble=True), tied=tied)
        with pytest.raises(NotImplementedError, match="pair classes"):
            m.conditional_probs(fd, tied=tied, classes=False)
    with pytest.raises(NotImplementedError, match="symmetry_residues"):
        m.conditional_probs(dict(fd, symmetry_residues=[[1, 2]], symmetry_weights=[[1.0, 1.0]]), classes=True)
    with pytest.raises(NotImplementedError, match="state_weights"):
        m.conditional_probs(dict(fd, state_weights=[0.5, 0.5]), classes=True)
    fd2 = {k: (torch.cat((v, v)) if torch.is_tensor(v) and k != "randn" else v) for k, v in fd.items()}
    for tied in (False, True):
        with pytest.raises(ValueError, match="one input complex"):
            m.conditional_probs(fd2, tied=tied, classes=True)
        with pytest.raises(ValueError, match="two pairs"):
            m.conditional_probs(dict(fd, paired_residues=pairs + [(pairs[0][0], 40)], paired_wobble=True, paired_wobble_bias=0.0), tied=tied,
                                classes=True)
        with pytest.raises(ValueError, match="entries for 5 pairs"):
            m.conditional_probs(dict(fd, paired_wobble=[True, False]), tied=tied, classes=True)
    with pytest.raises(ValueError, match="wobble pairs do not join symmetry groups"):
        m.conditional_probs(dict(fd, symmetry_residues=[[pairs[0][0], 30]], symmetry_weights=[[1.0, 1.0]]), tied=True, classes=True)
    with pytest.raises(ValueError, match="at most 16"):
        m.conditional_probs(dict(fd, symmetry_residues=[list(range(17))], symmetry_weights=[[1.0] * 17], paired_wobble=False), tied=True,
                            classes=True)
    with pytest.raises(ValueError, match="method"):
        m.conditional_probs(fd, method="fast", classes=True)


def test_class_tables_of_the_host_section():
    """The input section the model uploads: tables and biases are told apart by (table, bias) — the per-pair bias of l48_k16 gives its
    pair tables of their own —, table 0 is the identity below the vocabulary with no class beyond, the caches key on `classes` (slots of
    their own), the wobble flags and the biases, and a classes=False call neither reads nor evicts them."""
    m = make_model()
    fd = C.case_inputs("l48_k16")
    L = fd["S"].shape[1]
    a = m._conditional_arguments(fd, 1, L, None, False, True)
    assert a is m._conditional_arguments(fd, 1, L, None, False, True)                        # served from the cache
    n = a["n_tables"]
    assert n == 5 and a["section"].numel() == 4 * L + 2 * 64 * n                             # identity, first / second, first / second with the bias
    tabs = a["section"][4 * L:4 * L + 64 * n].view(n, 64)
    bias = a["section"][4 * L + 64 * n:].view(torch.float32).view(n, 64)
    assert tabs[0].tolist() == wobble_ref.IDENT and float(bias[0].abs().max()) == 0
    i, j = fd["paired_residues"][2]
    ti, tj = int(a["section"][2 * L + i]), int(a["section"][2 * L + j])
    assert bias[tj, C.GU] == bias[tj, C.UG] == 1.5 and bias[ti, C.GU] == 1.5 and float(bias[tj, :V].abs().max()) == 0
    assert a["index"].tolist() == [list(p) for p in fd["paired_residues"]]
    b = m._conditional_arguments(dict(fd, paired_wobble_bias=[0.0, 0.0, 0.5, 0.0, 0.0]), 1, L, None, False, True)
    assert b is not a and float(b["section"][4 * L + 64 * n:].view(torch.float32).max()) == 0.5
    c = m._conditional_arguments(dict(fd, paired_wobble=False), 1, L, None, False, True)
    assert c["n_tables"] == 2 and bool((c["section"][4 * L:4 * L + 128].view(2, 64)[:, V:] == -1).all())
    g = m._conditional_arguments(fd, 1, L, None, True, True)
    assert g is not a and torch.equal(g["section"], a["section"])                            # a pair's successor cycle IS its partner table
    plain = {k: v for k, v in fd.items() if k not in ("paired_wobble", "paired_wobble_bias")}
    p = m._conditional_arguments(plain, 1, L)
    assert p["section"].numel() == 4 * L + 64 * p["n_tables"] and "base" not in p
    a2 = m._conditional_arguments(fd, 1, L, None, False, True)
    assert a2 is not p and torch.equal(a2["section"], a["section"])
    assert m._conditional_arguments(plain, 1, L) is p and m._conditional_arguments(fd, 1, L, None, False, True) is a2      # neither evicts the other
    assert m._conditional_arguments(fd, 1, L, None, True, True) is g


def test_class_entry_points_validate_without_a_gpu():
    L = hip.lib()
    for groups in (0, 1):
        ride = (L.namp_loo_groups_workspace_bytes if groups else L.namp_loo_pairs_workspace_bytes)(1, 1000, 48, 3, 3)
        off = L.namp_loo_classes_out_offset(1, 1000, 48, 3, 3, groups)
        need = L.namp_loo_classes_workspace_bytes(1, 1000, 48, 3, 3, groups)
        assert off % 256 == 0 and off == ride + 256 * 3 and need == off + 4 * 64 * 1000      # the biases (3 x 64 words), then the class rows
        for args in ((1, 100, 24, 4, 2, groups), (0, 100, 24, 3, 2, groups), (1, 100, 24, 3, 0, groups), (1, 100, 24, 3, 65, groups)):
            assert L.namp_loo_classes_workspace_bytes(*args) == 0 and L.namp_loo_classes_out_offset(*args) == 0, args
    assert L.namp_loo_classes_workspace_bytes(1, 100, 24, 3, 2, 2) == 0
    for bad in ((0, 35, 0), (65, 35, 0), (-1, 35, 1)):
        assert L.namp_loo_classes(*bad) == -1 and b"n_tables" in L.namp_last_error()
    for bad in ((3, 0, 0), (3, 65, 1), (3, -2, 0)):
        assert L.namp_loo_classes(*bad) == -1 and b"n_classes" in L.namp_last_error()
    assert L.namp_loo_classes(3, 35, 2) == -1 and b"groups" in L.namp_last_error()
    # the attachment replaces a pair / group attachment and is replaced by them; a failed call clears it; an invalid attach leaves nothing
    null_call = lambda: L.namp_decoder_loo(None, None, None, None, None, None, None, None, None, None, 0, 1, 10, 4, None)
    assert L.namp_loo_classes(3, 35, 0) == 0
    assert null_call() == -1 and b"pair tables were attached" in L.namp_last_error()
    assert null_call() == -1 and b"attached" not in L.namp_last_error()
    assert L.namp_loo_pairs(3) == 0 and L.namp_loo_classes(3, 35, 1) == 0
    assert null_call() == -1 and b"group tables were attached" in L.namp_last_error()
    assert L.namp_loo_classes(3, 35, 1) == 0 and L.namp_loo_pairs(3) == 0
    assert null_call() == -1 and b"pair tables were attached" in L.namp_last_error()
    assert L.namp_loo_classes(3, 35, 1) == 0 and L.namp_loo_classes(3, 99, 1) == -1
    assert null_call() == -1 and b"attached" not in L.namp_last_error()


def test_command_line_argument_errors(tmp_path):
    """--conditional_classes 1 without --conditional_probs_only 1, and a value that is neither 0 nor 1: ValueError before anything is loaded."""
    from na_mpnn_amd import cli
    base = ["--mode", "design", "--pdb_path", "none.pdb", "--out_folder", str(tmp_path), "--random_init_seed", "0", "--device", "cpu"]
    with pytest.raises(ValueError, match="conditional_probs_only"):
        cli.main(base + ["--conditional_classes", "1"])
    with pytest.raises(ValueError, match="conditional_classes is 0 or 1"):
        cli.main(base + ["--conditional_probs_only", "1", "--conditional_classes", "2"])
    assert cli.build_parser().parse_args(base).conditional_classes == 0
