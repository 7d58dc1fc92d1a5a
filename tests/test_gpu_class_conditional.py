"""GPU tests of the pair-class conditionals — ProteinMPNN.conditional_probs(classes=True): the cone with class tables
(namp_loo_classes + namp_decoder_loo) against the CPU oracle's streams with the fp64 class combine, against the slow route, the
bit identities with the classes=False paths, and the command line."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import ProteinMPNN
import class_loo_ref as C
from loo_numpy import near_tie_rows

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
TOL = 1e-3                                                   # the project's parity bound
WOBBLE = ("paired_wobble", "paired_wobble_bias")
TIES = ("paired_residues", "paired_weights", "symmetry_residues", "symmetry_weights", "symmetry_token_maps") + WOBBLE


def make_model(weights_np, k, prec="x3"):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    m = m.to(DEV).eval()
    m.message_precision = prec
    return m


def to_dev(fd):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def without(fd, keys):
    return {k: v for k, v in fd.items() if k not in keys}


def keys_of(tied):
    return ("groups", "group_log_probs", "group_class_log_probs") if tied else ("pairs", "pair_log_probs", "pair_class_log_probs")


def finite_diff(got, ref):
    """max |got - ref| on the finite entries, after asserting that the -inf pattern is the same."""
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and not bool(torch.isnan(got).any())
    both = torch.isfinite(ref)
    return float((got.double() - ref.double())[both].abs().max()) if bool(both.any()) else 0.0


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", C.CASES)
def test_class_conditionals_match_the_oracle(weights_np, name, prec):
    """Parity of the cone with class tables with the oracle's pair / group stream and the fp64 class combine, from coordinates, on the
    six cases of class_loo_ref.case_inputs: log_probs rows and class rows within 1e-3 on the finite entries, the -inf pattern equal,
    the arg-max of EVERY unmasked row and of every class row equal (the oracle leaves none out: asserted in
    test_class_conditional_host.py), every row a distribution within 1e-5, the tied pairs / groups named in listed order.
    Measured max |dlogp| (MI355X), x3 / fp32, rows and class rows alike: 1.0e-5 / 4.3e-6 (l48_k16), 1.3e-5 / 4.3e-6 (l12_lt_k), 2.8e-5 /
    3.8e-6 (hybrid), 1.1e-5 / 2.9e-6 (states_pairs), 6.2e-6 / 2.4e-6 (cap16), 3.2e-5 / 4.3e-6 (4oqu)."""
    fd_cpu, ref, ref_cls, _, specs, _ = C.oracle_case(name)
    tied = C.TIED[name]
    L = fd_cpu["S"].shape[1]
    m = make_model(weights_np, C.K_OF[name], prec)
    out = m.conditional_probs(to_dev(fd_cpu), method="cone", tied=tied, classes=True)
    k_list, k_rows, k_cls = keys_of(tied)
    got, cls = out["log_probs"].cpu(), out[k_cls].cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32 and cls.shape == (len(specs), 64) and cls.dtype == torch.float32
    d, dc = finite_diff(got, ref), finite_diff(cls, ref_cls.float())
    print(f"class conditional parity {name} {prec}: max|dlogp| rows {d:.3e}, class rows {dc:.3e}; {len(specs)} groups of sizes "
          f"{sorted({len(s[0]) for s in specs})}, {sum(C.can_wobble(s) for s in specs)} with wobble lanes")
    assert d < TOL and dc < TOL, (d, dc)
    compared, left_out = near_tie_rows(ref, fd_cpu["mask"])
    assert left_out == 0 and C.near_tie(ref_cls) == 0
    assert torch.equal(got.argmax(-1)[compared], ref.argmax(-1)[compared])
    assert torch.equal(cls.argmax(-1), ref_cls.argmax(-1))
    width = 2 if not tied else max(len(s[0]) for s in specs)
    assert out[k_list].dtype == torch.int64 and out[k_list].cpu().tolist() == [s[0] + [-1] * (width - len(s[0])) for s in specs]
    assert torch.equal(out[k_rows].cpu(), got[0, [s[0][0] for s in specs]])
    assert float((got.exp().sum(-1) - 1).abs().max()) < 1e-5 and float((cls.exp().sum(-1) - 1).abs().max()) < 1e-5
    assert not any(k in out for k in keys_of(not tied))


@pytest.mark.parametrize("name,prec", [("l48_k16", "x3"), ("l48_k16", "fp32"), ("states_pairs", "x3"), ("states_pairs", "fp32")])
def test_cone_equals_the_slow_route(weights_np, name, prec):
    """The cone with class tables against the slow route (method="dense": the L streams for the other rows, ONE teacher-forced design
    call of the sampler per pair / group, the class combine in torch) within 1e-3, class rows included.  Measured (MI355X), x3 / fp32:
    l48_k16 3.7e-5 / 2.9e-6, states_pairs 3.1e-5 / 2.9e-6."""
    fd_cpu, _, _, _, specs, _ = C.oracle_case(name)
    tied = C.TIED[name]
    m = make_model(weights_np, C.K_OF[name], prec)
    fd = to_dev(fd_cpu)
    cone, slow = m.conditional_probs(fd, tied=tied, classes=True), m.conditional_probs(fd, method="dense", tied=tied, classes=True)
    k_list, k_rows, k_cls = keys_of(tied)
    assert "cone_items" in cone and "cone_items" not in slow and torch.equal(cone[k_list], slow[k_list])
    d = finite_diff(cone["log_probs"].cpu(), slow["log_probs"].cpu())
    dc = finite_diff(cone[k_cls].cpu(), slow[k_cls].cpu())
    print(f"cone vs slow route {name} {prec}: max|dlogp| rows {d:.3e}, class rows {dc:.3e} over {len(specs)} groups")
    assert d < TOL and dc < TOL, (d, dc)
    assert torch.equal(slow[k_rows].cpu(), slow["log_probs"].cpu()[0, [s[0][0] for s in specs]])


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", ["l48_k16", "hybrid", "states_pairs"])
def test_without_wobble_lanes_the_bits_are_the_canonical_call(weights_np, name, prec):
    """classes=True without paired_wobble (the pair path: l48_k16, hybrid; the group path: states_pairs), and with
    paired_wobble_bias = -1e9, gives the bits of the classes=False call — rows, the rows of the tied pairs / groups, cone_items —;
    without wobble the class rows hold -inf on lanes 33 / 34, and their lanes below the vocabulary are the listed-first rows."""
    fd = to_dev(C.case_inputs(name))
    tied = C.TIED[name]
    m = make_model(weights_np, C.K_OF[name], prec)
    k_list, k_rows, k_cls = keys_of(tied)
    canon = m.conditional_probs(without(fd, WOBBLE), tied=tied)
    none = m.conditional_probs(without(fd, WOBBLE), tied=tied, classes=True)
    off = m.conditional_probs(dict(fd, paired_wobble=False), tied=tied, classes=True)
    silenced = m.conditional_probs(dict(fd, paired_wobble=True, paired_wobble_bias=-1e9), tied=tied, classes=True)
    assert k_cls not in canon
    for other in (none, off, silenced):
        assert sorted(other) == sorted(list(canon) + [k_cls])
        for k in ("log_probs", "cone_items", k_list, k_rows):
            assert torch.equal(other[k], canon[k]), k
    for other in (none, off):
        cls = other[k_cls]
        assert bool((cls[:, 33:] == -float("inf")).all()) and torch.equal(cls[:, :33], canon[k_rows])
    live = m.conditional_probs(fd, tied=tied, classes=True)
    assert torch.equal(live["cone_items"], canon["cone_items"]) and not torch.equal(live["log_probs"], canon["log_probs"])
    assert bool(torch.isfinite(live[k_cls][:, 33:35]).any())


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_class_conditional_invariants(weights_np, prec):
    """l48_k16: a pair through tied=True is the pair through tied=False bit for bit, class rows included; two identical calls are
    bit-identical; the rows of unpaired residues are those of a call without pairs; classes=True without anything to tie is the plain
    call; hybrid: a DNA-DNA pair's class row has -inf on lanes 33 / 34 and the pair with a masked member keeps its leave-one-out rows."""
    fd = to_dev(C.case_inputs("l48_k16"))
    m = make_model(weights_np, 16, prec)
    a, b = m.conditional_probs(fd, classes=True), m.conditional_probs(fd, classes=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    g = m.conditional_probs(fd, tied=True, classes=True)
    assert torch.equal(g["log_probs"], a["log_probs"]) and torch.equal(g["cone_items"], a["cone_items"])
    assert torch.equal(g["groups"], a["pairs"]) and torch.equal(g["group_log_probs"], a["pair_log_probs"])
    assert torch.equal(g["group_class_log_probs"], a["pair_class_log_probs"])
    plain = m.conditional_probs(without(fd, TIES))
    paired = sorted({r for p in fd["paired_residues"] for r in p})
    rest = [r for r in range(48) if r not in paired]
    assert torch.equal(a["log_probs"][0, rest], plain["log_probs"][0, rest])
    assert float((a["log_probs"] - plain["log_probs"])[0, paired].abs().amax(-1).min()) > 1e-2
    for tied in (False, True):
        same = m.conditional_probs(without(fd, TIES), tied=tied, classes=True)
        assert sorted(same) == sorted(plain) and torch.equal(same["log_probs"], plain["log_probs"])
    fd_h = to_dev(C.case_inputs("hybrid"))
    mh = make_model(weights_np, 24, prec)
    h = mh.conditional_probs(fd_h, classes=True)
    pairs = h["pairs"].cpu().tolist()
    assert [50, 61] not in pairs and len(pairs) == 8
    cls = h["pair_class_log_probs"].cpu()
    for p, row in zip(pairs, cls):
        assert bool(torch.isfinite(row[:33]).all()) and bool((row[35:] == -float("inf")).all())
        assert bool((row[33:35] == -float("inf")).all()) == (p in ([28, 43], [29, 42])), p
    plain_h = mh.conditional_probs(without(fd_h, TIES))
    assert torch.equal(h["log_probs"][0, [50, 61]], plain_h["log_probs"][0, [50, 61]])


def test_cli_conditional_classes(tmp_path, golden_dir):
    """--conditional_probs_only 1 --conditional_classes 1 --paired_wobble 1 on the tests/golden/cli input (DNA with DNA: no pair can
    wobble), without and with --conditional_tied 1: the keys and shapes of the file; the rows are those of the run without
    --conditional_classes, and the class rows hold -inf from lane 33 on."""
    from na_mpnn_amd import cli, pdbio
    gd = os.path.join(golden_dir, "cli")
    out = os.path.join(str(tmp_path), "out")
    P = pdbio.parse_pdb(os.path.join(gd, "input.pdb"))
    enc = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    b = [i for i, c in enumerate(P["chain_letters"]) if c == "B"][-3:]
    c = [i for i, c in enumerate(P["chain_letters"]) if c == "C"][:3]
    want = list(zip(b, reversed(c)))
    base = ["--mode", "design", "--pdb_path", os.path.join(gd, "input.pdb"), "--out_folder", out, "--random_init_seed", "0", "--seed", "7",
            "--conditional_probs_only", "1", "--paired_residues", ",".join(f"{enc[i]}:{enc[j]}" for i, j in want)]
    load = lambda: dict(np.load(os.path.join(out, "conditional_probs", "input.npz"), allow_pickle=True))
    common = ["log_probs", "S", "mask", "chain_mask", "chain_labels", "decoding_order", "encoded_residues"]
    cli.main(base)
    z0 = load()
    cli.main(base + ["--conditional_classes", "1", "--paired_wobble", "1", "--paired_wobble_bias", "0.5"])
    z = load()
    assert sorted(z) == sorted(common + ["pairs", "pair_class_log_probs"])
    L = z["S"].shape[0]
    assert z["log_probs"].shape == (L, 33) and z["pairs"].tolist() == [list(p) for p in want]
    assert z["pair_class_log_probs"].shape == (3, 64) and z["pair_class_log_probs"].dtype == np.float32
    assert np.array_equal(z["log_probs"], z0["log_probs"]) and np.all(np.isneginf(z["pair_class_log_probs"][:, 33:]))
    assert np.array_equal(z["pair_class_log_probs"][:, :33], z["log_probs"][[p[0] for p in want]])
    cli.main(base + ["--conditional_classes", "1", "--paired_wobble", "1", "--conditional_tied", "1"])
    zt = load()
    assert sorted(zt) == sorted(common + ["groups", "group_log_probs", "group_class_log_probs"])
    assert zt["groups"].tolist() == [list(p) for p in want] and zt["group_class_log_probs"].shape == (3, 64)
    assert np.array_equal(zt["log_probs"], z["log_probs"]) and np.array_equal(zt["group_class_log_probs"], z["pair_class_log_probs"])
    with pytest.raises(ValueError, match="paired_wobble"):
        cli.main(base + ["--paired_wobble", "1"])
