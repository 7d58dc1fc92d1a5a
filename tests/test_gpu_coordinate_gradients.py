"""Coordinate gradients on the GPU: dL/dX through the edge featuriser, carried by namp_train_feat_wgrad.

Kernel level: X.grad of (y * R).sum() through train.edge_embedding against the fp64 autograd of tests/xgrad_ref.py on the call's own
neighbour lists, bar 1e-4 of the largest entry — the project's bar for edge_embedding.weight from the same g_pre, the same regenerated RBFs
and the same fp32 MFMA products (tests/test_gpu_train.py::test_feature_weight_gradient).
End to end: dL/dX of the label-smoothed loss against fp64 autograd through oracle/cpu_ref.py, bar 2e-4 of the largest entry — the bar the
same shapes meet for every parameter gradient through the same backward chain (test_training_gradients_odd_shapes).

"Atoms with X_m == 0 have gradient exactly 0" holds for the featuriser's own 18 atoms (a masked atom of X18 gets exactly 0 from the
kernel).  In fd["X"] an absent N, CA or C of a protein residue (O4', C1', C2' of a nucleotide) is still a PARENT of the residue's virtual
Cb (N_na), whose mask is the polymer mask: autograd — the oracle's too — hands it the virtual atom's gradient.  The assertion below is
therefore exact zero for every absent atom that is not such a parent, and equality with the reference for all of them.
"""
import numpy as np
import pytest
import torch

from na_mpnn_amd import shard, spec, synth, train
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import call_history as ch
import xgrad_ref
from xgrad_ref import rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MC = synth.make_complex

# name -> (complexes, k, model kind)
CASES = {
    "46x14": (lambda: [MC(seed=31, n=46, n_chains=2, missing_atom_frac=0.05, masked_frac=0.04)], 14, "N"),     # the sibling test's case
    "9x9": (lambda: [MC(seed=32, n=9, n_chains=1)], 9, "N"),                      # K = L: E = 81 = one tile + 17, self edges
    "batch20_7k5": (lambda: [MC(seed=33, n=20, n_chains=2), MC(seed=34, n=7, n_chains=1)], 5, "N"),             # batch offsets, padded rows
    "64x16": (lambda: [MC(seed=35, n=64, n_chains=3, missing_atom_frac=0.03)], 16, "N"),                        # E an exact multiple of 64
    "all18": (lambda: [MC(seed=36, n=30, n_chains=3, frac_protein=0.4, frac_dna=0.3)], 12, "N"),                # protein + DNA + RNA chains
    "noN": (lambda: [MC(seed=37, n=25, n_chains=2, missing_atom_frac=0.05)], 10, "noN"),                         # include_pred_na_N = 0
}
_W = {}


def weights(kind):
    if kind not in _W:
        _W[kind] = synth.make_weights(0) if kind == "N" else synth.make_weights_noN(0)
    return _W[kind]


def make_model(kind, k):
    extra = {} if kind == "N" else {"include_pred_na_N": 0}
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, dropout=0.0, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int(), **extra)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights(kind).items()})
    return m.to(DEV)


def batch_of(cxs):
    fd = shard.pad_batch(cxs)
    fd["S"] = fd["S"].long()
    return fd


def parents_of_live_virtual_atoms(fd, with_Nna):
    """bool [B,L,16]: N, CA, C of protein residues; O4', C1', C2' of nucleotides (when the model has the virtual N_na atom)."""
    A = cpu_ref.ATOM
    p = torch.zeros(fd["X_m"].shape, dtype=torch.bool)
    prot = fd["protein_mask"].bool()
    na = (fd["dna_mask"] + fd["rna_mask"]).bool()
    for a in ("N", "CA", "C"):
        p[:, :, A[a]] = prot
    if with_Nna:
        for a in ("O4'", "C1'", "C2'"):
            p[:, :, A[a]] = na
    return p


_KERNEL_REF = {}


def kernel_reference(name, E_idx, R):
    """fp64 dX [B,L,16,3] on the call's own neighbour lists; computed once per case (the modes share lists and cotangent)."""
    key = (name, E_idx.cpu().numpy().tobytes())
    if key not in _KERNEL_REF:
        cxs, _, kind = CASES[name]
        fd = cpu_ref.to_dtype(batch_of(cxs()), torch.float64)
        W = torch.from_numpy(weights(kind)["features.edge_embedding.weight"]).double()
        _KERNEL_REF[key] = xgrad_ref.dX_autograd(W, fd["X"], fd, E_idx.cpu(), R.cpu().double())
    return _KERNEL_REF[key]


def test_the_all18_fixture_has_every_atom_and_both_virtual_atoms():
    fd = batch_of(CASES["all18"][0]())
    _, M18 = xgrad_ref.atom_frames(fd["X"].double(), fd)
    assert bool((M18[0].sum(0) > 0).all()) and M18.shape[-1] == 18
    assert int(fd["protein_mask"].sum()) > 0 and int(fd["dna_mask"].sum()) > 0 and int(fd["rna_mask"].sum()) > 0
    assert len(set(fd["chain_labels"][0].tolist())) == 3


@pytest.mark.parametrize("prec", ["fp32", "x3", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_level_gradient_matches_fp64_autograd(name, prec, monkeypatch):
    cxs, k, kind = CASES[name]
    fd_cpu = batch_of(cxs())
    fd = {k_: v.to(DEV) for k_, v in fd_cpu.items()}
    m = make_model(kind, k)
    m.message_precision = prec
    monkeypatch.setattr(train, "X3", train.PREC_CODE[prec])
    got = []
    for _ in range(2):
        X = fd["X"].clone().float().requires_grad_(True)
        with torch.enable_grad():
            y, E_idx = train.edge_embedding(m, dict(fd, X=X))
            R = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
            (y * R).sum().backward()
        assert X.grad is not None, "train.edge_embedding is not differentiable in fd['X']"
        got.append(X.grad.clone())
        m.zero_grad()
    assert torch.equal(got[0], got[1])                              # deterministic: no atomics, one summation order
    dX = got[0].cpu()
    ref = kernel_reference(name, E_idx, R)
    e = rel(dX, ref)
    inv = float(dX.double().sum((1, 2)).abs().max() / dX.double().abs().sum())
    print(f"{name} {prec}: rel {e:.2e}  translation {inv:.2e}")
    assert torch.isfinite(dX).all() and float(ref.abs().max()) > 0
    absent = (fd_cpu["X_m"] == 0) & ~parents_of_live_virtual_atoms(fd_cpu, kind == "N")
    assert bool(absent.any()) and bool((dX[absent] == 0).all())    # absent atoms, every atom of a padded residue among them
    if len(cxs()) > 1:
        pad = fd_cpu["X_m"].sum(-1) == 0
        assert bool(pad.any()) and bool((dX[pad] == 0).all())
    assert e < 1e-4
    assert inv < 1e-4                                               # sum over the atoms of a complex, relative to sum |dX|


# ---- end to end ----------------------------------------------------------------------------------------------------------
# the first three: of test_training_gradients_odd_shapes, same seeds.  The fourth has K % 16 == 0, the one condition under which the training
# step's backward is free of fp32 atomics (train.py: gpa_tiles; include/namp.h, flag 8 of the backward entry points) and repeats its own
# parameter gradients bit for bit.  Measured on the unchanged step at the first three shapes: 94 to 109 of the parameter gradients differ
# between two identical runs WITHOUT X.requires_grad.  "torch.equal to a run without X.requires_grad" is therefore asserted as such for
# log_probs and the loss at every shape, and for the parameter gradients under the project's rule for this very situation
# (call_history.assert_within_spread, as test_train_step_with_metrics_is_unchanged): equality where four identical runs without
# X.requires_grad coincide — K % 16 == 0, where it is also asserted outright —, else within 10 x their spread.
E2E = [([9], 48), ([20, 7], 5), ([40, 33, 24], 17), ([40, 33], 16)]
_E2E_REF = {}


def e2e_inputs(ns, k):
    cxs = [MC(seed=600 + 10 * i + n, n=n, n_chains=min(3, n), masked_frac=0.1 if n > 15 else 0.0) for i, n in enumerate(ns)]
    fd = batch_of(cxs)
    randn = torch.randn(len(ns), max(ns), generator=torch.Generator().manual_seed(k))
    return fd, randn


def e2e_reference(ns, k):
    key = (tuple(ns), k)
    if key not in _E2E_REF:
        fd, randn = e2e_inputs(ns, k)
        rti = spec.restype_to_int()
        w = cpu_ref.to_dtype({k_: torch.from_numpy(v) for k_, v in weights("N").items()}, torch.float64)
        fd64 = cpu_ref.to_dtype(fd, torch.float64)
        X = fd64["X"].clone().requires_grad_(True)
        fd64["X"] = X
        with torch.enable_grad():
            log_probs, _ = cpu_ref.forward_train(w, fd64, k, randn)
            S = fd64["S"].long()
            no_loss = torch.tensor([rti[t] for t in cpu_ref.NO_LOSS_TOKENS])
            S_mask = 1 - torch.any(S[:, :, None] == no_loss[None, None, :], dim=-1).long()
            rm, rn = cpu_ref.restype_masks(rti, log_probs.shape[-1])
            pm = {"protein": fd64["protein_mask"], "dna": fd64["dna_mask"], "rna": fd64["rna_mask"]}
            _, loss = cpu_ref.loss_smoothed(S, log_probs, fd64["mask"] * S_mask, pm, rm, rn, 0.1, 2000.0, log_probs.shape[-1])
            loss.backward()
        _E2E_REF[key] = (loss.detach(), X.grad.clone())
    return _E2E_REF[key]


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("ns,k", E2E)
def test_end_to_end_gradient_matches_the_oracle(ns, k, prec):
    fd_cpu, randn = e2e_inputs(ns, k)
    loss_ref, dX_ref = e2e_reference(ns, k)
    rti = spec.restype_to_int()
    m = make_model("N", k).train()
    m.message_precision = prec
    fd = {k_: v.to(DEV) for k_, v in fd_cpu.items()}
    rm, rn = train.polymer_restype_tables(rti, 33, DEV)
    no_loss = torch.tensor([rti[t] for t in cpu_ref.NO_LOSS_TOKENS], device=DEV)
    S, mask_for_loss = train._mask_for_loss(fd, no_loss)
    pm = {"protein": fd["protein_mask"], "dna": fd["dna_mask"], "rna": fd["rna_mask"]}

    def step(with_x):
        m.zero_grad()
        X = fd["X"].clone().float().requires_grad_(with_x)
        with torch.enable_grad():
            lp, _ = train.forward_train(m, dict(fd, X=X), randn.to(DEV))
            _, loss = train.loss_smoothed(S, lp, mask_for_loss, pm, rm, rn, weight=0.1, tokens=2000.0, num_letters=lp.shape[-1])
            loss.backward()
        return lp.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}, X.grad

    flat = lambda g: torch.cat([g[n].flatten() for n in sorted(g)])
    solos = [step(False) for _ in range(4)]
    lp0, loss0, g0, x0 = solos[0]
    lp1, loss1, g1, dX = step(True)
    assert x0 is None and dX is not None, "train.forward_train is not differentiable in fd['X']"
    # the unchanged outputs: what the step without X.requires_grad gives
    assert torch.equal(lp0, lp1) and torch.equal(loss0, loss1) and g0.keys() == g1.keys()
    spread = ch.assert_within_spread(flat(g1), [flat(s_[2]) for s_ in solos], f"{ns}/{k} {prec}: parameter gradients with X.requires_grad")
    if min(k, max(ns)) % 16 == 0:
        assert spread == 0.0
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n
    assert abs(float(loss1) - float(loss_ref)) <= 1e-5 * max(1e-3, abs(float(loss_ref)))
    e = rel(dX, dX_ref)
    print(f"{ns}/{k} {prec}: dL/dX rel {e:.2e} (max |ref| {float(dX_ref.abs().max()):.3e})")
    assert e < 2e-4

    # model.coordinate_gradients = the manual backward of sum w (-log p(S)) under score()'s order
    m.eval()
    w = (fd["mask"] * fd["chain_mask"]).float()
    X = fd["X"].clone().float().requires_grad_(True)
    with torch.enable_grad():
        lp, _ = train.forward_train(m, dict(fd, X=X), randn.to(DEV), order_mask=fd["mask"] * fd["chain_mask"])
        nll = -(w * torch.gather(lp, -1, fd["S"].long().unsqueeze(-1)).squeeze(-1)).sum()
        nll.backward()
    before = {n: p.grad.clone() for n, p in m.named_parameters()}
    out = m.coordinate_gradients(fd, decoding_randn=randn.to(DEV))
    assert torch.equal(out["loss"], nll.detach())
    if min(k, max(ns)) % 16 == 0:                                   # no atomics upstream of g_pre: the same bits
        assert torch.equal(out["dX"], X.grad)
    else:                                                           # two runs of one backward chain with fp32 atomics: the end-to-end bar
        assert rel(out["dX"], X.grad) < 2e-4
    assert out["dX"].shape == fd["X"].shape and out["residue_norm"].shape == fd["mask"].shape
    assert torch.equal(out["residue_norm"], out["dX"].reshape(*fd["mask"].shape, -1).norm(dim=-1))
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, before[n]), n                   # the call leaves parameter gradients alone


def test_coordinate_gradients_honours_chain_mask_order_and_weights():
    """Fixed residues (chain_mask = 0) come first in the order and carry no weight by default; explicit weights are used as given."""
    fd_cpu, randn = e2e_inputs([40, 33], 16)                        # K % 16 == 0: repeated calls give the same bits (see E2E)
    fd = {k_: v.to(DEV) for k_, v in fd_cpu.items()}
    fd["chain_mask"] = fd["chain_mask"].clone()
    fd["chain_mask"][:, ::3] = 0
    m = make_model("N", 16).eval()
    a = m.coordinate_gradients(fd, decoding_randn=randn.to(DEV))
    b = m.coordinate_gradients(fd, decoding_randn=randn.to(DEV), weights=(fd["mask"] * fd["chain_mask"]).float())
    c = m.coordinate_gradients(fd, decoding_randn=randn.to(DEV), weights=fd["mask"].float())
    assert torch.equal(a["dX"], b["dX"]) and torch.equal(a["loss"], b["loss"])
    assert float(c["loss"]) > float(a["loss"]) and not torch.equal(a["dX"], c["dX"])
    sc = m.score({**fd, "batch_size": 1, "randn": randn.to(DEV)})
    w = (fd["mask"] * fd["chain_mask"]).float()
    nll = -(w * torch.gather(sc["log_probs"], -1, fd["S"].long().unsqueeze(-1)).squeeze(-1)).sum()
    assert abs(float(nll) - float(a["loss"])) < 1e-3 * abs(float(nll))      # score()'s order: the same likelihood (two kernels' rounding)


def test_cli_coordinate_gradients(tmp_path, golden_dir):
    """--coordinate_gradients 1 end to end on tests/golden/cli/input.pdb: gradients/<name>.npz equals the Python call (K = 32: a
    multiple of 16, the same bits)."""
    import os
    from na_mpnn_amd import cli, pdbio
    pdb = os.path.join(golden_dir, "cli", "input.pdb")
    base = os.path.join(str(tmp_path), "out")
    cli.main(["--mode", "design", "--pdb_path", pdb, "--out_folder", base, "--random_init_seed", "0", "--seed", "7", "--design_na_only", "1",
              "--coordinate_gradients", "1"])
    z = np.load(os.path.join(base, "gradients", "input.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["dX", "residue_norm", "loss", "encoded_residues", "mask", "chain_mask", "decoding_randn"])
    P = pdbio.parse_pdb(pdb)
    L = len(P["S"])
    assert L >= 32
    dev = torch.device(DEV)
    m = make_model("N", 32).eval()
    chain_mask = np.array([c in P["na_chain_letters"] for c in P["chain_letters"]], np.int32)      # --design_na_only 1
    fd = pdbio.to_feature_dict(P, chain_mask, dev)
    torch.manual_seed(7)
    fd["randn"] = torch.randn(1, L, device=dev)
    out = m.coordinate_gradients(fd)
    assert z["dX"].shape == (L, 16, 3) and z["dX"].dtype == np.float32 and z["residue_norm"].shape == (L,)
    assert np.array_equal(z["decoding_randn"], fd["randn"][0].cpu().numpy())
    assert np.array_equal(z["dX"], out["dX"][0].cpu().numpy()) and np.array_equal(z["residue_norm"], out["residue_norm"][0].cpu().numpy())
    assert float(z["loss"]) == float(out["loss"]) and float(np.abs(z["dX"]).max()) > 0
    assert list(z["encoded_residues"]) == [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    assert np.array_equal(z["chain_mask"], chain_mask)
