"""Writes tests/golden/metrics_ref.npz: the reference's training-loop epilogue on small seeded batches.

Imports the real reference (na_model_utils.py: featurize, loss_nll, loss_smoothed, compute_canonical_base_pair_accuracy;
na_metric_manager.py: generate_metric_manager), as oracle/make_goldens.py does, and records arrays and strings only:
the inputs, the canonical-pair accuracy, for each of the three metric modes the table before / after compute_metrics()
and the print string, the featurize output of a two-item batch, and the 16 canonical pairs as read from na_data_utils.py.

    python tools/make_metrics_golden.py [/path/to/NA-MPNN checkout]   (default: ../reference beside this repository)
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NAMP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import na_metric_manager as ref_mm     # noqa: E402
import na_model_utils as ref_mu        # noqa: E402

from na_mpnn_amd import spec, train    # noqa: E402
from oracle import cpu_ref             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics_ref.npz")
B, L, V = 3, 60, 33
WEIGHTS = {"train": 0.1, "valid": 0.05}
PRINT_ARGS = (2, 17, "12.346", "1.500")


def reference_pairs():
    """The (name, name) list PDBDataset.__init__ assigns to self.na_canonical_base_pair_restypes, read as a literal."""
    tree = ast.parse(open(os.path.join(REF, "na_data_utils.py")).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Attribute) and \
                node.targets[0].attr == "na_canonical_base_pair_restypes":
            return ast.literal_eval(node.value)
    raise RuntimeError("na_canonical_base_pair_restypes not found")


def make_batch(seed, rti, interface, ties):
    g = torch.Generator().manual_seed(seed)
    na = [rti[n] for n in ("DA", "DC", "DG", "DT", "A", "C", "G", "U")]
    poly = torch.randint(0, 4, (B, L), generator=g)                          # 0 protein, 1 dna, 2 rna, 3 none
    S = torch.randint(0, 20, (B, L), generator=g)
    S = torch.where(poly == 1, torch.tensor(na[:4])[torch.randint(0, 4, (B, L), generator=g)], S)
    S = torch.where(poly == 2, torch.tensor(na[4:])[torch.randint(0, 4, (B, L), generator=g)], S)
    S = torch.where(poly == 3, torch.full((B, L), rti["UNK"]), S)
    lengths = [L, L - 9, L - 23]
    mask = torch.zeros(B, L, dtype=torch.int32)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    S = torch.where(mask.bool(), S, torch.full((B, L), rti["PAD"]))
    logits = torch.randn(B, L, V, generator=g) + 2.5 * torch.nn.functional.one_hot(S, V)
    if ties:                                                                  # rows whose maximum is shared by two or more entries
        for b, l in [(0, 3), (1, 10), (2, 20), (0, 41)]:
            top = logits[b, l].max()
            logits[b, l, [5, 24, 27]] = top
        logits[2, 30] = 0.0                                                   # a constant row: argmax 0
    log_probs = torch.log_softmax(logits, -1).float()
    cbp_mask = torch.zeros(B, L, dtype=torch.int32)
    cbp_index = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):                                                        # pair up NA positions of each row
        pos = [int(i) for i in torch.nonzero((poly[b] == 1) | (poly[b] == 2)).flatten() if mask[b, i]]
        perm = torch.randperm(len(pos), generator=g).tolist()
        for k in range(0, len(perm) - 1, 2):
            i, j = pos[perm[k]], pos[perm[k + 1]]
            cbp_mask[b, i] = cbp_mask[b, j] = 1
            cbp_index[b, i], cbp_index[b, j] = j, i
    return {"log_probs": log_probs, "S": S, "mask": mask, "protein_mask": (poly == 0).int() * mask, "dna_mask": (poly == 1).int() * mask,
            "rna_mask": (poly == 2).int() * mask,
            "interface_mask": ((torch.rand(B, L, generator=g) > 0.6).int() * mask) if interface else torch.zeros(B, L, dtype=torch.int32),
            "canonical_base_pair_mask": cbp_mask, "canonical_base_pair_index": cbp_index,
            "ppm_mask": (torch.rand(B, L, generator=g) > 0.8).int() * mask,
            "aligned_ppm": torch.softmax(torch.randn(B, L, V, generator=g), -1).double()}


class _Dataset:
    def __init__(self, pairs):
        self.na_canonical_base_pair_ints = pairs


def epilogue(mm, fd, which, pairs, rm, rn, no_loss, mode):
    """na_run.py:240-273 (train) / :302-326 (valid) with the reference's functions."""
    S, log_probs = fd["S"], fd["log_probs"]
    S_mask = 1 - (torch.any(S[:, :, None] == no_loss[None, None, :], dim=-1)).long()
    mask_for_loss = fd["mask"] * S_mask
    polymer_masks = {k: fd[k + "_mask"] for k in mm.polymer_mask_names}
    interface_masks = {"interface": fd["interface_mask"], "nonInterface": 1 - fd["interface_mask"]} if mode == "all" else {}
    _, _, true_false = ref_mu.loss_nll(S, log_probs, mask_for_loss)
    cbp_acc = ref_mu.compute_canonical_base_pair_accuracy(log_probs, fd["canonical_base_pair_mask"], fd["canonical_base_pair_index"],
                                                          _Dataset(pairs))
    S_pred = torch.argmax(log_probs, -1)
    loss_pm = {k: fd[k + "_mask"] for k in ("protein", "dna", "rna")}
    loss, _ = ref_mu.loss_smoothed(S, log_probs, mask_for_loss, polymer_masks=loss_pm, polymer_restype_masks=rm, polymer_restype_nums=rn,
                                   weight=WEIGHTS[which], tokens=2000.0, num_letters=V, ppm_mask=fd["ppm_mask"], aligned_ppm=fd["aligned_ppm"])
    mm.accumulate(loss, true_false, cbp_acc, fd["canonical_base_pair_mask"], S, S_pred, which, mask_for_loss, polymer_masks, interface_masks)
    return cbp_acc


def featurize_items(rti):
    g = torch.Generator().manual_seed(77)
    items = []
    for n, name in [(7, "a.cif"), (11, "b.pdb")]:
        d = {"X": torch.randn(n, 16, 3, generator=g), "X_m": torch.randint(0, 2, (n, 16), generator=g).int(),
             "S": torch.randint(0, 32, (n,), generator=g), "R_idx": torch.arange(n, dtype=torch.int32) + 5,
             "chain_labels": torch.randint(0, 3, (n,), generator=g), "protein_mask": torch.randint(0, 2, (n,), generator=g).int(),
             "dna_mask": torch.randint(0, 2, (n,), generator=g).int(), "rna_mask": torch.randint(0, 2, (n,), generator=g).int(),
             "R_polymer_type": torch.randint(0, 5, (n,), generator=g), "interface_mask": torch.randint(0, 2, (n,), generator=g).int(),
             "base_pair_mask": torch.randint(0, 2, (n,), generator=g).int(), "base_pair_index": torch.randint(0, n, (n,), generator=g),
             "canonical_base_pair_mask": torch.randint(0, 2, (n,), generator=g).int(),
             "canonical_base_pair_index": torch.randint(0, n, (n,), generator=g),
             "aligned_ppm": torch.rand(n, len(rti), generator=g).double(), "ppm_mask": torch.randint(0, 2, (n,), generator=g).int(),
             "structure_path": name, "assembly_id": name[0] + "1"}
        items.append((d, torch.tensor(n)))
    return items


def main():
    rti = spec.restype_to_int()
    names = reference_pairs()
    pairs = [(rti[a], rti[b]) for a, b in names]
    rti_shared = spec.restype_to_int(na_shared_tokens=True)
    out = {"pair_names": np.array(["%s-%s" % p for p in names]), "pair_ints": np.array(pairs, dtype=np.int64),
           "pair_ints_shared": np.array([(rti_shared[a], rti_shared[b]) for a, b in names], dtype=np.int64)}
    rm, rn = train.polymer_restype_tables(rti, V, "cpu")
    no_loss = torch.tensor([rti[t] for t in cpu_ref.NO_LOSS_TOKENS])
    batches = [make_batch(11, rti, interface=True, ties=False), make_batch(12, rti, interface=False, ties=True)]
    for bi, fd in enumerate(batches):
        for k, v in fd.items():
            out[f"b{bi}_{k}"] = v.numpy()
    for mode in ("basic", "all", "na_only_inference"):
        mm = ref_mm.generate_metric_manager(rti, mode)
        for which in mm.dataset_names:
            for bi in ((0, 1) if which == "train" else (1, 0)):
                cbp = epilogue(mm, batches[bi], which, pairs, rm, rn, no_loss, mode)
                out[f"b{bi}_cbp_accuracy"] = cbp.numpy()
        out[f"{mode}_rows"] = np.array(mm.all_mask_names)
        out[f"{mode}_cols"] = np.array(mm.metric_names)
        out[f"{mode}_sums"] = mm.metrics.copy()
        mm.compute_metrics()
        out[f"{mode}_normalised"] = mm.metrics.copy()
        out[f"{mode}_print"] = np.array(mm.create_print_string(*PRINT_ARGS))
    items = featurize_items(rti)
    fd = ref_mu.featurize(items + [([], 0)], spec.polytype_to_int(), rti, spec.atom_dict(), "cpu")
    for k, v in fd.items():
        out["feat_" + k] = np.array(v) if isinstance(v, list) else v.numpy()
        if not isinstance(v, list):
            out["featdtype_" + k] = np.array(str(v.dtype))
    for i, (d, n) in enumerate(items):
        for k, v in d.items():
            out[f"featin{i}_{k}"] = np.array(v) if isinstance(v, str) else v.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
