"""Cost of the metric epilogue of the training loop (na_run.py:240-326) at the cfg5 shape: the reference-style epilogue (stock ops and
one synchronising device->host copy per table cell, restated below) against the fused metric launches of na_mpnn_amd.metrics.

    python tools/metrics_time.py [--B 16] [--N 1500] [--K 48] [--mode basic] [--rounds 3] [--window 1.0] [--precisions x3,bf16]

Variants, alternated round by round in one process, each timed over a device-synchronised window of >= --window seconds after warm-up:
  train+ref    train_step(...) followed by the reference-style epilogue
  train+fused  train_step(..., metrics=mm)
  valid+ref    no-grad forward followed by the reference-style epilogue
  valid+fused  train.valid_step(...)
  epi+ref / epi+fused   the two epilogues alone on fixed log_probs
Prints ms per step (median over rounds) and the device kernels each epilogue launches (torch.profiler), one JSON line per precision.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from na_mpnn_amd import metrics, spec, synth, train   # noqa: E402
from na_mpnn_amd.model import ProteinMPNN            # noqa: E402


def make_batch(B, N, dev, seed=5):
    cxs = [synth.make_complex(seed=seed + b, n=N, n_chains=4) for b in range(B)]
    fd = {k: torch.from_numpy(np.stack([c[k] for c in cxs])).to(dev) for k in cxs[0]}
    fd["S"] = fd["S"].long()
    g = torch.Generator().manual_seed(seed)
    na = ((fd["dna_mask"] + fd["rna_mask"]) > 0).cpu()
    fd["canonical_base_pair_mask"] = (na & (torch.rand(B, N, generator=g) > 0.3)).int().to(dev)
    fd["canonical_base_pair_index"] = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(dev)
    fd["interface_mask"] = (torch.rand(B, N, generator=g) > 0.5).int().to(dev)
    fd["ppm_mask"] = (torch.rand(B, N, generator=g) > 0.9).int().to(dev)
    fd["aligned_ppm"] = torch.softmax(torch.randn(B, N, 33, generator=g), -1).double().to(dev)
    return fd


def ref_epilogue(table, names, lp, fd, which, mfl, pm, im, rm, rn, pairs, weight, counts, rti):
    """The reference's epilogue with stock ops: loss_nll, canonical-pair accuracy, argmax, label-smoothed loss, and an accumulate
    that copies every cell's sum to the host on its own."""
    S = fd["S"]
    S_pred = torch.argmax(lp, -1)
    nll = F.nll_loss(lp.reshape(-1, lp.shape[-1]), S.reshape(-1), reduction="none").view(S.shape)
    _ = torch.sum(nll * mfl) / torch.sum(mfl)
    true_false = (S == torch.argmax(lp, -1)).float()
    pred = torch.argmax(lp, -1)
    partner = torch.gather(pred, 1, fd["canonical_base_pair_index"])
    hit = torch.zeros_like(pred, dtype=torch.bool)
    for a, b in pairs:
        hit = torch.logical_or(hit, torch.logical_and(pred == a, partner == b))
    cbp_mask = fd["canonical_base_pair_mask"]
    cbp = hit.long() * cbp_mask
    target = F.one_hot(S, lp.shape[-1]).to(torch.float64)
    ppm = fd["ppm_mask"].bool()
    target[ppm] = fd["aligned_ppm"][ppm]
    polys = {"protein": fd["protein_mask"], "dna": fd["dna_mask"], "rna": fd["rna_mask"]}
    eps = sum(polys[k][:, :, None] * rm[k][None, None, :] * (weight / rn[k]) for k in polys)
    target[:, :, (rm["protein"] + rm["dna"] + rm["rna"]).bool()] *= (1 - weight)
    target += eps
    loss = -(target * lp).sum(-1)
    for p in [""] + list(pm):
        for i in [""] + list(im):
            mask = mfl * (pm[p] if p else 1) * (im[i] if i else 1)
            r = names[which + ("_" + p if p else "") + ("_" + i if i else "")]
            table[r, 0] += torch.sum(mask).cpu().numpy()
            table[r, 1] += torch.sum(mask * cbp_mask).cpu().numpy()
            table[r, 2] += torch.sum(loss * mask).cpu().numpy()
            table[r, 3] += torch.sum(true_false * mask).cpu().numpy()
            table[r, 4] += torch.sum(cbp * mask * cbp_mask).cpu().numpy()
            for k, res in enumerate(counts):
                table[r, 5 + k] += torch.sum((S == rti[res]).long() * mask).cpu().numpy()
                table[r, 5 + len(counts) + k] += torch.sum((S_pred == rti[res]).long() * mask).cpu().numpy()


def window(fn, seconds):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def kernel_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type.name == "CUDA")
    except Exception as e:      # noqa: BLE001 — the count is optional
        return f"n/a ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16); ap.add_argument("--N", type=int, default=1500); ap.add_argument("--K", type=int, default=48)
    ap.add_argument("--mode", default="basic"); ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--precisions", default="x3,bf16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rti = spec.restype_to_int()
    fd = make_batch(a.B, a.N, dev)
    rm, rn = train.polymer_restype_tables(rti, 33, dev)
    no_loss = torch.tensor([rti[t] for t in ("UNK", "DX", "RX", "MAS", "PAD")], device=dev)
    S = fd["S"]
    mfl = fd["mask"] * (1 - torch.any(S[:, :, None] == no_loss[None, None, :], dim=-1).long())
    pairs = spec.na_canonical_base_pair_ints(rti)
    mm = metrics.generate_metric_manager(rti, a.mode)
    pm, im = mm.masks_for(fd)
    counts = list(mm.count_metrics)
    host_table = np.zeros((len(mm.all_mask_names), 5 + 2 * len(counts)))
    for prec in a.precisions.split(","):
        m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=a.K, dropout=0.1, atom_dict=spec.atom_dict(), restype_to_int=rti,
                        polytype_to_int=spec.polytype_to_int(), augment_eps=0.1)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
        m.to(dev).train()
        m.message_precision = prec
        opt = train.get_std_opt(m.parameters(), 128, 0)
        step = lambda **kw: train.train_step(m, opt, fd, rm, rn, no_loss, loss_tokens=6000.0, gradient_norm=1.0, **kw)
        lp_fixed = step()[1]
        epi_ref = lambda lp, which: ref_epilogue(host_table, mm.mask_to_row, lp, fd, which, mfl, pm, im, rm, rn, pairs, 0.1, counts, rti)
        epi_fused = lambda lp, which: mm.accumulate_from_log_probs(lp, fd, which, mfl, pm, im, polymer_restype_masks=rm,
                                                                   polymer_restype_nums=rn, weight=0.1)

        def valid_ref():
            m.eval()
            with torch.no_grad():
                lp, _ = m(fd)
                epi_ref(lp, "valid")
            m.train()

        def valid_fused():
            m.eval()
            train.valid_step(m, fd, mm, rm, rn, no_loss)
            m.train()

        variants = {"train+ref": lambda: epi_ref(step()[1], "train"), "train+fused": lambda: step(metrics=mm),
                    "valid+ref": valid_ref, "valid+fused": valid_fused,
                    "epi+ref": lambda: epi_ref(lp_fixed, "train"), "epi+fused": lambda: epi_fused(lp_fixed, "train")}
        for fn in variants.values():                       # warm-up
            fn(); fn()
        res = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                res[k].append(window(fn, a.window))
        mm.zero_metrics()
        out = {"precision": prec, "B": a.B, "N": a.N, "K": a.K, "mode": a.mode,
               "ms": {k: round(statistics.median(v), 3) for k, v in res.items()},
               "ms_all": {k: [round(x, 3) for x in v] for k, v in res.items()},
               "launches": {"epi+ref": kernel_launches(lambda: epi_ref(lp_fixed, "train")),
                            "epi+fused": kernel_launches(lambda: epi_fused(lp_fixed, "train"))}}
        print(json.dumps(out), flush=True)
        del m, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
