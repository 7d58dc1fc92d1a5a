"""Host path of na_mpnn_amd.metrics and train.featurize against tests/golden/metrics_ref.npz, which the real reference wrote
(tools/make_metrics_golden.py): metric tables (sums and normalised, NaN in the same places), print strings, row / column names,
the canonical-pair accuracy, the batched featurize, the canonical pair list, and the two-rank gloo all_reduce of the table."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from na_mpnn_amd import metrics, spec, train
from oracle import cpu_ref

MODES = ("basic", "all", "na_only_inference")
WEIGHTS = {"train": 0.1, "valid": 0.05}
PRINT_ARGS = (2, 17, "12.346", "1.500")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "metrics_ref.npz")))


def golden_batch(gold, b):
    keys = ["log_probs", "S", "mask", "protein_mask", "dna_mask", "rna_mask", "interface_mask", "canonical_base_pair_mask",
            "canonical_base_pair_index", "ppm_mask", "aligned_ppm"]
    return {k: torch.from_numpy(gold[f"b{b}_{k}"]) for k in keys}


def run_epilogue(mm, fd, which, fused, rm, rn, no_loss):
    """na_run.py's epilogue through our module: the fused entry point, or the reference's sequence of calls + accumulate."""
    S = fd["S"]
    mask_for_loss = fd["mask"] * (1 - torch.any(S[:, :, None] == no_loss[None, None, :], dim=-1).long())
    polymer_masks, interface_masks = mm.masks_for(fd)
    if fused:
        mm.accumulate_from_log_probs(fd["log_probs"], fd, which, mask_for_loss, polymer_masks, interface_masks, polymer_restype_masks=rm,
                                     polymer_restype_nums=rn, weight=WEIGHTS[which])
        return
    lp = fd["log_probs"]
    _, _, true_false = train.loss_nll(S, lp, mask_for_loss)
    cbp = metrics.compute_canonical_base_pair_accuracy(lp, fd["canonical_base_pair_mask"], fd["canonical_base_pair_index"], mm)
    loss, _ = train.loss_smoothed(S, lp, mask_for_loss, {k: fd[k + "_mask"] for k in ("protein", "dna", "rna")}, rm, rn,
                                  weight=WEIGHTS[which], num_letters=lp.shape[-1], ppm_mask=fd["ppm_mask"], aligned_ppm=fd["aligned_ppm"])
    mm.accumulate(loss, true_false, cbp, fd["canonical_base_pair_mask"], S, torch.argmax(lp, -1), which, mask_for_loss, polymer_masks,
                  interface_masks)


def golden_run(mm, batches, fused, device="cpu"):
    """The golden's schedule: train <- batches 0, 1 (weight 0.1); valid <- batches 1, 0 (weight 0.05)."""
    rti = spec.restype_to_int()
    rm, rn = train.polymer_restype_tables(rti, 33, device)
    no_loss = torch.tensor([rti[t] for t in cpu_ref.NO_LOSS_TOKENS], device=device)
    for which in mm.dataset_names:
        for b in ((0, 1) if which == "train" else (1, 0)):
            run_epilogue(mm, {k: v.to(device) for k, v in batches[b].items()}, which, fused, rm, rn, no_loss)


def assert_table(ours, ref):
    assert ours.shape == ref.shape
    assert np.array_equal(np.isnan(ours), np.isnan(ref))
    np.testing.assert_array_equal(ours[~np.isnan(ours)], ref[~np.isnan(ref)])


def test_canonical_base_pair_ints(gold):
    assert spec.na_canonical_base_pair_ints(spec.restype_to_int()) == [tuple(p) for p in gold["pair_ints"].tolist()]
    shared = spec.na_canonical_base_pair_ints(spec.restype_to_int(na_shared_tokens=True))
    assert shared == [tuple(p) for p in gold["pair_ints_shared"].tolist()]
    assert len(set(shared)) < 16                          # the shared DNA / RNA tokens alias pairs: duplicates kept
    assert ["%s-%s" % p for p in spec.NA_CANONICAL_BASE_PAIRS] == gold["pair_names"].tolist()


@pytest.mark.parametrize("b", [0, 1])
def test_canonical_base_pair_accuracy_host(gold, b):
    fd = golden_batch(gold, b)
    pairs = spec.na_canonical_base_pair_ints(spec.restype_to_int())
    out = metrics.compute_canonical_base_pair_accuracy(fd["log_probs"], fd["canonical_base_pair_mask"], fd["canonical_base_pair_index"], pairs)
    assert out.dtype == torch.int64
    np.testing.assert_array_equal(out.numpy(), gold[f"b{b}_cbp_accuracy"])
    assert int(out.sum()) > 0


@pytest.mark.parametrize("mode", MODES)
def test_names_match_the_reference(gold, mode):
    mm = metrics.generate_metric_manager(spec.restype_to_int(), mode)
    assert mm.all_mask_names == gold[f"{mode}_rows"].tolist()
    assert mm.metric_names == gold[f"{mode}_cols"].tolist()
    assert mm.mask_to_row == {n: i for i, n in enumerate(mm.all_mask_names)}
    assert mm.metric_to_col == {n: i for i, n in enumerate(mm.metric_names)}
    assert mm.metrics.shape == (len(mm.all_mask_names), len(mm.metric_names)) and not mm.metrics.any()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_host_tables_and_print_string_match_the_reference(gold, mode, fused):
    mm = metrics.generate_metric_manager(spec.restype_to_int(), mode)
    golden_run(mm, [golden_batch(gold, 0), golden_batch(gold, 1)], fused)
    assert_table(mm.metrics, gold[f"{mode}_sums"])
    mm.compute_metrics()
    assert_table(mm.metrics, gold[f"{mode}_normalised"])
    assert mm.create_print_string(*PRINT_ARGS) == str(gold[f"{mode}_print"])
    mm.zero_metrics()
    assert not mm.metrics.any()


def test_out_of_range_pair_index_raises_on_compute(gold):
    fd = golden_batch(gold, 0)
    fd["canonical_base_pair_index"][1, 4] = 60                  # == L
    mm = metrics.generate_metric_manager(spec.restype_to_int(), "basic")
    rm, rn = train.polymer_restype_tables(spec.restype_to_int(), 33, "cpu")
    mm.accumulate_from_log_probs(fd["log_probs"], fd, "train", fd["mask"], *mm.masks_for(fd), polymer_restype_masks=rm, polymer_restype_nums=rn)
    with pytest.raises(ValueError):
        mm.compute_metrics()


def test_featurize_matches_the_reference(gold):
    rti = spec.restype_to_int()
    items = []
    for i in range(2):
        pre = f"featin{i}_"
        d = {k[len(pre):]: (str(v) if v.dtype.kind == "U" else torch.from_numpy(v)) for k, v in gold.items() if k.startswith(pre)}
        items.append((d, torch.tensor(d["S"].shape[0])))
    fd = train.featurize(items + [([], 0)], spec.polytype_to_int(), rti, spec.atom_dict(), "cpu")
    ref_keys = [k[len("feat_"):] for k in gold if k.startswith("feat_")]
    assert sorted(fd) == sorted(ref_keys)
    assert list(fd) == ref_keys                                  # same key order
    for k in ref_keys:
        ref = gold["feat_" + k]
        if isinstance(fd[k], list):
            assert fd[k] == ref.tolist(), k
            continue
        assert str(fd[k].dtype) == str(gold["featdtype_" + k]), k
        np.testing.assert_array_equal(fd[k].numpy(), ref, err_msg=k)
    assert fd["S"][0, 7:].eq(rti["PAD"]).all() and fd["R_idx"][0, 7:].eq(-100).all() and fd["chain_labels"][0, 7:].eq(-1).all()
    assert train.featurize([([], 0)], spec.polytype_to_int(), rti, spec.atom_dict(), "cpu") == "pass"


def _worker(rank, world, port, table, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mm = metrics.generate_metric_manager(spec.restype_to_int(), "basic")
    mm.metrics = table * (rank + 1)
    mm.all_reduce()
    q.put((rank, mm.metrics.copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_all_reduce(gold):
    table = gold["basic_sums"]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, table, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        np.testing.assert_array_equal(res[r], table * 3)
