"""GPU tests of the metric kernels (namp_train_metrics / namp_canonical_pair_accuracy, csrc/namp_metrics.h) against the host path of
na_mpnn_amd.metrics on the same inputs, the reference golden, determinism, the absence of host syncs, and train_step / valid_step."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import metrics, spec, synth, train
from oracle import cpu_ref
from test_gpu_train import make_model
from test_metrics import MODES, PRINT_ARGS, assert_table, golden_batch, golden_run, gold  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTI = spec.restype_to_int()


def loss_col(mm):
    return mm.metric_to_col["loss"]


def assert_device_equals_host(dev, host, mm):
    """Integer-valued columns exactly equal, the loss column within 1e-12 relative."""
    assert np.array_equal(np.isnan(dev), np.isnan(host))
    c = loss_col(mm)
    other = [j for j in range(dev.shape[1]) if j != c]
    np.testing.assert_array_equal(dev[:, other], host[:, other])
    np.testing.assert_allclose(dev[:, c], host[:, c], rtol=1e-12, atol=0)


@pytest.mark.parametrize("b", [0, 1])
def test_canonical_pair_accuracy_device_equals_host(gold, b):
    fd = golden_batch(gold, b)
    lp = fd["log_probs"].clone()
    lp[0, 5, 7] = float("nan")                                  # a NaN row (its argmax is the NaN) ...
    j = int(fd["canonical_base_pair_index"][0, 5])
    lp[0, j, [2, 30]] = float("nan")                            # ... and a partner row with two NaNs
    pairs = spec.na_canonical_base_pair_ints(RTI)
    args = (fd["canonical_base_pair_mask"], fd["canonical_base_pair_index"])
    host = metrics.compute_canonical_base_pair_accuracy(lp, *args, pairs)
    dev = metrics.compute_canonical_base_pair_accuracy(lp.to(DEV), *[t.to(DEV) for t in args], pairs)
    assert dev.dtype == torch.int64
    assert torch.equal(dev.cpu(), host)
    assert torch.equal(torch.argmax(lp.to(DEV), -1).cpu(), torch.argmax(lp, -1))       # tie / NaN rule of the reference's argmax


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_device_tables_equal_host_and_golden(gold, mode, fused):
    batches = [golden_batch(gold, 0), golden_batch(gold, 1)]
    dev = metrics.generate_metric_manager(RTI, mode)
    golden_run(dev, batches, fused, DEV)
    assert dev._dev is not None                                 # accumulated on the device
    host = metrics.generate_metric_manager(RTI, mode)
    golden_run(host, batches, fused)
    sums = dev.metrics
    assert_device_equals_host(sums, host.metrics, dev)
    assert_device_equals_host(sums, gold[f"{mode}_sums"], dev)
    dev.compute_metrics()
    ref = gold[f"{mode}_normalised"]
    assert np.array_equal(np.isnan(dev.metrics), np.isnan(ref))
    np.testing.assert_allclose(dev.metrics[~np.isnan(ref)], ref[~np.isnan(ref)], rtol=1e-12, atol=0)
    assert dev.create_print_string(*PRINT_ARGS) == str(gold[f"{mode}_print"])


def cfg5_batch(seed=3, B=16, L=1500, V=33):
    """cfg5-sized epilogue inputs: padded rows, ppm rows, canonical pairs within each row."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(B, L, dtype=torch.int32)
    for b in range(B):
        mask[b, :L - 37 * b] = 1
    poly = torch.randint(0, 4, (B, L), generator=g)
    S = torch.randint(0, 32, (B, L), generator=g)
    S = torch.where(mask.bool(), S, torch.full_like(S, RTI["PAD"]))
    lp = torch.log_softmax(torch.randn(B, L, V, generator=g) + 3.0 * torch.nn.functional.one_hot(S, V), -1).float()
    idx = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    fd = {"S": S, "mask": mask, "protein_mask": (poly == 0).int() * mask, "dna_mask": (poly == 1).int() * mask,
          "rna_mask": (poly == 2).int() * mask, "interface_mask": (torch.rand(B, L, generator=g) > 0.5).int() * mask,
          "canonical_base_pair_mask": ((poly > 0) & (poly < 3)).int() * mask, "canonical_base_pair_index": idx,
          "ppm_mask": (torch.rand(B, L, generator=g) > 0.7).int() * mask, "aligned_ppm": torch.softmax(torch.randn(B, L, V, generator=g), -1).double()}
    return lp.to(DEV), {k: v.to(DEV) for k, v in fd.items()}


def fused(mm, lp, fd, which="train", weight=0.1):
    rm, rn = train.polymer_restype_tables(RTI, 33, DEV)
    no_loss = torch.tensor([RTI[t] for t in cpu_ref.NO_LOSS_TOKENS], device=DEV)
    mfl = fd["mask"] * (1 - torch.any(fd["S"][:, :, None] == no_loss[None, None, :], dim=-1).long())
    mm.accumulate_from_log_probs(lp, fd, which, mfl, *mm.masks_for(fd), polymer_restype_masks=rm, polymer_restype_nums=rn, weight=weight)
    return mfl, rm, rn


@pytest.mark.parametrize("mode", MODES)
def test_cfg5_fused_equals_the_given_path(mode):
    lp, fd = cfg5_batch()
    which = "valid" if mode == "na_only_inference" else "train"
    a = metrics.generate_metric_manager(RTI, mode)
    mfl, rm, rn = fused(a, lp, fd, which)
    b = metrics.generate_metric_manager(RTI, mode)
    S = fd["S"]
    loss, _ = train.loss_smoothed(S, lp, mfl, {k: fd[k + "_mask"] for k in ("protein", "dna", "rna")}, rm, rn, weight=0.1, num_letters=33,
                                  ppm_mask=fd["ppm_mask"], aligned_ppm=fd["aligned_ppm"])
    _, _, tf = train.loss_nll(S, lp, mfl)
    cbp = metrics.compute_canonical_base_pair_accuracy(lp, fd["canonical_base_pair_mask"], fd["canonical_base_pair_index"], b)
    b.accumulate(loss, tf, cbp, fd["canonical_base_pair_mask"], S, torch.argmax(lp, -1), which, mfl, *b.masks_for(fd))
    ta, tb = a.metrics, b.metrics
    assert_device_equals_host(ta, tb, a)
    rows = [a.mask_to_row[n] for n in a.all_mask_names if n.startswith(which)]
    assert ta[rows, a.metric_to_col["weights"]].min() > 0
    # per row: the loss column against torch.sum(loss_smoothed(...)[0] * row_mask) (same per-token function; fp64 order only)
    pm, im = a.masks_for(fd)
    for pname in [""] + list(pm):
        for iname in [""] + list(im):
            row = mfl * (pm[pname] if pname else 1) * (im[iname] if iname else 1)
            name = which + ("_" + pname if pname else "") + ("_" + iname if iname else "")
            ref = float(torch.sum(loss * row))
            assert abs(ta[a.mask_to_row[name], loss_col(a)] - ref) <= 1e-12 * abs(ref), name


def test_two_runs_are_bit_identical():
    lp, fd = cfg5_batch(seed=4)
    tabs = []
    for _ in range(2):
        mm = metrics.generate_metric_manager(RTI, "all")
        fused(mm, lp, fd)
        fused(mm, lp, fd, "valid", 0.2)
        tabs.append(mm.metrics.copy())
    assert tabs[0].tobytes() == tabs[1].tobytes()


def test_accumulate_does_not_synchronise():
    lp, fd = cfg5_batch(seed=5, B=2, L=300)
    mm = metrics.generate_metric_manager(RTI, "all")
    rm, rn = train.polymer_restype_tables(RTI, 33, DEV)
    mfl = fd["mask"].long()
    loss, _ = train.loss_smoothed(fd["S"], lp, mfl, {k: fd[k + "_mask"] for k in ("protein", "dna", "rna")}, rm, rn)
    tf = (fd["S"] == torch.argmax(lp, -1)).float()
    pm, im = mm.masks_for(fd)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            fd["S"].cpu()
        except RuntimeError:
            control = True
        else:
            control = False
        if control:
            mm.accumulate_from_log_probs(lp, fd, "train", mfl, pm, im, polymer_restype_masks=rm, polymer_restype_nums=rn)
            mm.accumulate(loss, tf, tf, fd["canonical_base_pair_mask"], fd["S"], fd["S"], "valid", mfl, pm, im)
            mm.accumulate_from_log_probs(lp, fd, "train", mfl, pm, im, polymer_restype_masks=rm, polymer_restype_nums=rn)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on a device->host copy on this build: the check would be vacuous")
    assert mm.metrics[mm.mask_to_row["train"], 0] == 2 * float(mfl.sum())


def test_out_of_range_pair_index_raises_on_device():
    lp, fd = cfg5_batch(seed=6, B=2, L=200)
    fd["canonical_base_pair_index"][1, 17] = -1
    mm = metrics.generate_metric_manager(RTI, "basic")
    fused(mm, lp, fd)
    with pytest.raises(ValueError):
        mm.compute_metrics()
    mm.zero_metrics()
    fd["canonical_base_pair_index"][1, 17] = 3
    fused(mm, lp, fd)
    mm.compute_metrics()


def _small_fd(B=2, N=120):
    cxs = [synth.make_complex(seed=900 + b, n=N, n_chains=3) for b in range(B)]
    fd = {k: torch.from_numpy(np.stack([c[k] for c in cxs])).to(DEV) for k in cxs[0]}
    fd["S"] = fd["S"].long()
    return fd


def test_train_step_with_metrics_is_unchanged(weights_np):
    """train_step(metrics=mm) against train_step(): the same loss and log_probs bit for bit, and the same parameters — bit for bit when
    two plain steps agree bit for bit; the backward's table gradients are accumulated with atomics, so where two plain steps already
    differ, the metric step may differ from them by no more than that."""
    fd = _small_fd()
    rm, rn = train.polymer_restype_tables(RTI, 33, DEV)
    no_loss = torch.tensor([RTI[t] for t in cpu_ref.NO_LOSS_TOKENS], device=DEV)
    randn = torch.randn(fd["S"].shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    outs = []
    for mm in (None, None, metrics.generate_metric_manager(RTI, "basic")):
        torch.manual_seed(1)
        m = make_model(weights_np, 24).train()
        opt = train.get_std_opt(m.parameters(), 128, 0)
        with torch.enable_grad():
            loss, lp = train.train_step(m, opt, fd, rm, rn, no_loss, gradient_norm=1.0, decoding_randn=randn, metrics=mm)
        outs.append((loss, lp, torch.cat([p.detach().flatten() for p in m.parameters()]), mm))
    (l0, lp0, p0, _), (_, _, p0b, _), (l1, lp1, p1, mm) = outs
    assert torch.equal(l0, l1) and torch.equal(lp0, lp1)
    spread = float((p0b - p0).abs().max())
    if spread == 0.0:
        assert torch.equal(p0, p1)
    else:
        assert float((p1 - p0).abs().max()) <= 10 * spread, (float((p1 - p0).abs().max()), spread)
    ref = metrics.generate_metric_manager(RTI, "basic")
    S = fd["S"]
    mfl = fd["mask"] * (1 - torch.any(S[:, :, None] == no_loss[None, None, :], dim=-1).long())
    ref.accumulate_from_log_probs(lp1, fd, "train", mfl, *ref.masks_for(fd), polymer_restype_masks=rm, polymer_restype_nums=rn, weight=0.1)
    assert mm.metrics.tobytes() == ref.metrics.tobytes()
    assert mm.metrics[mm.mask_to_row["train"], 0] > 0 and not mm.metrics[mm.mask_to_row["valid"]].any()
    print(f"parameter spread of two plain steps: {spread:.3e}")


def test_valid_step(weights_np):
    fd = _small_fd()
    rm, rn = train.polymer_restype_tables(RTI, 33, DEV)
    no_loss = torch.tensor([RTI[t] for t in cpu_ref.NO_LOSS_TOKENS], device=DEV)
    randn = torch.randn(fd["S"].shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    m = make_model(weights_np, 24).eval()
    mm = metrics.generate_metric_manager(RTI, "basic")
    lp = train.valid_step(m, fd, mm, rm, rn, no_loss, decoding_randn=randn)
    with torch.no_grad():
        lp_ref, _ = m(fd, randn)
    assert torch.equal(lp, lp_ref)
    host = metrics.generate_metric_manager(RTI, "basic")
    S = fd["S"].cpu()
    fd_c = {k: v.cpu() for k, v in fd.items() if isinstance(v, torch.Tensor)}
    mfl = fd_c["mask"] * (1 - torch.any(S[:, :, None] == no_loss.cpu()[None, None, :], dim=-1).long())
    host.accumulate_from_log_probs(lp.cpu(), fd_c, "valid", mfl, *host.masks_for(fd_c), polymer_restype_masks={k: v.cpu() for k, v in rm.items()},
                                   polymer_restype_nums=rn, weight=0.1)
    assert_device_equals_host(mm.metrics, host.metrics, mm)
    assert mm.metrics[mm.mask_to_row["valid"], 0] > 0
