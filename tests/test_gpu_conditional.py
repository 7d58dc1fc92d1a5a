"""GPU tests of ProteinMPNN.conditional_probs — leave-one-out scoring of every residue in one call: the dense (L-stream) form
and the cone kernels (namp_decoder_loo) against the CPU oracle, against each other at sizes the oracle cannot reach, and their
invariants; the CLI's --conditional_probs_only."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import shard, spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
from loo_numpy import loo_grids, near_tie_rows, oracle_conditional

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MAX_LEFT_OUT = 0.05          # near-tie rows (oracle top-two gap < 2e-3) whose arg-max is not compared: at most 5 % of a case's rows


def make_model(weights_np, k, dev, n_dec=3):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, num_decoder_layers=n_dec, atom_dict=spec.atom_dict(),
                    restype_to_int=spec.restype_to_int(), polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def cpu_fd(cxs):
    if len(cxs) == 1:
        fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cxs[0].items()}
    else:
        fd = shard.pad_batch(cxs)
    fd["batch_size"] = 1
    return fd


def to_dev(fd, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def parity_cases():
    """name -> (k_neighbors, complexes).  Rows the oracle itself leaves out of the arg-max comparison (mask == 1, top-two gap < 2e-3),
    counted on the CPU: none in any of the four cases."""
    return {"n97_k32": (32, [synth.make_complex(seed=497, n=97, missing_atom_frac=0.05, masked_frac=0.04)]),
            "n150_k48": (48, [synth.make_complex(seed=550, n=150)]),
            "n32_k48_LltK": (48, [synth.make_complex(seed=432, n=32)]),
            "padded_b2": (32, [synth.make_complex(seed=497, n=97, missing_atom_frac=0.05, masked_frac=0.04),
                               synth.make_complex(seed=460, n=60)])}


_oracle_cache = {}


def oracle_case(name, weights_np):
    if name not in _oracle_cache:
        k, cxs = parity_cases()[name]
        fd = cpu_fd(cxs)
        lp, order, _ = oracle_conditional(cpu_ref.to_torch(weights_np), fd, k)
        _oracle_cache[name] = (k, fd, lp, order)
    return _oracle_cache[name]


def check_argmax(got, ref, mask):
    compared, left_out = near_tie_rows(ref, mask)
    assert left_out <= MAX_LEFT_OUT * mask.numel(), (left_out, mask.numel())
    assert torch.equal(got.argmax(-1)[compared], ref.argmax(-1)[compared])
    return left_out


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("method", ["dense", "cone"])
@pytest.mark.parametrize("name", list(parity_cases()))
def test_conditional_probs_match_the_oracle(weights_np, name, method, prec):
    """Parity with the oracle's L-stream brute force from coordinates: max |dlogp| < 1e-3 on EVERY row (masked rows included),
    arg-max identical on every unmasked row whose oracle top-two gap is at least 2e-3.
    Measured max |dlogp| (MI355X), dense / cone: x3 3.2e-5 / 2.1e-5 (n97), 4.2e-5 / 2.0e-5 (n150), 2.4e-5 / 1.8e-5 (n32), 3.3e-5 / 2.5e-5
    (padded); fp32 <= 3.4e-6 in every case; no near-tie row left out."""
    dev = torch.device("cuda:0")
    k, fd_cpu, ref, order = oracle_case(name, weights_np)
    m = make_model(weights_np, k, dev)
    m.message_precision = prec
    out = m.conditional_probs(to_dev(fd_cpu, dev), method=method)
    got = out["log_probs"].cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(out["decoding_order"].cpu(), order[0])
    assert torch.equal(out["S"].cpu(), fd_cpu["S"])
    d = float((got - ref).abs().max())
    print(f"conditional parity {name} {method} {prec}: max|dlogp| = {d:.3e}, near-tie rows left out {near_tie_rows(ref, fd_cpu['mask'])[1]}")
    assert d < 1e-3, d
    check_argmax(got, ref, fd_cpu["mask"])


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("n,k,n_dec", [(1000, 48, 3), (1000, 32, 3), (3000, 48, 3), (120, 24, 4)])
def test_cone_equals_the_dense_form(weights_np, n, k, n_dec, prec):
    """The cone kernels against the L streams on the ordinary decoder at sizes the oracle cannot reach (one evaluation in two
    summation orders): max |dlogp| < 2e-4, arg-max identical outside near ties; the item counts the call reports equal the numpy
    restatement of the grids on the same E_idx and rank — a "cone" that ran the dense form would report nothing.  The 4-layer model
    takes the dense form under "auto" (the cone kernels walk three layers) and refuses "cone"."""
    dev = torch.device("cuda:0")
    w = weights_np if n_dec == 3 else synth.make_weights(0, 3, n_dec)
    cx = synth.make_complex(seed=8000 + n + k, n=n, masked_frac=0.02)
    fd = to_dev(cpu_fd([cx]), dev)
    m = make_model(w, k, dev, n_dec)
    m.message_precision = prec
    dense = m.conditional_probs(fd, method="dense")["log_probs"].cpu()
    if n_dec != 3:
        with pytest.raises(NotImplementedError):
            m.conditional_probs(fd, method="cone")
        out = m.conditional_probs(fd)
        assert "cone_items" not in out
    else:
        out = m.conditional_probs(fd)
        o, rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])
        E_idx = m.featurize(fd)[2][0].cpu().numpy()
        _, act1, act2 = loo_grids(E_idx, rank[0].cpu().numpy(), cx["mask"])
        counts = out["cone_items"].cpu().numpy()
        print(f"cone items n={n} k={k}: {counts.tolist()} (per residue {counts[0] / n:.1f}, {counts[1] / n:.1f})")
        assert counts.tolist() == [int(act1.sum()), int(act2.sum())]
        assert counts[0] > 0 and counts[1] > 0
    got = out["log_probs"].cpu()
    d = float((got - dense).abs().max())
    print(f"cone vs dense n={n} k={k} n_dec={n_dec} {prec}: max|dlogp| = {d:.3e}")
    assert d < 2e-4, d          # measured: x3 3.3e-5 (1000, 48), 3.8e-5 (1000, 32), 3.4e-5 (3000, 48); fp32 <= 2.9e-6; 4 layers: 0 (same path)
    check_argmax(got, dense, torch.from_numpy(cx["mask"])[None])


@pytest.mark.parametrize("method", ["dense", "cone"])
def test_conditional_probs_invariants(weights_np, method):
    """Two calls agree bit for bit; a complex inside a padded batch is within 2e-4 of the same complex alone; every row is a
    distribution; and the result is NOT score(): more than half of the rows at (97, 32) differ from score()'s by more than 1e-2."""
    dev = torch.device("cuda:0")
    k, cxs = parity_cases()["padded_b2"]
    m = make_model(weights_np, k, dev)
    fd2 = to_dev(cpu_fd(cxs), dev)
    a = m.conditional_probs(fd2, method=method)["log_probs"]
    b = m.conditional_probs(fd2, method=method)["log_probs"]
    assert torch.equal(a, b)
    assert float((a.exp().sum(-1) - 1).abs().max()) < 1e-5
    for i, cx in enumerate(cxs):
        fd1 = to_dev(cpu_fd([cx]), dev)
        alone = m.conditional_probs(fd1, method=method)["log_probs"][0]
        n = cx["S"].shape[0]
        real = torch.from_numpy(cx["mask"]).bool()
        alone = alone.cpu()
        d = float((a[i, :n].cpu()[real] - alone[real]).abs().max())
        print(f"padded vs alone ({method}) complex {i}: max|dlogp| = {d:.3e}")
        assert d < 2e-4, d      # measured: 0 (cone; dense complex 0), 1.9e-6 (dense, complex 1)
        mk = torch.zeros(n, dtype=torch.int32); mk[real] = 1
        check_argmax(a[i, :n].cpu()[None], alone[None], mk[None])
    fd1 = to_dev(cpu_fd(cxs[:1]), dev)
    cond = m.conditional_probs(fd1, method=method)["log_probs"][0]
    sc = m.score(fd1)["log_probs"][0]
    differ = int(((cond - sc).abs().amax(-1) > 1e-2).sum())
    assert differ >= cond.shape[0] / 2, differ


def test_conditional_probs_arguments(weights_np):
    dev = torch.device("cuda:0")
    k, cxs = parity_cases()["n32_k48_LltK"]
    m = make_model(weights_np, k, dev)
    fd = to_dev(cpu_fd(cxs), dev)
    with pytest.raises(ValueError):
        m.conditional_probs(fd, method="sparse")
    m.message_precision = "bf16"                                     # throughput mode: the dense form under "auto", no cone
    with pytest.raises(NotImplementedError):
        m.conditional_probs(fd, method="cone")
    assert "cone_items" not in m.conditional_probs(fd)
    with pytest.raises(RuntimeError):
        make_model(weights_np, k, dev).conditional_probs(cpu_fd(cxs))   # CPU feature dicts raise as for the other methods


def test_cli_conditional_probs_only(tmp_path, golden_dir):
    """--conditional_probs_only 1 writes conditional_probs/<name>.npz (and no sequences) with the listed keys and shapes."""
    from na_mpnn_amd import cli, pdbio
    gd = os.path.join(golden_dir, "cli")
    out = os.path.join(str(tmp_path), "out")
    cli.main(["--mode", "design", "--pdb_path", os.path.join(gd, "input.pdb"), "--out_folder", out, "--random_init_seed", "0",
              "--seed", "7", "--conditional_probs_only", "1"])
    P = pdbio.parse_pdb(os.path.join(gd, "input.pdb"))
    L = len(P["S"])
    z = np.load(os.path.join(out, "conditional_probs", "input.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["log_probs", "S", "mask", "chain_mask", "chain_labels", "decoding_order", "encoded_residues"])
    assert z["log_probs"].shape == (L, 33) and z["log_probs"].dtype == np.float32
    for key in ("S", "mask", "chain_mask", "chain_labels", "decoding_order", "encoded_residues"):
        assert z[key].shape == (L,), key
    assert np.array_equal(z["S"], P["S"]) and sorted(z["decoding_order"].tolist()) == list(range(L))
    assert np.allclose(np.exp(z["log_probs"].astype(np.float64)).sum(-1), 1.0, atol=1e-5)
    assert not os.path.exists(os.path.join(out, "seqs")) and not os.path.exists(os.path.join(out, "backbones"))
