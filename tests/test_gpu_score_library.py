"""GPU tests of ProteinMPNN.score_sequences — a library of candidate sequences scored on one complex: the dense route (every
sequence a stream of the ordinary decoder) and the active-row route (namp_library: only the rows a varying token reaches are
evaluated per sequence) against the CPU oracle, against each other where the oracle does not reach, and their invariants; the
CLI's --score_fasta."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import library_ref as LR

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def make_model(weights_np, k, dev, n_dec=3):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, num_decoder_layers=n_dec, atom_dict=spec.atom_dict(),
                    restype_to_int=spec.restype_to_int(), polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    return m.to(dev).eval()


def cpu_fd(cx):
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd["batch_size"] = 1
    return fd


def to_dev(fd, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


_oracle = {}


def oracle_case(name, weights_np):
    """(k, complex, CPU feature_dict, positions, tokens, full sequences, oracle token_log_probs, order, numpy act counts): computed
    once per case and shared, never modified."""
    if name not in _oracle:
        k, cx, pos, tok = LR.make_case(name)
        fd = cpu_fd(cx)
        S_full = LR.full_sequences(cx["S"], pos, tok)
        ref, order, E_idx = LR.oracle_library(cpu_ref.to_torch(weights_np), fd, k, S_full, key=name)
        counts = LR.active_counts(E_idx.numpy(), LR.ranks_of(order.numpy()), cx["mask"], pos)
        _oracle[name] = (k, cx, fd, pos, tok, S_full, ref, order, counts)
    return _oracle[name]


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", ["n97", "crossing", "LltK", "all"])
def test_score_sequences_match_the_oracle(weights_np, name, prec):
    """Dense and active against the oracle (one encode, score() per sequence, the token's own entry): max |d token_log_probs| < 1e-3
    on EVERY entry (the project's parity bound); active against dense < 2e-4 (the bound of test_cone_equals_the_dense_form); the
    native sequence's row against score() < 2e-4; active_rows equals the numpy restatement on the oracle's E_idx and order, and in
    the case n97 sum(active_rows) < 3 L / 2 — an "active" route that ran the dense form would report nothing.  n97: 13 sequences
    (no multiple of the 16-row tile); crossing: a designed residue decodes before the fixed ones and fixed rows are active (86 of 97
    rows in layer 3); LltK: L = 32 < K = 48; all: every residue designed (58 of 60 rows in every layer).
    Measured max |d| (MI355X) over the four cases: dense / active vs oracle x3 1.9e-5 / 1.7e-5, fp32 3.1e-6 / 3.1e-6; active vs dense
    x3 1.2e-5, fp32 1.9e-6; native row vs score() x3 2.7e-5, fp32 1.9e-6; active rows n97 [26, 26, 26], crossing [54, 62, 86],
    LltK [9, 9, 9], all [58, 58, 58]."""
    dev = torch.device("cuda:0")
    k, cx, fd_cpu, pos, tok, S_full, ref, order, counts = oracle_case(name, weights_np)
    m = make_model(weights_np, k, dev)
    m.message_precision = prec
    fd = to_dev(fd_cpu, dev)
    L = len(cx["S"])
    lib = torch.from_numpy(tok)
    got = {}
    for method in ("dense", "active"):
        out = m.score_sequences(fd, lib, torch.from_numpy(pos), method=method)
        t = out["token_log_probs"].cpu()
        assert t.shape == ref.shape and t.dtype == torch.float32
        assert torch.equal(out["S"].cpu(), torch.from_numpy(S_full))
        assert torch.equal(out["decoding_order"].cpu(), order)
        assert out["base_log_probs"].shape == (1, L, 33)
        d = float((t - ref).abs().max())
        print(f"library parity {name} {method} {prec}: max|d token_log_probs| = {d:.3e}")
        assert d < 1e-3, d
        cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(np.float32))
        loss = (-ref * cm).sum(-1) / (cm.sum() + 1e-8)
        assert float((out["loss"].cpu() - loss).abs().max()) < 1e-3
        assert ("active_rows" in out) == (method == "active")
        got[method] = (t, out)
    d = float((got["active"][0] - got["dense"][0]).abs().max())
    print(f"library active vs dense {name} {prec}: max|d| = {d:.3e}")
    assert d < 2e-4, d
    sc = m.score(fd)["log_probs"][0].cpu()
    native = sc.gather(1, torch.from_numpy(cx["S"]).long()[:, None])[:, 0]
    for method in ("dense", "active"):
        d = float((got[method][0][-1] - native).abs().max())                 # (the native sequence is the library's last)
        print(f"library native row vs score() {name} {method} {prec}: max|d| = {d:.3e}")
        assert d < 2e-4, d
        base = got[method][1]["base_log_probs"][0].cpu()
        assert float((base - sc).abs().max()) < 2e-4
    rows = got["active"][1]["active_rows"]
    assert rows.dtype == torch.int32 and rows.shape == (3,) and rows.is_cuda
    print(f"library active rows {name}: {rows.tolist()} of L = {L}")
    assert rows.tolist() == counts
    if name == "n97":
        assert sum(counts) < 3 * L / 2
    if name == "crossing":
        assert counts[2] > len(pos)                                           # fixed rows are active


def n97(weights_np, dev, prec="x3"):
    k, cx, fd_cpu, pos, tok, S_full, ref, order, counts = oracle_case("n97", weights_np)
    m = make_model(weights_np, k, dev)
    m.message_precision = prec
    return m, to_dev(fd_cpu, dev), cx, torch.from_numpy(pos), torch.from_numpy(tok), ref


@pytest.mark.parametrize("method", ["dense", "active"])
def test_score_sequences_without_positions_and_with_one_sequence(weights_np, method):
    """n_var = 0: every row of token_log_probs equals the base row's entries (bit for bit), whatever the full-form library holds
    outside the (empty) positions, and no row is active.  n = 1: the oracle's row."""
    dev = torch.device("cuda:0")
    m, fd, cx, pos, tok, ref = n97(weights_np, dev)
    L = len(cx["S"])
    lib = torch.from_numpy(np.random.default_rng(5).integers(0, 33, (3, L)))
    out = m.score_sequences(fd, lib, torch.zeros(0, dtype=torch.long), method=method)
    base = out["base_log_probs"][0].gather(1, fd["S"][0].long()[:, None])[:, 0]
    assert torch.equal(out["token_log_probs"], base[None].expand(3, L))
    assert torch.equal(out["S"].cpu(), torch.from_numpy(cx["S"]).long()[None].expand(3, L))
    if method == "active":
        assert out["active_rows"].tolist() == [0, 0, 0]
    one = m.score_sequences(fd, tok[4:5], pos, method=method)["token_log_probs"].cpu()
    assert one.shape == (1, L) and float((one - ref[4:5]).abs().max()) < 1e-3


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("method,n", [("auto", 40), ("active", 40), ("dense", 40), ("dense", 24)])
def test_score_sequences_chunking_and_determinism(weights_np, method, n, prec):
    """n = 40 with score_library_tokens lowered so that the call takes three chunks (14 + 14 + 12 sequences): bit-identical to the
    one-chunk call, row for row — a sequence's bits do not depend on its chunk —, and two calls are bit-identical.  On the dense
    route a stream's bits are the ordinary decoder's, and namp_decoder_fwd changes its launch form at 2,500 residues per call
    (namp_fused_tail_max_residues): 40 x 97 residues in one call lie beyond it and 14 x 97 below, so there the three-chunk call is
    held to the 2e-4 of two summation orders (measured: x3 2.2e-5, fp32 1.9e-6), and to bit identity at n = 24 (24 x 97 and 8 x 97
    residues: one launch form).  The active route and "auto": 0 in both precisions."""
    dev = torch.device("cuda:0")
    m, fd, cx, pos, tok, ref = n97(weights_np, dev, prec)
    L = len(cx["S"])
    rng = np.random.default_rng(40)
    lib = torch.from_numpy(LR.random_library(rng, cx["S"], pos.numpy(), n, cx["protein_mask"], cx["dna_mask"], cx["rna_mask"]))
    one = m.score_sequences(fd, lib, pos, method=method)
    assert one["chunks"] == 1 and ("active_rows" in one) == (method != "dense")
    again = m.score_sequences(fd, lib, pos, method=method)
    assert torch.equal(one["token_log_probs"], again["token_log_probs"]) and torch.equal(one["loss"], again["loss"])
    per = -(-n // 3)                                                          # sequences per call: three chunks
    if method == "dense":
        m.score_library_tokens = per * L + L // 2
    else:                                                                     # (the active route spends 3 * tokens on the rows of act_l + var)
        o, rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])
        var, acts = LR.active_sets(m.featurize(fd)[2][0].cpu().numpy(), rank[0].cpu().numpy(), cx["mask"], pos.numpy())
        rows = sum(int((a | var).sum()) for a in acts)
        m.score_library_tokens = (per * rows + rows // 2) // 3 + 1
    three = m.score_sequences(fd, lib, pos, method=method)
    assert three["chunks"] == 3, three["chunks"]
    d = float((one["token_log_probs"] - three["token_log_probs"]).abs().max())
    print(f"library three chunks vs one {method} n={n} {prec}: max|d| = {d:.3e}")
    if method == "dense" and n * L > m_fused_max():
        assert d < 2e-4, d
    else:
        assert torch.equal(one["token_log_probs"], three["token_log_probs"])


def m_fused_max():
    from na_mpnn_amd import hip
    return int(hip.lib().namp_fused_tail_max_residues())


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_active_equals_dense_at_scale(weights_np, prec):
    """Active against dense at (1000, 48) with 40 designed residues and n = 64, where the oracle does not reach: < 2e-4; the active
    route evaluates a small part of the rows.  Measured (MI355X): x3 2.7e-5, fp32 1.9e-6; active rows [37, 37, 37] (38 positions:
    two of the 40 are masked)."""
    dev = torch.device("cuda:0")
    cx = synth.make_complex(seed=9048, n=1000, masked_frac=0.02)
    cx["chain_mask"] = np.zeros_like(cx["chain_mask"])
    cx["chain_mask"][700:740] = 1                                             # 40 DNA residues
    fd = to_dev(cpu_fd(cx), dev)
    pos = np.nonzero(cx["mask"] * cx["chain_mask"])[0]
    lib = torch.from_numpy(LR.random_library(np.random.default_rng(64), cx["S"], pos, 64, cx["protein_mask"], cx["dna_mask"], cx["rna_mask"]))
    m = make_model(weights_np, 48, dev)
    m.message_precision = prec
    dense = m.score_sequences(fd, lib, method="dense")
    act = m.score_sequences(fd, lib, method="active")
    assert torch.equal(dense["S"], act["S"])
    d = float((dense["token_log_probs"] - act["token_log_probs"]).abs().max())
    rows = act["active_rows"].tolist()
    print(f"library active vs dense (1000, 48) n_var={len(pos)} {prec}: max|d| = {d:.3e}, active rows {rows}")
    assert d < 2e-4, d
    o, rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])
    E_idx = m.featurize(fd)[2][0].cpu().numpy()
    assert rows == LR.active_counts(E_idx, rank[0].cpu().numpy(), cx["mask"], pos)
    assert 0 < sum(rows) < 3 * 1000 / 2


@pytest.mark.parametrize("method", ["dense", "active"])
def test_positions_as_a_subset_of_the_designed_set(weights_np, method):
    """`positions` as a proper subset of the designed set equals the full-form call with the other designed positions held at
    native (bit for bit on the dense route, which evaluates the same streams; < 2e-4 on the active route, whose plan differs)."""
    dev = torch.device("cuda:0")
    m, fd, cx, pos, tok, ref = n97(weights_np, dev)
    sub = pos[::3]
    tok_sub = tok[:5, ::3]
    a = m.score_sequences(fd, tok_sub, sub, method=method)
    held = torch.from_numpy(cx["S"]).long()[pos][None].repeat(5, 1)
    held[:, ::3] = tok_sub
    b = m.score_sequences(fd, torch.from_numpy(LR.full_sequences(cx["S"], pos.numpy(), held.numpy())), method=method)
    assert torch.equal(a["S"], b["S"])
    d = float((a["token_log_probs"] - b["token_log_probs"]).abs().max())
    print(f"library positions subset {method}: max|d| = {d:.3e}")
    assert d == 0.0 if method == "dense" else d < 2e-4, d
    if method == "active":
        assert sum(a["active_rows"].tolist()) <= sum(b["active_rows"].tolist())


def test_score_sequences_routes(weights_np):
    """The 4-layer model and the bf16 throughput mode take the dense route under "auto" and refuse "active"; a 3-layer x3 model
    takes the active route under "auto"; CPU feature dicts raise as for the other methods."""
    dev = torch.device("cuda:0")
    k, cx, pos, tok = LR.make_case("LltK")
    fd = to_dev(cpu_fd(cx), dev)
    lib, p = torch.from_numpy(tok), torch.from_numpy(pos)
    m4 = make_model(synth.make_weights(0, 3, 4), k, dev, 4)
    with pytest.raises(NotImplementedError):
        m4.score_sequences(fd, lib, p, method="active")
    out = m4.score_sequences(fd, lib, p)
    assert "active_rows" not in out and out["token_log_probs"].shape == (len(tok), len(cx["S"]))
    m = make_model(weights_np, k, dev)
    assert "active_rows" in m.score_sequences(fd, lib, p)
    with pytest.raises(ValueError):
        m.score_sequences(fd, lib, p, method="sparse")
    m.message_precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.score_sequences(fd, lib, p, method="active")
    assert "active_rows" not in m.score_sequences(fd, lib, p)
    with pytest.raises(RuntimeError):
        make_model(weights_np, k, dev).score_sequences(cpu_fd(cx), lib, p)


def test_cli_score_fasta(tmp_path, golden_dir):
    """--score_fasta end to end on tests/golden/pdb: the designs of a seqs/*.fa the CLI wrote are scored on the structure they were
    designed on, and scores/<name>.npz equals the Python call."""
    import lzma
    from na_mpnn_amd import cli, pdbio
    pdb = os.path.join(str(tmp_path), "1am9.pdb")
    with lzma.open(os.path.join(golden_dir, "pdb", "1am9.pdb.xz"), "rb") as fh, open(pdb, "wb") as out:
        out.write(fh.read())
    base = os.path.join(str(tmp_path), "out")
    common = ["--mode", "design", "--pdb_path", pdb, "--out_folder", base, "--random_init_seed", "0", "--seed", "7", "--design_na_only", "1"]
    cli.main(common + ["--batch_size", "3", "--output_pdbs", "0"])
    fa = os.path.join(base, "seqs", "1am9.fa")
    cli.main(common + ["--score_fasta", fa])
    z = np.load(os.path.join(base, "scores", "1am9.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["token_log_probs", "loss", "sequences", "mask", "chain_mask", "decoding_order", "seed"])
    P = pdbio.parse_pdb(pdb)
    L = len(P["S"])
    assert z["token_log_probs"].shape == (4, L) and z["token_log_probs"].dtype == np.float32     # the native line and three designs
    assert z["loss"].shape == (4,) and z["sequences"].shape == (4, L) and int(z["seed"]) == 7
    assert np.array_equal(z["sequences"][0], P["S"])
    names, seqs = cli.read_fasta(fa)
    assert len(seqs) == 4
    dev = torch.device("cuda:0")
    m = make_model(synth.make_weights(0), 32, dev)
    fd = pdbio.to_feature_dict(P, z["chain_mask"], dev)
    fd["batch_size"] = 1
    torch.manual_seed(7)
    fd["randn"] = torch.randn(1, L, device=dev)
    out = m.score_sequences(fd, torch.from_numpy(z["sequences"]).to(dev))
    assert np.array_equal(out["decoding_order"].cpu().numpy(), z["decoding_order"])
    assert np.array_equal(out["token_log_probs"].cpu().numpy(), z["token_log_probs"])
    assert np.array_equal(out["loss"].cpu().numpy(), z["loss"])
