"""GPU tests of ProteinMPNN.score_mutations — a mutational scan scored on per-site cones (namp_mutations): the cone route against the
CPU oracle, against score_sequences on both of its routes, its own invariants (the sparse layout, the fp32 sum of delta, chunks,
determinism), the rule of "auto", the scan form with pairs, and the CLI's --mutation_scan."""
import os

import numpy as np
import pytest
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN, mutation_chunks, mutations_dense
from oracle import cpu_ref
import library_ref as LR
import mutation_ref as MR

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
    """Per case, computed once and shared, never modified: k, the complex, its CPU feature_dict, sites, site_tokens, site names, the
    explicit sequences, the oracle's token log-probs [n, L], its order, and the numpy restatement of site_rows / row_offsets /
    row_residue on the oracle's E_idx and order."""
    if name not in _oracle:
        k, cx, pos, tok = LR.make_case(name)
        fd = cpu_fd(cx)
        w = cpu_ref.to_torch(weights_np)
        E_idx = LR.encoded(w, fd, k, "mut-" + name)[2][0].numpy()
        order = cpu_ref.decoding_order_of(fd["mask"] * fd["chain_mask"], fd["randn"])[0]
        sites, site_tokens, names = MR.case_sites(cx, E_idx, order.numpy())
        S_full = MR.expand(cx["S"], sites, site_tokens)
        ref, order2, _ = MR.oracle(w, fd, k, S_full, key="mut-" + name)
        assert torch.equal(order, order2)
        rank = LR.ranks_of(order.numpy())
        rows, _ = MR.site_rows(E_idx, rank, cx["mask"], sites)
        offsets, residues = MR.sparse_rows(E_idx, rank, cx["mask"], sites, site_tokens)
        _oracle[name] = dict(k=k, cx=cx, fd=fd, sites=sites, site_tokens=site_tokens, names=names, S_full=S_full, ref=ref, order=order,
                             rows=rows, offsets=offsets, residues=residues)
    return _oracle[name]


def setup(name, weights_np, prec):
    dev = torch.device("cuda:0")
    c = oracle_case(name, weights_np)
    m = make_model(weights_np, c["k"], dev)
    m.message_precision = prec
    return c, m, to_dev(c["fd"], dev), torch.from_numpy(c["sites"]), torch.from_numpy(c["site_tokens"])


def delta_bound(out):
    """delta[v] against the fp64 sum of the call's own fp32 terms w_i * (entry - base entry), in units of the bound of an fp32
    recursive sum, (rows - 1) * 2^-24 * sum |terms| -> the largest |error| and the largest error / bound (0 where both are 0)."""
    offs = out["row_offsets"].cpu().numpy()
    res = out["row_residue"].cpu().numpy().astype(np.int64)
    w = out["w"].cpu().numpy().astype(np.float32)
    terms = w[res] * (out["row_token_log_prob"].cpu().numpy() - out["base_token_log_probs"].cpu().numpy()[res])
    assert terms.dtype == np.float32
    delta = out["delta_log_likelihood"].cpu().numpy()
    worst, worst_abs = 0.0, 0.0
    for v in range(len(delta)):
        t = terms[offs[v]:offs[v + 1]].astype(np.float64)
        err, bound = abs(float(delta[v]) - t.sum()), (len(t) - 1) * 2.0 ** -24 * np.abs(t).sum()
        assert err <= bound, (v, err, bound, len(t))
        worst_abs = max(worst_abs, err)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst_abs, worst


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", ["n97", "crossing", "LltK", "all"])
def test_score_mutations_match_the_oracle(weights_np, name, prec):
    """The cone route on the sites of mutation_ref.case_sites — the first-decoded designed residue, the last-decoded residue, a
    masked residue (n97, crossing), two graph neighbours, two residues with disjoint cones (not in LltK, where L < K lets every
    residue reach all later ones), one site of 8 residues; three random variants per site and two wild types.
    mutations_dense(out) against the oracle (one encode, score() per explicit sequence): < 1e-3 on EVERY entry, loss < 1e-3; against
    score_sequences(method="dense") on the explicit library and, per site, score_sequences(method="active") with positions = the
    site: < 2e-4 on every entry; delta against the fp64 sum of the call's own fp32 terms within (rows - 1) * 2^-24 * sum |terms|;
    the wild-type variants' sparse entries within 2e-4 of the base entries; site_rows, row_offsets and row_residue equal the numpy
    restatement on the oracle's E_idx and order exactly; some cone size is no multiple of the 16-row item tile; the dense route of
    score_mutations itself < 1e-3 against the oracle.
    Measured max over the four cases (MI355X): cone vs oracle x3 1.9e-5, fp32 2.7e-6; loss 4.3e-6 / 9.6e-7; cone vs
    score_sequences dense 1.3e-5 / 1.9e-6; cone vs score_sequences active 0 / 0, the bits are equal in all eight runs; delta: error /
    bound at most 0.078 / 0.067 (|error| at most 1.8e-6); dense route vs oracle 2.1e-5 / 2.9e-6, delta cone vs dense 8.9e-5 / 5.5e-6;
    site rows n97 [14, 20, 23], [1, 1, 1], [1, 1, 1], [7, 7, 7], [9, 9, 9], [23, 23, 23]; crossing [42, 63, 87] ... [55, 63, 87];
    LltK [10, 10, 10] and [1, 1, 1]; all [44, 59, 59] ... [13, 14, 16], [59, 59, 59]."""
    c, m, fd, sites, site_tokens = setup(name, weights_np, prec)
    cx, ref, L = c["cx"], c["ref"], len(c["cx"]["S"])
    n = len(site_tokens)
    out = m.score_mutations(fd, sites=sites, site_tokens=site_tokens, method="cone")
    assert out["method"] == "cone" and out["chunks"] == 1
    assert torch.equal(out["decoding_order"].cpu(), c["order"])
    assert out["site_rows"].dtype == torch.int32 and np.array_equal(out["site_rows"].cpu().numpy(), c["rows"])
    assert out["row_offsets"].dtype == torch.int64 and np.array_equal(out["row_offsets"].cpu().numpy(), c["offsets"])
    assert out["row_residue"].dtype == torch.int32 and np.array_equal(out["row_residue"].cpu().numpy(), c["residues"])
    assert (c["rows"] % 16 != 0).any()
    assert c["rows"][c["names"].index("last")].tolist() == [1, 1, 1]
    assert out["base_log_probs"].shape == (1, L, 33) and out["delta_log_likelihood"].shape == (n,)
    assert torch.equal(out["site_index"].cpu(), site_tokens[:, 0]) and torch.equal(out["sites"].cpu(), sites)
    dense = mutations_dense(out, L).cpu()
    d = float((dense - ref).abs().max())
    print(f"mutations parity {name} cone {prec}: max|d token_log_probs| = {d:.3e}; site rows {c['rows'].tolist()}")
    assert d < 1e-3, d
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(np.float32))
    loss = (-ref * cm).sum(-1) / (cm.sum() + 1e-8)
    d = float((out["loss"].cpu() - loss).abs().max())
    print(f"mutations parity {name} cone {prec}: max|d loss| = {d:.3e}")
    assert d < 1e-3, d
    # against the library call, both routes
    S_full = torch.from_numpy(c["S_full"])
    union = torch.tensor(sorted({int(r) for r in c["sites"].reshape(-1) if r >= 0}))
    lib = m.score_sequences(fd, S_full, union, method="dense")["token_log_probs"].cpu()
    d = float((dense - lib).abs().max())
    print(f"mutations cone vs score_sequences dense {name} {prec}: max|d| = {d:.3e}")
    assert d < 2e-4, d
    worst, equal = 0.0, True
    for s in range(len(sites)):
        mine = np.nonzero(c["site_tokens"][:, 0] == s)[0]
        pos = torch.tensor(sorted(int(r) for r in c["sites"][s] if r >= 0))
        act = m.score_sequences(fd, S_full[mine], pos, method="active")["token_log_probs"].cpu()
        worst = max(worst, float((dense[mine] - act).abs().max()))
        equal = equal and torch.equal(dense[mine], act)
    print(f"mutations cone vs score_sequences active {name} {prec}: max|d| = {worst:.3e}, bits equal: {equal}")
    assert worst < 2e-4, worst
    # delta: the fp32 sum of the call's own terms
    out["w"] = cm
    err, rel = delta_bound(out)
    print(f"mutations delta vs the fp64 sum {name} {prec}: max |err| = {err:.3e}, max err / bound = {rel:.3f}")
    # the wild types
    offs = out["row_offsets"].cpu().numpy()
    wild = [v for v in range(n) if np.array_equal(c["S_full"][v], cx["S"])]
    assert len(wild) >= 2
    for v in wild:
        res = out["row_residue"][offs[v]:offs[v + 1]].long()
        d = float((out["row_token_log_prob"][offs[v]:offs[v + 1]] - out["base_token_log_probs"][res]).abs().max())
        assert d < 2e-4, (v, d)
        assert abs(float(out["delta_log_likelihood"][v])) < 2e-4 * (offs[v + 1] - offs[v])
    # the dense route of the call itself
    dn = m.score_mutations(fd, sites=sites, site_tokens=site_tokens, method="dense")
    assert dn["method"] == "dense" and dn["site_rows"] is None
    d = float((mutations_dense(dn, L).cpu() - ref).abs().max())
    dd = float((dn["delta_log_likelihood"] - out["delta_log_likelihood"]).abs().max())
    print(f"mutations parity {name} dense {prec}: max|d token_log_probs| = {d:.3e}; delta cone vs dense {dd:.3e}")
    assert d < 1e-3 and float((dn["loss"].cpu() - loss).abs().max()) < 1e-3
    assert dd < 2e-4 * L


def budget_for(site_index, rows, chunks):
    """The smallest item budget at which the cutter makes `chunks` chunks."""
    total = sum(int(sum(rows[s])) for s in site_index)
    for b in range(max(1, total // (chunks + 1)), total + 1):
        if len(mutation_chunks(site_index, rows, b)[1]) == chunks:
            return b
    raise AssertionError("no such budget")


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_chunks_and_company_do_not_change_a_variant(weights_np, prec):
    """n97, the variants given in an order that is NOT grouped by site: two calls give identical bits; the call cut into 3 chunks
    (score_library_tokens lowered) gives the bits of the one-chunk call, rows and deltas; every fourth variant alone gives its bits
    in the full call."""
    c, m, fd, sites, site_tokens = setup("n97", weights_np, prec)
    shuffle = torch.from_numpy(np.random.default_rng(2).permutation(len(site_tokens)))
    site_tokens = site_tokens[shuffle]
    keys = ("delta_log_likelihood", "loss", "row_offsets", "row_residue", "row_token_log_prob", "base_log_probs", "site_rows")
    one = m.score_mutations(fd, sites=sites, site_tokens=site_tokens, method="cone")
    again = m.score_mutations(fd, sites=sites, site_tokens=site_tokens, method="cone")
    assert one["chunks"] == 1 and all(torch.equal(one[k], again[k]) for k in keys)
    ordered = m.score_mutations(fd, sites=sites, site_tokens=torch.from_numpy(c["site_tokens"]), method="cone")
    assert torch.equal(ordered["delta_log_likelihood"][shuffle], one["delta_log_likelihood"])
    L = len(c["cx"]["S"])
    assert torch.equal(mutations_dense(ordered, L)[shuffle], mutations_dense(one, L))
    budget = budget_for(site_tokens[:, 0].tolist(), c["rows"].tolist(), 3)
    m.score_library_tokens = budget // 3
    assert 3 * m.score_library_tokens <= budget and len(mutation_chunks(site_tokens[:, 0].tolist(), c["rows"].tolist(), 3 * m.score_library_tokens)[1]) >= 3
    three = m.score_mutations(fd, sites=sites, site_tokens=site_tokens, method="cone")
    assert three["chunks"] >= 3, three["chunks"]
    assert all(torch.equal(one[k], three[k]) for k in keys)
    m.score_library_tokens = 65536
    offs = one["row_offsets"].cpu().numpy()
    for v in range(0, len(site_tokens), 4):
        alone = m.score_mutations(fd, sites=sites, site_tokens=site_tokens[v:v + 1], method="cone")
        assert torch.equal(alone["delta_log_likelihood"], one["delta_log_likelihood"][v:v + 1])
        assert torch.equal(alone["row_token_log_prob"], one["row_token_log_prob"][offs[v]:offs[v + 1]])
        assert torch.equal(alone["row_residue"], one["row_residue"][offs[v]:offs[v + 1]])


@pytest.mark.parametrize("method", ["auto", "cone", "dense"])
def test_zero_variants(weights_np, method):
    """No variants (the general form with an empty site_tokens, the scan form with empty positions): empty results, and
    base_log_probs equal to score()'s bits."""
    c, m, fd, sites, site_tokens = setup("n97", weights_np, "x3")
    sc = m.score(fd)
    for out in (m.score_mutations(fd, sites=sites, site_tokens=site_tokens[:0], method=method),
                m.score_mutations(fd, positions=torch.zeros(0, dtype=torch.long), method=method)):
        assert out["delta_log_likelihood"].shape == (0,) and out["loss"].shape == (0,) and out["row_residue"].shape == (0,)
        assert out["row_token_log_prob"].shape == (0,) and out["row_offsets"].tolist() == [0] and out["chunks"] == 0
        assert torch.equal(out["base_log_probs"], sc["log_probs"]) and torch.equal(out["decoding_order"], sc["decoding_order"])
        assert mutations_dense(out, len(c["cx"]["S"])).shape == (0, len(c["cx"]["S"]))
    assert out["delta"].shape == (0, 0)


def test_auto_takes_the_route_the_counts_ask_for(weights_np):
    """ "auto" is decided after the read-back: the cone where the mean of sum_l |U_l(site)| over the variants is at most 2 L (n97:
    the default scan of the designed nucleic acid), the dense route beyond (LltK with everything designed, the three first-decoded
    residues: every later residue is in their cones, about 3 L rows per variant).  A 4-layer model and the bf16 mode take the dense
    route without a plan and refuse "cone"."""
    dev = torch.device("cuda:0")
    c, m, fd, sites, site_tokens = setup("n97", weights_np, "x3")
    L = len(c["cx"]["S"])
    out = m.score_mutations(fd)
    rows = out["site_rows"].cpu().numpy()
    n = len(out["site_index"])
    assert out["method"] == "cone" and out["chunks"] == 1 and rows[out["site_index"].cpu().numpy()].sum() <= 2 * L * n
    assert out["delta"].shape == (len(out["positions"]), len(out["tokens"])) and n == int((~torch.isnan(out["delta"])).sum())
    forced = m.score_mutations(fd, method="cone")
    assert torch.equal(torch.isnan(forced["delta"]), torch.isnan(out["delta"])) and bool(torch.isnan(out["delta"]).any())
    assert torch.equal(torch.nan_to_num(forced["delta"]), torch.nan_to_num(out["delta"]))
    k, cx, pos, tok = LR.make_case("LltK")
    cx = dict(cx, chain_mask=np.ones_like(cx["chain_mask"]))
    fd2 = to_dev(cpu_fd(cx), dev)
    m2 = make_model(weights_np, k, dev)
    order = m2.order_and_rank(fd2["mask"], fd2["chain_mask"], fd2["randn"])[0][0].cpu().numpy()
    early = torch.tensor(sorted(int(i) for i in order[:3]))
    out2 = m2.score_mutations(fd2, positions=early)
    rows2 = out2["site_rows"].cpu().numpy()
    n2, L2 = len(out2["site_index"]), len(cx["S"])
    assert rows2[out2["site_index"].cpu().numpy()].sum() > 2 * L2 * n2
    assert out2["method"] == "dense" and out2["row_offsets"].tolist() == [v * L2 for v in range(n2 + 1)]
    cone2 = m2.score_mutations(fd2, positions=early, method="cone")
    assert cone2["method"] == "cone"
    assert float((torch.nan_to_num(cone2["delta"]) - torch.nan_to_num(out2["delta"])).abs().max()) < 2e-4 * L2
    m4 = make_model(synth.make_weights(0, 3, 4), k, dev, 4)
    with pytest.raises(NotImplementedError):
        m4.score_mutations(fd2, positions=early, method="cone")
    out4 = m4.score_mutations(fd2, positions=early)
    assert out4["method"] == "dense" and out4["site_rows"] is None and out4["delta"].shape == out2["delta"].shape
    m2.message_precision = "bf16"
    with pytest.raises(NotImplementedError):
        m2.score_mutations(fd2, positions=early, method="cone")
    assert m2.score_mutations(fd2, positions=early)["method"] == "dense"


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_cone_equals_dense_at_scale(weights_np, prec):
    """The cone against the dense route at (1000, 48), everything designed, 64 variants on 16 evenly spaced sites, where the oracle
    does not reach: < 2e-4 on every entry; the cones are a small part of the rows.  Measured (MI355X): x3 3.0e-5, fp32 2.9e-6 (delta:
    8.4e-4 / 1.3e-5 over up to 381 rows); mean rows per site [20.4, 53.7, 87.4]."""
    dev = torch.device("cuda:0")
    cx = synth.make_complex(seed=9048, n=1000, masked_frac=0.02)
    fd = to_dev(cpu_fd(cx), dev)
    pos = np.arange(30, 1000, 62)[:16]
    rng = np.random.default_rng(64)
    sites, site_tokens = MR.scan(cx["S"], pos, [rng.choice(list(MR.alphabet(cx, p)), 4, replace=False).tolist() for p in pos])
    assert len(site_tokens) == 64
    m = make_model(weights_np, 48, dev)
    m.message_precision = prec
    cone = m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(site_tokens), method="cone")
    dense = m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(site_tokens), method="dense")
    d = float((mutations_dense(cone, 1000) - mutations_dense(dense, 1000)).abs().max())
    dd = float((cone["delta_log_likelihood"] - dense["delta_log_likelihood"]).abs().max())
    rows = cone["site_rows"].cpu().numpy()
    print(f"mutations cone vs dense (1000, 48) {prec}: max|d| = {d:.3e}, max|d delta| = {dd:.3e}, mean rows per site {rows.mean(0).tolist()}")
    assert d < 2e-4, d
    E_idx = m.featurize(fd)[2][0].cpu().numpy()
    rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])[1][0].cpu().numpy()
    want, _ = MR.site_rows(E_idx, rank, cx["mask"], sites)
    assert np.array_equal(rows, want) and 0 < rows.sum(1).mean() < 3 * 1000 / 4
    assert m.score_mutations(fd, sites=torch.from_numpy(sites), site_tokens=torch.from_numpy(site_tokens))["method"] == "cone"


def test_pairs_equal_the_general_form(weights_np):
    """pairs=True on a 16-residue protein with a 2 x 12 RNA duplex: equal, bit for bit, to the general form with the explicit pair
    sites and complementary tokens; every variant is a canonical duplex."""
    dev = torch.device("cuda:0")
    cx = synth.make_complex(seed=41, n=40, n_chains=3, frac_protein=0.4, frac_dna=0.0)
    assert int(cx["rna_mask"].sum()) == 24
    pairs = [(16 + i, 39 - i) for i in range(12)]
    fd = to_dev(cpu_fd(cx), dev)
    fd["paired_residues"] = pairs
    fd["chain_mask"] = fd["rna_mask"].clone()
    m = make_model(weights_np, 24, dev)
    out = m.score_mutations(fd, pairs=True)
    assert out["sites"].cpu().tolist() == [list(p) for p in pairs] and out["delta"].shape == (12, 4) and not torch.isnan(out["delta"]).any()
    P = spec.token_map(spec.restype_to_int(), "same")
    rows = [[s, t, P[t]] for s in range(12) for t in range(26, 30)]
    assert out["site_tokens"].cpu().tolist() == rows
    gen = m.score_mutations({k: v for k, v in fd.items() if k != "paired_residues"}, sites=torch.tensor(pairs), site_tokens=torch.tensor(rows))
    for k in ("delta_log_likelihood", "loss", "row_offsets", "row_residue", "row_token_log_prob", "site_rows"):
        assert torch.equal(out[k], gen[k]), k
    assert torch.equal(out["delta"].reshape(-1), gen["delta_log_likelihood"])
    single = m.score_mutations(fd, pairs=False)                              # the ties are not read: 24 sites of one residue
    assert single["delta"].shape == (24, 4)


def test_cli_mutation_scan(tmp_path, golden_dir):
    """--mutation_scan 1 end to end on tests/golden/pdb: mutations/<name>.npz equals the Python call."""
    import lzma
    from na_mpnn_amd import cli, pdbio
    pdb = os.path.join(str(tmp_path), "1am9.pdb")
    with lzma.open(os.path.join(golden_dir, "pdb", "1am9.pdb.xz"), "rb") as fh, open(pdb, "wb") as out:
        out.write(fh.read())
    base = os.path.join(str(tmp_path), "out")
    cli.main(["--mode", "design", "--pdb_path", pdb, "--out_folder", base, "--random_init_seed", "0", "--seed", "7", "--design_na_only", "1",
              "--mutation_scan", "1"])
    z = np.load(os.path.join(base, "mutations", "1am9.npz"), allow_pickle=True)
    assert sorted(z.files) == sorted(["residues", "tokens", "delta", "base_loss", "wild_type_token", "site_rows"])
    P = pdbio.parse_pdb(pdb)
    L = len(P["S"])
    dev = torch.device("cuda:0")
    m = make_model(synth.make_weights(0), 32, dev)
    chain_mask = np.array([c in P["na_chain_letters"] for c in P["chain_letters"]], np.int32)      # --design_na_only 1
    fd = pdbio.to_feature_dict(P, chain_mask, dev)
    fd["batch_size"] = 1
    torch.manual_seed(7)
    fd["randn"] = torch.randn(1, L, device=dev)
    out = m.score_mutations(fd)
    n_pos = len(out["positions"])
    assert z["delta"].shape == (n_pos, len(out["tokens"])) and z["delta"].dtype == np.float32 and n_pos > 0
    assert np.array_equal(z["delta"], out["delta"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(z["site_rows"], out["site_rows"].cpu().numpy())
    assert float(z["base_loss"]) == float(out["base_loss"])
    assert np.array_equal(z["wild_type_token"], np.asarray(P["S"])[out["positions"].cpu().numpy()])
    assert len(z["residues"]) == n_pos and len(z["tokens"]) == len(out["tokens"])
    wt = z["delta"][np.arange(n_pos), [out["tokens"].tolist().index(int(t)) for t in z["wild_type_token"]]]
    assert np.abs(wt).max() < 2e-4 * L                                       # the wild-type column changes nothing
