"""GPU tests on real structures: every path of the product — featuriser, score / unconditional / conditional probabilities, the
sampler with its routes, base-paired design (canonical and wobble), multi-state design, a training step, the bf16 throughput mode — on
the two public PDB entries of tests/golden/pdb (1AM9: protein + two DNA duplexes, 8 chains, 4 masked 5' nucleotides; 4OQU: a 97-nt
RNA) and exact variants of them (tests/real_structures.py), against the CPU oracle in fp64, computed once per (variant, K).  The bars
are the suite's existing ones; tests/test_real_structures_host.py proves on the CPU that the oracle is a reference on these inputs and
asserts the caps of the two rules that leave rows out (near-tie arg-max, neighbour order)."""
import functools

import numpy as np
import pytest
import torch

import paired_ref
import real_structures as rs
import tied_states_ref
from loo_numpy import oracle_conditional
from na_mpnn_amd import hip, shard, spec, train
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref, cpu_ref_mixed
from test_gpu_paired import check_complement
from test_gpu_tied_states import check_against_oracle as check_tied_against_oracle
from test_gpu_wobble import check_against_oracle as check_wobble_against_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
TOL_LOGP, TOL_E = rs.TOL_LOGP, rs.TOL_E
PRECS = ["x3", "fp32"]
SINGLE_LAUNCH, TWO_PARTS = 11, 11 | 32              # namp_set_bf16p masks: the edge-feature launch whole / in two parts (bit 5)


def make_model(k, prec="x3", shared=False):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(shared),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict(rs.weights())
    m = m.to(DEV).eval()
    m.message_precision = prec
    return m


def maxdiff(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def check_log_probs(tag, logp, ref, valid, max_left_out=rs.MAX_LEFT_OUT):
    """The parity bars on log-probabilities: finite, rows normalised, within 1e-3 of the fp64 oracle on unmasked residues, arg-max
    identical wherever the oracle's top two are at least 2e-3 apart — a rule that may leave out at most 2 % of the unmasked residues
    (test_real_structures_host.py asserts that on the CPU for score and unconditional_probs)."""
    logp = logp.detach().cpu()
    assert torch.isfinite(logp).all(), tag
    assert float(torch.logsumexp(logp.double(), -1).abs().max()) < 1e-5, tag
    err = float((logp.double() - ref.double())[valid].abs().max())
    decided = rs.argmax_decided(ref, valid)
    print(f"REAL {tag}: max|dlogp| = {err:.2e}; arg-max compared on {int(decided.sum())} of {int(valid.sum())} unmasked residues")
    assert int(decided.sum()) >= (1 - max_left_out) * int(valid.sum()), tag
    assert err < TOL_LOGP, (tag, err)
    assert torch.equal(logp.argmax(-1)[decided], ref.argmax(-1)[decided]), tag
    return err


def check_neighbours(tag, E_idx, key, K):
    """E_idx [L, K] against the fp64 oracle's: in order on every unmasked row on which the fp32 and the fp64 oracle agree in order, as
    a set on the other unmasked rows.  Returns the permutation [L, K] that puts our columns into the oracle's order."""
    ref = rs.oracle(key, K)["E_idx"]
    valid = torch.from_numpy(rs.variant(key)["mask"].astype(bool))
    decided = rs.order_decided(key, K)
    idx = E_idx.cpu().long()
    assert idx.shape == ref.shape, tag
    assert int(decided.sum()) >= ((1 - rs.MAX_LEFT_OUT) if key.endswith("_shift") else 1) * int(valid.sum()), tag
    rest = valid & ~decided
    assert torch.equal(torch.sort(idx[rest], -1)[0], torch.sort(ref[rest], -1)[0]), tag
    wrong = (idx != ref).any(-1) & decided
    assert not bool(wrong.any()), (tag, "neighbour lists differ from the oracle's on rows", wrong.nonzero().view(-1).tolist()[:10])
    return torch.gather(idx.argsort(-1), 1, ref.argsort(-1).argsort(-1))


def check_edge_rows(tag, rows, perm, ref_rows, valid, tol=TOL_E):
    """rows [L, K, 128] (ours) against the oracle's on ALL unmasked residues, in chunks of 64 residues."""
    rows = rows.detach().cpu()
    worst = 0.0
    for i0 in range(0, rows.shape[0], 64):
        sl = slice(i0, i0 + 64)
        ours = torch.gather(rows[sl], 1, perm[sl][..., None].expand(-1, -1, rows.shape[-1])).double()
        assert torch.isfinite(ours).all(), tag
        d = (ours - ref_rows[sl].double()).abs().amax((-1, -2))[valid[sl]]
        worst = max(worst, float(d.max()) if d.numel() else 0.0)
    print(f"REAL {tag}: max|d| over all unmasked rows = {worst:.2e}")
    assert worst < tol, (tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# a. featuriser
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key,K", rs.ORACLE_CASES)
def test_featuriser(key, K, prec):
    """prep_atoms / knn_select / edge_features on real geometry (residues of exactly 4, 8, 11 or 12 atoms, bonded distances below the
    first RBF centre, coordinates to 213 A and to 1213 A): neighbour lists and E against the fp64 oracle, as one launch, in two parts
    with E alone and with h_E alone (the embedded rows against W_e E of the oracle).  4oqu runs one residue per workgroup."""
    cx = rs.variant(key)
    fd = rs.to_dev(rs.fd_cpu(cx), DEV)
    ref = rs.oracle(key, K)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    m = make_model(K, prec)
    L = hip.lib()
    prev = L.namp_set_bf16p(SINGLE_LAUNCH)
    try:
        _, E1, _, I1 = m._featurize_hip(fd, want_E=True, want_hE=False)
        E1, I1 = E1[0].clone(), I1[0].clone()
        L.namp_set_bf16p(TWO_PARTS)
        _, E2, _, I2 = m._featurize_hip(fd, want_E=True, want_hE=False)
        E2, I2 = E2[0].clone(), I2[0].clone()
        _, _, H2, I3 = m._featurize_hip(fd, want_E=False, want_hE=True)
        H2, I3 = H2[0].float().clone(), I3[0].clone()
    finally:
        L.namp_set_bf16p(prev)
    assert torch.equal(I1, I2) and torch.equal(I1, I3)
    tag = f"featuriser {key} K={K} {prec}"
    perm = check_neighbours(tag, I1, key, K)
    check_edge_rows(tag + " E, one launch", E1, perm, ref["E"], valid)
    check_edge_rows(tag + " E, two parts", E2, perm, ref["E"], valid)
    # h_E = W_e E + b: the activation bar, or twice the deviation of the reference's own fp32 evaluation from fp64 where that is larger
    # (1am9 + 1000 A: the virtual Cb / N_na atoms are rounded to 6e-5 A at |x| = 1000, E of the fp32 oracle sits at 1.98e-4 there)
    w64, w32 = rs.weights64(), rs.weights()
    hE_ref = torch.nn.functional.linear(ref["E"], w64["W_e.weight"], w64["W_e.bias"])
    hE_32 = torch.nn.functional.linear(rs.oracle(key, K, torch.float32)["E"], w32["W_e.weight"], w32["W_e.bias"])
    assert bool(rs.order_decided(key, K)[valid].all())                         # (the two oracles' rows are in the same order)
    own = float((hE_32.double() - hE_ref)[valid].abs().max())
    check_edge_rows(tag + f" h_E, two parts (the fp32 oracle: {own:.2e})", H2, perm, hE_ref, valid, tol=max(TOL_E, 2 * own))


@pytest.mark.parametrize("key,K", rs.ORACLE_CASES + (("1am9+duplex", 48),))
def test_knn_selection_equals_the_full_row_sort_on_real_structures(key, K, monkeypatch):
    """knn_select_kernel (radix select + small sort) against the bitonic sort of the whole row: bit-equal lists, masked rows included
    (neighbour gaps down to 2.4e-5 A; the masked 5' nucleotides tie with the row maximum).  "1am9+duplex": 1am9 padded next to its own
    duplex E + H alone (38 nt, 36 of them unmasked, fewer than K): every row of the duplex reaches past its farthest real residue into the
    masked and padded ones that tie with it at the row maximum, where the real residue must come first."""
    if key == "1am9+duplex":
        cxs = [rs.variant("1am9"), rs.crop(rs.variant("1am9"), rs.rows_of_chains("1am9", "EH"))]
        assert int(cxs[1]["mask"].sum()) == 36 < K
        fd = dict(shard.pad_batch(cxs, device=DEV), batch_size=1)
    else:
        fd = rs.to_dev(rs.fd_cpu(rs.variant(key)), DEV)
    m = make_model(K)
    monkeypatch.delenv("NAMP_KNN_FULL_SORT", raising=False)
    sel = m.featurize(fd)[2].clone()
    monkeypatch.setenv("NAMP_KNN_FULL_SORT", "1")
    full = m.featurize(fd)[2].clone()
    assert torch.equal(sel, full)


# ------------------------------------------------------------------------------------------------------------------------------------
# b. score, unconditional_probs, conditional_probs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key,K", rs.ORACLE_CASES)
def test_score_and_unconditional(key, K, prec):
    cx = rs.variant(key)
    fd = rs.to_dev(rs.fd_cpu(cx), DEV)
    ref = rs.oracle(key, K)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    m = make_model(K, prec)
    sc, un = m.score(fd), m.unconditional_probs(fd)
    assert torch.equal(sc["decoding_order"].cpu(), ref["decoding_order"])
    tag = f"{key} K={K} {prec}"
    check_log_probs(tag + " score", sc["log_probs"][0], ref["score"], valid)
    check_log_probs(tag + " unconditional", un["log_probs"][0], ref["unconditional"], valid)


@pytest.mark.parametrize("prec", PRECS)
def test_padded_batch_of_both_structures(prec):
    """[1am9, 4oqu] as one padded batch (389 and 97 residues, K = 48): every complex against its own oracle run — neighbour lists, E on
    all unmasked rows, score and unconditional log-probs, the decoding order of its residues."""
    K = 48
    cxs = [rs.variant("1am9"), rs.variant("4oqu")]
    fd = dict(shard.pad_batch(cxs, device=DEV), batch_size=1)
    m = make_model(K, prec)
    _, E, I = m.featurize(fd)
    sc, un = m.score(fd), m.unconditional_probs(fd)
    order = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])[0].cpu()
    for b, key in enumerate(("1am9", "4oqu")):
        n = cxs[b]["S"].shape[0]
        ref = rs.oracle(key, K)
        valid = torch.from_numpy(cxs[b]["mask"].astype(bool))
        tag = f"padded batch, {key} {prec}"
        assert int(I[b, :n].max()) < n
        perm = check_neighbours(tag, I[b, :n], key, K)
        check_edge_rows(tag + " E", E[b, :n], perm, ref["E"], valid)
        assert torch.equal(order[b][order[b] < n], ref["decoding_order"])
        check_log_probs(tag + " score", sc["log_probs"][b, :n], ref["score"], valid)
        check_log_probs(tag + " unconditional", un["log_probs"][b, :n], ref["unconditional"], valid)


CONDITIONAL_CASES = {"4oqu": 32, "1am9_crop": 48}


@functools.lru_cache(maxsize=None)
def conditional_oracle(key):
    fd = rs.fd_cpu(rs.variant(key))
    lp, order, _ = oracle_conditional(rs.weights(), fd, CONDITIONAL_CASES[key])
    return fd, lp, order


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("method", ["dense", "cone"])
@pytest.mark.parametrize("key", list(CONDITIONAL_CASES))
def test_conditional_probs(key, method, prec):
    """Leave-one-out conditionals, dense and cone, against the oracle's L-stream brute force on 4oqu and on the 118-residue crop of
    1am9 (chains E + H + A: a duplex with a masked 5' nucleotide, and the protein bound to it)."""
    fd_cpu, ref, order = conditional_oracle(key)
    m = make_model(CONDITIONAL_CASES[key], prec)
    out = m.conditional_probs(rs.to_dev(fd_cpu, DEV), method=method)
    assert torch.equal(out["decoding_order"].cpu(), order[0])
    if method == "cone":
        assert "cone_items" in out
    check_log_probs(f"conditional {key} {method} {prec}", out["log_probs"][0], ref[0], fd_cpu["mask"][0].bool(), max_left_out=0.05)   # test_gpu_conditional.py's cap


# ------------------------------------------------------------------------------------------------------------------------------------
# c. exact rotations
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("copies", [1, 2])
def test_rotated_images_in_one_batch(copies, prec):
    """The four images of 1am9 under the 180-degree rotations (exact in fp32: every distance keeps its bits) in ONE batch — B = 4 on
    the fused path, each image twice for B = 8 = 3,112 residues on the unfused one: identical neighbour lists, every image within 1e-3
    of the ONE oracle run of the unrotated structure, and the images bit-identical to each other (measured: they are)."""
    K = 48
    keys = [k for k in rs.ROTATIONS for _ in range(copies)]
    cxs = [rs.variant(k) for k in keys]
    n = cxs[0]["S"].shape[0]
    if copies == 2:
        assert len(keys) * n == 3112 > hip.lib().namp_fused_tail_max_residues()
    else:
        assert len(keys) * n <= hip.lib().namp_fused_tail_max_residues()
    fd = dict(shard.pad_batch(cxs, device=DEV), batch_size=1)
    ref = rs.oracle("1am9", K)
    valid = torch.from_numpy(cxs[0]["mask"].astype(bool))
    m = make_model(K, prec)
    _, E, I = m.featurize(fd)
    lp = m.score(fd)["log_probs"]
    tag = f"rotations B={len(keys)} {prec}"
    for b in range(1, len(keys)):
        assert torch.equal(I[b], I[0]), (tag, keys[b])
    perm = check_neighbours(tag, I[0], "1am9", K)
    check_edge_rows(tag + " E of image 0", E[0], perm, ref["E"], valid)
    for b, key in enumerate(keys):
        check_log_probs(f"{tag} image {b} ({key})", lp[b], ref["score"], valid)
    between = max(maxdiff(lp[b][valid], lp[0][valid]) for b in range(1, len(keys)))
    between_E = max(maxdiff(E[b][valid], E[0][valid]) for b in range(1, len(keys)))
    print(f"REAL {tag}: images among each other max|dlogp| = {between:.2e}, max|dE| = {between_E:.2e}")
    assert between < 1e-5, between
    assert between == 0.0 and between_E == 0.0, (between, between_E)


# ------------------------------------------------------------------------------------------------------------------------------------
# d. sampler
# ------------------------------------------------------------------------------------------------------------------------------------
def design_case(name):
    """(variant, K, streams, T, chain_mask): 1am9 with the DNA designed and the protein fixed, and the other way round (one stream: with
    masked AND fixed residues the reference masks every stream with stream 0's mask); 4oqu with every ninth residue fixed."""
    if name == "4oqu":
        cx = rs.variant("4oqu")
        cx["chain_mask"][::9] = 0
        return cx, 32, 2, 0.3
    cx = rs.variant("1am9")
    cx["chain_mask"] = (cx["dna_mask"] if name == "1am9_dna" else cx["protein_mask"]).astype(np.int32)
    return cx, 32, 1, 0.5


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["4oqu", "1am9_dna", "1am9_protein"])
def test_sampler_free_running(name, prec):
    """The checks of test_sample_free_running — (i) draws follow the returned distributions through the inverse CDF of the returned
    uniforms, (ii) fixed residues keep their tokens and no special token appears, (iii) score() on the sampled sequence reproduces the
    log_probs on designed residues, (iv) the oracle teacher-forced with the sampled sequence agrees within 1e-3 — with a real design
    mask; the persistent level walk, per-level launches and the sequential walk are bit-identical."""
    cx, K, bs, T = design_case(name)
    n = cx["S"].shape[0]
    fd_cpu = rs.sample_fd(cx, bs, T, seed=n + len(name))
    fd = rs.to_dev(fd_cpu, DEV)
    m = make_model(K, prec)
    outs = []
    for lvl, walk in ((True, True), (True, False), (False, False)):
        m.sample_level_parallel, m.sample_level_walk = lvl, walk
        torch.manual_seed(5)
        outs.append(m.sample(fd))
    out, per_level, seq = outs
    assert m.sample_walk_status() == 0
    assert int(out["levels"]) == per_level["levels"] < n and "levels" not in seq
    for o in (per_level, seq):
        for key in ("uniform", "decoding_order", "S", "sampling_probs", "log_probs"):
            assert torch.equal(out[key], o[key]), key
    S, P, U, order = out["S"].cpu(), out["sampling_probs"].cpu(), out["uniform"].cpu(), out["decoding_order"].cpu()
    assert torch.isfinite(P).all() and torch.isfinite(out["log_probs"]).all()
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    assert 0 < int(cm.sum()) < n
    assert torch.equal(S[:, ~cm], torch.from_numpy(cx["S"].astype(np.int64))[~cm].expand(bs, -1))
    for tok in cpu_ref.SPECIAL_TOKENS:
        assert not (S[:, cm] == tok).any()
    for b in range(bs):
        for t in range(n):
            i = int(order[b, t])
            if not cm[i]:
                continue
            cdf = torch.cumsum(P[b, i].double(), 0)
            u = float(U[b, t])
            expect = int((cdf > u).nonzero()[0]) if (cdf > u).any() else int(P[b, i].nonzero()[-1])
            if expect != int(S[b, i]):
                assert abs(float(cdf[min(expect, int(S[b, i]))]) - u) < 1e-5, (b, t, i)
    d_sc = 0.0
    for b in range(bs):
        fdb = dict(fd, batch_size=1, S=S[b:b + 1].to(DEV), randn=fd["randn"][b:b + 1])
        d_sc = max(d_sc, maxdiff(m.score(fdb)["log_probs"][0].cpu()[cm], out["log_probs"][b].cpu()[cm]))
    ref = cpu_ref.sample(rs.weights64(), cpu_ref.to_dtype(fd_cpu, rs.F64), K, S_forced=S)
    assert torch.equal(ref["decoding_order"], order)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp = maxdiff(out["log_probs"][:, valid], ref["log_probs"][:, valid])
    d_p = maxdiff(out["sampling_probs"][:, valid], ref["sampling_probs"][:, valid])
    print(f"REAL sampler {name} {prec}: oracle max|dlogp| = {d_lp:.2e}, max|dp| = {d_p:.2e}; score() max|dlogp| = {d_sc:.2e}; "
          f"{int(cm.sum())} of {n} residues designed in {int(out['levels'])} levels")
    assert d_sc < 2e-4, d_sc
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)


# ------------------------------------------------------------------------------------------------------------------------------------
# e. base-paired design
# ------------------------------------------------------------------------------------------------------------------------------------
def paired_case(name, bs=2, T=0.5, shared=True):
    """(cx, fd, pairs, K): 1am9 with its two duplexes (34 pairs; residues 0 and 38, first members of a pair each, are masked), the same
    with the four 5' nucleotides unmasked, or 4oqu with its 26 canonical stem pairs (one chain) under the shared DNA / RNA tokens.  As
    in paired_ref.make_case the bias keeps a nucleotide on the four bases of its polymer: synthetic weights know no chemistry."""
    key, pairs, K = {"1am9": ("1am9", rs.pairs_1am9(), 32), "1am9_missing": ("1am9_missing", rs.pairs_1am9(), 32),
                     "4oqu": ("4oqu", rs.stems_4oqu(), 32), "4oqu_legacy": ("4oqu_legacy", None, 32)}[name]
    cx = rs.variant(key)
    rti = spec.restype_to_int(shared)
    if pairs is None:                 # separate RNA tokens: the stacked pairs whose native tokens are a Watson-Crick or a G-U pair
        ok = set(spec.na_canonical_base_pair_ints(rti)) | {(rti["G"], rti["U"]), (rti["U"], rti["G"])}
        pairs = [(i, j) for i, j in rs.stems_4oqu(False) if (int(cx["S"][i]), int(cx["S"][j])) in ok]
    L = cx["S"].shape[0]
    bias = torch.zeros(1, L, 33)
    for i in range(L):
        if not cx["protein_mask"][i]:
            bias[0, i] = -1e8
            bias[0, i, [rti[n] for n in (("DA", "DC", "DG", "DT") if cx["dna_mask"][i] else ("A", "C", "G", "U"))]] = 0.0
    fd = rs.sample_fd(cx, bs, T, seed=L + 3, bias=bias)
    fd["paired_residues"] = [tuple(p) for p in pairs]
    return cx, fd, pairs, K


def apart(E_idx, pairs):
    """The pairs neither member of which lists the other among its neighbours (the sampler's split route decodes them as two items)."""
    E = E_idx.cpu().tolist()
    return [(i, j) for i, j in pairs if j not in E[i] and i not in E[j]]


def check_paired(name, m, cx, fd_cpu, K, out, rti):
    """test_gpu_paired.check_against_oracle for pairs that may hold a MASKED member: the complement holds and every pair is canonical;
    fixed residues keep S and have zero rows; no special token; the fp64 oracle teacher-forced with the sampled S agrees within 1e-3
    on log_probs and sampling_probs; every draw is the inverse CDF of the oracle's distribution at the call's uniform (a draw may
    differ only where u lies within 1e-5 of a boundary, at most once).  A masked member's decoder state is zeroed (dec_layer's
    mask_V), so its logits are W_out's bias whatever its neighbours are; paired_ref's oracle zeroes such a row, so the row is put in
    before the pair's distribution is recombined.  The parser gives such a nucleotide no polymer flag: the oracle's feature_dict flags
    it as DNA, which is what its token says (a masked residue's features reach no unmasked output)."""
    special = paired_ref.special_tokens(rti)
    L, bs = fd_cpu["S"].shape[1], fd_cpu["batch_size"]
    S, P, U, order, LP = (out[k].cpu() for k in ("S", "sampling_probs", "uniform", "decoding_order", "log_probs"))
    assert torch.isfinite(LP).all() and torch.isfinite(P).all() and m.sample_walk_status() == 0
    cm = torch.from_numpy((cx["mask"] * cx["chain_mask"]).astype(bool))
    assert torch.equal(S[:, ~cm], torch.from_numpy(cx["S"].astype(np.int64))[~cm].expand(bs, -1))
    for tok in special:
        assert not (S[:, cm] == tok).any()
    assert (LP[:, ~cm] == 0).all() and (P[:, ~cm] == 0).all()
    w64 = rs.weights64()
    fd_o = cpu_ref.to_dtype(fd_cpu, rs.F64)
    masked_members = [int(r) for p in fd_cpu["paired_residues"] for r in p if not cx["mask"][r]]
    if masked_members:                                                        # (paired_ref reads a member's polymer from dna_mask / rna_mask)
        fd_o["dna_mask"] = fd_cpu["dna_mask"].clone()
        fd_o["dna_mask"][0, masked_members] = 1
    lp_ref, p_ref, order_ref, (groups, weights, maps), lp_g = paired_ref.oracle_paired(w64, fd_o, K, S, rti, special)
    if masked_members:
        lp_g = lp_g.clone()
        lp_g[:, masked_members] = torch.log_softmax(w64["W_out.bias"], -1)
        p_ref = paired_ref.paired_probs(lp_g, fd_cpu, groups, weights, maps, special)
    check_complement(S, fd_cpu, groups, maps, rti)                            # (canonical-pair accuracy 1 on the paired positions)
    assert torch.equal(order_ref, order)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    d_lp, d_p = maxdiff(LP[:, valid], lp_ref[:, valid]), maxdiff(P[:, valid], p_ref[:, valid])
    rank = torch.empty(L, dtype=torch.int64); rank[order[0]] = torch.arange(L)
    in_group = {i: (g, gm) for g, gm in zip(groups, maps) for i in g}
    margin, off, n = 1.0, 0, 0
    for i in range(L):
        g, gm = in_group.get(i, ([i], [list(range(33))]))
        if i != g[-1] or not all(bool(cm[j]) for j in g):
            continue                                                          # (a fixed member decides the group's token, not the draw)
        Pc = torch.tensor(gm[-1])
        for b in range(bs):
            pr = p_ref[b, i][Pc].double()
            cdf = torch.cumsum(pr, 0)
            u = float(U[b, int(rank[i])])                                     # the closing visit reads the uniform
            pos = pr > 0
            a = int((pos & (cdf > u)).nonzero()[0]) if (pos & (cdf > u)).any() else int(pos.nonzero()[-1])
            dist = float((cdf[pos] - u).abs().min())
            margin, n = min(margin, dist), n + 1
            if int(Pc[a]) != int(S[b, i]):
                off += 1
                assert dist < 1e-5, (b, i, dist)
    print(f"REAL paired {name}: {len(groups)} pairs ({len(masked_members)} masked members), oracle max|dlogp| = {d_lp:.2e}, max|dp| = {d_p:.2e}; "
          f"{n} draws, min |cdf - u| = {margin:.2e}, off the oracle's: {off}; levels {int(out['levels'])}, work items {out['work_items']}")
    assert off <= 1
    assert d_lp < 1e-3 and d_p < 1e-3, (d_lp, d_p)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["1am9", "4oqu"])
def test_paired_design(name, prec):
    """Free-running base-paired design (device plan) on real duplexes: 1am9's two (inter-chain pairs, unequal strands, one masked member
    each) and the stems of 4oqu (pairs inside one chain, shared tokens).  2 / T <= 4 keeps the sampler's 1e-3 bar on a pair's sum."""
    cx, fd_cpu, pairs, K = paired_case(name)
    bs, L = fd_cpu["batch_size"], cx["S"].shape[0]
    m = make_model(K, prec, shared=True)
    torch.manual_seed(5)
    out = m.sample(rs.to_dev(fd_cpu, DEV))
    assert out["work_items"] == bs * (L - len(pairs))
    check_paired(f"{name} {prec}", m, cx, fd_cpu, K, out, spec.restype_to_int(True))
    S = out["S"].cpu()
    assert all(rs.is_canonical(S[b, i], S[b, j]) for i, j in pairs for b in range(bs))


@pytest.mark.parametrize("name", ["1am9", "4oqu"])
def test_fixed_strand_forces_the_complement_on_real_duplexes(name):
    """chain_mask 0 on the member listed second in every pair (1am9: strands H and F): every partner holds the complement of the
    native token in all streams — the native one, the duplexes being complementary."""
    cx, fd_cpu, pairs, K = paired_case(name)
    for _, j in pairs:
        cx["chain_mask"][j] = 0
    fd_cpu["chain_mask"] = torch.from_numpy(cx["chain_mask"])[None]
    rti = spec.restype_to_int(True)
    m = make_model(K, shared=True)
    torch.manual_seed(8)
    out = m.sample(rs.to_dev(fd_cpu, DEV))
    S, P = out["S"].cpu(), out["sampling_probs"].cpu()
    S_true = torch.from_numpy(cx["S"].astype(np.int64))
    for i, j in pairs:
        comp = spec.token_map(rti, "same")[int(S_true[j])]
        assert comp == int(S_true[i]) and (S[:, j] == S_true[j]).all() and (S[:, i] == comp).all(), (i, j)
        assert (P[:, j] == 0).all()
        if cx["mask"][i]:
            assert float(P[:, i].sum(-1).min()) > 0.999
    check_paired(f"{name}, one strand fixed", m, cx, fd_cpu, K, out, rti)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["1am9", "1am9_missing", "4oqu"])
def test_paired_routes_on_real_duplexes(name, prec):
    """The sequential walk, per-level launches, the persistent walk with split groups on and off (host route) and the device plan give
    bit-identical results under the same uniforms, and the device plan's arrays equal the host route's.  Real partners are graph
    neighbours, so the split route keeps every pair ONE work item — all 34 once the 5' nucleotides are unmasked and all 26 stems; on
    1am9 as parsed, a masked residue lists arbitrary neighbours and is listed by nobody: the count follows the device's own lists."""
    cx, fd_cpu, pairs, K = paired_case(name)
    bs, L = fd_cpu["batch_size"], cx["S"].shape[0]
    fd = rs.to_dev(fd_cpu, DEV)
    m = make_model(K, prec, shared=True)
    split = apart(m.featurize(fd)[2][0], pairs)
    if name != "1am9":
        assert split == []
    assert all(not (cx["mask"][i] and cx["mask"][j]) for i, j in split)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(3)).to(DEV)
    outs, plans = {}, {}
    routes = {"sequential": (False, True, True, False), "per_level": (True, False, True, False), "host_split": (True, True, True, False),
              "host_whole": (True, True, False, False), "device": (True, True, True, True)}
    for route, (par, walk, sp, plan) in routes.items():
        m.sample_level_parallel, m.sample_split_groups, m.sample_pairs_device_plan = par, sp, plan
        plans[route] = {}
        outs[route] = m._sample(fd, walk, uniform=u, plan_out=plans[route])
        if par and walk:
            assert m.sample_walk_status() == 0
    ref = outs["sequential"]
    assert torch.isfinite(ref["log_probs"]).all()
    for route, o in outs.items():
        for key in ("decoding_order", "S", "sampling_probs", "log_probs"):
            assert torch.equal(o[key], ref[key]), (route, key)
    assert outs["device"]["work_items"] == outs["host_whole"]["work_items"] == bs * (L - len(pairs))
    assert outs["host_split"]["work_items"] == bs * (L - len(pairs) + len(split))
    assert int(outs["device"]["levels"]) == int(outs["host_whole"]["levels"]) == int(outs["per_level"]["levels"])
    for k, v in plans["host_whole"].items():
        assert torch.equal(torch.as_tensor(v).cpu().to(torch.float64), torch.as_tensor(plans["device"][k]).cpu().to(torch.float64)), k


@pytest.mark.parametrize("name", ["1am9", "1am9_missing", "4oqu"])
def test_pairs_plan_on_real_duplexes(name):
    """namp_pairs_plan + namp_sample_levels_dep + namp_pairs_work_lists on the device's own neighbour lists of a real duplex against the
    host route's building blocks (symmetry_visits, level_work_lists), array for array, as test_pairs_plan_equals_the_host_route does on
    random lists: here the members of a pair ARE neighbours, every pair is one work item of two visits, and the split route of the
    host agrees (no closing list entry outside the pairs with a masked member)."""
    from na_mpnn_amd.model import level_work_lists, symmetry_visits
    cx, fd_cpu, pairs, K = paired_case(name)
    bs, L = fd_cpu["batch_size"], cx["S"].shape[0]
    fd = rs.to_dev(fd_cpu, DEV)
    m = make_model(K, shared=True)
    E_d = m.featurize(fd)[2][0].to(torch.int32).contiguous()
    Kk = E_d.shape[-1]
    o_all, r_all = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"][:1])
    o_d, r_d = o_all[0].to(torch.int32).contiguous(), r_all[0].to(torch.int32).contiguous()
    partner, first = np.full(L, -1, np.int32), np.zeros(L, np.int32)
    for i, j in pairs:
        partner[i], partner[j], first[i] = j, i, 1
    p_d, f_d = torch.from_numpy(partner).to(DEV), torch.from_numpy(first).to(DEV)
    i32e = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    order, rank, gf, gl, level = (i32e(bs, L) for _ in range(5))
    work, work_n, level_off, n_levels = i32e(bs * L, 2), i32e(bs * L), i32e(L + 2), i32e(1)
    Lb, st = hip.lib(), hip.current_stream()
    hip.check(Lb.namp_pairs_plan(p_d.data_ptr(), f_d.data_ptr(), o_d.data_ptr(), r_d.data_ptr(), order.data_ptr(), rank.data_ptr(),
                                 gf.data_ptr(), gl.data_ptr(), bs, L, st), "pairs_plan")
    hip.check(Lb.namp_sample_levels_dep(E_d.data_ptr(), order.data_ptr(), rank.data_ptr(), None, 0, gf.data_ptr(), gl.data_ptr(),
                                        level.data_ptr(), bs, 1, L, Kk, st), "sample_levels")
    hip.check(Lb.namp_pairs_work_lists(level.data_ptr(), gf.data_ptr(), work.data_ptr(), work_n.data_ptr(), level_off.data_ptr(),
                                       n_levels.data_ptr(), bs, L, st), "pairs_work_lists")
    visits, gf_h, gl_h, _ = symmetry_visits([list(p) for p in pairs], [[1.0, 1.0]] * len(pairs), o_d.tolist(), L)
    order_h = torch.tensor(visits, dtype=torch.int32, device=DEV).repeat(bs, 1)
    gf_t = torch.tensor(gf_h, dtype=torch.int32, device=DEV).repeat(bs, 1).contiguous()
    gl_t = torch.tensor(gl_h, dtype=torch.int32, device=DEV).repeat(bs, 1).contiguous()
    rank_h = ProteinMPNN.ranks_of(order_h.long()).to(torch.int32).contiguous()
    assert torch.equal(order, order_h) and torch.equal(rank, rank_h) and torch.equal(gf, gf_t) and torch.equal(gl, gl_t)
    n = bs * (L - len(pairs))
    sel, flat, wn_h, close_h, _ = level_work_lists(level, gf_t, gl_t, order_h[0], E_d.long(), split=False)
    assert close_h is None and sel.numel() == n
    assert torch.equal(work[:n], torch.stack((sel // L, sel % L), 1).to(torch.int32)) and torch.equal(work_n[:n], wn_h.to(torch.int32))
    assert int((work_n[:n] == 2).sum()) == bs * len(pairs) and int((work_n[:n] == 1).sum()) == n - bs * len(pairs)
    assert (work[n:] == -7).all() and (work_n[n:] == -7).all()                 # nothing written past the items
    hist = torch.zeros(L + 1, dtype=torch.int64, device=DEV).scatter_add_(0, flat, torch.ones_like(flat))
    assert torch.equal(level_off, torch.cat((hist.new_zeros(1), hist.cumsum(0))).to(torch.int32))
    assert int(n_levels) == int((hist > 0).sum())
    sel_s, _, wn_s, _, _ = level_work_lists(level, gf_t, gl_t, order_h[0], E_d.long(), split=True)
    n_apart = len(apart(E_d, pairs))
    assert sel_s.numel() == n + bs * n_apart and (n_apart == 0 or name == "1am9")
    if n_apart == 0:
        assert torch.equal(sel_s, sel) and torch.equal(wn_s, wn_h)


@pytest.mark.parametrize("prec", PRECS)
def test_wobble_design_on_the_4oqu_stems(weights_np, prec):
    """4oqu parsed with separate RNA tokens, its stacked pairs whose native tokens are Watson-Crick or G-U, paired_wobble on: the
    checks of test_gpu_wobble.py against wobble_ref.oracle_wobble."""
    cx, fd_cpu, pairs, K = paired_case("4oqu_legacy", bs=2, T=0.5, shared=False)
    assert len(pairs) >= 26 and int(cx["S"].min()) >= 26
    fd_cpu.update(paired_wobble=True, paired_wobble_bias=1.0)
    m = make_model(K, prec, shared=False)
    torch.manual_seed(5)
    out = m.sample(rs.to_dev(fd_cpu, DEV))
    assert out["work_items"] == 2 * (cx["S"].shape[0] - len(pairs))
    n_w, n_c = check_wobble_against_oracle(m, weights_np, cx, fd_cpu, K, out, shared=False)
    assert n_w >= 1 and n_c >= 1, (n_w, n_c)


# ------------------------------------------------------------------------------------------------------------------------------------
# f. multi-state design
# ------------------------------------------------------------------------------------------------------------------------------------
STATE_CASES = {"4oqu": (3, 32, 2, 0.5, (0.5, 0.3, 0.2)), "1am9_crop": (2, 48, 1, 1.0, (0.6, 0.4))}     # M, K, streams, T, state weights


def states_case(key):
    M, K, bs, T, sw = STATE_CASES[key]
    cx = rs.variant(key)
    cx["chain_mask"][::9] = 0
    L = cx["S"].shape[0]
    assert sum(abs(v) for v in sw) / T <= 4.0
    randn = np.random.default_rng(L + M).standard_normal((bs, L)).astype(np.float32)
    return cx, tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, M, seed=L + 7 * M), sw, bs, T, randn), K


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", list(STATE_CASES))
def test_multi_state_design(weights_np, key, prec):
    """One sequence over M deformed states of a real structure (tied_states_ref.make_states) against the per-state oracle, the checks
    of test_gpu_tied_states.py; the device plan, the host routes and the per-level launches are bit-identical."""
    cx, fd_cpu, K = states_case(key)
    M, L = fd_cpu["X"].shape[:2]
    bs = fd_cpu["batch_size"]
    fd = rs.to_dev(fd_cpu, DEV)
    m = make_model(K, prec)
    outs = {}
    for name, (plan, split, walk) in {"device": (True, True, True), "host_split": (False, True, True), "host_whole": (False, False, True),
                                      "per_level": (False, True, False)}.items():
        m.sample_states_device_plan, m.sample_split_groups, m.sample_level_walk = plan, split, walk
        torch.manual_seed(21)
        outs[name] = m.sample(fd)
        if walk:
            assert m.sample_walk_status() == 0
    ref = outs["per_level"]
    for name, o in outs.items():
        for k in ("uniform", "decoding_order", "S", "sampling_probs", "log_probs"):
            assert torch.equal(o[k], ref[k]), (name, k)
        assert int(o["levels"]) == int(ref["levels"]) < L, name
    assert outs["device"]["work_items"] == outs["host_split"]["work_items"] == bs * M * L
    assert outs["host_whole"]["work_items"] == bs * L
    m.sample_states_device_plan, m.sample_split_groups, m.sample_level_walk = True, True, True
    check_tied_against_oracle(m, weights_np, cx, fd_cpu, K, outs["device"])


# ------------------------------------------------------------------------------------------------------------------------------------
# g. training step
# ------------------------------------------------------------------------------------------------------------------------------------
TRAIN_K = 24


@functools.lru_cache(maxsize=None)
def train_case():
    """The padded batch [4oqu, 1am9 crop] (97 + 118 residues, two of them masked) and its decoding-order noise."""
    fd = shard.pad_batch([rs.variant("4oqu"), rs.variant("1am9_crop")])
    fd["S"] = fd["S"].long()
    return fd, torch.randn(2, 118, generator=torch.Generator().manual_seed(TRAIN_K))


def train_step_on_device(prec, monkeypatch):
    monkeypatch.setattr(train, "X3", train.X3)               # forward_train sets the module's precision code: put it back for later tests
    fd, randn = train_case()
    rti = spec.restype_to_int()
    m = make_model(TRAIN_K, prec).train()
    rm, rn = train.polymer_restype_tables(rti, 33, DEV)
    no_loss = torch.tensor([rti[t] for t in cpu_ref.NO_LOSS_TOKENS], device=DEV)
    opt = train.get_std_opt(m.parameters(), 128, 0)
    with torch.enable_grad():
        loss, _ = train.train_step(m, opt, {k: v.to(DEV) for k, v in fd.items()}, rm, rn, no_loss, decoding_randn=randn.to(DEV))
    return float(loss), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def train_oracle(mixed):
    fd, randn = train_case()
    with torch.enable_grad():
        if mixed:
            return cpu_ref_mixed.train_loss_and_grads(rs.weights(), fd, TRAIN_K, randn, spec.restype_to_int())
        return cpu_ref.train_loss_and_grads(rs.weights64(), cpu_ref.to_dtype(fd, rs.F64), TRAIN_K, randn, spec.restype_to_int())


@pytest.mark.parametrize("prec", PRECS)
def test_training_step(prec, monkeypatch):
    """train.train_step on [4oqu, 1am9 crop], K = 24, against cpu_ref.train_loss_and_grads in fp64, the bars of
    test_training_gradients_odd_shapes: loss 1e-5 relative, every parameter gradient within 2e-4 of its tensor's max."""
    loss_ref, _, g_ref = train_oracle(False)
    loss, grads = train_step_on_device(prec, monkeypatch)
    worst = ("", 0.0)
    for key, gr in grads.items():
        assert torch.isfinite(gr).all(), key
        scale = float(g_ref[key].abs().max())
        if scale >= 1e-12:
            worst = max(worst, (key, float((gr - g_ref[key]).abs().max()) / scale), key=lambda x: x[1])
    print(f"REAL train {prec}: loss {abs(loss - float(loss_ref)) / abs(float(loss_ref)):.1e} relative, worst gradient {worst[1]:.2e} of its "
          f"tensor's max ({worst[0]})")
    assert abs(loss - float(loss_ref)) <= 1e-5 * max(1e-3, abs(float(loss_ref)))
    for key, gr in grads.items():
        scale = float(g_ref[key].abs().max())
        if scale < 1e-12:
            assert float(gr.abs().max()) < 1e-9, key
        else:
            assert float((gr - g_ref[key]).abs().max()) / scale < 2e-4, (key, float((gr - g_ref[key]).abs().max()) / scale)


def test_training_step_mixed_precision(monkeypatch):
    """message_precision "bf16" on the same batch against the CPU emulation of its rounding points (oracle/cpu_ref_mixed.py), the bars
    of test_mixed_precision_training_mode: loss within 0.2 %, every gradient within 2 % of the emulation's (relative to its norm)."""
    l_em, _, g_em = train_oracle(True)
    loss, grads = train_step_on_device("bf16", monkeypatch)
    gnorm = float(torch.cat([g.double().flatten() for g in g_em.values()]).norm())
    worst = ("", 0.0)
    for key, gb in grads.items():
        assert torch.isfinite(gb).all(), key
        ge = g_em[key].double()
        if float(ge.norm()) > 1e-6 * gnorm:
            worst = max(worst, (key, float((gb - ge).norm() / ge.norm())), key=lambda x: x[1])
    print(f"REAL train bf16 vs the CPU emulation: loss {loss:.6f} / {float(l_em):.6f}, worst gradient {worst[0]} {worst[1]:.4f}")
    assert abs(loss - float(l_em)) < 2e-3 * abs(float(l_em)), (loss, float(l_em))
    assert worst[1] < 0.02, worst


# ------------------------------------------------------------------------------------------------------------------------------------
# h. bf16 throughput mode
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [0, 2])
def test_bf16_throughput_mode_on_real_structures(copies):
    """message_precision "bf16" through score() on 1am9 alone and on the B = 8 batch of its rotated images (unfused path) against exact
    fp32 on the device, the bars of test_bf16_throughput_mode: log-probs within 0.15, arg-max agreement at least 97 %."""
    cxs = [rs.variant(k) for k in rs.ROTATIONS for _ in range(copies)] or [rs.variant("1am9")]
    fd = dict(shard.pad_batch(cxs, device=DEV), batch_size=1)
    valid = fd["mask"].bool()
    lp = {}
    for prec in ("fp32", "bf16"):
        lp[prec] = make_model(48, prec).score(fd)["log_probs"]
    assert torch.isfinite(lp["bf16"]).all()
    assert float(torch.logsumexp(lp["bf16"].double(), -1).abs().max()) < 1e-5
    err = maxdiff(lp["bf16"][valid], lp["fp32"][valid])
    agree = float((lp["bf16"].argmax(-1) == lp["fp32"].argmax(-1))[valid].float().mean())
    print(f"REAL bf16 mode B={len(cxs)}: max|dlogp| vs exact fp32 = {err:.4f}, arg-max agreement = {agree:.4f}")
    assert err < 0.15 and agree >= 0.97, (err, agree)
