"""CPU facts behind test_gpu_real_structures.py: what the two real structures of tests/golden/pdb look like (atoms per residue,
coordinate range, chains, base pairs), that their exact variants are exact, and that the CPU oracle is a reference on them — its own
fp32 evaluation sits within a tenth of the parity bar of its fp64 evaluation, with the same neighbour lists — so that a failure of the
GPU tests means the kernels.  Every cap the GPU tests rely on (near ties, neighbour order) is asserted here."""
import collections

import numpy as np
import pytest
import torch

import real_structures as rs
from na_mpnn_amd import spec
from oracle import cpu_ref

F32 = torch.float32


def test_fixture_facts():
    a, r = rs.load("1am9"), rs.load("4oqu")
    la = rs.chain_letters("1am9")
    assert len(a["S"]) == 389 and list(dict.fromkeys(la)) == list("EFGHABCD")            # the DNA chains come first
    assert [la.count(c) for c in "EFGH"] == [17, 21, 17, 21] and int(a["protein_mask"].sum()) == 313      # unequal strands: overhangs
    assert np.where(a["mask"] == 0)[0].tolist() == [0, 17, 38, 55]                       # the four 5' nucleotides without a phosphate
    assert collections.Counter(a["X_m"].sum(1).tolist()) == {4: 313, 11: 72, 8: 4}
    assert (a["X_m"].sum(1)[a["mask"] == 0] == 8).all() and np.abs(a["X"][a["mask"] == 0]).max() > 1.0    # masked, but with coordinates
    assert 200.0 < float(np.abs(a["X"]).max()) < 250.0                                   # synth.make_complex stays within ~30 A
    assert a["R_idx"][:76].tolist() == list(range(1, 77)) and a["R_idx"][76] == 319 and a["R_idx"].max() == 400
    assert len(r["S"]) == 97 and set(rs.chain_letters("4oqu")) == {"A"} and int(r["mask"].sum()) == 97
    assert collections.Counter(r["X_m"].sum(1).tolist()) == {12: 97}
    m = rs.load("1am9", load_residues_with_missing_atoms=True)
    assert int(m["mask"].sum()) == 389 and np.array_equal(m["X"], a["X"]) and np.array_equal(m["S"], a["S"])
    c = rs.variant("1am9_crop")
    assert len(c["S"]) == 118 and int(c["protein_mask"].sum()) == 80 and int((c["mask"] == 0).sum()) == 2
    # bonded atoms sit below the first RBF centre (2 A)
    d = np.linalg.norm(r["X"][:, spec.ATOM_TYPES.index("P")] - r["X"][:, spec.ATOM_TYPES.index("OP1")], axis=-1)
    assert 1.2 < d.min() and d.max() < 1.7
    # the helper's dict is what synth.make_complex returns
    from na_mpnn_amd import synth
    s = synth.make_complex(seed=1, n=5)
    assert set(a) == set(s) and all(a[k].dtype == s[k].dtype for k in s), {k: (a[k].dtype, s[k].dtype) for k in s}


def neighbour_lists(cx, K):
    fd = rs.fd_cpu(cx)
    X = fd["X"].double()
    return cpu_ref.knn(X[:, :, 1] + X[:, :, rs.C1P], fd["mask"], K)[1][0].tolist()


def test_pair_lists():
    a, r = rs.load("1am9"), rs.load("4oqu")
    pairs = rs.pairs_1am9()
    assert len(pairs) == 34 and len({i for p in pairs for i in p}) == 68
    la = rs.chain_letters("1am9")
    assert {(la[i], la[j]) for i, j in pairs} == {("E", "H"), ("G", "F")}
    assert all(9.7 < rs.c1_distance(a, i, j) < 10.9 for i, j in pairs)
    assert all(rs.is_canonical(a["S"][i], a["S"][j]) for i, j in pairs)                  # native tokens complementary 17 / 17
    assert [(i, j) for i, j in pairs if not (a["mask"][i] and a["mask"][j])] == [(0, 75), (38, 37)]      # one masked member per duplex
    stems, canon = rs.stems_4oqu(False), rs.stems_4oqu()
    assert len(stems) == 31 and len(canon) == 26 and len({i for p in stems for i in p}) == 62
    assert all(j - i >= 4 and 9.8 <= rs.c1_distance(r, i, j) <= 11.2 for i, j in stems)
    assert all(rs.is_canonical(r["S"][i], r["S"][j]) for i, j in canon)
    # real partners are graph neighbours (on the synthetic duplexes of test_gpu_paired.py most are not), in the sense the sampler's plan
    # uses: one member lists the other.  A masked residue has no neighbour list of its own and is in nobody else's, so the two pairs
    # with a masked member count on the variant that unmasks them.
    am = rs.load("1am9", load_residues_with_missing_atoms=True)
    near = lambda E, prs: sum(j in E[i] or i in E[j] for i, j in prs)
    for K in (16, 32, 48):
        assert near(neighbour_lists(am, K), pairs) == 34, K
        assert near(neighbour_lists(a, K), pairs) == 32, K
        E = neighbour_lists(r, K)
        assert all(j in E[i] and i in E[j] for i, j in canon), K


def test_a_masked_pair_member_takes_its_partners_polymer_type():
    """1am9 as parsed: residues 0 and 38 (5' nucleotides without a phosphate) are masked and carry no polymer flag.  The plan of a
    base-paired design accepts them — fixed members, listed first, under the map of their partner's polymer type —, and still refuses
    a protein residue, masked or not."""
    from na_mpnn_amd.model import ProteinMPNN
    a = rs.load("1am9")
    assert not a["dna_mask"][[0, 38]].any() and not a["rna_mask"][[0, 38]].any() and not a["protein_mask"][[0, 38]].any()
    L = len(a["S"])
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=8, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(True),
                    polytype_to_int=spec.polytype_to_int())
    fd = rs.fd_cpu(a, paired_residues=[tuple(p) for p in rs.pairs_1am9()])
    groups, weights, table, idx, pair_list, bias = m._mapped_arguments(fd, 1, L)
    assert bias is None and len(pair_list) == 34 and len(table) == 2
    assert [p[:2] for p in pair_list if not (a["mask"][p[0]] and a["mask"][p[1]])] == [(0, 75), (38, 37)]
    assert all(kind == "same" for *_, kind in pair_list) and idx[75] == idx[37] == 1
    prot = int(np.where(a["protein_mask"] == 1)[0][0])
    for masked in (1, 0):
        b = {k: v.copy() for k, v in a.items()}
        b["mask"][prot] = masked
        with pytest.raises(ValueError, match=f"residue {prot} is not a nucleic acid"):
            m._mapped_arguments(rs.fd_cpu(b, paired_residues=[(prot, 75)]), 1, L)


def test_exact_variants():
    a = rs.load("1am9")
    present = a["X_m"].astype(bool)
    s = rs.shifted(a)
    assert np.array_equal(s["X"][~present], np.zeros_like(s["X"][~present])) and float(s["X"][present].min()) > 700.0
    assert float(np.abs(s["X"]).max()) < 9999.0                                          # PDB-legal (%8.3f)
    assert np.abs((s["X"] - a["X"])[present] - 1000.0).max() < 1e-4
    P = a["X"].reshape(-1, 3)[present.reshape(-1)]
    d2 = ((P[:, None, :] - P[None, ::7, :]) ** 2)                                        # fp32, as the featuriser forms them
    for axis in "xyz":
        q = rs.rot180(a, axis)
        assert np.array_equal(np.abs(q["X"]), np.abs(a["X"])) and int((np.sign(q["X"]) != np.sign(a["X"])).any(-1).sum()) > 0
        Q = q["X"].reshape(-1, 3)[present.reshape(-1)]
        e2 = ((Q[:, None, :] - Q[None, ::7, :]) ** 2)
        assert np.array_equal(e2, d2) and np.array_equal(np.sqrt(e2.sum(-1) + np.float32(1e-6)), np.sqrt(d2.sum(-1) + np.float32(1e-6)))
        assert np.array_equal(rs.rot180(q, axis)["X"], a["X"])
    fd, fq = rs.fd_cpu(a), rs.fd_cpu(rs.rot180(a, "y"))
    D = lambda f: cpu_ref.knn(f["X"][:, :, 1] + f["X"][:, :, rs.C1P], f["mask"], 48)[0]
    assert torch.equal(D(fd), D(fq))                                                     # the reference's own fp32 neighbour distances


@pytest.mark.parametrize("key,K", rs.ORACLE_CASES)
def test_reference_precision_and_caps(key, K):
    """The oracle in fp32 against fp64: identical neighbour sets on every unmasked row, log-probs within a tenth of the parity bar
    (measured 3.4e-6 on 1am9, 2.8e-6 on 4oqu, 1.3e-5 on 1am9 + 1000 A); the arg-max rule (fp64 top two at least 2e-3 apart) leaves out
    at most 2 % of the unmasked residues (measured: score 3, unconditional 6 of 385 on 1am9, 7 of 389 with the 5' nucleotides, 0 of 97
    on 4oqu); the neighbour-order rule leaves out no row on the unshifted structures and at most 2 % on the shifted one (measured 0)."""
    o64, o32 = rs.oracle(key, K), rs.oracle(key, K, F32)
    cx = rs.variant(key)
    valid = torch.from_numpy(cx["mask"].astype(bool))
    n = int(valid.sum())
    assert torch.equal(torch.sort(o64["E_idx"], -1)[0][valid], torch.sort(o32["E_idx"], -1)[0][valid])
    assert torch.equal(o64["decoding_order"], o32["decoding_order"])
    left_out = n - int(rs.order_decided(key, K).sum())
    assert left_out <= (rs.MAX_LEFT_OUT * n if key.endswith("_shift") else 0), left_out
    for what in ("score", "unconditional"):
        d = float((o32[what].double() - o64[what])[valid].abs().max())
        ties = n - int(rs.argmax_decided(o64[what], valid).sum())
        print(f"REAL host {key} K={K} {what}: fp32 oracle vs fp64 max|dlogp| = {d:.2e}; near ties {ties} of {n}; order rule leaves out {left_out}")
        assert d < 0.1 * rs.TOL_LOGP, (what, d)
        assert ties <= rs.MAX_LEFT_OUT * n, (what, ties, n)

