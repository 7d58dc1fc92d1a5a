"""The two real structures of tests/golden/pdb (public PDB entries 1AM9: 313 protein + 76 DNA residues in 8 chains, and 4OQU: a 97-nt
RNA) as test inputs: parsed by na_mpnn_amd.pdbio and completed to the dict synth.make_complex returns, exact numpy variants of them
(a +1000 A shift, the 180-degree rotations, crops), their base-pair lists, and the CPU oracle's results per (variant, K), computed
once.  Helper module of test_real_structures_host.py / test_gpu_real_structures.py (not a test)."""
import contextlib
import functools
import lzma
import os
import tempfile

import numpy as np
import torch

from na_mpnn_amd import pdbio, spec, synth
from oracle import cpu_ref

GOLDEN_PDB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdb")
PER_RESIDUE = ("X", "X_m", "mask", "S", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type", "chain_mask",
               "randn")
F64 = torch.float64
C1P = spec.ATOM_TYPES.index("C1'")
SHIFT = 1000.0                        # Angstrom: the coordinate range of a large cryo-EM entry, still inside the PDB format's %8.3f
TOL_LOGP, TOL_E = 1e-3, 2e-4          # the parity bars of test_gpu_parity.py (log-probs, activations)
NEAR_TIE = 2 * TOL_LOGP               # arg-max is compared where the fp64 oracle's top two are at least this far apart
MAX_LEFT_OUT = 0.02                   # ... and that rule, like the neighbour-order rule, may leave out at most this share of the rows


# ------------------------------------------------------------------------------------------------------------------------------------
# structures and variants
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parsed(name, kw):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, name + ".pdb")
        with lzma.open(os.path.join(GOLDEN_PDB, name + ".pdb.xz")) as src, open(path, "wb") as dst:
            dst.write(src.read())
        return pdbio.parse_pdb(path, **dict(kw))


def load(name, **parse_kw):
    """tests/golden/pdb/<name>.pdb.xz parsed with pdbio.parse_pdb(**parse_kw) -> a fresh copy of the dict synth.make_complex returns
    (every residue designable, a seeded `randn`)."""
    P = _parsed(name, tuple(sorted(parse_kw.items())))
    L = len(P["S"])
    cx = {k: np.array(P[k]) for k in PER_RESIDUE[:-2]}
    cx["R_polymer_type"] = cx["R_polymer_type"].astype(np.int64)
    cx["chain_mask"] = np.ones(L, np.int32)
    cx["randn"] = np.random.default_rng(sum(map(ord, name)) + L).standard_normal(L).astype(np.float32)
    return cx


def chain_letters(name, **parse_kw):
    return list(_parsed(name, tuple(sorted(parse_kw.items())))["chain_letters"])


def rows_of_chains(name, letters):
    """The residues of the listed chains, in the order the chains are listed."""
    cl = chain_letters(name)
    return np.array([i for c in letters for i, x in enumerate(cl) if x == c])


def shifted(cx, d=SHIFT):
    """Every PRESENT atom moved by +d along x, y and z; an absent atom stays at 0, as the parser stores it."""
    out = {k: v.copy() for k, v in cx.items()}
    out["X"] = (cx["X"] + np.float32(d) * cx["X_m"][:, :, None].astype(np.float32)).astype(np.float32)
    return out


def rot180(cx, axis):
    """The rotation by 180 degrees about the x, y or z axis: two sign flips, exact in fp32 — every coordinate difference keeps its
    magnitude, so every squared difference and every distance keeps its bits, and the cross products of the virtual atoms transform
    exactly."""
    sign = np.full(3, -1.0, np.float32)
    sign["xyz".index(axis)] = 1.0
    out = {k: v.copy() for k, v in cx.items()}
    out["X"] = cx["X"] * sign
    return out


def crop(cx, rows):
    return {k: np.ascontiguousarray(v[np.asarray(rows)]) for k, v in cx.items()}


CROP_CHAINS = "EHA"                   # a DNA duplex (21 + 17 nt) and the protein chain bound to it: 118 residues


@functools.lru_cache(maxsize=None)
def _variant(key):
    if key == "4oqu":
        return load("4oqu")
    if key == "4oqu_legacy":          # separate RNA tokens (needed by G-U wobble)
        return load("4oqu", na_shared_tokens=False)
    if key == "1am9":
        return load("1am9")
    if key == "1am9_missing":         # the four 5' nucleotides without a phosphate are unmasked
        return load("1am9", load_residues_with_missing_atoms=True)
    if key == "1am9_shift":
        return shifted(load("1am9"))
    if key == "1am9_crop":
        return crop(load("1am9"), rows_of_chains("1am9", CROP_CHAINS))
    if key.startswith("1am9_rot"):
        return rot180(load("1am9"), key[-1])
    raise KeyError(key)


def variant(key):
    """A fresh copy of the named variant."""
    return {k: v.copy() for k, v in _variant(key).items()}


ORACLE_CASES = (("4oqu", 32), ("4oqu", 48), ("1am9", 48), ("1am9_missing", 48), ("1am9_shift", 48))
ROTATIONS = ("1am9", "1am9_rotx", "1am9_roty", "1am9_rotz")      # the identity and the three rotations: the four images of §c


def fd_cpu(cx, **extra):
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
    fd["batch_size"] = 1
    fd.update(extra)
    return fd


def sample_fd(cx, bs, T, seed, bias=None):
    """CPU feature_dict of a sample() call: `bs` streams with seeded decoding noise."""
    L = cx["S"].shape[0]
    return fd_cpu(cx, batch_size=bs, temperature=T, bias=torch.zeros(1, L, 33) if bias is None else bias, symmetry_residues=[[]],
                  symmetry_weights=[[]], randn=torch.from_numpy(np.random.default_rng(seed).standard_normal((bs, L)).astype(np.float32)))


def to_dev(fd, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


# ------------------------------------------------------------------------------------------------------------------------------------
# base pairs
# ------------------------------------------------------------------------------------------------------------------------------------
def c1_distance(cx, i, j):
    return float(np.linalg.norm(cx["X"][i, C1P].astype(np.float64) - cx["X"][j, C1P].astype(np.float64)))


def pairs_1am9():
    """The two duplexes of 1am9 (chains E-H and G-F; the DNA chains come first in the file): 17 pairs each."""
    return [(i, 75 - i) for i in range(17)] + [(38 + i, 37 - i) for i in range(17)]


def is_canonical(a, b, rti=None):
    return (int(a), int(b)) in set(spec.na_canonical_base_pair_ints(rti or spec.restype_to_int(True)))


@functools.lru_cache(maxsize=None)
def _stems_4oqu():
    cx = _variant("4oqu")
    L = cx["S"].shape[0]
    P = cx["X"][:, C1P].astype(np.float64)
    D = np.linalg.norm(P[:, None] - P[None], axis=-1)
    ok = lambda i, j: 0 <= i < L and 0 <= j < L and j - i >= 4 and 9.8 <= D[i, j] <= 11.2
    used, pairs = set(), []
    for i in range(L):
        for j in range(i + 4, L):
            if ok(i, j) and (ok(i + 1, j - 1) or ok(i - 1, j + 1)) and i not in used and j not in used:
                pairs.append((i, j)); used.update((i, j))
    return tuple(pairs)


def stems_4oqu(canonical_only=True):
    """Stacked base pairs of 4oqu read off the geometry: j - i >= 4, C1'-C1' within [9.8, 11.2] A, and the stacked neighbour
    (i + 1, j - 1) or (i - 1, j + 1) qualifying too; made disjoint greedily in index order.  canonical_only: those whose native
    tokens are a Watson-Crick pair."""
    S = _variant("4oqu")["S"]
    return [(i, j) for i, j in _stems_4oqu() if not canonical_only or is_canonical(S[i], S[j])]


# ------------------------------------------------------------------------------------------------------------------------------------
# the CPU oracle, once per (variant, K)
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights():
    return cpu_ref.to_torch(synth.make_weights(0))


@functools.lru_cache(maxsize=None)
def weights64():
    return cpu_ref.to_dtype(weights(), F64)


@contextlib.contextmanager
def _features_once():
    """score() and unconditional_probs() of the oracle each featurise again; inside this block the first result is reused."""
    real, memo = cpu_ref.features, {}

    def features(w, fd, top_k, *a):
        key = (id(w), id(fd), top_k) + a
        if key not in memo:
            memo[key] = real(w, fd, top_k, *a)
        return memo[key]

    cpu_ref.features = features
    try:
        yield
    finally:
        cpu_ref.features = real


@functools.lru_cache(maxsize=None)
def oracle(key, K, dtype=F64):
    """cpu_ref.features / score / unconditional_probs of the variant, evaluated in `dtype` (fp64: the reference of the GPU tests; fp32:
    the reference's own arithmetic)."""
    fd = fd_cpu(_variant(key))
    w = weights()
    if dtype == F64:
        fd, w = cpu_ref.to_dtype(fd, F64), weights64()
    with torch.no_grad(), _features_once():
        _, E, E_idx = cpu_ref.features(w, fd, K)
        sc = cpu_ref.score(w, fd, K)
        un = cpu_ref.unconditional_probs(w, fd, K)
    return {"E": E[0], "E_idx": E_idx[0], "score": sc["log_probs"][0], "decoding_order": sc["decoding_order"],
            "unconditional": un["log_probs"][0]}


def order_decided(key, K):
    """Unmasked rows on which the fp32 and the fp64 oracle list the K neighbours in the same order [L] bool: there a neighbour list is
    compared in order, elsewhere as a set."""
    a, b = oracle(key, K, F64)["E_idx"], oracle(key, K, torch.float32)["E_idx"]
    return torch.from_numpy(_variant(key)["mask"].astype(bool)) & (a == b).all(-1)


def argmax_decided(ref_log_probs, valid):
    """Rows whose arg-max is compared: unmasked, and the reference's top two at least NEAR_TIE apart."""
    top2 = torch.topk(ref_log_probs.double(), 2, dim=-1).values
    return valid & ((top2[..., 0] - top2[..., 1]) >= NEAR_TIE)
