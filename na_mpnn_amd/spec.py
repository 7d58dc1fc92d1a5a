"""Static vocabulary / shape contract of the NA-MPNN hot path.

These tables are *data* the reference hard-codes inside its CLI
(/root/reference/inference/run.py:15-66 atom / polymer / residue vocabularies,
:112-117 the shared DNA/RNA token aliasing) and that the model constructors take
as ``atom_dict`` / ``polytype_to_int`` / ``restype_to_int``.  They are restated
here so that the drop-in module, the oracle and the tests agree on one copy.
"""
from __future__ import annotations

from collections import OrderedDict

H = 128            # hidden / node / edge feature width
FFN = 4 * H        # PositionWiseFeedForward inner width (model_utils.py:634)
VOCAB = 33         # num_letters == vocab (run.py:130-131)
NUM_RBF = 16
NUM_POS = 16
MAX_REL = 32       # PositionalEncodings.max_relative_feature (model_utils.py:607)
NUM_POS_CLASSES = 2 * MAX_REL + 2   # relative offsets -32..32 within a chain + one class for other chains
MSG_SCALE = 30.0   # EncLayer/DecLayer ``scale`` (model_utils.py:620,660)
LN_EPS = 1e-5

ATOM_TYPES = ["N", "CA", "C", "O",
              "OP1", "OP2", "P", "O5'", "C5'", "C4'", "O4'", "C3'", "O3'", "C2'", "O2'", "C1'"]
POLYTYPES = ["PP", "DNA", "RNA", "UNK", "MAS", "PAD"]
RESTYPES = ["ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE",
            "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP", "TYR", "VAL", "UNK",
            "DA", "DC", "DG", "DT", "DX", "A", "C", "G", "U", "RX", "MAS", "PAD"]
RESTYPE_3TO1 = dict(zip(RESTYPES, list("ARNDCQEGHILKMFPSTWYVXacgtxbdhuy-+")))

N_ATOMS = len(ATOM_TYPES)          # 16
N_ATOMS_AUG = N_ATOMS + 2          # + virtual Cb + virtual N_na (model_utils.py:478-482)
EDGE_IN = NUM_POS + NUM_RBF * N_ATOMS_AUG * N_ATOMS_AUG   # 5200


def atom_dict():
    return dict(zip(ATOM_TYPES, range(N_ATOMS)))


def polytype_to_int():
    return dict(zip(POLYTYPES, range(len(POLYTYPES))))


def restype_to_int(na_shared_tokens: bool = False):
    d = dict(zip(RESTYPES, range(len(RESTYPES))))
    if na_shared_tokens:   # run.py:112-117
        d["A"], d["C"], d["G"], d["U"], d["RX"] = d["DA"], d["DC"], d["DG"], d["DT"], d["DX"]
    return d


# the 16 Watson-Crick pairs a canonical base pair may form, DNA and RNA mixed (na_data_utils.py:286-303)
NA_CANONICAL_BASE_PAIRS = [("DA", "DT"), ("DA", "U"), ("DC", "DG"), ("DC", "G"), ("DG", "DC"), ("DG", "C"), ("DT", "DA"), ("DT", "A"),
                           ("A", "DT"), ("A", "U"), ("C", "DG"), ("C", "G"), ("G", "DC"), ("G", "C"), ("U", "DA"), ("U", "A")]


def na_canonical_base_pair_ints(restype_to_int):
    """``PDBDataset.na_canonical_base_pair_ints`` (na_data_utils.py:305-308): the pairs as token ids.  Under the shared DNA/RNA
    tokens of ``restype_to_int(na_shared_tokens=True)`` the list holds duplicates, as the reference's does."""
    return [(restype_to_int[a], restype_to_int[b]) for a, b in NA_CANONICAL_BASE_PAIRS]


# Token maps of base-paired design (ProteinMPNN.sample with feature_dict["paired_residues"]): the partner of a residue receives the
# Watson-Crick complement of its token.  WC_SAME pairs two residues of one polymer type; WC_CROSS pairs a DNA residue with an RNA
# residue.  A map expresses the canonical pairs only; the G-U wobble pair is expressed by the class tables below.  Every other residue
# type maps to itself.
WC_SAME = {"DA": "DT", "DT": "DA", "DC": "DG", "DG": "DC", "A": "U", "U": "A", "C": "G", "G": "C"}
WC_CROSS = {"DA": "U", "U": "DA", "DT": "A", "A": "DT", "DC": "G", "G": "DC", "DG": "C", "C": "DG"}
SPECIAL_RESTYPES = ("UNK", "DX", "RX", "MAS", "PAD")


def token_map(restype_to_int, kind):
    """The token map `kind` ("same" / WC_SAME or "cross" / WC_CROSS) as a list over the vocabulary: entry t is the token paired with
    token t.  An involution that fixes the amino acids and the special tokens; under the shared DNA/RNA tokens both kinds coincide."""
    names = {"same": WC_SAME, "cross": WC_CROSS}[kind] if isinstance(kind, str) else kind
    out = list(range(len(RESTYPES)))
    for a, b in names.items():
        out[restype_to_int[a]] = restype_to_int[b]
    return out


def check_token_map(restype_to_int, tmap, what="token map"):
    """ValueError unless `tmap` is a permutation of the vocabulary that is its own inverse and fixes every special token."""
    tmap = [int(t) for t in tmap]
    n = len(RESTYPES)
    if len(tmap) != n or any(not 0 <= t < n for t in tmap):
        raise ValueError(f"{what}: expected {n} token ids in [0, {n}); got {tmap}")
    for t, u in enumerate(tmap):
        if tmap[u] != t:
            raise ValueError(f"{what} is not an involution: token {t} -> {u} -> {tmap[u]}")
    for name in SPECIAL_RESTYPES:
        if tmap[restype_to_int[name]] != restype_to_int[name]:
            raise ValueError(f"{what} moves the special token {name}")
    return tmap


# Pair classes of base-paired design with G-U wobble ("G pairs with C or U" is no map of the vocabulary): a pair draws one of N_CLASSES
# classes and each member reads its token from a class table.  Class a < VOCAB: the first-listed member holds token a, the second its
# Watson-Crick complement (the token maps above).  CLASS_GU: the first member holds its G, the second its U / T; CLASS_UG: the first its
# U / T, the second its G — "its" base by the member's own polymer type (WOBBLE_G / WOBBLE_U).  A pair has the two wobble classes only
# if wobble was asked for on it and at least one member is RNA.
N_CLASS_LANES = 64
CLASS_GU, CLASS_UG = VOCAB, VOCAB + 1
N_CLASSES = VOCAB + 2
WOBBLE_G = {"dna": "DG", "rna": "G"}
WOBBLE_U = {"dna": "DT", "rna": "U"}
PAIR_KINDS = ("dna-dna", "dna-rna", "rna-dna", "rna-rna")          # polymer type of the first-listed member - of the second


def class_table(restype_to_int, kind, wobble, first):
    """The class table of one member of a base pair as a list of N_CLASS_LANES token ids: entry c is the member's token under pair class
    c, -1 where the pair has no such class.  kind: the polymer types of the two members in listed order, one of PAIR_KINDS ("same" /
    "cross" are accepted for a pair without wobble); first: the first-listed member (the identity on the classes below VOCAB) or the
    second (the Watson-Crick map of the kind).  The wobble classes are filled only with `wobble` and an RNA member in the pair."""
    if kind in ("same", "cross"):
        if wobble:
            raise ValueError(f"class_table: kind '{kind}' does not say which member is RNA; name it as one of {PAIR_KINDS}")
        wc = kind
    elif kind in PAIR_KINDS:
        wc = "same" if kind in ("dna-dna", "rna-rna") else "cross"
    else:
        raise ValueError(f"class_table: unknown kind '{kind}'")
    out = (list(range(len(RESTYPES))) if first else token_map(restype_to_int, wc)) + [-1] * (N_CLASS_LANES - len(RESTYPES))
    if wobble and kind != "dna-dna":
        own = kind.split("-")[0 if first else 1]
        g, u = restype_to_int[WOBBLE_G[own]], restype_to_int[WOBBLE_U[own]]
        out[CLASS_GU], out[CLASS_UG] = (g, u) if first else (u, g)
    return out


def check_class_table(restype_to_int, table, what="class table"):
    """ValueError unless `table` has N_CLASS_LANES entries in [-1, vocab), is a token map (check_token_map) on the classes below the
    vocabulary's size, is -1 from N_CLASSES on and holds a special token on no other lane than that token's own."""
    table = [int(t) for t in table]
    n = len(RESTYPES)
    if len(table) != N_CLASS_LANES or any(not -1 <= t < n for t in table):
        raise ValueError(f"{what}: expected {N_CLASS_LANES} entries in [-1, {n}); got {table}")
    check_token_map(restype_to_int, table[:n], what)
    special = {restype_to_int[name]: name for name in SPECIAL_RESTYPES}
    for c in range(n, N_CLASS_LANES):
        if table[c] in special:
            raise ValueError(f"{what} moves the special token {special[table[c]]} to class {c}")
        if c >= N_CLASSES and table[c] != -1:
            raise ValueError(f"{what}: class {c} is beyond the {N_CLASSES} pair classes and must be -1")
    return table


def state_dict_spec(num_encoder_layers: int = 3, num_decoder_layers: int = 3,
                    hidden: int = H, vocab: int = VOCAB, num_letters: int = VOCAB):
    """Ordered {key: shape} of the reference ``ProteinMPNN.state_dict()``.

    Same key set for the inference copy (inference/model_utils.py:8-69) and the
    training copy (na_model_utils.py:519-587); SURVEY App. A.6.
    """
    s = OrderedDict()
    h = hidden

    def lin(name, out_f, in_f, bias=True):
        s[name + ".weight"] = (out_f, in_f)
        if bias:
            s[name + ".bias"] = (out_f,)

    def ln(name):
        s[name + ".weight"] = (h,)
        s[name + ".bias"] = (h,)

    lin("W_v", h, h)
    lin("features.embeddings.linear", NUM_POS, 2 * MAX_REL + 2)
    lin("features.node_embedding", h, len(POLYTYPES), bias=False)
    ln("features.norm_nodes")
    lin("features.edge_embedding", h, EDGE_IN, bias=False)
    ln("features.norm_edges")
    lin("W_e", h, h)
    s["W_s.weight"] = (vocab, h)
    for i in range(num_encoder_layers):
        p = f"encoder_layers.{i}."
        ln(p + "norm1"); ln(p + "norm2"); ln(p + "norm3")
        lin(p + "W1", h, 3 * h); lin(p + "W2", h, h); lin(p + "W3", h, h)
        lin(p + "W11", h, 3 * h); lin(p + "W12", h, h); lin(p + "W13", h, h)
        lin(p + "dense.W_in", 4 * h, h); lin(p + "dense.W_out", h, 4 * h)
    for i in range(num_decoder_layers):
        p = f"decoder_layers.{i}."
        ln(p + "norm1"); ln(p + "norm2")
        lin(p + "W1", h, 4 * h); lin(p + "W2", h, h); lin(p + "W3", h, h)
        lin(p + "dense.W_in", 4 * h, h); lin(p + "dense.W_out", h, 4 * h)
    lin("W_out", num_letters, h)
    return s
