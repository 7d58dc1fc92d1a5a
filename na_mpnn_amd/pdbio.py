"""Minimal PDB ATOM-record reader/writer producing the NA-MPNN ``feature_dict``.

Restates the semantics of the reference's prody-based ``parse_PDB`` + ``featurize``
(/root/reference/inference/data_utils.py:84-439) without prody (absent from this image):

* atoms with occupancy > 0, altloc blank or 'A', first MODEL only (another one through ``model=``; ``parse_states`` stacks the
  MODELs of an ensemble — the states of a multi-state design — after checking that they list the same residues);
* residues are keyed chain / resnum / insertion-code and ordered by the first appearance of their
  reference atom (CA for amino acids, C1' for nucleotides; data_utils.py:258-276);
* the 16 backbone atoms in the order N, CA, C, O, OP1, OP2, P, O5', C5', C4', O4', C3', O3', C2', O2', C1';
* polymer masks from backbone completeness (protein: N CA C O; RNA: the 12 NA atoms; DNA: the 11 without
  O2', minus RNA; data_utils.py:316-321), ``mask`` = their sum, ``R_polymer_type`` PP/DNA/RNA/UNK;
* tokens from residue names with polymer-dependent unknowns (UNK / DX / RX; data_utils.py:333-345),
  optionally sharing DNA tokens for RNA (``na_shared_tokens``, run.py:112-117);
* ``featurize``: residue numbers bumped by the count of repeated numbers (insertion codes; data_utils.py:409-416).

Parity note: prody cannot be imported here, so this reader is checked by write->read round trips and against
the facts SURVEY App. B records for the reference's two example files (when /root/reference is present).
"""
from __future__ import annotations

import numpy as np

from . import spec

# Residue-name classes of the reference's prody selections ("protein", "nucleic", "water": prody/atomic/flags.py as
# documented for ProDy 2.x — standard + non-standard amino acids; nucleobases, nucleotides, nucleosides).  prody is not
# installable here, so these tables are a restatement from its documentation, not a pinned import.
PROTEIN_NAMES = set(spec.RESTYPES[:20]) | {"ASX", "GLX", "CSO", "HIP", "HSD", "HSE", "HSP", "MSE", "SEC", "SEP", "TPO", "PTR",
                                           "XLE", "XAA"}      # (UNK is in neither of prody's amino-acid tables: "other atoms")
NUCLEIC_NAMES = {"GUN", "ADE", "CYT", "THY", "URA",                                    # nucleobase
                 "DA", "DC", "DG", "DT", "DU", "A", "C", "G", "T", "U",                # nucleotide
                 "AMP", "ADP", "ATP", "CDP", "CTP", "GMP", "GDP", "GTP", "TMP", "TTP", "UMP", "UDP", "UTP",   # nucleoside
                 "DX", "RX"}                                                           # the reference's own unknown-NA names
WATER_NAMES = {"HOH", "DOD", "WAT", "TIP3", "H2O", "OH2", "TIP", "TIP2", "TIP4", "SOL"}
PROTEIN_BB = ["N", "CA", "C", "O"]
DNA_BB = ["OP1", "OP2", "P", "O5'", "C5'", "C4'", "O4'", "C3'", "O3'", "C2'", "C1'"]
RNA_BB = ["OP1", "OP2", "P", "O5'", "C5'", "C4'", "O4'", "C3'", "O3'", "C2'", "O2'", "C1'"]
LEGACY_ATOM_NAMES = {"O1P": "OP1", "O2P": "OP2"}       # pre-remediation PDB names; '*' -> "'" is applied to every name


class Atom:
    """One coordinate record of either file format."""
    __slots__ = ("het", "serial", "name", "altloc", "resname", "chain", "resnum", "icode", "xyz", "occ", "bfac", "element")

    def __init__(self, het, serial, name, altloc, resname, chain, resnum, icode, xyz, occ, bfac, element):
        self.het, self.serial, self.name, self.altloc, self.resname, self.chain = het, serial, name, altloc, resname, chain
        self.resnum, self.icode, self.xyz, self.occ, self.bfac, self.element = resnum, icode, xyz, occ, bfac, element


def _pdb_atoms(path, model=None):
    """ATOM / HETATM records of the first MODEL of a PDB file (prody parsePDB: model 1, HETATM included), or of MODEL `model` (its
    serial number; a file without MODEL records is model 1)."""
    cur = 1
    with open(path) as fh:
        for line in fh:
            rec = line[:6]
            if rec == "MODEL ":
                cur = _model_serial(line, cur)
                continue
            if rec == "ENDMDL":
                if model is None or cur == model:
                    break
                cur = None                                    # between two models
                continue
            if rec not in ("ATOM  ", "HETATM") or (model is not None and cur != model):
                continue
            try:
                occ = float(line[54:60]) if line[54:60].strip() else 1.0
                bfac = float(line[60:66]) if line[60:66].strip() else 0.0
                xyz = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
                resnum = int(line[22:26])
                serial = int(line[6:11]) if line[6:11].strip().isdigit() else 0
            except ValueError:
                continue
            yield Atom(rec == "HETATM", serial, line[12:16].strip(), line[16].strip(), line[17:20].strip(), line[21],
                       resnum, line[26].strip(), xyz, occ, bfac, line[76:78].strip() if len(line) >= 78 else "")


def _model_serial(line, cur):
    f = line[6:].split()
    return int(f[0]) if f and f[0].lstrip("-").isdigit() else (cur or 0) + 1


def _split_cif_row(line):
    """Tokens of one mmCIF data line: whitespace separated, with '...' / "..." quoting."""
    out, i, n = [], 0, len(line)
    while i < n:
        c = line[i]
        if c.isspace():
            i += 1
        elif c in "'\"":
            j = i + 1
            while j < n and not (line[j] == c and (j + 1 == n or line[j + 1].isspace())):
                j += 1
            out.append(line[i + 1:j]); i = j + 1
        else:
            j = i
            while j < n and not line[j].isspace():
                j += 1
            out.append(line[i:j]); i = j
    return out


def _mmcif_site(path):
    """(column names, rows) of the `_atom_site` loop of an mmCIF file."""
    cols, rows, in_loop, in_site = [], [], False, False
    with open(path) as fh:
        for raw in fh:
            line = raw.rstrip("\n")
            st = line.strip()
            if st == "loop_":
                if in_site and rows:
                    break
                in_loop, in_site, cols = True, False, []
                continue
            if in_loop and st.startswith("_"):
                if st.startswith("_atom_site."):
                    in_site = True
                    cols.append(st.split()[0][len("_atom_site."):])
                elif in_site:
                    break
                continue
            if in_site:
                if not st or st.startswith("#") or st.startswith("data_"):
                    if rows:
                        break
                    continue
                rows.append(_split_cif_row(line))
            elif st and not st.startswith("_"):
                in_loop = False
    if not cols:
        raise ValueError(f"{path}: no _atom_site loop found")
    return cols, rows


def _mmcif_atoms(path, model=None):
    """The `_atom_site` loop of an mmCIF file, first model (or the one whose pdbx_PDB_model_num is `model`), with the author (auth_*)
    identifiers PDB files carry — chain = auth_asym_id, residue number = auth_seq_id, insertion code = pdbx_PDB_ins_code."""
    cols, rows = _mmcif_site(path)
    ix = {c: i for i, c in enumerate(cols)}
    need = ("Cartn_x", "Cartn_y", "Cartn_z")
    if any(c not in ix for c in need):
        raise ValueError(f"{path}: _atom_site lacks coordinates")
    get = lambda row, key, alt=None, default="": (row[ix[key]] if key in ix else (row[ix[alt]] if alt and alt in ix else default))
    nul = lambda v: "" if v in (".", "?") else v
    first_model = None
    for row in rows:
        if len(row) < len(cols):
            continue
        row_model = get(row, "pdbx_PDB_model_num", default="1")
        if model is not None:
            if row_model != str(model):
                continue
        else:
            if first_model is None:
                first_model = row_model
            if row_model != first_model:
                break
        try:
            xyz = (float(row[ix["Cartn_x"]]), float(row[ix["Cartn_y"]]), float(row[ix["Cartn_z"]]))
            resnum = int(get(row, "auth_seq_id", "label_seq_id", "0"))
            occ = float(nul(get(row, "occupancy", default="1.0")) or 1.0)
            bfac = float(nul(get(row, "B_iso_or_equiv", default="0.0")) or 0.0)
            serial = int(get(row, "id", default="0"))
        except ValueError:
            continue
        yield Atom(get(row, "group_PDB", default="ATOM") == "HETATM", serial, get(row, "auth_atom_id", "label_atom_id"),
                   nul(get(row, "label_alt_id")), get(row, "auth_comp_id", "label_comp_id"), get(row, "auth_asym_id", "label_asym_id"),
                   resnum, nul(get(row, "pdbx_PDB_ins_code")), xyz, occ, bfac, nul(get(row, "type_symbol")))


def model_ids(path):
    """The model numbers of a structure file in file order: the serials of the MODEL records of a PDB file, the distinct
    pdbx_PDB_model_num values of an mmCIF file; [1] for a file without either."""
    if str(path).lower().endswith((".cif", ".mmcif")):
        cols, rows = _mmcif_site(path)
        if "pdbx_PDB_model_num" not in cols:
            return [1]
        i, ids = cols.index("pdbx_PDB_model_num"), []
        for row in rows:
            if len(row) >= len(cols) and row[i].lstrip("-").isdigit() and int(row[i]) not in ids:
                ids.append(int(row[i]))
        return ids or [1]
    ids, cur = [], 0
    with open(path) as fh:
        for line in fh:
            if line[:6] == "MODEL ":
                cur = _model_serial(line, cur)
                ids.append(cur)
    return ids or [1]


def read_atoms(path, chains=None, normalize_legacy_names=False, chain_order=None, ca_residues=None, model=None):
    """Coordinate records the reference's parse_PDB keeps before any polymer logic (data_utils.py:232-238): first model,
    altloc blank or 'A' (prody's default), occupancy > 0, optionally only the given chains.  `.cif` / `.mmcif` files go
    through the mmCIF reader.  normalize_legacy_names maps pre-remediation nucleic atom names (O1P, O2P, C1*, ...) to the
    current ones; the reference (prody) does not, so it is off by default.  chain_order (a list) receives the chain ids in
    order of first appearance over EVERY parsed record — before the occupancy / chain filters, hetero atoms and waters
    included: that is the numbering prody's getChindices() reports (data_utils.py:303).  ca_residues (a set) receives the
    (chain, number, insertion code) keys of the residues that have an atom named CA, likewise over every parsed record.
    model: the model to read (see model_ids) instead of the first one."""
    low = str(path).lower()
    if model is not None and int(model) not in model_ids(path):
        raise ValueError(f"{path}: no model {model} (the file has {model_ids(path)})")
    model = None if model is None else int(model)
    src = _mmcif_atoms(path, model) if low.endswith((".cif", ".mmcif")) else _pdb_atoms(path, model)
    chains = set(chains) if chains else None
    records = [a for a in src if a.altloc in ("", "A")]
    for a in records:                                   # properties of the WHOLE parsed structure, like prody's flags / hierarchy
        if chain_order is not None and a.chain not in chain_order:
            chain_order.append(a.chain)
        if ca_residues is not None and a.name == "CA":
            ca_residues.add((a.chain, a.resnum, a.icode))
    for a in records:
        if a.occ <= 0 or (chains and a.chain not in chains):
            continue
        if normalize_legacy_names:
            a.name = LEGACY_ATOM_NAMES.get(a.name.replace("*", "'"), a.name.replace("*", "'"))
        yield a


def parse_pdb(path, chains=None, parse_na_only=False, na_shared_tokens=True, load_residues_with_missing_atoms=False,
              normalize_legacy_names=False, model=None):
    """parse_PDB of the reference (data_utils.py:84-405) for PDB and mmCIF files -> dict of numpy arrays (no batch
    dimension) + 'chain_letters', 'icodes', 'na_chain_letters', and the atom records the backbone writer needs
    ('backbone_atoms': protein N/CA/C/O and the 12 nucleic backbone atoms; 'other_atoms': neither polymer nor water).
    model: the model to parse (see model_ids); None = the first one."""
    return _parse(path, chains, parse_na_only, na_shared_tokens, load_residues_with_missing_atoms, normalize_legacy_names, model)[0]


def parse_states(path, chains=None, parse_na_only=False, na_shared_tokens=True, load_residues_with_missing_atoms=False,
                 normalize_legacy_names=False, contexts=False):
    """Every model of a structure file as the states of ONE molecule (an NMR ensemble, the folds of a riboswitch): the first
    model's parse_pdb dict with 'X' [M, L, 16, 3] and 'X_m' [M, L, 16] stacked over the models, and 'model_ids'.  Raises ValueError
    unless all models give the same residues — chain, number, insertion code, residue name and `mask`.
    contexts=True: the models are CONTEXT states — they may differ in residue names and lack residues or whole
    chains (a fixed partner with another sequence, the unbound form).  The residue list is the union: chains in order of first
    appearance over the models, inside a chain the order of the model with the most residues of it (the first such model), of which
    every other model's residues of that chain must be a subsequence (ValueError names the model otherwise); a residue's polymer type
    must agree across the models that have it.  Also returns 'state_S' int32 [M, L] (an absent residue: the token of the first model
    that has it) and 'state_mask' int32 [M, L] (the model's own `mask`; 0 where it lacks the residue); 'S' and the other per-residue
    entries come from the first model that has the residue, `mask` is the OR of state_mask, X / X_m of an absent residue are zero."""
    ids = model_ids(path)
    parsed = [_parse(path, chains, parse_na_only, na_shared_tokens, load_residues_with_missing_atoms, normalize_legacy_names, i) for i in ids]
    if contexts:
        return _union_of_states(path, ids, parsed)
    key = lambda P, names: (P["chain_letters"], P["R_idx"].tolist(), P["icodes"], names, P["mask"].tolist())
    first = key(*parsed[0])
    for i, pn in zip(ids[1:], parsed[1:]):
        other = key(*pn)
        if other != first:
            what = [n for n, a, b in zip(("chains", "residue numbers", "insertion codes", "residue names", "mask"), first, other) if a != b]
            raise ValueError(f"{path}: model {i} does not list the same residues as model {ids[0]} ({', '.join(what)} differ): "
                             "the states of a multi-state design must be conformations of one molecule")
    out = dict(parsed[0][0])
    out["X"] = np.stack([P["X"] for P, _ in parsed])
    out["X_m"] = np.stack([P["X_m"] for P, _ in parsed])
    out["model_ids"] = ids
    return out


def _union_of_states(path, ids, parsed):
    """parse_states(contexts=True): the models' parses merged over the union of their residues."""
    keys = [list(zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])) for P, _ in parsed]
    chain_order = []
    for ks in keys:
        for k in ks:
            if k[0] not in chain_order:
                chain_order.append(k[0])
    union = []
    for c in chain_order:
        per_model = [[k for k in ks if k[0] == c] for ks in keys]
        longest = max(per_model, key=len)                                    # (max returns the first of equals)
        for i, mine in zip(ids, per_model):
            it = iter(longest)
            if not all(k in it for k in mine):                               # (consumes `it`: a subsequence test)
                raise ValueError(f"{path}: the residues of chain {c} in model {i} are not a subsequence of the chain's longest model: "
                                 "context states list one molecule's residues in one order")
        union += longest
    L, M = len(union), len(parsed)
    at = {k: i for i, k in enumerate(union)}
    rows = [np.array([at[k] for k in ks], np.int64) for ks in keys]
    X = np.zeros((M, L) + parsed[0][0]["X"].shape[1:], np.float32)
    X_m = np.zeros((M, L) + parsed[0][0]["X_m"].shape[1:], np.int32)
    state_mask, has = np.zeros((M, L), np.int32), np.zeros((M, L), bool)
    state_S = np.zeros((M, L), np.int32)
    for m, ((P, _), r) in enumerate(zip(parsed, rows)):
        X[m, r], X_m[m, r], state_mask[m, r], state_S[m, r], has[m, r] = P["X"], P["X_m"], P["mask"], P["S"], True
    if not has.any(0).all():
        raise ValueError(f"{path}: internal error: a residue of the union is in no model")
    first = has.argmax(0)                                                    # the first model that has the residue
    shared = ("S", "R_idx", "protein_mask", "dna_mask", "rna_mask", "rna_mask_for_token_conversion", "R_polymer_type")
    out = dict(parsed[0][0])
    for k in shared:
        out[k] = np.zeros(L, parsed[0][0][k].dtype)
    for m, ((P, _), r) in enumerate(zip(parsed, rows)):
        sel = first[r] == m
        for k in shared:
            out[k][r[sel]] = P[k][sel]
    # the polymer type of a residue: the same in every model that resolves it (mask 1; an unresolved residue has none)
    ptype = np.full((M, L), -1, np.int64)
    for m, ((P, _), r) in enumerate(zip(parsed, rows)):
        ptype[m, r] = P["R_polymer_type"]
    resolved = state_mask != 0
    ref = ptype[resolved.argmax(0), np.arange(L)]                            # ... of the first model that resolves it
    clash = resolved & (ptype != ref[None, :])
    if clash.any():
        m, i = (int(v[0]) for v in np.nonzero(clash))
        c, n, ic = union[i]
        raise ValueError(f"{path}: residue {c}{n}{ic} is another polymer type in model {ids[m]} than in model {ids[int(resolved[:, i].argmax())]}")
    state_S = np.where(has, state_S, out["S"][None, :]).astype(np.int32)
    # chain labels: the first model's that has the chain, moved aside where two chains of different models would share one
    label = {}
    for c in chain_order:
        P = next(P for (P, _), ks in zip(parsed, keys) if any(k[0] == c for k in ks))
        v = int(P["chain_labels"][P["chain_letters"].index(c)])
        while v in label.values():
            v = max(label.values()) + 1
        label[c] = v
    letters = [k[0] for k in union]
    out.update({"X": X, "X_m": X_m, "state_S": state_S, "state_mask": state_mask, "mask": state_mask.max(0).astype(np.int32),
                "chain_labels": np.array([label[c] for c in letters], np.int32), "chain_letters": letters, "icodes": [k[2] for k in union],
                "na_chain_letters": [c for i, c in enumerate(letters) if out["dna_mask"][i] or out["rna_mask"][i]], "model_ids": ids})
    return out


def _parse(path, chains, parse_na_only, na_shared_tokens, load_residues_with_missing_atoms, normalize_legacy_names, model):
    """parse_pdb's work -> (its dict, the residue names)."""
    atom_index = {a: i for i, a in enumerate(spec.ATOM_TYPES)}
    rti = spec.restype_to_int(na_shared_tokens)
    residues, order = {}, []        # key -> {"resname", "kind", "atoms": {name: xyz}}
    chain_order = []
    backbone_atoms, other_atoms = [], []
    bb_names = {"protein": set(PROTEIN_BB), "nucleic": set(RNA_BB)}
    ca_residues = set()
    for at in read_atoms(path, chains, normalize_legacy_names, chain_order, ca_residues, model):
        name, resname, chain = at.name, at.resname, at.chain
        # prody's `protein` flag: a qualifying residue name AND an atom named CA in the residue (manual, Atom Flags)
        kind = "protein" if (resname in PROTEIN_NAMES and (chain, at.resnum, at.icode) in ca_residues) else \
            ("nucleic" if resname in NUCLEIC_NAMES else None)
        if parse_na_only and kind != "nucleic":
            continue
        if kind is None:
            if resname not in WATER_NAMES:
                other_atoms.append(at)
            continue
        if name in bb_names[kind]:
            backbone_atoms.append(at)
        key = (chain, at.resnum, at.icode)
        r = residues.get(key)
        if r is None:
            r = residues[key] = {"resname": resname, "kind": kind, "atoms": {}, "ref": False}
        r["atoms"][name] = at.xyz
        if name == ("CA" if kind == "protein" else "C1'") and not r["ref"]:
            r["ref"] = True
            order.append(key)                       # residue order = order of reference atoms
    n = len(order)
    X = np.zeros((n, spec.N_ATOMS, 3), np.float32)
    X_m = np.zeros((n, spec.N_ATOMS), np.int32)
    for i, key in enumerate(order):
        for a, xyz in residues[key]["atoms"].items():
            j = atom_index.get(a)
            if j is not None:
                X[i, j] = xyz
                X_m[i, j] = 1
    resnames = [residues[k]["resname"] for k in order]
    prod = lambda names: np.prod(X_m[:, [atom_index[a] for a in names]], axis=-1).astype(np.int32)
    if load_residues_with_missing_atoms:
        protein_mask = np.array([r in spec.RESTYPES[:21] for r in resnames], np.int32)
        dna_mask = np.array([r in ("DA", "DC", "DG", "DT", "DX") for r in resnames], np.int32)
        rna_mask = np.array([r in ("A", "C", "G", "U", "RX") for r in resnames], np.int32)
    else:
        protein_mask = prod(PROTEIN_BB)
        rna_mask = prod(RNA_BB)
        dna_mask = prod(DNA_BB) - rna_mask           # RNA also carries every DNA backbone atom
    mask = protein_mask + dna_mask + rna_mask
    pti = spec.polytype_to_int()
    R_polymer_type = (protein_mask * pti["PP"] + dna_mask * pti["DNA"] + rna_mask * pti["RNA"] +
                      (1 - protein_mask - dna_mask - rna_mask) * pti["UNK"]).astype(np.int64)
    S = np.empty(n, np.int32)
    for i, rn in enumerate(resnames):
        unk = "DX" if dna_mask[i] == 1 else ("RX" if rna_mask[i] == 1 else "UNK")
        S[i] = rti.get(rn, rti[unk])
    chain_letters = [k[0] for k in order]
    return {
        "X": X, "X_m": X_m, "mask": mask.astype(np.int32), "S": S,
        "R_idx": np.array([k[1] for k in order], np.int32),
        "chain_labels": np.array([chain_order.index(c) for c in chain_letters], np.int32),
        "protein_mask": protein_mask, "dna_mask": dna_mask, "rna_mask": rna_mask,
        "rna_mask_for_token_conversion": X_m[:, atom_index["O2'"]].copy(),
        "R_polymer_type": R_polymer_type,
        "chain_letters": chain_letters, "icodes": [k[2] for k in order],
        "na_chain_letters": [c for i, c in enumerate(chain_letters) if dna_mask[i] or rna_mask[i]],
        "backbone_atoms": backbone_atoms, "other_atoms": other_atoms,
    }, resnames


def renumber(R_idx):
    """data_utils.featurize: consecutive equal residue numbers (insertion codes) are pushed apart."""
    out, count, prev = [], 0, -100000
    for r in R_idx.tolist():
        if r == prev:
            count += 1
        out.append(r + count)
        prev = r
    return np.array(out, dtype=np.int64)


def to_feature_dict(parsed, chain_mask, device):
    """Batch-of-one torch feature_dict with the reference's dtypes (data_utils.py:361-439)."""
    import torch
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=device)[None]
    fd = {"X": t(parsed["X"], torch.float32), "X_m": t(parsed["X_m"], torch.int32), "mask": t(parsed["mask"], torch.int32),
          "S": t(parsed["S"], torch.int32), "R_idx": t(renumber(parsed["R_idx"]), torch.int64),
          "R_idx_original": t(parsed["R_idx"], torch.int32), "chain_labels": t(parsed["chain_labels"], torch.int32),
          "chain_mask": t(chain_mask, torch.int32), "R_polymer_type": t(parsed["R_polymer_type"], torch.int64)}
    for k in ("protein_mask", "dna_mask", "rna_mask", "rna_mask_for_token_conversion"):
        fd[k] = t(parsed[k], torch.int32)
    return fd


def write_pdb(path, X, X_m, resnames, chain_letters, R_idx, icodes=None):
    """Write the 16 backbone atoms as ATOM records (used by tests and for round trips)."""
    lines, serial = [], 1
    for i in range(X.shape[0]):
        for a, name in enumerate(spec.ATOM_TYPES):
            if not X_m[i, a]:
                continue
            nm = name if len(name) == 4 else " " + name
            ic = (icodes[i] if icodes else "") or " "
            lines.append("ATOM  %5d %-4s %3s %1s%4d%1s   %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (
                serial, nm, resnames[i], chain_letters[i], R_idx[i], ic, X[i, a, 0], X[i, a, 1], X[i, a, 2], 1.0, 0.0,
                name[0]))
            serial += 1
    lines.append("END")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _pdb_line(het, serial, name, resname, chain, resnum, icode, xyz, occ, bfac, element):
    nm = name if len(name) >= 4 else " " + name          # PDB columns 13-16: short names start in column 14
    return "%-6s%5d %-4s %3s %1s%4d%1s   %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (
        "HETATM" if het else "ATOM", serial % 100000, nm, resname[-3:], (chain or " ")[0], resnum, icode or " ",
        xyz[0], xyz[1], xyz[2], occ, bfac, element or name[0])


def write_backbone_pdb(path, parsed, resnames3, bfactors):
    """The design output of run.py:475-491: the parsed BACKBONE atoms (protein N, CA, C, O; the 12 nucleic backbone atoms)
    with every residue renamed to its designed 3-letter name and the B-factor column carrying the per-residue confidence,
    followed by the non-polymer, non-water atoms of the input ('backbone + other_atoms').  resnames3 / bfactors are per
    residue, in the order of parsed['chain_letters'] / ['R_idx'].  The reference writes this with prody's writePDB; this
    writer emits standard fixed-column ATOM / HETATM records (prody absent: byte-for-byte parity with its writer unpinned)."""
    by_res = {}
    for i, (c, r) in enumerate(zip(parsed["chain_letters"], parsed["R_idx"].tolist())):
        by_res.setdefault((c, int(r)), i)             # the reference selects "chain c and resnum r": insertion codes share it
    # PDB has ONE column for the chain id: mmCIF auth_asym_id values longer than that would collide once truncated
    long_ids = sorted({at.chain for at in list(parsed["backbone_atoms"]) + list(parsed["other_atoms"]) if at.chain and len(at.chain) > 1})
    if long_ids:
        raise ValueError(f"write_backbone_pdb: chain ids {long_ids} do not fit the PDB format's one-character chain column "
                         "(mmCIF input with multi-character auth_asym_id): rename the chains before asking for --output_pdbs")
    lines, serial = [], 1
    for at in parsed["backbone_atoms"]:
        i = by_res.get((at.chain, at.resnum))
        rn = resnames3[i] if i is not None else at.resname
        bf = float(bfactors[i]) if i is not None else at.bfac
        lines.append(_pdb_line(at.het, serial, at.name, rn, at.chain, at.resnum, at.icode, at.xyz, at.occ, bf, at.element))
        serial += 1
    for at in parsed["other_atoms"]:
        # run.py:336-338: other_atoms.setBetas(other_bfactors * 0.0) — the non-polymer atoms are written with B-factor 0.00
        lines.append(_pdb_line(at.het, serial, at.name, at.resname, at.chain, at.resnum, at.icode, at.xyz, at.occ, 0.0, at.element))
        serial += 1
    lines.append("END")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def write_mmcif(path, X, X_m, resnames, chain_letters, R_idx, icodes=None, name="x"):
    """Minimal mmCIF with one `_atom_site` loop (tests and round trips; the column set wwPDB files carry)."""
    cols = ["group_PDB", "id", "type_symbol", "label_atom_id", "label_alt_id", "label_comp_id", "label_asym_id", "label_entity_id",
            "label_seq_id", "pdbx_PDB_ins_code", "Cartn_x", "Cartn_y", "Cartn_z", "occupancy", "B_iso_or_equiv", "auth_seq_id",
            "auth_comp_id", "auth_asym_id", "auth_atom_id", "pdbx_PDB_model_num"]
    out = [f"data_{name}", "#", "loop_"] + ["_atom_site." + c for c in cols]
    serial = 1
    for i in range(X.shape[0]):
        for a, an in enumerate(spec.ATOM_TYPES):
            if not X_m[i, a]:
                continue
            q = f'"{an}"' if "'" in an else an
            ic = (icodes[i] if icodes else "") or "?"
            out.append(" ".join(["ATOM", str(serial), an[0], q, ".", resnames[i], chain_letters[i], "1", str(i + 1), ic,
                                 "%.3f" % X[i, a, 0], "%.3f" % X[i, a, 1], "%.3f" % X[i, a, 2], "1.00", "0.00", str(int(R_idx[i])),
                                 resnames[i], chain_letters[i], q, "1"]))
            serial += 1
    out.append("#")
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")
