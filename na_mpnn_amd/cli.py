"""Command-line front end with the reference's flags and output files.

Mirrors the contract of /root/reference/inference/run.py — the flags of :519-555, the mode defaults of
:559-583, ``seqs/<name>.fa`` with the header lines of :445-455 / :501-511 and ``specificity/<name>.npz`` with the
keys of :426-443, ``backbones/<name>_<id>.pdb`` (:475-491) — on top of ``na_mpnn_amd.model.ProteinMPNN`` and
``na_mpnn_amd.pdbio`` (no prody; PDB and mmCIF input).

    python -m na_mpnn_amd.cli --mode design --pdb_path in.pdb --out_folder out/ [--checkpoint_na_mpnn ckpt.pt]

``--random_init_seed N`` replaces the checkpoint by seeded synthetic weights (the trained checkpoints are not
part of the reference tree).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np
import torch

from . import pdbio, spec, synth
from .model import ProteinMPNN


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    a = p.add_argument
    a("--model_type", type=str, default="na_mpnn")
    a("--checkpoint_na_mpnn", type=str, default=None)
    a("--random_init_seed", type=int, default=None, help="use seeded synthetic weights instead of a checkpoint")
    a("--out_folder", type=str, required=True)
    a("--file_ending", type=str, default="")
    a("--pdb_path", type=str, default="")
    a("--fixed_pos_by_pdb", type=str, default="")
    a("--zero_indexed", type=int, default=0)
    a("--seed", type=int, default=0)
    a("--batch_size", type=int, default=None)
    a("--number_of_batches", type=int, default=1)
    a("--temperature", type=float, default=None)
    a("--save_stats", type=int, default=0)
    a("--chains_to_design", type=str, default=None)
    a("--omit_AA", type=str, default="X")
    a("--fixed_residues", type=str, default="")
    a("--redesigned_residues", type=str, default="")
    a("--parse_these_chains_only", type=str, default="")
    a("--bias_AA", type=str, default="")
    a("--pair_bias_AA", type=str, default="", help="pair bias for sequence neighbours, e.g. 'KK:-10.0,KE:-10.0'; goes with "
      "--paired_residues / --paired_strands / --paired_wobble / --multi_state")
    a("--pair_bias_members", type=str, default="auto", choices=("auto", "closing", "all"), help="which members of a tied group feel "
      "--pair_bias_AA: 'closing' - the group's last member only (the reference's rule); 'all' - every member, each in its own alphabet "
      "(both strands of a base pair feel their neighbours); 'auto' (default) - 'all' when base pairs are given, else 'closing'")
    a("--forbidden_motifs", type=str, default="", help="sequence motifs of 2..8 residues no design may hold on one chain, e.g. "
      "'gggg,cccc,dna:GAATTC,rna:GGGG': plain items in the one-letter alphabet of --bias_AA, 'dna:' / 'rna:' items in ACGT / ACGU; goes "
      "with every tie flag and with --pair_bias_AA; every design's fasta header reports motif_hits")
    a("--max_homopolymer", type=int, default=0, help="N in 1..7: no run of more than N equal residues (forbids the run of N + 1 of every "
      "residue type of the polymers being designed)")
    a("--symmetry_residues", type=str, default="", help="tied residues, e.g. 'A12,A13,A14|C2,C3'")
    a("--symmetry_weights", type=str, default="", help="weights matching --symmetry_residues, e.g. '1.0,1.0,1.0|-1.0,2.0'")
    a("--multi_state", type=int, default=0, help="1 - the MODELs of --pdb_path are states of one molecule: ONE sequence is designed "
      "to fit all of them (ProteinMPNN.sample with state_weights)")
    a("--state_weights", type=str, default="", help="weights of the states in model order, e.g. '0.5,0.3,0.2' (default: 1/M each)")
    a("--state_contexts", type=int, default=0, help="1 (with --multi_state 1) - the MODELs are context states: they may differ in the "
      "names of FIXED residues and lack residues or whole chains (on-target against off-target partner, bound against unbound; signed "
      "--state_weights such as '1,-0.5'); the residue list is the union of the models (ProteinMPNN.sample with state_S / state_mask)")
    a("--paired_residues", type=str, default="", help="base pairs, e.g. 'A5:B20,A6:B19' (residues named as in --fixed_residues): the "
      "second residue of a pair receives the Watson-Crick complement of the first (canonical pairs; G-U as well with --paired_wobble 1; "
      "a fixed residue decides)")
    a("--paired_strands", type=str, default="", help="chains paired antiparallel over their full lengths, e.g. 'A:B' or 'A:B,C:D'")
    a("--paired_wobble", type=int, default=0, help="1 - a pair with an RNA residue may also be the G-U wobble pair (G with U, or with T "
      "of a DNA partner), as the model weighs it against the canonical pairs")
    a("--paired_wobble_bias", type=float, default=None, help="added to the logit sums of the two wobble classes of every pair before "
      "the temperature (default 0; negative: fewer G-U pairs); needs --paired_wobble 1")
    a("--na_shared_tokens", type=int, default=1)
    a("--parse_na_only", type=int, default=0)
    a("--design_na_only", type=int, default=0)
    a("--k_neighbors", type=int, default=None)
    a("--catch_failed_inferences", type=int, default=0)
    a("--output_pdbs", type=int, default=1, help="1 - write backbones/<name>_<id>.pdb with the designed residue names")
    a("--output_sequences", type=int, default=1)
    a("--output_specificity", type=int, default=0)
    a("--conditional_probs_only", type=int, default=0, help="1 - no sampling: write conditional_probs/<name>.npz with "
      "log p(s_i | structure, all other residues) for every residue (ProteinMPNN.conditional_probs); with --paired_residues / "
      "--paired_strands the rows of a pair hold the pair's conditional, log p(pair | structure, everything else), and `pairs` is added")
    a("--conditional_tied", type=int, default=0, help="1 - with --conditional_probs_only 1: honour every tie of the design call — "
      "--symmetry_residues / --symmetry_weights, --multi_state 1 with --state_weights, and base pairs joined with either "
      "(ProteinMPNN.conditional_probs(tied=True)): the rows of a tied group hold the GROUP's conditional, and `groups` (padded with -1; "
      "flat indices state * L + residue with --multi_state) and `group_log_probs` are added")
    a("--conditional_classes", type=int, default=0, help="1 - with --conditional_probs_only 1: score base pairs in PAIR CLASSES "
      "(ProteinMPNN.conditional_probs(classes=True)), so that --paired_wobble 1 / --paired_wobble_bias are accepted and a pair with an "
      "RNA member may also be G-U; with and without --conditional_tied 1; `pair_class_log_probs` or `group_class_log_probs` [n, 64] "
      "(-inf on absent classes) is added")
    a("--score_fasta", type=str, default="", help="no sampling: score the sequences of FILE (the format of seqs/<name>.fa: the "
      "alphabet of the designs, chains in alphabetical order separated by '/', header lines ignored) on --pdb_path with "
      "ProteinMPNN.score_sequences and write scores/<name>.npz; the sequences may differ from the structure only where the usual flags "
      "(--chains_to_design, --fixed_residues, --redesigned_residues, --design_na_only) make it designable")
    a("--score_tied", type=int, default=0, help="1 - with --score_fasta: the sequences are scored with ProteinMPNN.score_tied, the joint "
      "log-likelihood under the distribution a TIED design draws from, so that --multi_state 1 / --state_weights, --symmetry_residues, "
      "--paired_residues / --paired_strands and --paired_wobble 1 are accepted; scores/<name>.npz then holds token_log_probs, leader, "
      "S, log_likelihood, member_log_probs, consistent, state_weights, decoding_order and chunks (a sequence that breaks a tie: -inf)")
    a("--mutation_scan", type=int, default=0, help="1: no sampling: every point mutation of the residues the usual flags make designable "
      "(--chains_to_design, --fixed_residues, --redesigned_residues, --design_na_only), over the letters of the residue's own polymer, "
      "scored with ProteinMPNN.score_mutations as the change of the structure's joint log-likelihood; with --paired_residues / "
      "--paired_strands a paired residue is mutated together with its partner (canonical duplexes, pairs=True); writes "
      "mutations/<name>.npz (residues, tokens, delta [P, T], base_loss, wild_type_token, site_rows); with --multi_state 1 "
      "[--state_contexts 1] the scan is the specificity scan under --state_weights (no pair or symmetry flags beside it) and "
      "state_delta [n, M], state_weights and base_state_log_likelihood are added")
    a("--mutation_tied", type=int, default=0, help="1, with --mutation_scan 1 and --symmetry_residues: the symmetric scan "
      "(score_mutations(tied=True)): a scanned residue stands for its whole symmetry group, every member gets the token and delta is the "
      "change of score_tied's log-likelihood; mutations/<name>.npz then also holds leader [L] and the sparse units unit_offsets, "
      "unit_residue, unit_log_prob (no pair flags, --multi_state or --pair_bias_AA beside it)")
    a("--mutation_classes", type=int, default=0, help="1, with --mutation_scan 1 --mutation_tied 1 and --paired_residues / "
      "--paired_strands [--paired_wobble 1 --paired_wobble_bias B] and/or --symmetry_residues: the paired scan "
      "(score_mutations(tied=True, classes=True)): the ties are read through pair classes as score_tied reads them; with pair flags every "
      "pair is scanned once over its classes (4 canonical, 6 with wobble on an RNA-containing pair) and mutations/<name>.npz also holds "
      "classes [T], class_tokens [P, T, 2] and the unit arrays (no --multi_state or --pair_bias_AA beside it)")
    a("--coordinate_gradients", type=int, default=0, help="1: no sampling: the gradient of the structure's negative log-likelihood, "
      "sum of -log p(s_i) over the residues the usual flags make designable (fixed residues decoded first, as score does), with respect to "
      "every atom coordinate (ProteinMPNN.coordinate_gradients); writes gradients/<name>.npz (dX [L, 16, 3], residue_norm [L], loss, "
      "encoded_residues, mask, chain_mask, decoding_randn)")
    a("--load_residues_with_missing_atoms", type=int, default=0)
    a("--mode", type=str, default=None)
    a("--device", type=str, default="cuda:0")
    a("--forced_draws_npz", type=str, default="", help="testing: npz with 'randn' [batches*batch_size, L] (decoding-order noise) and "
      "'S_forced' [batches*batch_size, L] (the tokens every draw is forced to) — makes a run reproducible across devices")
    return p


def apply_mode_defaults(args):
    """run.py:559-583."""
    def need(v):
        if v is None:
            print("Choose mode from: design, specificity")
            sys.exit()
        return v
    m = {"design": ("./models/design_model/s_19137.pt", 1, 0.1), "specificity": ("./models/specificity_model/s_70114.pt", 30, 0.6)}.get(args.mode)
    if args.checkpoint_na_mpnn is None and args.random_init_seed is None:
        args.checkpoint_na_mpnn = need(m and m[0])
    if args.batch_size is None:
        args.batch_size = need(m and m[1])
    if args.temperature is None:
        args.temperature = need(m and m[2])
    return args


def seq_string(tokens, rna_flag, int_to_str, dna_to_rna, chain_letters):
    chars = [dna_to_rna.get(int_to_str[int(t)], int_to_str[int(t)]) if rna_flag[i] == 1 else int_to_str[int(t)]
             for i, t in enumerate(tokens)]
    out, seen = [], []
    for c in chain_letters:
        if c not in seen:
            seen.append(c)
    for c in sorted(seen):
        out.append("".join(ch for ch, cl in zip(chars, chain_letters) if cl == c))
    return "/".join(out)


def make_pair_bias(chain_labels, R_idx, pair_bias_AA):
    """[1,L,33,L,33] bias between sequence neighbours on one chain (semantics of data_utils.py:7-16):
    out[0,i,a,i+1,b] = pair_bias_AA[a,b] and out[0,i+1,a,i,b] = pair_bias_AA[b,a] where R_idx[i+1]-R_idx[i]==1."""
    L = R_idx.shape[0]
    adj = ((R_idx[1:] - R_idx[:-1]) == 1) & (chain_labels[1:] == chain_labels[:-1])
    out = torch.zeros(1, L, pair_bias_AA.shape[0], L, pair_bias_AA.shape[1], dtype=torch.float32, device=pair_bias_AA.device)
    i = torch.nonzero(adj)[:, 0]
    out[0, i, :, i + 1, :] = pair_bias_AA
    out[0, i + 1, :, i, :] = pair_bias_AA.t()
    return out


def make_pair_terms(chain_labels, R_idx, pair_bias_AA, members="closing"):
    """make_pair_bias's quantity in the compact form of ProteinMPNN.sample's feature_dict["pair_terms"]: tables [AA, AA.t()]; residue i
    reads i-1 through AA.t() and i+1 through AA where the two are sequence neighbours on one chain (R_idx one apart)."""
    L = R_idx.shape[0]
    adj = (((R_idx[1:] - R_idx[:-1]) == 1) & (chain_labels[1:] == chain_labels[:-1])).cpu()
    partner = torch.full((1, L, 2), -1, dtype=torch.int32)
    table = torch.zeros(1, L, 2, dtype=torch.int32)
    i = torch.nonzero(adj)[:, 0]
    partner[0, i + 1, 0], table[0, i + 1, 0] = i.to(torch.int32), 1
    partner[0, i, 1] = (i + 1).to(torch.int32)
    AA = pair_bias_AA.detach().float().cpu()
    return {"partner": partner, "table": table, "tables": torch.stack((AA, AA.t())).contiguous(), "members": members}


def parse_forbidden_motifs(forbidden_motifs, max_homopolymer, rti, polymers=("protein", "dna", "rna")):
    """--forbidden_motifs 'gggg,dna:GAATTC,rna:GGGG' and --max_homopolymer N as the list of token tuples of
    feature_dict["forbidden_motifs"].  rti: the run's restype_to_int (with --na_shared_tokens 1 the RNA names hold the shared tokens);
    polymers: the polymer types being designed, whose residue types --max_homopolymer expands over."""
    one = {spec.RESTYPE_3TO1[k]: int(v) for k, v in rti.items()}
    named = {"dna": dict(zip("ACGT", ("DA", "DC", "DG", "DT"))), "rna": dict(zip("ACGU", ("A", "C", "G", "U")))}
    out = []
    for item in filter(None, (t.strip() for t in forbidden_motifs.split(","))):
        kind, _, body = item.rpartition(":")
        if kind and kind not in named:
            raise ValueError(f"--forbidden_motifs: '{item}': the prefix is 'dna:' or 'rna:'")
        try:
            out.append(tuple(int(rti[named[kind][c]]) for c in body.upper()) if kind else tuple(one[c] for c in body))
        except KeyError as e:
            raise ValueError(f"--forbidden_motifs: '{item}' holds the unknown letter {e}") from None
    if max_homopolymer:
        if not 1 <= max_homopolymer <= 7:
            raise ValueError(f"--max_homopolymer is in 1..7; got {max_homopolymer}")
        names = {"protein": spec.RESTYPES[:20], "dna": ("DA", "DC", "DG", "DT"), "rna": ("A", "C", "G", "U")}
        for tok in sorted({int(rti[n]) for kind in polymers for n in names[kind]}):
            out.append((tok,) * (max_homopolymer + 1))
    return list(dict.fromkeys(out))


def parse_pairs(paired_residues, paired_strands, encoded, chain_letters):
    """--paired_residues 'A5:B20,A6:B19' and --paired_strands 'A:B' as a list of residue-index pairs.  `encoded`: the residue names
    (chain letter + number + insertion code, as --fixed_residues takes them), `chain_letters`: the chain of every residue.  Two paired
    strands pair antiparallel: residue k of the first chain with residue n - 1 - k of the second."""
    index = dict(zip(encoded, range(len(encoded))))
    pairs = []
    for item in filter(None, (t.strip() for t in paired_residues.split(","))):
        names = item.split(":")
        if len(names) != 2:
            raise ValueError(f"--paired_residues: '{item}' is not of the form RES:RES")
        for nm in names:
            if nm not in index:
                raise ValueError(f"--paired_residues: no residue '{nm}' in the structure")
        pairs.append((index[names[0]], index[names[1]]))
    for item in filter(None, (t.strip() for t in paired_strands.split(","))):
        names = item.split(":")
        if len(names) != 2 or names[0] == names[1]:
            raise ValueError(f"--paired_strands: '{item}' is not of the form CHAIN:CHAIN with two different chains")
        a, b = ([i for i, c in enumerate(chain_letters) if c == nm] for nm in names)
        if not a or not b:
            raise ValueError(f"--paired_strands: '{item}' names a chain that is not in the structure")
        if len(a) != len(b):
            raise ValueError(f"--paired_strands: chains {names[0]} and {names[1]} have {len(a)} and {len(b)} residues; "
                             "paired strands must have equal lengths")
        pairs += list(zip(a, reversed(b)))
    return pairs


def read_fasta(path):
    """The sequences of a seqs/<name>.fa: -> (names, sequences), one name per sequence (its header line without '>', or 'sequence k')."""
    names, seqs, header = [], [], None
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                header = line[1:]
                continue
            seqs.append(line)
            names.append(header if header is not None else f"sequence {len(seqs)}")
            header = None
    return names, seqs


def fasta_tokens(names, seqs, S, chain_letters, designable, str_to_int, encoded):
    """The sequences of read_fasta as tokens int64 [n, L] in residue order — seq_string inverted: the chains in alphabetical order,
    separated by '/'.  A sequence of the wrong length, with an unknown letter, or one that differs from the structure's S outside
    `designable` (bool [L]) is a ValueError that names the sequence (and the first offending residue)."""
    L = len(S)
    index = [i for c in sorted(set(chain_letters)) for i, cl in enumerate(chain_letters) if cl == c]
    lengths = [sum(1 for cl in chain_letters if cl == c) for c in sorted(set(chain_letters))]
    out = np.empty((len(seqs), L), np.int64)
    for k, (nm, seq) in enumerate(zip(names, seqs)):
        parts = seq.split("/")
        if [len(p) for p in parts] != lengths:
            raise ValueError(f"--score_fasta: sequence '{nm}' has chains of {[len(p) for p in parts]} residues; the structure has "
                             f"{lengths} ({L} residues)")
        for i, ch in zip(index, "".join(parts)):
            if ch not in str_to_int:
                raise ValueError(f"--score_fasta: sequence '{nm}' holds the unknown letter '{ch}' at residue {encoded[i]}")
            out[k, i] = str_to_int[ch]
        bad = np.nonzero((out[k] != np.asarray(S)) & ~np.asarray(designable, bool))[0]
        if len(bad):
            raise ValueError(f"--score_fasta: sequence '{nm}' differs from the structure at residue {encoded[int(bad[0])]}, which is "
                             "not designable")
    return out


def wobble_arguments(args, have_pairs):
    """--paired_wobble / --paired_wobble_bias as the feature_dict keys of ProteinMPNN.sample ({} without wobble)."""
    if args.paired_wobble not in (0, 1):
        raise ValueError(f"--paired_wobble is 0 or 1; got {args.paired_wobble}")
    if (args.paired_wobble or args.paired_wobble_bias is not None) and not have_pairs:
        raise ValueError("--paired_wobble / --paired_wobble_bias need --paired_residues or --paired_strands")
    if args.paired_wobble_bias is not None and not args.paired_wobble:
        raise ValueError("--paired_wobble_bias needs --paired_wobble 1")
    if not args.paired_wobble:
        return {}
    return {"paired_wobble": True, "paired_wobble_bias": float(args.paired_wobble_bias or 0.0)}


def main(argv=None):
    args = apply_mode_defaults(build_parser().parse_args(argv))
    if args.conditional_classes not in (0, 1):
        raise ValueError(f"--conditional_classes is 0 or 1; got {args.conditional_classes}")
    if args.conditional_classes and not args.conditional_probs_only:
        raise ValueError("--conditional_classes 1 goes with --conditional_probs_only 1")
    if args.score_tied not in (0, 1):
        raise ValueError(f"--score_tied is 0 or 1; got {args.score_tied}")
    if args.score_tied and (not args.score_fasta or args.conditional_probs_only):
        raise ValueError("--score_tied 1 goes with --score_fasta FILE (and not with --conditional_probs_only)")
    if args.score_fasta and not args.score_tied and (args.multi_state or args.paired_residues or args.paired_strands or args.paired_wobble or
                             args.conditional_probs_only):
        raise ValueError("--score_fasta scores given sequences on one structure: it does not go with --multi_state, --paired_residues, "
                         "--paired_strands, --paired_wobble or --conditional_probs_only")
    if args.state_contexts not in (0, 1):
        raise ValueError(f"--state_contexts is 0 or 1; got {args.state_contexts}")
    if args.state_contexts and not args.multi_state:
        raise ValueError("--state_contexts 1 reads the MODELs of the file as states: it needs --multi_state 1")
    if args.state_contexts and args.conditional_probs_only:
        raise ValueError("--state_contexts 1 does not go with --conditional_probs_only: conditional_probs() takes no context states")
    if args.mutation_scan not in (0, 1):
        raise ValueError(f"--mutation_scan is 0 or 1; got {args.mutation_scan}")
    if args.mutation_classes not in (0, 1):
        raise ValueError(f"--mutation_classes is 0 or 1; got {args.mutation_classes}")
    if args.mutation_classes and not (args.mutation_scan and args.mutation_tied):
        raise ValueError("--mutation_classes 1 needs --mutation_scan 1 --mutation_tied 1")
    if args.mutation_classes and not (args.paired_residues or args.paired_strands or args.symmetry_residues):
        raise ValueError("--mutation_classes 1 needs --paired_residues, --paired_strands or --symmetry_residues")
    if args.mutation_classes and (args.multi_state or args.pair_bias_AA):
        raise ValueError("--mutation_classes 1 scans the ties of one backbone: it does not go with --multi_state or --pair_bias_AA")
    if args.mutation_scan and (args.score_fasta or args.conditional_probs_only or (args.paired_wobble and not args.mutation_classes)):
        raise ValueError("--mutation_scan 1 scans one structure: it does not go with --score_fasta, --conditional_probs_only "
                         "or --paired_wobble")
    if args.mutation_scan and args.multi_state and (args.paired_residues or args.paired_strands or args.symmetry_residues or args.pair_bias_AA):
        raise ValueError("--mutation_scan 1 with --multi_state 1 scans backbone states alone: it does not go with --paired_residues, "
                         "--paired_strands, --symmetry_residues or --pair_bias_AA")
    if args.mutation_tied not in (0, 1):
        raise ValueError(f"--mutation_tied is 0 or 1; got {args.mutation_tied}")
    if args.mutation_tied and not args.mutation_classes and not (args.mutation_scan and args.symmetry_residues):
        raise ValueError("--mutation_tied 1 needs --mutation_scan 1 and --symmetry_residues")
    if args.mutation_tied and not args.mutation_classes and (args.multi_state or args.paired_residues or args.paired_strands or args.pair_bias_AA):
        raise ValueError("--mutation_tied 1 scans symmetry groups on one backbone: it does not go with --multi_state, --paired_residues, "
                         "--paired_strands or --pair_bias_AA")
    if args.coordinate_gradients not in (0, 1):
        raise ValueError(f"--coordinate_gradients is 0 or 1; got {args.coordinate_gradients}")
    if args.coordinate_gradients and (args.score_fasta or args.conditional_probs_only or args.multi_state or args.mutation_scan):
        raise ValueError("--coordinate_gradients 1 differentiates one structure's likelihood: it does not go with --score_fasta, "
                         "--conditional_probs_only, --multi_state or --mutation_scan")
    if (args.forbidden_motifs or args.max_homopolymer) and (args.score_fasta or args.conditional_probs_only or args.mutation_scan
                                                             or args.coordinate_gradients):
        raise ValueError("--forbidden_motifs / --max_homopolymer constrain designs: they do not go with --score_fasta, "
                         "--conditional_probs_only, --mutation_scan or --coordinate_gradients")
    if args.max_homopolymer and not 1 <= args.max_homopolymer <= 7:
        raise ValueError(f"--max_homopolymer is in 1..7; got {args.max_homopolymer}")
    if args.model_type != "na_mpnn":
        print("Choose --model_type flag from currently available models")
        sys.exit()
    seed = args.seed if args.seed else int(np.random.randint(0, high=99999, size=1, dtype=int)[0])
    torch.manual_seed(seed); random.seed(seed); np.random.seed(seed)
    device = torch.device(args.device)
    shared = bool(args.na_shared_tokens)
    rti = spec.restype_to_int(shared)
    alphabet = [spec.RESTYPE_3TO1[r] for r in spec.RESTYPES]
    str_to_int = {spec.RESTYPE_3TO1[k]: v for k, v in rti.items()}
    int_to_str = {}
    for k, v in str_to_int.items():
        int_to_str.setdefault(v, k)
    dna_to_rna = {spec.RESTYPE_3TO1[d]: spec.RESTYPE_3TO1[r] for d, r in
                  (("DA", "A"), ("DC", "C"), ("DG", "G"), ("DT", "U"), ("DX", "RX"))} if shared else {}

    k_neighbors = args.k_neighbors if args.k_neighbors is not None else 32          # run.py:176-182
    model = ProteinMPNN(node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3, num_decoder_layers=3,
                        k_neighbors=k_neighbors, model_type=args.model_type, vocab=33, num_letters=33,
                        atom_dict=spec.atom_dict(), restype_to_int=rti, polytype_to_int=spec.polytype_to_int())
    if args.random_init_seed is not None:
        ckpt_name = f"random_init_seed_{args.random_init_seed}"
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(args.random_init_seed).items()})
    else:
        ckpt_name = args.checkpoint_na_mpnn
        model.load_state_dict(torch.load(ckpt_name, map_location="cpu", weights_only=False)["model_state_dict"])
    model.to(device).eval()

    bias_AA = torch.zeros(33, device=device)
    if args.bias_AA:
        for item in args.bias_AA.split(","):
            aa, val = item.split(":")
            bias_AA[str_to_int[aa]] = float(val)
    pair_bias_AA = None
    if args.pair_bias_AA:                                                           # run.py:215-223
        pair_bias_AA = torch.zeros(33, 33, device=device)
        for item in args.pair_bias_AA.split(","):
            pair, val = item.split(":")
            pair_bias_AA[str_to_int[pair[0]], str_to_int[pair[1]]] = float(val)
    omit_list = args.omit_AA + ("bdhuy" if shared else "")
    omit_AA = torch.tensor([float(c in omit_list) for c in alphabet], device=device)

    base = args.out_folder if args.out_folder.endswith("/") else args.out_folder + "/"
    if args.conditional_tied and not args.conditional_probs_only:
        raise ValueError("--conditional_tied 1 goes with --conditional_probs_only 1")
    if args.conditional_probs_only:
        os.makedirs(base + "conditional_probs", exist_ok=True)
        args.output_pdbs = args.output_sequences = args.output_specificity = 0
    elif args.score_fasta:
        os.makedirs(base + "scores", exist_ok=True)
        args.output_pdbs = args.output_sequences = args.output_specificity = 0
    elif args.mutation_scan:
        os.makedirs(base + "mutations", exist_ok=True)
        args.output_pdbs = args.output_sequences = args.output_specificity = 0
    elif args.coordinate_gradients:
        os.makedirs(base + "gradients", exist_ok=True)
        args.output_pdbs = args.output_sequences = args.output_specificity = 0
    else:
        os.makedirs(base + "seqs", exist_ok=True)
    if args.output_pdbs:
        os.makedirs(base + "backbones", exist_ok=True)
    if args.output_specificity:
        os.makedirs(base + "specificity", exist_ok=True)
    if args.fixed_pos_by_pdb:
        with open(args.fixed_pos_by_pdb) as fh:
            fixed_pos_by_pdb = json.load(fh)
            fixed_pos_by_pdb = {k: (v.split() if isinstance(v, str) else v) for k, v in fixed_pos_by_pdb.items()}
    else:
        fixed_pos_by_pdb = {args.pdb_path: args.fixed_residues.split()}

    for pdb, fixed_residues in fixed_pos_by_pdb.items():
        name = os.path.basename(pdb)
        if name[-4:] in (".pdb", ".cif"):
            name = name[:-4]
        try:
            run_one(args, model, pdb, name, fixed_residues, device, seed, ckpt_name, bias_AA, omit_AA, int_to_str, dna_to_rna,
                    rti, base, pair_bias_AA)
        except Exception as e:                     # run.py:585-617
            if not args.catch_failed_inferences:
                raise
            os.makedirs(base + "failed_inferences", exist_ok=True)
            with open(base + "failed_inferences/" + name + ".txt", "w") as fh:
                fh.write(repr(e))


def run_one(args, model, pdb, name, fixed_residues, device, seed, ckpt_name, bias_AA, omit_AA, int_to_str, dna_to_rna, rti, base,
            pair_bias_AA=None):
    parse = pdbio.parse_states if args.multi_state else pdbio.parse_pdb
    more = {"contexts": True} if args.state_contexts else {}
    P = parse(pdb, chains=list(args.parse_these_chains_only) or None, parse_na_only=bool(args.parse_na_only),
              na_shared_tokens=bool(args.na_shared_tokens),
              load_residues_with_missing_atoms=bool(args.load_residues_with_missing_atoms), **more)
    state_w = None
    if args.multi_state:
        if args.conditional_probs_only and not args.conditional_tied:
            raise ValueError("--conditional_probs_only scores one structure: it does not go with --multi_state (without --conditional_tied 1)")
        X_states, X_m_states = P["X"], P["X_m"]
        P = dict(P, X=X_states[0], X_m=X_m_states[0])       # everything per residue (and the backbones written) comes from state 1
        M = X_states.shape[0]
        state_w = [float(v) for v in args.state_weights.split(",")] if args.state_weights else [1.0 / M] * M
        if len(state_w) != M:
            raise ValueError(f"--state_weights lists {len(state_w)} weights for the {M} models of {pdb}")
    L = len(P["S"])
    encoded = [f"{c}{r}{ic}" for c, r, ic in zip(P["chain_letters"], P["R_idx"].tolist(), P["icodes"])]
    encoded_dict = dict(zip(encoded, range(L)))
    fixed_positions = np.array([int(e not in fixed_residues) for e in encoded], np.int32)
    if args.redesigned_residues:
        red = args.redesigned_residues.split()
        redesigned = np.array([int(e not in red) for e in encoded], np.int32)
    else:
        redesigned = np.zeros(L, np.int32)
    chains = args.chains_to_design.split(",") if isinstance(args.chains_to_design, str) else P["chain_letters"]
    if args.design_na_only:
        chains = [c for c in chains if c in P["na_chain_letters"]]
    chain_mask = np.array([c in chains for c in P["chain_letters"]], np.int32) * fixed_positions * (1 - redesigned)

    if args.symmetry_residues:                                                      # run.py:313-332
        sym_res = [[encoded_dict[t] for t in grp.split(",")] for grp in args.symmetry_residues.split("|")]
        sym_w = ([[float(v) for v in grp.split(",")] for grp in args.symmetry_weights.split("|")] if args.symmetry_weights
                 else [[1.0] * len(grp) for grp in sym_res])
    else:
        sym_res, sym_w = [[]], [[]]

    pairs = parse_pairs(args.paired_residues, args.paired_strands, encoded, list(P["chain_letters"]))
    wobble = wobble_arguments(args, bool(pairs))
    if pairs and args.conditional_probs_only and wobble and not args.conditional_classes:
        raise ValueError("--conditional_probs_only scores base pairs by their Watson-Crick maps: it does not go with --paired_wobble")

    with torch.no_grad():
        fd = pdbio.to_feature_dict(P, chain_mask, device)
        if pairs:
            fd["paired_residues"] = pairs
            fd.update(wobble)
        fd.update({"batch_size": args.batch_size, "temperature": args.temperature,
                   "bias": (-1e8 * omit_AA[None, None, :] + bias_AA).repeat(1, L, 1),
                   "symmetry_residues": sym_res, "symmetry_weights": sym_w})
        if state_w is not None:
            fd["X"] = torch.as_tensor(X_states, dtype=torch.float32, device=device)
            fd["X_m"] = torch.as_tensor(X_m_states, dtype=torch.int32, device=device)
            fd["state_weights"] = state_w
            if args.state_contexts:
                fd["state_S"] = torch.as_tensor(P["state_S"], dtype=torch.int64, device=device)
                fd["state_mask"] = torch.as_tensor(P["state_mask"], dtype=torch.int32, device=device)
            wn = torch.tensor(state_w, device=device)
            wn = wn / wn.sum() if float(wn.sum()) != 0 else torch.full_like(wn, 1.0 / len(state_w))
        if pair_bias_AA is not None:
            members = args.pair_bias_members if args.pair_bias_members != "auto" else ("all" if pairs else "closing")
            fd["pair_terms"] = make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], pair_bias_AA, members)
        if args.forbidden_motifs or args.max_homopolymer:
            designed = (fd["mask"] * fd["chain_mask"])[0] != 0
            polymers = [k for k in ("protein", "dna", "rna") if bool(((fd[k + "_mask"][0] != 0) & designed).any())]
            fd["forbidden_motifs"] = parse_forbidden_motifs(args.forbidden_motifs, args.max_homopolymer, rti, polymers)
        if args.conditional_probs_only:
            # one deterministic leave-one-out profile instead of draws: the decoding order's noise is the only random input
            fd["randn"] = torch.randn(1, L, device=device)
            if args.conditional_classes:
                out = model.conditional_probs(fd, tied=bool(args.conditional_tied), classes=True)
            else:
                out = model.conditional_probs(fd, tied=bool(args.conditional_tied))
            # with --paired_residues / --paired_strands the rows of paired residues hold the PAIR's conditional (each in its member's
            # alphabet) and `pairs` [n, 2] lists the pairs that were tied; without pair flags the file keeps its keys
            # with --conditional_tied 1 the rows of every tied group hold the GROUP's conditional; `groups` / `group_log_probs` name them
            extra = {"pairs": out["pairs"].cpu().numpy()} if pairs and "pairs" in out else {}
            if "groups" in out:
                extra.update(groups=out["groups"].cpu().numpy(), group_log_probs=out["group_log_probs"].cpu().numpy())
            # with --conditional_classes 1 the class rows of the tied pairs / groups
            extra.update({k: out[k].cpu().numpy() for k in ("pair_class_log_probs", "group_class_log_probs") if k in out})
            np.savez(os.path.join(base, "conditional_probs", name + ".npz"),
                     log_probs=out["log_probs"][0].cpu().numpy(), S=P["S"].astype(np.int64), mask=P["mask"],
                     chain_mask=chain_mask, chain_labels=P["chain_labels"], decoding_order=out["decoding_order"].cpu().numpy(),
                     encoded_residues=encoded, **extra)
            return
        if args.score_fasta:
            # the library of the file on this structure: one decoding order (its noise is the only random input), every sequence scored
            # as it stands
            fd["randn"] = torch.randn(1, L, device=device)
            names, seqs = read_fasta(args.score_fasta)
            str_to_int = {}
            for t, ch in int_to_str.items():
                str_to_int[ch] = t
                if ch in dna_to_rna:
                    str_to_int[dna_to_rna[ch]] = t
            lib = fasta_tokens(names, seqs, P["S"], list(P["chain_letters"]), (P["mask"] * chain_mask) != 0, str_to_int, encoded)
            if args.score_tied:
                # the joint log-likelihood under the ties of the flags: a unit (a tied group, or a residue alone) counts once
                out = model.score_tied(fd, torch.from_numpy(lib).to(device))
                np.savez(os.path.join(base, "scores", name + ".npz"), token_log_probs=out["token_log_probs"].cpu().numpy(),
                         leader=out["leader"].cpu().numpy(), log_likelihood=out["log_likelihood"].cpu().numpy(),
                         member_log_probs=out["member_log_probs"].cpu().numpy(), consistent=out["consistent"].cpu().numpy(),
                         state_weights=np.asarray(state_w if state_w is not None else [1.0], np.float32), S=lib,
                         decoding_order=out["decoding_order"].cpu().numpy(), chunks=out["chunks"],
                         **({"state_log_likelihood": out["state_log_likelihood"].cpu().numpy()} if "state_log_likelihood" in out else {}))
                return
            out = model.score_sequences(fd, torch.from_numpy(lib).to(device))
            np.savez(os.path.join(base, "scores", name + ".npz"), token_log_probs=out["token_log_probs"].cpu().numpy(),
                     loss=out["loss"].cpu().numpy(), sequences=lib, mask=P["mask"], chain_mask=chain_mask,
                     decoding_order=out["decoding_order"].cpu().numpy(), seed=seed)
            return
        if args.mutation_scan:
            # the saturation scan of the designable residues under one decoding order (its noise is the only random input); a paired
            # residue is mutated with its partner and listed once, under the pair's first member
            fd["randn"] = torch.randn(1, L, device=device)
            if args.mutation_classes:
                out = model.score_mutations(fd, pairs=bool(pairs), tied=True, classes=True)
            else:
                out = model.score_mutations(fd, pairs=bool(pairs), tied=bool(args.mutation_tied))
            scanned = out["positions"].cpu().numpy()
            states = {k: out[k].cpu().numpy() for k in ("state_delta", "state_weights", "base_state_log_likelihood", "leader", "unit_offsets",
                                                        "unit_residue", "unit_log_prob", "classes", "class_tokens")
                      if k in out and (args.mutation_tied or k.startswith(("state", "base")))}
            np.savez(os.path.join(base, "mutations", name + ".npz"), residues=np.array([encoded[i] for i in scanned]),
                     tokens=np.array([int_to_str.get(int(t), "?") for t in out["tokens"].tolist()]), delta=out["delta"].cpu().numpy(),
                     base_loss=out["base_loss"].cpu().numpy(), wild_type_token=np.asarray(P["S"])[scanned],
                     site_rows=(out["site_rows"].cpu().numpy() if out["site_rows"] is not None else np.zeros((0, 3), np.int32)), **states)
            return
        if args.coordinate_gradients:
            # per-atom saliency of the structure's own sequence under one decoding order (its noise is the only random input)
            if args.multi_state:
                raise ValueError("--coordinate_gradients differentiates one structure: it does not go with --multi_state")
            fd["randn"] = torch.randn(1, L, device=device)
            out = model.coordinate_gradients(fd)
            np.savez(os.path.join(base, "gradients", name + ".npz"), dX=out["dX"][0].cpu().numpy(),
                     residue_norm=out["residue_norm"][0].cpu().numpy(), loss=float(out["loss"]), encoded_residues=encoded,
                     mask=P["mask"], chain_mask=chain_mask, decoding_randn=fd["randn"][0].cpu().numpy())
            return
        S_l, lp_l, sp_l, loss_l, lpr_l, Ss_l, hits_l = [], [], [], [], [], [], []
        cmask = (fd["mask"] * fd["chain_mask"]).float()
        forced = np.load(args.forced_draws_npz) if args.forced_draws_npz else None
        model.sample_check_walk = True      # verify the persistent level walk's barriers per design call; falls back to per-level launches
        for ib in range(args.number_of_batches):
            fd["randn"] = torch.randn(args.batch_size, L, device=device)
            if forced is not None:
                rows = slice(ib * args.batch_size, (ib + 1) * args.batch_size)
                fd["randn"] = torch.from_numpy(forced["randn"][rows]).to(device)
                fd["S_forced"] = torch.from_numpy(forced["S_forced"][rows]).to(device)
            out = model.sample(fd)
            onehot = torch.nn.functional.one_hot(out["S"], 33)
            if state_w is None:
                lpr = -(onehot * out["log_probs"]).sum(-1)                               # get_score, data_utils.py:36-52
            else:                                       # log_probs [bs, M, L, V]: the weight-averaged per-state log-prob of the drawn tokens
                lpr = (-(onehot[:, None] * out["log_probs"]).sum(-1) * wn[None, :, None]).sum(1)
            lpr_l.append(lpr)
            loss_l.append((lpr * cmask).sum(-1) / (cmask.sum(-1) + 1e-8))
            S_l.append(out["S"]); lp_l.append(out["log_probs"]); sp_l.append(out["sampling_probs"])
            if "S_states" in out:
                Ss_l.append(out["S_states"])
            if "motif_hits" in out:
                hits_l.append(out["motif_hits"])
        S_stack, sp_stack, loss_stack, lpr_stack = torch.cat(S_l), torch.cat(sp_l), torch.cat(loss_l), torch.cat(lpr_l)
        rec = ((fd["S"][:1] == S_stack) * cmask).sum(-1) / cmask.sum(-1)               # get_seq_rec, data_utils.py:18-30

    rna_flag = P["rna_mask_for_token_conversion"]
    entries = ['>{}, T={}, seed={}, num_res={}, batch_size={}, number_of_batches={}, model_path={}\n{}'.format(
        name, args.temperature, seed, (fd["mask"] * fd["chain_mask"]).sum().cpu().numpy(), args.batch_size, args.number_of_batches, ckpt_name,
        seq_string(P["S"], rna_flag, int_to_str, dna_to_rna, P["chain_letters"]))]
    motif_hits = torch.cat(hits_l).cpu().tolist() if hits_l else None
    for ix in range(S_stack.shape[0]):
        conf = np.format_float_positional(np.exp(-loss_stack[ix].cpu().numpy()), unique=False, precision=4)
        srec = np.format_float_positional(rec[ix].cpu().numpy(), unique=False, precision=4)
        if motif_hits is not None:                                                    # (with --forbidden_motifs / --max_homopolymer only)
            srec += f" motif_hits={motif_hits[ix]}"
        entries.append('>{}, id={}, T={}, seed={}, overall_confidence={} seq_rec={}\n{}'.format(
            name, ix if args.zero_indexed else ix + 1, args.temperature, seed, conf, srec,
            seq_string(S_stack[ix].cpu().numpy(), rna_flag, int_to_str, dna_to_rna, P["chain_letters"])))
        if args.output_pdbs:                                                          # run.py:475-491
            one_to_three = {v: k for k, v in spec.RESTYPE_3TO1.items()}
            chars = [dna_to_rna.get(int_to_str[int(t)], int_to_str[int(t)]) if rna_flag[i] == 1 else int_to_str[int(t)]
                     for i, t in enumerate(S_stack[ix].cpu().numpy())]
            lp_res = lpr_stack[ix].cpu().numpy()
            pdbio.write_backbone_pdb(base + "backbones/" + name + "_" + str(ix if args.zero_indexed else ix + 1) + ".pdb" + args.file_ending,
                                     P, [one_to_three[c] for c in chars], np.exp(-lp_res) * (lp_res > 0.01).astype(np.float32))
    if args.output_sequences:
        with open(base + "seqs/" + name + ".fa" + args.file_ending, "w") as fh:
            fh.write("\n".join(entries))
    if args.output_specificity:
        np.savez(os.path.join(base, "specificity", name + ".npz"),
                 predicted_ppm=np.mean(sp_stack.cpu().numpy().astype(np.float64), axis=0),
                 true_sequence=P["S"].astype(np.int64), chain_labels=P["chain_labels"], mask=P["mask"],
                 protein_mask=P["protein_mask"], dna_mask=P["dna_mask"], rna_mask=P["rna_mask"],
                 encoded_residues=encoded, encoded_residues_dict=encoded_dict, restype_to_int=rti)
    if args.save_stats:
        os.makedirs(base + "stats", exist_ok=True)
        stats = {"generated_sequences": S_stack.cpu(), "sampling_probs": sp_stack.cpu(), "log_probs": torch.cat(lp_l).cpu(),
                 "native_sequence": fd["S"][0].cpu(), "mask": fd["mask"][0].cpu(), "chain_mask": fd["chain_mask"][0].cpu(),
                 "seed": seed, "temperature": args.temperature}
        if Ss_l:                                        # context states: the token every state's copy holds [n, M, L]
            stats["S_states"] = torch.cat(Ss_l).cpu()
        torch.save(stats, base + "stats/" + name + ".pt")


if __name__ == "__main__":
    main()
