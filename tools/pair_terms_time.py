"""Time the compact pair terms — ProteinMPNN.sample() with feature_dict["pair_terms"] — on cuda:0:
  1. a sequence-neighbour bias (--pair_bias_AA's shape) on an L-residue protein: the compact key against the dense pair_bias tensor
     [1, L, 33, L, 33] it stands for (kept resident: its 4.36 GB at L = 1000 are built once) and against the unbiased call;
  2. base-paired designs (the shapes of tools/paired_time.py: a protein with a short duplex, a long duplex) with the pair terms, every
     member counted, against the same paired call without them — the combination the dense key refuses.
Synthetic backbones (synth.make_complex); all calls start from coordinates, in split-bf16; they are alternated in one process,
synchronised, and reported as medians with their [min, max] spread after warm-up.  The host set-up of a key (building it from the
residue numbering; for the dense key make_pair_bias and the scan pair_bias_dependencies, which sample() repeats on every call) is
timed apart from the calls.

    python tools/pair_terms_time.py [--reps 7] [--plain 1000x48x1] [--paired 300x20x32x1,0x150x48x8] [--no-dense]
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from na_mpnn_amd import cli, spec, synth
from na_mpnn_amd.model import ProteinMPNN, pair_bias_dependencies
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
torch.manual_seed(0)                                              # (the decoding orders, hence the level counts, of every run)
w = synth.make_weights(0)
RTI = spec.restype_to_int()


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=RTI,
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()}); return m.to(dev).eval()


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(calls, reps):
    for f in calls.values():
        f(); f()                                                    # warm-up: weights packed, allocator warm
    t = {name: [] for name in calls}
    for _ in range(reps):                                           # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f)[0])
    med = {name: float(np.median(v)) for name, v in t.items()}
    txt = "  ".join(f"{name} {med[name]:.2f} ms [{min(v):.2f}, {max(v):.2f}]" for name, v in t.items())
    return t, med, txt


def pair_table(pairs):
    AA = torch.zeros(33, 33)
    for a, b, v in pairs:
        AA[RTI[a], RTI[b]] = v
    return AA


def steps(S, fd, toks):
    """Adjacent residues of one chain that both hold a token of `toks`, over all samples."""
    adj = (fd["chain_labels"][0, 1:] == fd["chain_labels"][0, :-1]) & (fd["R_idx"][0, 1:] - fd["R_idx"][0, :-1] == 1)
    t = torch.tensor(toks, device=S.device)
    return int((torch.isin(S[:, :-1], t) & torch.isin(S[:, 1:], t) & adj).sum())


reps = int(arg("--reps", "7"))
for size in filter(None, arg("--plain", "1000x48x1").split(",")):
    L, K, bs = map(int, size.split("x"))
    m = model(K)
    cx = synth.make_complex(seed=3, n=L, n_chains=3, frac_protein=1.0, frac_dna=0.0)
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=bs, temperature=0.1, symmetry_residues=[[]], symmetry_weights=[[]], bias=torch.zeros(1, L, 33, device=dev),
              randn=torch.randn(bs, L, device=dev))
    AA = pair_table([("LYS", "LYS", -10.0), ("LYS", "GLU", -10.0), ("GLY", "GLY", -10.0)]).to(dev)
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA)
    t_compact = float(np.median([timed(lambda: cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA))[0] for _ in range(3)]))
    calls = {"compact": lambda: m.sample(dict(fd, pair_terms=pt)), "unbiased": lambda: m.sample(fd)}
    setup = f"host set-up: make_pair_terms {t_compact:.2f} ms"
    same = "not compared (--no-dense)"
    if "--no-dense" not in sys.argv:
        t_dense, pb = timed(lambda: cli.make_pair_bias(fd["chain_labels"][0], fd["R_idx"][0], AA))
        t_deps = float(np.median([timed(lambda: pair_bias_dependencies(pb))[0] for _ in range(3)]))
        calls["dense"] = lambda: m.sample(dict(fd, pair_bias=pb))
        setup += (f"; dense: make_pair_bias {t_dense:.1f} ms ({pb.numel() * 4 / 1e9:.2f} GB) + pair_bias_dependencies {t_deps:.1f} ms "
                  f"(the scan is part of every dense call below)")
        torch.manual_seed(1); a = calls["compact"]()
        torch.manual_seed(1); b = calls["dense"]()
        same = bool(torch.equal(a["S"], b["S"]) and torch.equal(a["log_probs"], b["log_probs"]) and torch.equal(a["sampling_probs"], b["sampling_probs"]))
    t, med, txt = alternate(calls, reps)
    print(f"L={L} K={K} batch_size={bs} sequence-neighbour bias: {txt}  ({setup}; compact == dense bit for bit: {same}; {reps} calls each, "
          f"from coordinates)", flush=True)
    if "dense" in med:
        spread = max(max(t[n]) - min(t[n]) for n in ("compact", "dense"))
        holds = med["compact"] <= med["dense"] + spread
        print(f"  expectation 'the compact call is not slower than the dense call beyond the min-max spread': "
              f"{'holds' if holds else 'MISSED'} (compact - dense {med['compact'] - med['dense']:+.2f} ms, spread {spread:.2f} ms; "
              f"compact - unbiased {med['compact'] - med['unbiased']:+.2f} ms)", flush=True)
    del calls
    pb = None
    torch.cuda.empty_cache()

for size in filter(None, arg("--paired", "300x20x32x1,0x150x48x8").split(",")):
    n_prot, n_strand, K, bs = map(int, size.split("x"))
    m = model(K)
    L = n_prot + 2 * n_strand
    cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=n_prot / L, frac_dna=2 * n_strand / L)
    cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
    for c in range(int(cx["chain_labels"].max()) + 1):
        sel = cx["chain_labels"] == c
        cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=bs, temperature=0.1, symmetry_residues=[[]], symmetry_weights=[[]], bias=torch.zeros(1, L, 33, device=dev),
              randn=torch.randn(bs, L, device=dev), paired_residues=[(n_prot + k, L - 1 - k) for k in range(n_strand)])
    G = [RTI["DG"], RTI["G"]]
    AA = pair_table([(a, b, -1e9) for a in ("DG", "G") for b in ("DG", "G")])
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA, "all")
    t_compact = float(np.median([timed(lambda: cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA, "all"))[0] for _ in range(3)]))
    calls = {"paired + pair terms": lambda: m.sample(dict(fd, pair_terms=pt)), "paired": lambda: m.sample(fd)}
    torch.manual_seed(1); a = calls["paired + pair terms"]()
    torch.manual_seed(1); b = calls["paired"]()
    t, med, txt = alternate(calls, reps)
    spread = max(max(v) - min(v) for v in t.values())
    print(f"protein={n_prot} duplex=2x{n_strand} K={K} batch_size={bs}: {txt}  (with - without {med['paired + pair terms'] - med['paired']:+.2f} ms, "
          f"larger min-max spread of the two {spread:.2f} ms; host set-up: make_pair_terms {t_compact:.2f} ms; {int(a['levels'])} levels / "
          f"{a['work_items']} work items with (host plan), {int(b['levels'])} / {b['work_items']} without (device plan); G G steps drawn: "
          f"{steps(a['S'], fd, G)} with, {steps(b['S'], fd, G)} without; {reps} calls each, from coordinates)", flush=True)
