"""Time the forbidden motifs — ProteinMPNN.sample() with feature_dict["forbidden_motifs"] — on cuda:0, three shapes, each three ways:
without motifs, with --max_homopolymer 3 on the designed polymers (the runs of four of their residue types), and with the pair terms
gg: -1e9 (tools/pair_terms_time.py) for comparison:
  1. a 300-residue protein with a 2 x 20 DNA duplex, K = 32, batch_size 1, base-paired;
  2. a 2 x 150 RNA duplex, K = 48, batch_size 8, base-paired with G-U wobble;
  3. a 1000-residue protein, K = 48, batch_size 1, no tie.
Synthetic backbones (synth.make_complex); all calls start from coordinates, in split-bf16; they are alternated in one process,
synchronised, and reported as medians with their [min, max] spread after warm-up, with the levels and work items of each call beside
them: the windows are dependencies of the level plan, and so are the pair terms' partners.

    python tools/motifs_time.py [--reps 7] [--shapes 300x20x32x1xdna,0x150x48x8xrna,1000x0x48x1xdna]   (protein x strand x K x batch x polymer)
    --parent DIR    a checkout of the parent commit with its library built: the calls WITHOUT motifs of every shape and the cfg1 design
                    call (97 residues, K = 32, batch_size 1, forced draws) run in child processes, this tree and DIR in turn (two
                    rounds of --reps calls each); per call this build's median - the parent's beside the larger min-max spread of the
                    two, and whether the results are the parent's bits.
"""
import os, subprocess, sys, tempfile, time
import numpy as np, torch


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, arg("--package-root", HERE))          # (a child of --parent imports the parent's package)
from na_mpnn_amd import cli, spec, synth                 # noqa: E402
from na_mpnn_amd.model import ProteinMPNN                # noqa: E402
torch.set_grad_enabled(False)
dev = "cuda:0"
RTI = spec.restype_to_int()
reps = int(arg("--reps", "7"))
shapes = arg("--shapes", "300x20x32x1xdna,0x150x48x8xrna,1000x0x48x1xdna").split(",")


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=RTI,
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in synth.make_weights(0).items()})
    return m.to(dev).eval()


def inputs(shape):
    """-> (K, the feature_dict without motifs, the polymers designed)."""
    n_prot, n_strand, K, bs, na = shape.split("x")
    n_prot, n_strand, K, bs = int(n_prot), int(n_strand), int(K), int(bs)
    L = n_prot + 2 * n_strand
    frac_na = 2 * n_strand / L
    cx = synth.make_complex(seed=3, n=L, n_chains=1 if n_strand else 3, frac_protein=n_prot / L, frac_dna=frac_na if na == "dna" else 0.0)
    if n_strand:
        cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
        for c in range(int(cx["chain_labels"].max()) + 1):
            sel = cx["chain_labels"] == c
            cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=bs, temperature=0.1, symmetry_residues=[[]], symmetry_weights=[[]], bias=torch.zeros(1, L, 33, device=dev),
              randn=torch.randn(bs, L, generator=torch.Generator().manual_seed(L)).to(dev))
    if n_strand:
        fd["paired_residues"] = [(n_prot + k, L - 1 - k) for k in range(n_strand)]
        if na == "rna":
            fd.update(paired_wobble=True, paired_wobble_bias=0.0)
    polymers = (["protein"] if n_prot else []) + ([na] if n_strand else [])
    return K, fd, polymers


def cfg1_inputs():
    cx = synth.make_complex(seed=3, n=97, n_chains=1, frac_protein=0.0, frac_dna=0.0)
    fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx.items()}
    fd.update(batch_size=1, temperature=0.1, bias=torch.zeros(1, 97, 33, device=dev), symmetry_residues=[[]], symmetry_weights=[[]],
              S_forced=fd["S"].long())                                 # (forced draws: two builds' results can be compared bit for bit)
    return fd


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(calls):
    for f in calls.values():
        f(); f()                                                        # warm-up: weights packed, workspaces allocated
    t = {name: [] for name in calls}
    for _ in range(reps):                                               # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    return t


def fmt(v):
    return f"{float(np.median(v)):.3f} ms [{min(v):.3f}, {max(v):.3f}]"


if "--child" in sys.argv:
    # one build's share of --parent: the call without motifs of every shape and the cfg1 design call, timed, with their results
    out = {}
    for shape in shapes:
        K, fd, _ = inputs(shape)
        m = model(K)
        u = torch.rand(fd["batch_size"], fd["S"].shape[1], generator=torch.Generator().manual_seed(1)).to(dev)
        res = m._sample(fd, True, uniform=u)
        out["without motifs " + shape] = (measure({"x": lambda: m.sample(fd)})["x"], {k: res[k].cpu() for k in ("S", "log_probs", "sampling_probs")})
    m, fd1 = model(32), cfg1_inputs()
    res = m.sample(fd1)
    out["cfg1 design call"] = (measure({"x": lambda: m.sample(fd1)})["x"], {k: res[k].cpu() for k in ("S", "log_probs")})
    torch.save(out, arg("--dump", ""))
    sys.exit(0)

if arg("--parent", ""):
    roots = {"this": HERE, "parent": os.path.abspath(arg("--parent", ""))}
    got = {k: {} for k in roots}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(2):
            for who, root in roots.items():                             # (a fresh child each: this process never opens the GPU)
                dump = os.path.join(tmp, f"{who}{rnd}.pt")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--package-root", root, "--dump", dump, "--reps", str(reps),
                                "--shapes", ",".join(shapes)], check=True, cwd=root, timeout=900)
                for name, (ts, res) in torch.load(dump, weights_only=False).items():
                    slot = got[who].setdefault(name, ([], res))
                    slot[0].extend(ts)
                    assert all(torch.equal(slot[1][k], res[k]) for k in res), (who, name, "differs between two processes of one build")
    for name in got["this"]:
        a, b = got["this"][name], got["parent"][name]
        same = all(torch.equal(a[1][k], b[1][k]) for k in a[1])
        spread = max(max(a[0]) - min(a[0]), max(b[0]) - min(b[0]))
        d = float(np.median(a[0]) - np.median(b[0]))
        print(f"parent check: {name} {fmt(a[0])}, parent {fmt(b[0])}: this - parent {d:+.3f} ms (larger min-max spread of the two "
              f"{spread:.3f} ms: {'within' if abs(d) <= spread else 'BEYOND'} it), the parent's bits: {same}; 2 x {reps} calls each in "
              "alternated processes, from coordinates", flush=True)
    sys.exit(0)

for shape in shapes:
    K, fd, polymers = inputs(shape)
    m = model(K)
    L, bs = fd["S"].shape[1], fd["batch_size"]
    motifs = cli.parse_forbidden_motifs("", 3, RTI, polymers)
    G = [(a, b, -1e9) for a in ("DG", "G") for b in ("DG", "G")] if "paired_residues" in fd else [("GLY", "GLY", -1e9)]
    AA = torch.zeros(33, 33)
    for a, b, v in G:
        AA[RTI[a], RTI[b]] = v
    pt = cli.make_pair_terms(fd["chain_labels"][0], fd["R_idx"][0], AA, "all" if "paired_residues" in fd else "closing")
    forms = {"without": fd, "max_homopolymer 3": dict(fd, forbidden_motifs=motifs), "gg pair terms": dict(fd, pair_terms=pt)}
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(1)).to(dev)
    first = {name: m._sample(f, True, uniform=u) for name, f in forms.items()}
    plan = "; ".join(f"{name}: {int(o['levels'])} levels / {o['work_items']} work items" for name, o in first.items())
    t = measure({name: (lambda f=f: m.sample(f)) for name, f in forms.items()})
    med = {name: float(np.median(v)) for name, v in t.items()}
    spread = max(max(t[n]) - min(t[n]) for n in ("max_homopolymer 3", "gg pair terms"))
    d = med["max_homopolymer 3"] - med["gg pair terms"]
    print(f"{shape} (L={L} K={K} batch_size={bs}, {len(motifs)} motifs of 4): " + "  ".join(f"{name} {fmt(v)}" for name, v in t.items())
          + f"  ({plan}; motif_hits with the key {int(first['max_homopolymer 3']['motif_hits'].sum())}; {reps} calls each, from coordinates)", flush=True)
    print(f"  motifs - gg pair terms {d:+.3f} ms (larger min-max spread of the two {spread:.3f} ms: {'within' if abs(d) <= spread else 'BEYOND'} it); "
          f"motifs - without {med['max_homopolymer 3'] - med['without']:+.3f} ms, gg pair terms - without {med['gg pair terms'] - med['without']:+.3f} ms",
          flush=True)
