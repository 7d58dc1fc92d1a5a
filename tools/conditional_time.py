"""Time ProteinMPNN.conditional_probs() on cuda:0, alternated synchronised calls in one process, medians [min, max] after warm-up.

Without a tie shape: the cone kernels (namp_decoder_loo) against the dense L-stream form of the same build, beside one score() call.

    python tools/conditional_time.py [--reps 5] [--prec x3,fp32] [--sizes 1000x48,1000x32,300x48,3000x48]
    rocprofv3 --kernel-trace --stats -d <dir> -o loo -- python tools/conditional_time.py --profile 1000x48
        (two warm-up calls and ONE traced steady-state cone call; tools/rocpd_summary.py reads the database, and --launches <db>
         lists the launches of the last call in order: the per-phase times)

With tie shapes: the tied conditionals (namp_loo_pairs / namp_loo_groups / namp_loo_classes + namp_decoder_loo), from coordinates,
in split-bf16 and exact fp32, on synthetic backbones:
  --pairs PROTxSTRANDxK,...       a protein of PROT residues (none for 0) with an RNA duplex of 2 x STRAND residues paired antiparallel:
                                  the plain call, the pair call (tied=False) and the pair call in pair classes (wobble on for every pair);
  --states MxPROTxSTRANDxK,...    M backbone states of such a complex, tied=True: groups of 2 M members and every other residue a group
                                  across the states, in token maps and in pair classes;
  --oligomers CxLxK,...           C chains of L residues tied residue by residue, tied=True, beside the call without groups and (--slow_reps
                                  calls, 0: none) the slow route of the same build with its distance from the cone.
  --parent PATH                   another build of the library (libnamp_hip.so of, say, the parent commit) as a second library of this
                                  process: every cone call also runs on it, and per call the line holds this build's median - its median
                                  beside the larger min-max spread of the two, and whether log_probs are its bits (True / False).

    python tools/conditional_time.py [--reps 7] [--pairs 300x20x32,0x150x48] [--states 4x210x20x48] [--oligomers 3x300x48] [--parent PATH]
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def launches(path, last=16):
    import re, sqlite3
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    ncol = "name" if "name" in cols else "kernel_name"
    rows = db.execute(f"select {ncol}, start, end from kernels order by start").fetchall()[-last:]
    t0 = rows[0][1]
    print("| launch | start us | duration us |\n|---|---:|---:|")
    for name, s, e in rows:
        print(f"| `{re.sub(r'[(<].*', '', name)[:60]}` | {(s - t0) / 1e3:.1f} | {(e - s) / 1e3:.1f} |")


if "--launches" in sys.argv:
    launches(arg("--launches", None), int(arg("--last", "16")))
    sys.exit(0)

from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
w = synth.make_weights(0)


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()}); return m.to(dev).eval()


def fd_of(n):
    cx = synth.make_complex(seed=3, n=n)
    fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx.items()}
    fd["batch_size"] = 1
    return fd


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


if "--profile" in sys.argv:
    n, k = map(int, arg("--profile", "1000x48").split("x"))
    m, fd = model(k), fd_of(n)
    m.message_precision = arg("--prec", "x3")
    for _ in range(3):
        m.conditional_probs(fd, method="cone")
    torch.cuda.synchronize()
    sys.exit(0)

TIE_SHAPES = ("--pairs", "--states", "--oligomers")
if any(k in sys.argv for k in TIE_SHAPES):
    import ctypes
    SHARED = ("S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def duplex_complex(n_prot, n_strand):
        """A protein of n_prot residues (none for 0) with an RNA duplex of 2 x n_strand residues -> (complex, the antiparallel pairs)."""
        L = n_prot + 2 * n_strand
        cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=n_prot / L, frac_dna=0.0)
        cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
        for c in range(int(cx["chain_labels"].max()) + 1):
            sel = cx["chain_labels"] == c
            cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
        return cx, [(n_prot + k, L - 1 - k) for k in range(n_strand)]

    def one_state(cx):
        L = cx["S"].shape[0]
        fd = {k: to_dev(v)[None] for k, v in cx.items()}
        fd.update(batch_size=1, temperature=1.0, bias=torch.zeros(1, L, 33, device=dev), randn=torch.randn(1, L, device=dev))
        return fd

    def states_of(cx, M):
        """M states of a complex: seeded smooth deformations (a few low-frequency sine waves plus jitter)."""
        L = cx["S"].shape[0]
        rng = np.random.default_rng(11)
        X = cx["X"].astype(np.float64)
        Xs, scale = [cx["X"]], max(1.0, float(np.abs(X).max()))
        for _ in range(1, M):
            D = sum(np.sin(X @ (rng.standard_normal(3) * 2.5 / scale) + rng.uniform(0, 6.28))[..., None] * rng.standard_normal(3) * 2.0 for _ in range(3))
            Xs.append(((X + D + 0.15 * rng.standard_normal(X.shape)) * cx["X_m"][:, :, None]).astype(np.float32))
        fd = {k: to_dev(cx[k])[None] for k in SHARED}
        fd.update(X=to_dev(np.stack(Xs)), X_m=to_dev(cx["X_m"])[None].repeat(M, 1, 1), batch_size=1, temperature=1.0,
                  bias=torch.zeros(1, L, 33, device=dev), randn=torch.randn(1, L, device=dev), state_weights=[1.0 / M] * M,
                  symmetry_residues=[[]], symmetry_weights=[[]])
        return fd

    def load_parent(path):
        """Another build as a second library of this process (it shares the packed weights): the same ABI version, and the symbols called."""
        lib = ctypes.CDLL(path)
        for name, (res, args) in hip._PROTOTYPES.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        assert lib.namp_abi_version() == hip.NAMP_ABI_VERSION
        missing = [n for n in hip._PROTOTYPES if n.startswith(("namp_loo_", "namp_decoder_loo", "namp_featurize", "namp_encoder_fwd")) and not hasattr(lib, n)]
        assert not missing, missing
        return lib

    def measure(calls, reps, slow=(), slow_reps=3):
        """Medians of `reps` alternated synchronised calls per form (the forms named in `slow`: slow_reps) -> {name: (median, min, max)}."""
        for f in calls.values():
            f(); f()                                                    # warm-up: weights packed, workspaces allocated, tables cached
        t = {name: [] for name in calls}
        for r in range(reps):                                           # alternated: a drift of the clocks hits every form alike
            for name, f in calls.items():
                if name not in slow or r < slow_reps:
                    t[name].append(timed(f))
        return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}

    reps, slow_reps = int(arg("--reps", "7")), int(arg("--slow_reps", "3"))
    this_lib = hip.lib()
    parent_lib = load_parent(arg("--parent", "")) if arg("--parent", "") else None

    def on_parent(f):
        def call():
            hip._lib = parent_lib
            try:
                return f()
            finally:
                hip._lib = this_lib
        return call

    for kind, size in [(k[2:], s) for k in TIE_SHAPES for s in arg(k, "").split(",") if s]:
        dims = list(map(int, size.split("x")))
        K, slow = dims[-1], None
        if kind == "oligomers":
            C, L, _ = dims
            plain = one_state(synth.make_complex(seed=3, n=C * L, n_chains=C))
            ties = dict(plain, symmetry_residues=[[i + c * L for c in range(C)] for i in range(L)], symmetry_weights=[[1.0 / C] * C] * L)
            forms = lambda m: {"plain": lambda: m.conditional_probs(plain), "group": lambda: m.conditional_probs(ties, tied=True)}
            slow = lambda m: m.conditional_probs(ties, method="dense", tied=True)
        else:
            cx, pairs = duplex_complex(*dims[-3:-1])
            tied = kind == "states"
            plain = states_of(cx, dims[0]) if tied else one_state(cx)
            ties = dict(plain, paired_residues=pairs)
            wobble = dict(ties, paired_wobble=True, paired_wobble_bias=0.0)
            name = "group" if tied else "pair"
            forms = lambda m: {"plain": lambda: m.conditional_probs(plain, tied=tied), name: lambda: m.conditional_probs(ties, tied=tied),
                               name + " in classes": lambda: m.conditional_probs(wobble, tied=tied, classes=True)}
        for prec in ("x3", "fp32"):
            m = model(K)
            m.message_precision = prec
            calls = forms(m)
            names = list(calls)
            out = calls[names[-1]]()
            line = f"{kind} {size} {prec}: "
            if parent_lib is not None:
                same = {n: bool(torch.equal(on_parent(calls[n])()["log_probs"], calls[n]()["log_probs"])) for n in names}
                calls.update({n + ", parent": on_parent(calls[n]) for n in names})
            if slow is not None and slow_reps:
                calls["slow route"] = lambda: slow(m)
                d_route = float((out["log_probs"] - calls["slow route"]()["log_probs"]).abs().max())
            t = measure(calls, reps, slow=("slow route",), slow_reps=slow_reps)
            line += "  ".join(f"{n} {md:.2f} ms [{lo:.2f}, {hi:.2f}]" for n, (md, lo, hi) in t.items())
            if parent_lib is not None:
                for n in names:
                    a, b = t[n], t[n + ", parent"]
                    line += (f"; {n} - parent {a[0] - b[0]:+.3f} ms (larger min-max spread of the two {max(a[2] - a[1], b[2] - b[1]):.3f} ms), "
                             f"the parent's bits: {same[n]}")
            if "slow route" in t:
                line += f"; slow route / cone {t['slow route'][0] / t[names[-1]][0]:.0f}x, max|dlogp| {d_route:.2e}"
            index = out.get("groups", out.get("pairs"))
            print(line + f"; {index.shape[0]} tied, up to {index.shape[1]} members; cone items {out['cone_items'].tolist()}; {reps} calls each, "
                  "from coordinates", flush=True)
    sys.exit(0)

reps = int(arg("--reps", "5"))
for prec in arg("--prec", "x3,fp32").split(","):
    for size in arg("--sizes", "1000x48,1000x32,300x48,3000x48").split(","):
        n, k = map(int, size.split("x"))
        m, fd = model(k), fd_of(n)
        m.message_precision = prec
        calls = {"cone": lambda: m.conditional_probs(fd, method="cone"), "dense": lambda: m.conditional_probs(fd, method="dense"),
                 "score": lambda: m.score(fd)}
        for f in calls.values():
            f()                                                     # warm-up: weights packed, workspaces allocated
        t = {name: [] for name in calls}
        for _ in range(reps):                                       # alternated: a drift of the clocks hits every method alike
            for name, f in calls.items():
                t[name].append(timed(f))
        med = {name: float(np.median(v)) for name, v in t.items()}
        spread = {name: (min(v), max(v)) for name, v in t.items()}
        ws = hip.lib().namp_loo_workspace_bytes(1, n, min(k, n), 3) / 2 ** 20
        print(f"N={n} K={k} {prec}: cone {med['cone']:.2f} ms [{spread['cone'][0]:.2f}, {spread['cone'][1]:.2f}]  "
              f"dense {med['dense']:.1f} ms [{spread['dense'][0]:.1f}, {spread['dense'][1]:.1f}]  ratio {med['dense'] / med['cone']:.1f}x  "
              f"score {med['score']:.2f} ms  (cone / score {med['cone'] / med['score']:.1f}x; cone workspace {ws:.0f} MiB; {reps} calls each, "
              f"from coordinates)", flush=True)
