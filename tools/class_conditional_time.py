"""Time the pair-class conditionals — ProteinMPNN.conditional_probs(classes=True): base pairs scored in pair classes (G-U wobble) on
the cone kernels (namp_loo_classes + namp_decoder_loo) — on cuda:0.  Per shape and evaluation (split-bf16, exact fp32):
  the classes call (paired_wobble on for every pair), the canonical call of this build (the same pairs, classes=False), the call
  without pairs, and the canonical and the plain call on the parent commit's build of the library (--parent /path/to/libnamp_hip.so:
  a second library in the same process that shares the packed weights; the ABI is the same), with
  (a) canonical / plain of this build - the parent's, beside the larger min-max spread of the two, and whether the rows are the parent's bits;
  (b) classes - canonical of this build, beside that spread (only the combine launch and a larger input section differ).
Shapes: --sizes PROTxSTRANDxK: a protein of PROT residues (none for 0) with an RNA duplex of 2 x STRAND residues paired antiparallel,
tied=False; --states MxPROTxSTRANDxK: M backbone states of such a complex, tied=True (groups of 2 M members, every other residue a
group across the states).  Synthetic backbones (synth.make_complex); all calls start from coordinates; they are alternated in one
process, synchronised, and reported as medians with their [min, max] spread after warm-up.

    python tools/class_conditional_time.py [--reps 7] [--sizes 300x20x32,0x150x48] [--states 4x210x20x48] [--parent PATH]
"""
import ctypes as C
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
w = synth.make_weights(0)
SHARED = ("S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def model(k, prec):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()})
    m = m.to(dev).eval()
    m.message_precision = prec
    return m


def duplex_complex(n_prot, n_strand):
    """A protein of n_prot residues (none for 0) with an RNA duplex of 2 x n_strand residues -> (complex, the antiparallel pairs)."""
    L = n_prot + 2 * n_strand
    cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=n_prot / L, frac_dna=0.0)
    cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
    for c in range(int(cx["chain_labels"].max()) + 1):
        sel = cx["chain_labels"] == c
        cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    return cx, [(n_prot + k, L - 1 - k) for k in range(n_strand)]


def duplex_inputs(n_prot, n_strand):
    cx, pairs = duplex_complex(n_prot, n_strand)
    L = cx["S"].shape[0]
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=1, randn=torch.randn(1, L, device=dev))
    return fd, dict(fd, paired_residues=pairs)


def states_inputs(M, n_prot, n_strand):
    """M states of the duplex complex: seeded smooth deformations (a few low-frequency sine waves plus jitter)."""
    cx, pairs = duplex_complex(n_prot, n_strand)
    L = cx["S"].shape[0]
    rng = np.random.default_rng(11)
    X = cx["X"].astype(np.float64)
    Xs, scale = [cx["X"]], max(1.0, float(np.abs(X).max()))
    for _ in range(1, M):
        D = sum(np.sin(X @ (rng.standard_normal(3) * 2.5 / scale) + rng.uniform(0, 6.28))[..., None] * rng.standard_normal(3) * 2.0 for _ in range(3))
        Xs.append(((X + D + 0.15 * rng.standard_normal(X.shape)) * cx["X_m"][:, :, None]).astype(np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fd = {k: t(cx[k])[None] for k in SHARED}
    fd.update(X=t(np.stack(Xs)), X_m=t(cx["X_m"])[None].repeat(M, 1, 1), batch_size=1, temperature=1.0, bias=torch.zeros(1, L, 33, device=dev),
              randn=torch.randn(1, L, device=dev), state_weights=[1.0 / M] * M, symmetry_residues=[[]], symmetry_weights=[[]])
    return fd, dict(fd, paired_residues=pairs)


def load_parent(path):
    """The parent commit's build as a second library of this process, with the prototypes of the symbols it has."""
    lib = C.CDLL(path)
    for name, (res, args) in hip._PROTOTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.namp_abi_version() == hip.NAMP_ABI_VERSION and hasattr(lib, "namp_loo_groups") and not hasattr(lib, "namp_loo_classes")
    return lib


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(calls, reps):
    """Medians of `reps` alternated synchronised calls per form -> {name: (median, min, max)}."""
    for f in calls.values():
        f(); f()                                                        # warm-up: weights packed, workspaces allocated, tables cached
    t = {name: [] for name in calls}
    for _ in range(reps):                                               # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}


def show(t):
    return "  ".join(f"{name} {m:.2f} ms [{lo:.2f}, {hi:.2f}]" for name, (m, lo, hi) in t.items())


reps = int(arg("--reps", "7"))
parent_path = arg("--parent", "")
this_lib = hip.lib()
parent_lib = load_parent(parent_path) if parent_path else None
shapes = [("pairs", s) for s in arg("--sizes", "300x20x32,0x150x48").split(",") if s] + \
         [("states", s) for s in arg("--states", "4x210x20x48").split(",") if s]
for kind, size in shapes:
    dims = list(map(int, size.split("x")))
    if kind == "pairs":
        (n_prot, n_strand, K), M, tied = dims, 1, False
        plain, paired = duplex_inputs(n_prot, n_strand)
    else:
        (M, n_prot, n_strand, K), tied = dims, True
        plain, paired = states_inputs(M, n_prot, n_strand)
    wobble = dict(paired, paired_wobble=True, paired_wobble_bias=0.0)
    for prec in ("x3", "fp32"):
        # one model per form: the host tables of a form stay cached as they do for a resident feature_dict that is scored again and again
        # (one model alternating the forms would rebuild the one-slot table caches of the canonical and the plain group call every time)
        m, m_canon, m_plain = model(K, prec), model(K, prec), model(K, prec)

        def on_parent(mo, fd):
            hip._lib = parent_lib
            try:
                return mo.conditional_probs(fd, tied=tied)
            finally:
                hip._lib = this_lib

        calls = {"classes": lambda: m.conditional_probs(wobble, tied=tied, classes=True), "canonical": lambda: m_canon.conditional_probs(paired, tied=tied),
                 "plain": lambda: m_plain.conditional_probs(plain, tied=tied)}
        line = f"{kind} states={M} protein={n_prot} duplex=2x{n_strand} K={K} {prec}: "
        if parent_lib is not None:
            calls.update({"canonical, parent build": lambda: on_parent(m_canon, paired), "plain, parent build": lambda: on_parent(m_plain, plain)})
            same = [bool(torch.equal(on_parent(mo, fd)["log_probs"], mo.conditional_probs(fd, tied=tied)["log_probs"]))
                    for mo, fd in ((m_plain, plain), (m_canon, paired))]
        out = calls["classes"]()
        n_groups = out["groups" if tied else "pairs"].shape[0]
        live = int(torch.isfinite(out["group_class_log_probs" if tied else "pair_class_log_probs"][:, 33]).sum())
        t = measure(calls, reps)
        line += show(t)
        spread = lambda a, b: max(a[2] - a[1], b[2] - b[1])
        if parent_lib is not None:
            for name in ("plain", "canonical"):
                a, b = t[name], t[name + ", parent build"]
                line += f"; (a) {name} - parent {a[0] - b[0]:+.3f} ms (larger min-max spread of the two {spread(a, b):.3f} ms)"
            line += f"; rows equal the parent's bit for bit: plain {same[0]}, canonical {same[1]}"
        a, b = t["classes"], t["canonical"]
        line += f"; (b) classes - canonical {a[0] - b[0]:+.3f} ms (larger min-max spread of the two {spread(a, b):.3f} ms)"
        print(line + f"; {n_groups} tied, {live} with wobble lanes; cone items {out['cone_items'].tolist()}; {reps} calls each, from coordinates",
              flush=True)
