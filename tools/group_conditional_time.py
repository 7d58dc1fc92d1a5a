"""Time the group conditionals — ProteinMPNN.conditional_probs(tied=True): leave-group-out scoring of every tied group in one call
on the cone kernels (namp_loo_groups + namp_decoder_loo) — on cuda:0:
  (a) what the change must not touch: the call without an attachment and the PAIR call of this build against the parent commit's build
      of the library (--parent /path/to/libnamp_hip.so: a second library in the same process that shares the packed weights; the ABI
      is the same), on the two shapes of tools/pair_conditional_time.py;
  (b) the group call on M tied states (--states MxLxK) and on a homo-oligomer of C chains of L residues tied residue by residue
      (--oligomers CxLxK) against the slow route of the same build (method="dense": one teacher-forced design call per group) and
      against the call without groups on a complex of the same flattened size, with the active-item counts of both.
Synthetic backbones (synth.make_complex); all calls start from coordinates, in split-bf16 and in exact fp32; they are alternated in one
process, synchronised, and reported as medians with their [min, max] spread after warm-up (the slow route: --slow_reps calls).

    python tools/group_conditional_time.py [--reps 7] [--slow_reps 3] [--sizes 300x20x32,0x150x48] [--states 4x250x48] [--oligomers 3x300x48]
                                           [--parent PATH]
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


def duplex_inputs(n_prot, n_strand):
    """A protein of n_prot residues (none for 0) with a DNA duplex of 2 x n_strand residues, the strands paired antiparallel."""
    L = n_prot + 2 * n_strand
    cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=n_prot / L, frac_dna=2 * n_strand / L)
    cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
    for c in range(int(cx["chain_labels"].max()) + 1):
        sel = cx["chain_labels"] == c
        cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=1, randn=torch.randn(1, L, device=dev))
    return fd, dict(fd, paired_residues=[(n_prot + k, L - 1 - k) for k in range(n_strand)])


def plain_inputs(n, n_chains):
    cx = synth.make_complex(seed=3, n=n, n_chains=n_chains)
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=1, temperature=1.0, bias=torch.zeros(1, n, 33, device=dev), randn=torch.randn(1, n, device=dev))
    return fd


def states_inputs(M, L):
    """M states of one complex of L residues: seeded smooth deformations (a few low-frequency sine waves plus jitter)."""
    cx = synth.make_complex(seed=3, n=L)
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
    return fd


def load_parent(path):
    """The parent commit's build as a second library of this process, with the prototypes of the symbols it has."""
    lib = C.CDLL(path)
    for name, (res, args) in hip._PROTOTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.namp_abi_version() == hip.NAMP_ABI_VERSION and hasattr(lib, "namp_loo_pairs") and not hasattr(lib, "namp_loo_groups")
    return lib


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(calls, reps, slow=(), slow_reps=3):
    """Medians of `reps` alternated synchronised calls per form (the forms named in `slow`: slow_reps) -> {name: (median, min, max)}."""
    for f in calls.values():
        f(); f()                                                        # warm-up: weights packed, workspaces allocated, tables cached
    t = {name: [] for name in calls}
    for r in range(reps):                                               # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            if name not in slow or r < slow_reps:
                t[name].append(timed(f))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}


def show(t):
    return "  ".join(f"{name} {m:.2f} ms [{lo:.2f}, {hi:.2f}]" for name, (m, lo, hi) in t.items())


reps, slow_reps = int(arg("--reps", "7")), int(arg("--slow_reps", "3"))
parent_path = arg("--parent", "")
this_lib = hip.lib()
parent_lib = load_parent(parent_path) if parent_path else None

# ---- (a) the call without an attachment and the pair call: this build against the parent's
for size in [s for s in arg("--sizes", "300x20x32,0x150x48").split(",") if s]:
    n_prot, n_strand, K = map(int, size.split("x"))
    plain, paired = duplex_inputs(n_prot, n_strand)
    for prec in ("x3", "fp32"):
        m = model(K, prec)

        def on_parent(fd):
            hip._lib = parent_lib
            try:
                return m.conditional_probs(fd)
            finally:
                hip._lib = this_lib

        calls = {"plain": lambda: m.conditional_probs(plain), "pair call": lambda: m.conditional_probs(paired)}
        line = f"(a) protein={n_prot} duplex=2x{n_strand} K={K} {prec}: "
        if parent_lib is not None:
            calls.update({"plain, parent build": lambda: on_parent(plain), "pair call, parent build": lambda: on_parent(paired)})
            same = [bool(torch.equal(on_parent(fd)["log_probs"], m.conditional_probs(fd)["log_probs"])) for fd in (plain, paired)]
        t = measure(calls, reps)
        line += show(t)
        if parent_lib is not None:
            for name in ("plain", "pair call"):
                a, b = t[name], t[name + ", parent build"]
                line += f"; {name} - parent {a[0] - b[0]:+.3f} ms (larger min-max spread of the two {max(a[2] - a[1], b[2] - b[1]):.3f} ms)"
            line += f"; rows equal the parent's bit for bit: plain {same[0]}, pair call {same[1]}"
        print(line + f"; {reps} calls each, from coordinates", flush=True)

# ---- (b) the group call: against the slow route and against the call without groups on the same flattened size
cases = [("states", s) for s in arg("--states", "4x250x48").split(",") if s] + [("oligomer", s) for s in arg("--oligomers", "3x300x48").split(",") if s]
for kind, size in cases:
    M, L, K = map(int, size.split("x"))
    if kind == "states":
        tied = states_inputs(M, L)
        flat = plain_inputs(M * L, M)
    else:
        flat = plain_inputs(M * L, M)
        tied = dict(flat, symmetry_residues=[[i + c * L for c in range(M)] for i in range(L)], symmetry_weights=[[1.0 / M] * M] * L)
    for prec in ("x3", "fp32"):
        m = model(K, prec)
        calls = {"group call": lambda: m.conditional_probs(tied, tied=True), "no groups, same size": lambda: m.conditional_probs(flat),
                 "slow route": lambda: m.conditional_probs(tied, method="dense", tied=True)}
        a, b, s = (f() for f in calls.values())
        d_route = float((a["log_probs"] - s["log_probs"]).abs().max())
        t = measure(calls, reps, slow=("slow route",), slow_reps=slow_reps)
        g, p, sl = t["group call"], t["no groups, same size"], t["slow route"]
        print(f"(b) {kind} M={M} L={L} K={K} {prec}: {show(t)}; group call - no groups {g[0] - p[0]:+.3f} ms (larger min-max spread of the two "
              f"{max(g[2] - g[1], p[2] - p[1]):.3f} ms); slow route / group call {sl[0] / g[0]:.0f}x; {a['groups'].shape[0]} groups of up to "
              f"{a['groups'].shape[1]}; cone items {a['cone_items'].tolist()} with groups / {b['cone_items'].tolist()} without; group call vs slow "
              f"route max|dlogp| {d_route:.2e}; {reps} calls each ({slow_reps} of the slow route), from coordinates", flush=True)
