"""Time the pair conditionals — ProteinMPNN.conditional_probs() with paired_residues: leave-pair-out scoring of every base pair in
one call on the cone kernels (namp_loo_pairs + namp_decoder_loo) — on cuda:0 against
  (a) the UNPAIRED conditional_probs() call on the same complex: of this build, and of the parent commit's build of the library
      (--parent /path/to/libnamp_hip.so; a second library in the same process — NAMP_LIB_PATH cannot select it here, because this
      package's binding refuses a library without the namp_loo_pairs* symbols — that shares the packed weights: the ABI is the same);
  (b) the sampler route of the same build (method="dense": the L streams for the unpaired rows, one teacher-forced design call per pair).
Synthetic backbones (synth.make_complex), the two shapes of tools/paired_time.py; all calls start from coordinates, in split-bf16
and in exact fp32; they are alternated in one process, synchronised, and reported as medians with their [min, max] spread after warm-up.

    python tools/pair_conditional_time.py [--reps 7] [--sizes 300x20x32,0x150x48] [--parent PATH]     (protein residues x strand length x K)
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


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def model(k, prec):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()})
    m = m.to(dev).eval()
    m.message_precision = prec
    return m


def inputs(n_prot, n_strand):
    """A protein of n_prot residues (none for 0) with a DNA duplex of 2 x n_strand residues, the strands paired antiparallel."""
    L = n_prot + 2 * n_strand
    cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=n_prot / L, frac_dna=2 * n_strand / L)
    cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
    for c in range(int(cx["chain_labels"].max()) + 1):
        sel = cx["chain_labels"] == c
        cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=1, randn=torch.randn(1, L, device=dev))
    pairs = [(n_prot + k, L - 1 - k) for k in range(n_strand)]
    return fd, dict(fd, paired_residues=pairs), pairs


def load_parent(path):
    """The parent commit's build as a second library of this process, with the prototypes of the symbols it has."""
    lib = C.CDLL(path)
    for name, (res, args) in hip._PROTOTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.namp_abi_version() == hip.NAMP_ABI_VERSION and not hasattr(lib, "namp_loo_pairs")
    return lib


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


reps = int(arg("--reps", "7"))
parent_path = arg("--parent", "")
this_lib = hip.lib()
parent_lib = load_parent(parent_path) if parent_path else None
for size in arg("--sizes", "300x20x32,0x150x48").split(","):
    n_prot, n_strand, K = map(int, size.split("x"))
    plain, paired, pairs = inputs(n_prot, n_strand)
    for prec in ("x3", "fp32"):
        m = model(K, prec)

        def on_parent():
            hip._lib = parent_lib
            try:
                return m.conditional_probs(plain)
            finally:
                hip._lib = this_lib

        calls = {"pair call": lambda: m.conditional_probs(paired), "unpaired": lambda: m.conditional_probs(plain)}
        if parent_lib is not None:
            calls["unpaired, parent build"] = on_parent
        calls["sampler route"] = lambda: m.conditional_probs(paired, method="dense")
        a, b, s = calls["pair call"](), calls["unpaired"](), calls["sampler route"]()
        rows = torch.tensor([r for p in pairs for r in p], device=dev)
        rest = torch.ones(a["log_probs"].shape[1], dtype=torch.bool, device=dev); rest[rows] = False
        same_rest = bool(torch.equal(a["log_probs"][0, rest], b["log_probs"][0, rest]))
        same_parent = bool(torch.equal(on_parent()["log_probs"], b["log_probs"])) if parent_lib is not None else None
        d_route = float((a["log_probs"] - s["log_probs"]).abs().max())
        for f in calls.values():
            f(); f()                                                    # warm-up: weights packed, workspaces allocated
        t = {name: [] for name in calls}
        for _ in range(reps):                                           # alternated: a drift of the clocks hits every form alike
            for name, f in calls.items():
                t[name].append(timed(f))
        med = {name: float(np.median(v)) for name, v in t.items()}
        txt = "  ".join(f"{name} {med[name]:.2f} ms [{min(v):.2f}, {max(v):.2f}]" for name, v in t.items())
        ref = "unpaired, parent build" if parent_lib is not None else "unpaired"
        spread = max(max(t[n]) - min(t[n]) for n in ("pair call", ref))
        line = (f"protein={n_prot} duplex=2x{n_strand} K={K} {prec}: {txt}  (pair call - {ref} {med['pair call'] - med[ref]:+.3f} ms, larger "
                f"min-max spread of the two {spread:.3f} ms")
        if parent_lib is not None:
            sp2 = max(max(t[n]) - min(t[n]) for n in ("unpaired", ref))
            line += f"; unpaired - parent build {med['unpaired'] - med[ref]:+.3f} ms, spread {sp2:.3f} ms; unpaired rows equal the parent's bit for bit: {same_parent}"
        print(line + f"; {len(a['pairs'])} of {len(pairs)} pairs tied, cone items {a['cone_items'].tolist()} with pairs / {b['cone_items'].tolist()} "
              f"without; unpaired rows of the pair call bit-identical to the unpaired call: {same_rest}; pair call vs sampler route max|dlogp| "
              f"{d_route:.2e}; {reps} calls each, from coordinates)", flush=True)
