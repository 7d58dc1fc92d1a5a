"""Time multi-state design — ProteinMPNN.sample() with state_weights, one sequence tied across M backbone states — on cuda:0:
the device plan (namp_states_plan) against the host route of the same build, against M independent plain sample() calls (one per state:
the work without the tie), and against the yardstick the parent build already had: sample() of a symmetric M-chain complex of M * L
residues with the same groups (what tools/sample_sym_time.py times).  All calls start from coordinates; they are alternated in one
process, synchronised, and reported as medians with their [min, max] spread after warm-up.

    python tools/tied_states_time.py [--reps 7] [--sizes 2x500x48x1,4x250x48x8,8x300x32x8]        (M x L x K x batch_size)
    rocprofv3 --kernel-trace --stats -d <dir> -o tied -- python tools/tied_states_time.py --profile 8x300x32x8
        (two warm-up calls and ONE traced steady-state call on the device route; tools/rocpd_summary.py reads the database)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
w = synth.make_weights(0)
SHARED = ("S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()}); return m.to(dev).eval()


def states_of(cx, M, seed):
    """Seeded smooth deformations of one complex (a few low-frequency sine waves of the coordinates plus jitter): states whose
    neighbour lists differ."""
    rng = np.random.default_rng(seed)
    X = cx["X"].astype(np.float64)
    out, scale = [cx["X"]], max(1.0, float(np.abs(X).max()))
    for _ in range(1, M):
        D = sum(np.sin(X @ (rng.standard_normal(3) * 2.5 / scale) + rng.uniform(0, 6.28))[..., None] * rng.standard_normal(3) * 2.0 for _ in range(3))
        out.append(((X + D + 0.15 * rng.standard_normal(X.shape)) * cx["X_m"][:, :, None]).astype(np.float32))
    return np.stack(out)


def inputs(M, L, bs):
    cx = synth.make_complex(seed=3, n=L)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    common = {"batch_size": bs, "temperature": 0.1, "symmetry_residues": [[]], "symmetry_weights": [[]]}
    tied = {k: t(cx[k])[None] for k in SHARED}
    Xs = states_of(cx, M, 11)
    tied.update(common, X=t(Xs), X_m=t(cx["X_m"])[None].repeat(M, 1, 1), bias=torch.zeros(1, L, 33, device=dev),
                randn=torch.randn(bs, L, device=dev), state_weights=[1.0 / M] * M)
    plain = []
    for m_ in range(M):
        fd = {k: v for k, v in tied.items() if k != "state_weights"}
        fd.update(X=tied["X"][m_:m_ + 1], X_m=tied["X_m"][m_:m_ + 1], randn=tied["randn"][:1].repeat(bs, 1))
        plain.append(fd)
    big = synth.make_complex(seed=3, n=M * L, n_chains=M)              # the yardstick: M chains of L residues, tied residue by residue
    sym = {k: t(v)[None] for k, v in big.items()}
    groups = [[i + c * L for c in range(M)] for i in range(L)]
    sym.update(common, bias=torch.zeros(1, M * L, 33, device=dev), symmetry_residues=groups,
               symmetry_weights=[[1.0 / M] * M for _ in groups], randn=torch.randn(bs, M * L, device=dev))
    return tied, plain, sym


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


if "--profile" in sys.argv:
    M, L, K, bs = map(int, arg("--profile", "8x300x32x8").split("x"))
    m, (tied, _, _) = model(K), inputs(M, L, bs)
    for _ in range(3):
        m.sample(tied)
    torch.cuda.synchronize()
    sys.exit(0)

reps = int(arg("--reps", "7"))
for size in arg("--sizes", "2x500x48x1,4x250x48x8,8x300x32x8").split(","):
    M, L, K, bs = map(int, size.split("x"))
    m = model(K)
    tied, plain, sym = inputs(M, L, bs)

    def route(device_plan):
        m.sample_states_device_plan = device_plan
        return m.sample(tied)

    calls = {"device plan": lambda: route(True), "host route": lambda: route(False),
             "M plain calls": lambda: [m.sample(fd) for fd in plain], "symmetric M-chain": lambda: m.sample(sym)}
    torch.manual_seed(1); a = route(True)
    torch.manual_seed(1); b = route(False)
    same = bool(torch.equal(a["S"], b["S"]) and torch.equal(a["log_probs"], b["log_probs"]))
    for f in calls.values():
        f(); f()                                                    # warm-up: weights packed, workspaces allocated
    t = {name: [] for name in calls}
    for _ in range(reps):                                           # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    med = {name: float(np.median(v)) for name, v in t.items()}
    txt = "  ".join(f"{name} {med[name]:.2f} ms [{min(v):.2f}, {max(v):.2f}]" for name, v in t.items())
    print(f"M={M} L={L} K={K} batch_size={bs}: {txt}  (device / symmetric {med['device plan'] / med['symmetric M-chain']:.2f}x, "
          f"device / host {med['device plan'] / med['host route']:.2f}x; {int(a['levels'])} levels, {a['work_items']} work items; "
          f"routes bit-identical: {same}; {reps} calls each, from coordinates)", flush=True)
