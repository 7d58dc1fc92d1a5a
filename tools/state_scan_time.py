"""Time the specificity scan — ProteinMPNN.score_mutations() with state_weights — on cuda:0: the cone route (namp_state_mutations) against
method="dense" (the explicit library through score_tied(method="stream")), from coordinates, in split-bf16 and exact fp32, medians
[min, max] of alternated synchronised calls in one process after warm-up; beside them the counted rows per variant (mean of
sum_l |U_l(site)| on the flat graph, against 3 M L) and the number of decoder calls.

    python tools/state_scan_time.py [--reps 7] [--prec x3,fp32] [--states 4] [--residues 250]
        4 states x 250 residues, K = 48, everything designed, the 20 amino acids at 100 evenly spaced protein positions (n = 2,000)
    --parent PATH   another build of the library (libnamp_hip.so of the parent commit) as a second library of this process: plain
                    score_mutations(), score_tied(), score() and the cfg1 design call (97 residues, K = 32, batch_size 1) run alternated
                    on both builds; per call this build's median - its median beside the larger min-max spread of the two, and whether
                    the results are its bits.
"""
import ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
w = synth.make_weights(0)


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()}); return m.to(dev).eval()


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(calls, reps):
    for f in calls.values():
        f(); f()                                                        # warm-up: weights packed, workspaces allocated
    t = {name: [] for name in calls}
    for _ in range(reps):                                               # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}


def to_fd(cx):
    fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx.items()}
    fd["batch_size"] = 1
    return fd


def states_of(cx, M, seed=5, amplitude=2.0, jitter=0.15):
    """X [M, L, A, 3]: state 0 is the complex; every other state a seeded smooth deformation of it plus jitter (absent atoms stay zero)."""
    rng = np.random.default_rng(seed)
    X, X_m = cx["X"].astype(np.float64), cx["X_m"]
    out, scale = [cx["X"].astype(np.float32)], max(1.0, float(np.abs(cx["X"]).max()))
    for _ in range(1, M):
        D = np.zeros_like(X)
        for _w in range(3):
            D += np.sin(X @ (rng.standard_normal(3) * (2.5 / scale)) + rng.uniform(0, 2 * np.pi))[..., None] * (rng.standard_normal(3) * amplitude)
        out.append(((X + D + jitter * rng.standard_normal(X.shape)) * X_m[:, :, None]).astype(np.float32))
    return np.stack(out)


reps = int(arg("--reps", "7"))

if arg("--parent", ""):
    def load_parent(path):
        lib = ctypes.CDLL(path)
        for name, (res, args) in hip._PROTOTYPES.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        assert lib.namp_abi_version() == hip.NAMP_ABI_VERSION
        return lib

    this_lib, parent_lib = hip.lib(), load_parent(arg("--parent", ""))

    def on_parent(f):
        def call():
            hip._lib = parent_lib
            try:
                return f()
            finally:
                hip._lib = this_lib
        return call

    for prec in arg("--prec", "x3,fp32").split(","):
        L, M = 390, 2
        cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=350 / L, frac_dna=40 / L)
        cx["chain_mask"] = cx["dna_mask"].astype(np.int32)
        fd = to_fd(cx)
        fds = dict(fd, X=torch.from_numpy(states_of(cx, M)).to(dev), X_m=fd["X_m"].repeat(M, 1, 1), state_weights=[1.0, -0.5])
        pos = np.nonzero(cx["mask"] * cx["chain_mask"])[0]
        lib = fd["S"].long().repeat(64, 1)
        lib[:, torch.from_numpy(pos).to(dev)] = torch.from_numpy(np.random.default_rng(1).integers(21, 25, (64, len(pos)))).to(dev)
        cx1 = synth.make_complex(seed=3, n=97, n_chains=1, frac_protein=0.0, frac_dna=0.0)
        fd1 = to_fd(cx1)
        fd1.update(temperature=0.1, bias=torch.zeros(1, 97, 33, device=dev), symmetry_residues=[[]], symmetry_weights=[[]],
                   S_forced=fd1["S"].long())                           # (forced draws: the two builds' results can be compared bit for bit)
        m = model(32)
        m.message_precision = prec
        forms = {"score()": (lambda: m.score(fd), "log_probs"),
                 "score_mutations(cone), 40 positions": (lambda: m.score_mutations(fd, method="cone"), "delta_log_likelihood"),
                 "score_tied(stream), 2 states, n = 64": (lambda: m.score_tied(fds, lib, method="stream"), "token_log_probs"),
                 "score_tied(items), 2 states, n = 64": (lambda: m.score_tied(fds, lib, method="items"), "token_log_probs"),
                 "cfg1 design call": (lambda: m.sample(fd1), "log_probs")}
        for name, (f, key) in forms.items():
            same = bool(torch.equal(on_parent(f)()[key], f()[key]))
            # one form at a time, its two builds alternated: each call follows the same call of the other build
            t = measure({name: f, name + ", parent": on_parent(f)}, reps)
            a, b = t[name], t[name + ", parent"]
            print(f"parent check {prec}: {name} {a[0]:.3f} ms [{a[1]:.3f}, {a[2]:.3f}], parent {b[0]:.3f} ms [{b[1]:.3f}, {b[2]:.3f}]: "
                  f"this - parent {a[0] - b[0]:+.3f} ms (larger min-max spread of the two {max(a[2] - a[1], b[2] - b[1]):.3f} ms), "
                  f"the parent's bits: {same}; {reps} alternated calls each, from coordinates", flush=True)
    sys.exit(0)

M, L, K = int(arg("--states", "4")), int(arg("--residues", "250")), 48
cx = synth.make_complex(seed=3, n=L)
cx["chain_mask"] = np.ones(L, np.int32)
prot = np.nonzero(cx["protein_mask"] * cx["mask"])[0]
pos = prot[np.linspace(0, len(prot) - 1, min(100, len(prot))).astype(np.int64)]
fd = to_fd(cx)
fd.update(X=torch.from_numpy(states_of(cx, M)).to(dev), X_m=fd["X_m"].repeat(M, 1, 1), state_weights=[1.0, -0.5, 0.5, -0.25, 0.25, 0.1, 0.1, 0.1][:M])
positions = torch.from_numpy(pos).to(dev)
for prec in arg("--prec", "x3,fp32").split(","):
    m = model(K)
    m.message_precision = prec
    calls = {"cone": lambda: m.score_mutations(fd, positions=positions, method="cone"),
             "dense": lambda: m.score_mutations(fd, positions=positions, method="dense")}
    c, d = calls["cone"](), calls["dense"]()
    n = len(c["site_index"])
    diff = float((c["delta_log_likelihood"] - d["delta_log_likelihood"]).abs().max())
    sdiff = float((c["state_delta"] - d["state_delta"]).abs().max())
    auto = m.score_mutations(fd, positions=positions)["method"]
    t = measure(calls, reps)
    rows = c["site_rows"][c["site_index"]].float()
    (cm, clo, chi), (dm, dlo, dhi) = t["cone"], t["dense"]
    print(f"{M} states x L={L} K={K} positions={len(pos)} n={n} {prec}: cone {cm:.2f} ms [{clo:.2f}, {chi:.2f}] in {c['chunks']} calls  "
          f"dense {dm:.2f} ms [{dlo:.2f}, {dhi:.2f}] in {d['chunks']} calls  dense / cone {dm / cm:.2f}x "
          f"(dense - cone {dm - cm:+.2f} ms, larger min-max spread {max(chi - clo, dhi - dlo):.2f} ms); rows per variant on the flat graph: mean "
          f"{[round(v, 1) for v in rows.mean(0).tolist()]} = {float(rows.sum(1).mean()):.0f}, max {int(rows.sum(1).max())}, dense {3 * M * L}; "
          f"'auto' takes {auto}; max|d delta| cone vs dense {diff:.2e}, max|d state_delta| {sdiff:.2e}; {reps} alternated calls each, "
          f"from coordinates", flush=True)
