"""Time the symmetric scan — ProteinMPNN.score_mutations(tied=True) — on cuda:0: the cone route (namp_group_mutations) against
method="dense" (the explicit library through score_tied), from coordinates, in split-bf16 and exact fp32, medians [min, max] of alternated
synchronised calls in one process after warm-up; beside them the counted rows per variant (mean of sum_l |U_l(site)|, against the dense
route's 3 L) and the number of decoder calls.

    python tools/group_scan_time.py [--reps 7] [--prec x3,fp32] [--copies 3] [--residues 300]
        a 3 x 300 homo-trimer (one chain copied under a three-fold rotation), K = 48, everything designed, groups (i, i + 300, i + 600),
        the 20 amino acids at 100 evenly spaced units (n = 2,000, three edits per variant)
    --pairs         the paired scan, score_mutations(pairs=True, tied=True, classes=True) (namp_class_mutations), in the place of the
                    symmetric one: a 2 x 150 RNA duplex, K = 48, wobble on, every pair over its 6 classes (n = 900), and a 300-residue
                    protein beside a 2 x 20 RNA duplex, K = 32 (n = 120); the second strand runs antiparallel 10 A beside the first
    --parent PATH   another build of the library (libnamp_hip.so of the parent commit) as a second library of this process: score(),
                    the plain, the state, the group and the paired scan on their cones, score_tied(items) on the trimer at n = 100, conditional_probs(tied=True)
                    and the cfg1 design call (97 residues, K = 32, batch_size 1) run alternated on both builds; per call this build's
                    median - its median beside the larger min-max spread of the two, and whether the results are its bits.
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


def oligomer(n, copies, seed=3):
    """One protein chain of n residues copied `copies` times under a rotation about an axis beside it: a homo-oligomer whose copies touch
    -> (cx of copies * n residues, the groups (i, i + n, ...))."""
    cx = synth.make_complex(seed=seed, n=n, n_chains=1, frac_protein=1.0, frac_dna=0.0)
    X = cx["X"].astype(np.float64)
    centre = X[cx["X_m"] != 0].mean(0)
    radius = np.linalg.norm(X[cx["X_m"] != 0] - centre, axis=1).mean()
    axis_at = centre + np.array([0.8 * radius, 0.0, 0.0])
    out = {k: [] for k in cx}
    for c in range(copies):
        a = 2 * np.pi * c / copies
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        for k, v in cx.items():
            if k == "X":
                v = (((X - axis_at) @ R.T + axis_at) * cx["X_m"][:, :, None]).astype(np.float32)
            elif k == "chain_labels":
                v = v + c
            out[k].append(v)
    big = {k: np.concatenate(v) for k, v in out.items()}
    big["chain_mask"] = np.ones(copies * n, np.int32)
    big["randn"] = np.random.default_rng(seed).standard_normal(copies * n).astype(np.float32)
    return big, [[i + c * n for c in range(copies)] for i in range(n)]


def states_of(cx, M, seed=5, amplitude=2.0, jitter=0.15):
    rng = np.random.default_rng(seed)
    X, X_m = cx["X"].astype(np.float64), cx["X_m"]
    out, scale = [cx["X"].astype(np.float32)], max(1.0, float(np.abs(cx["X"]).max()))
    for _ in range(1, M):
        D = np.zeros_like(X)
        for _w in range(3):
            D += np.sin(X @ (rng.standard_normal(3) * (2.5 / scale)) + rng.uniform(0, 2 * np.pi))[..., None] * (rng.standard_normal(3) * amplitude)
        out.append(((X + D + jitter * rng.standard_normal(X.shape)) * X_m[:, :, None]).astype(np.float32))
    return np.stack(out)


def duplex(n_prot, n_strand, seed=7):
    """A protein of n_prot residues (none: 0) and an RNA duplex of 2 x n_strand: the second strand is the first one read backwards, 10 A
    beside it, with the Watson-Crick complement of its tokens -> (cx, the pairs (first strand k, its partner))."""
    n = n_prot + n_strand
    cx = synth.make_complex(seed=seed, n=n, n_chains=1, frac_protein=n_prot / n, frac_dna=0.0)
    rti = spec.restype_to_int()
    wc = {rti[a]: rti[b] for a, b in spec.WC_SAME.items()}
    a = np.arange(n_prot, n)
    out = {}
    for k, v in cx.items():
        tail = v[a][::-1]
        if k == "X":
            tail = (tail + np.array([10.0, 0.0, 0.0], np.float32)) * cx["X_m"][a][::-1][:, :, None]
        elif k == "S":
            tail = np.array([wc.get(int(t), int(t)) for t in tail], v.dtype)
        out[k] = np.concatenate((v, tail.astype(v.dtype)))
    L2 = n + n_strand
    out["chain_labels"] = np.repeat(np.arange(3, dtype=cx["chain_labels"].dtype), (n_prot, n_strand, n_strand))      # the protein, the two strands
    out["chain_mask"] = np.ones(L2, np.int32)
    out["randn"] = np.random.default_rng(seed).standard_normal(L2).astype(np.float32)
    pairs = [(int(r), L2 - 1 - q) for q, r in enumerate(a)]
    return out, [p for p in pairs if out["mask"][p[0]] and out["mask"][p[1]]]


reps = int(arg("--reps", "7"))
if "--pairs" in sys.argv:
    for n_prot, n_strand, Kp in ((0, 150, 48), (300, 20, 32)):
        cxp, prs = duplex(n_prot, n_strand)
        Lp = len(cxp["S"])
        fdp = to_fd(cxp)
        fdp.update(paired_residues=prs, paired_wobble=True, paired_wobble_bias=0.0, symmetry_residues=[[]], symmetry_weights=[[]],
                   temperature=1.0, bias=torch.zeros(1, Lp, 33, device=dev))
        firsts = torch.tensor(sorted(p[0] for p in prs), device=dev)
        for prec in arg("--prec", "x3,fp32").split(","):
            m = model(Kp)
            m.message_precision = prec
            calls = {"cone": lambda: m.score_mutations(fdp, positions=firsts, pairs=True, method="cone", tied=True, classes=True),
                     "dense": lambda: m.score_mutations(fdp, positions=firsts, pairs=True, method="dense", tied=True, classes=True)}
            c, d = calls["cone"](), calls["dense"]()
            n = len(c["site_index"])
            diff = float((c["delta_log_likelihood"] - d["delta_log_likelihood"]).abs().max())
            auto = m.score_mutations(fdp, positions=firsts, pairs=True, tied=True, classes=True)["method"]
            t = measure(calls, reps)
            rows = c["site_rows"][c["site_index"]].float()
            (cm, clo, chi), (dm, dlo, dhi) = t["cone"], t["dense"]
            print(f"{n_prot} protein + 2 x {n_strand} RNA duplex L={Lp} K={Kp} pairs={len(prs)} n={n} {prec}: cone {cm:.2f} ms [{clo:.2f}, {chi:.2f}] in "
                  f"{c['chunks']} calls  dense {dm:.2f} ms [{dlo:.2f}, {dhi:.2f}] in {d['chunks']} calls  dense / cone {dm / cm:.2f}x "
                  f"(dense - cone {dm - cm:+.2f} ms, larger min-max spread {max(chi - clo, dhi - dlo):.2f} ms); rows per variant: mean "
                  f"{[round(v, 1) for v in rows.mean(0).tolist()]} = {float(rows.sum(1).mean()):.0f}, max {int(rows.sum(1).max())}, dense {3 * Lp}; "
                  f"'auto' takes {auto}; max|d delta| cone vs dense {diff:.2e}; {reps} alternated calls each, from coordinates", flush=True)
    sys.exit(0)
copies, n_res, K = int(arg("--copies", "3")), int(arg("--residues", "300")), 48
cx, groups = oligomer(n_res, copies)
L = copies * n_res
fd = to_fd(cx)
fd.update(symmetry_residues=groups, symmetry_weights=[[1.0] * copies for _ in groups], temperature=1.0, bias=torch.zeros(1, L, 33, device=dev))
lead = np.nonzero(cx["mask"][:n_res])[0]
lead = lead[[all(cx["mask"][r] for r in groups[i]) for i in lead]]
pos = lead[np.linspace(0, len(lead) - 1, min(100, len(lead))).astype(np.int64)]
positions = torch.from_numpy(pos).to(dev)

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
        Ls, M = 390, 2
        cxs = synth.make_complex(seed=3, n=Ls, n_chains=1, frac_protein=350 / Ls, frac_dna=40 / Ls)
        cxs["chain_mask"] = cxs["dna_mask"].astype(np.int32)
        fd0 = to_fd(cxs)
        fds = dict(fd0, X=torch.from_numpy(states_of(cxs, M)).to(dev), X_m=fd0["X_m"].repeat(M, 1, 1), state_weights=[1.0, -0.5])
        lib = fd["S"].long().repeat(100, 1)
        cols = torch.from_numpy(np.array([groups[i] for i in pos])).to(dev)                        # [100, copies]
        lib[torch.arange(100, device=dev)[:, None], cols] = torch.from_numpy(np.random.default_rng(1).integers(0, 20, (100, 1))).to(dev)
        cx1 = synth.make_complex(seed=3, n=97, n_chains=1, frac_protein=0.0, frac_dna=0.0)
        fd1 = to_fd(cx1)
        fd1.update(temperature=0.1, bias=torch.zeros(1, 97, 33, device=dev), symmetry_residues=[[]], symmetry_weights=[[]],
                   S_forced=fd1["S"].long())                           # (forced draws: the two builds' results can be compared bit for bit)
        cxp, prs = duplex(0, 150)                                      # (the first duplex of --pairs)
        fdp = to_fd(cxp)
        fdp.update(paired_residues=prs, paired_wobble=True, paired_wobble_bias=0.0, symmetry_residues=[[]], symmetry_weights=[[]],
                   temperature=1.0, bias=torch.zeros(1, len(cxp["S"]), 33, device=dev))
        firsts = torch.tensor(sorted(p[0] for p in prs), device=dev)
        m, m48 = model(32), model(K)
        m.message_precision = m48.message_precision = prec
        forms = {"score()": (lambda: m.score(fd0), "log_probs"),
                 "score_mutations(cone), 40 positions": (lambda: m.score_mutations(fd0, method="cone"), "delta_log_likelihood"),
                 "score_mutations(cone), 2 states, 40 positions": (lambda: m.score_mutations(fds, method="cone"), "delta_log_likelihood"),
                 f"score_mutations(cone, tied=True), {copies} x {n_res} trimer, 100 units x 20":
                     (lambda: m48.score_mutations(fd, positions=positions, method="cone", tied=True), "delta_log_likelihood"),
                 f"score_mutations(cone, pairs=True, tied=True, classes=True), 2 x 150 RNA duplex, {len(prs)} pairs x 6 classes":
                     (lambda: m48.score_mutations(fdp, positions=firsts, pairs=True, method="cone", tied=True, classes=True), "delta_log_likelihood"),
                 f"score_tied(items), {copies} x {n_res} trimer, n = 100": (lambda: m48.score_tied(fd, lib, method="items"), "token_log_probs"),
                 "conditional_probs(tied=True), the trimer": (lambda: m48.conditional_probs(fd, tied=True), "log_probs"),
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

for prec in arg("--prec", "x3,fp32").split(","):
    m = model(K)
    m.message_precision = prec
    calls = {"cone": lambda: m.score_mutations(fd, positions=positions, method="cone", tied=True),
             "dense": lambda: m.score_mutations(fd, positions=positions, method="dense", tied=True)}
    c, d = calls["cone"](), calls["dense"]()
    n = len(c["site_index"])
    diff = float((c["delta_log_likelihood"] - d["delta_log_likelihood"]).abs().max())
    auto = m.score_mutations(fd, positions=positions, tied=True)["method"]
    t = measure(calls, reps)
    rows = c["site_rows"][c["site_index"]].float()
    (cm, clo, chi), (dm, dlo, dhi) = t["cone"], t["dense"]
    print(f"{copies} x {n_res} homo-oligomer L={L} K={K} units={len(pos)} n={n} {prec}: cone {cm:.2f} ms [{clo:.2f}, {chi:.2f}] in {c['chunks']} calls  "
          f"dense {dm:.2f} ms [{dlo:.2f}, {dhi:.2f}] in {d['chunks']} calls  dense / cone {dm / cm:.2f}x "
          f"(dense - cone {dm - cm:+.2f} ms, larger min-max spread {max(chi - clo, dhi - dlo):.2f} ms); rows per variant: mean "
          f"{[round(v, 1) for v in rows.mean(0).tolist()]} = {float(rows.sum(1).mean()):.0f}, max {int(rows.sum(1).max())}, dense {3 * L}; "
          f"'auto' takes {auto}; max|d delta| cone vs dense {diff:.2e}; {reps} alternated calls each, from coordinates", flush=True)
