"""Time ProteinMPNN.score_tied() on cuda:0: the item route (namp_tied_score) and the stream route against the sampler route of the same
build (teacher-forced design calls), from coordinates, in split-bf16 and exact fp32, medians [min, max] of alternated synchronised
calls in one process after warm-up.

    python tools/tied_score_time.py [--reps 7] [--shapes states,duplex,trimer] [--prec x3,fp32]
        states   4 backbone states x 250 residues, K = 48, n = 1 and n = 1,000: stream, items, sampler
        duplex   a 300-residue protein + a 2 x 20 RNA duplex, 20 wobble pairs, K = 32, n = 1,000: items, sampler
        trimer   a 3 x 300 homo-trimer, 300 groups of three, K = 48, n = 100: items, sampler
    --parent PATH   another build of the library (libnamp_hip.so of the parent commit) as a second library of this process: score(),
                    score_sequences() on both routes, conditional_probs() and the cfg1 design call (97 residues, K = 32, batch_size 1)
                    run alternated on both builds; per call this build's median - its median beside the larger min-max spread of the
                    two, and whether the results are its bits.
"""
import ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


from na_mpnn_amd import hip, spec, synth
from na_mpnn_amd.model import ProteinMPNN
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
w = synth.make_weights(0)
RTI = spec.restype_to_int()


def model(k, prec):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=RTI, polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()})
    m = m.to(dev).eval()
    m.message_precision = prec
    return m


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
    L = len(cx["S"])
    fd.update(batch_size=1, temperature=1.0, bias=torch.zeros(1, L, 33, device=dev), symmetry_residues=[[]], symmetry_weights=[[]])
    fd["S"] = fd["S"].long()
    return fd


def shape(name):
    """-> (K, feature_dict on the device, library sizes, routes)."""
    if name == "states":
        import tied_states_ref as ts
        cx = synth.make_complex(seed=3, n=250)
        fd = to_fd(cx)
        Xs = ts.make_states(cx, 4, 8)
        fd.update(X=torch.from_numpy(Xs).to(dev), X_m=fd["X_m"].repeat(4, 1, 1), state_weights=[0.4, 0.3, 0.2, 0.1])
        return 48, fd, (1, 1000), ("stream", "items", "sampler")
    if name == "duplex":
        L = 340
        cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=300 / L, frac_dna=0.0)
        cx["chain_labels"] = np.searchsorted([300, 320], np.arange(L), side="right").astype(np.int32)
        for c in range(3):
            sel = cx["chain_labels"] == c
            cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
        fd = to_fd(cx)
        fd.update(paired_residues=[(300 + t, 339 - t) for t in range(20)], paired_wobble=True, paired_wobble_bias=0.0)
        return 32, fd, (1000,), ("items", "sampler")
    cx = synth.make_complex(seed=3, n=900, n_chains=3)
    fd = to_fd(cx)
    fd.update(symmetry_residues=[[i, i + 300, i + 600] for i in range(300)], symmetry_weights=[[1.0, 1.0, 1.0]] * 300)
    return 48, fd, (100,), ("items", "sampler")


def library(m, fd, n):
    """n tie-consistent sequences: the sampler's own draws under the ties of the feature_dict."""
    torch.manual_seed(n)
    L = fd["S"].shape[1]
    out = []
    for k0 in range(0, n, 50):
        bs = min(50, n - k0)
        draw = m.sample(dict(fd, batch_size=bs, randn=torch.randn(bs, L, device=dev)))
        out.append(draw["S"].long())
    return torch.cat(out)


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
        L = 390
        cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=350 / L, frac_dna=40 / L)
        cx["chain_mask"] = cx["dna_mask"].astype(np.int32)
        fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx.items()}
        fd["batch_size"] = 1
        pos = np.nonzero(cx["mask"] * cx["chain_mask"])[0]
        lib = torch.from_numpy(np.random.default_rng(1).integers(21, 25, (1000, len(pos))).astype(np.int64)).to(dev)
        cx1 = synth.make_complex(seed=3, n=97, n_chains=1, frac_protein=0.0, frac_dna=0.0)
        fd1 = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx1.items()}
        fd1.update(batch_size=1, temperature=0.1, bias=torch.zeros(1, 97, 33, device=dev), symmetry_residues=[[]], symmetry_weights=[[]],
                   S_forced=fd1["S"].long())                           # (forced draws: the two builds' results can be compared bit for bit)
        m = model(32, prec)
        forms = {"score()": (lambda: m.score(fd), "log_probs"), "conditional_probs()": (lambda: m.conditional_probs(fd), "log_probs"),
                 "score_sequences(active)": (lambda: m.score_sequences(fd, lib, method="active"), "token_log_probs"),
                 "score_sequences(dense)": (lambda: m.score_sequences(fd, lib, method="dense"), "token_log_probs"),
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

for name in arg("--shapes", "states,duplex,trimer").split(","):
    K, fd, sizes, routes = shape(name)
    L = fd["S"].shape[1]
    M = 1 if fd.get("state_weights") is None else len(fd["state_weights"])
    fd["randn"] = torch.from_numpy(np.random.default_rng(5).standard_normal((1, L)).astype(np.float32)).to(dev)
    for prec in arg("--prec", "x3,fp32").split(","):
        m = model(K, prec)
        for n in sizes:
            lib = library(m, fd, n)
            calls = {r: (lambda r=r: m.score_tied(fd, lib, method=r)) for r in routes}
            outs = {r: f() for r, f in calls.items()}
            ok = bool(outs["items"]["consistent"].all())
            diff = {r: float((outs[r]["token_log_probs"] - outs["sampler"]["token_log_probs"])[:, fd["mask"][0] != 0].abs().max()) for r in routes[:-1]}
            t = measure(calls, reps)
            sm, slo, shi = t["sampler"]
            line = f"{name} M={M} L={L} K={K} n={n} {prec}: sampler {sm:.2f} ms [{slo:.2f}, {shi:.2f}] in {outs['sampler']['chunks']} calls"
            for r in routes[:-1]:
                rm, rlo, rhi = t[r]
                line += (f"  {r} {rm:.2f} ms [{rlo:.2f}, {rhi:.2f}] in {outs[r]['chunks']} calls, sampler / {r} {sm / rm:.2f}x (sampler - {r} "
                         f"{sm - rm:+.2f} ms, larger min-max spread {max(shi - slo, rhi - rlo):.2f} ms), {n * M * L / rm / 1e3:.2f} M rows/s, "
                         f"max|d| vs sampler {diff[r]:.2e}")
            print(line + f"; the library satisfies the ties: {ok}; {reps} alternated calls each, from coordinates", flush=True)
