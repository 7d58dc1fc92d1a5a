"""Time ProteinMPNN.score_sequences() on cuda:0: the active-row route (namp_library) against the dense route of the same build (every
sequence a stream of the parent's unchanged namp_decoder_fwd), from coordinates, in split-bf16 and exact fp32, medians [min, max] of
alternated synchronised calls in one process after warm-up; beside them the counted layer evaluations per sequence (sum(active_rows)
and the rows evaluated, against 3 L) and the workspace bytes of one attached call.

    python tools/score_library_time.py [--reps 7] [--n 1000,10000] [--shapes na,all,big] [--prec x3,fp32]
        na    a 350-residue protein + 2 x 20 duplex, the nucleic acid designed, K = 32
        all   the same complex, everything designed (nothing to save: this shape sets method="auto")
        big   a 1,000-residue complex, 40 residues designed, K = 48
    --parent PATH   another build of the library (libnamp_hip.so of the parent commit) as a second library of this process: score(),
                    conditional_probs() and the cfg1 design call (97 residues, K = 32, batch_size 1) run alternated on both builds; per
                    call this build's median - its median beside the larger min-max spread of the two, and whether the results are
                    its bits.
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


def shape(name):
    """-> (K, complex with its chain_mask set)."""
    if name in ("na", "all"):
        L = 390
        cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=350 / L, frac_dna=40 / L)
        cx["chain_labels"] = np.searchsorted([350, 370], np.arange(L), side="right").astype(np.int32)
        for c in range(3):
            sel = cx["chain_labels"] == c
            cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
        cx["chain_mask"] = np.ones(L, np.int32) if name == "all" else cx["dna_mask"].astype(np.int32)
        return 32, cx
    cx = synth.make_complex(seed=3, n=1000)
    cx["chain_mask"] = np.zeros(1000, np.int32)
    cx["chain_mask"][700:740] = 1
    return 48, cx


def library(cx, n):
    pos = np.nonzero(cx["mask"] * cx["chain_mask"])[0]
    rng = np.random.default_rng(n)
    lo = np.where(cx["protein_mask"][pos] != 0, 0, np.where(cx["dna_mask"][pos] != 0, 21, 26))
    hi = np.where(cx["protein_mask"][pos] != 0, 20, np.where(cx["dna_mask"][pos] != 0, 25, 30))
    return torch.from_numpy(rng.integers(lo[None], hi[None], (n, len(pos))).astype(np.int64)).to(dev), len(pos)


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
        K, cx = shape("na")
        fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx.items()}
        fd["batch_size"] = 1
        cx1 = synth.make_complex(seed=3, n=97, n_chains=1, frac_protein=0.0, frac_dna=0.0)
        fd1 = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx1.items()}
        fd1.update(batch_size=1, temperature=0.1, bias=torch.zeros(1, 97, 33, device=dev), symmetry_residues=[[]], symmetry_weights=[[]],
                   S_forced=fd1["S"].long())                           # (forced draws: the two builds' results can be compared bit for bit)
        m = model(K)
        m.message_precision = prec
        forms = {"score()": (lambda: m.score(fd), "log_probs"), "conditional_probs()": (lambda: m.conditional_probs(fd), "log_probs"),
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

for name in arg("--shapes", "na,all,big").split(","):
    K, cx = shape(name)
    L = len(cx["S"])
    fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k_, v in cx.items()}
    fd["batch_size"] = 1
    for n in map(int, arg("--n", "1000,10000").split(",")):
        lib, n_var = library(cx, n)
        for prec in arg("--prec", "x3,fp32").split(","):
            m = model(K)
            m.message_precision = prec
            calls = {"active": lambda: m.score_sequences(fd, lib, method="active"), "dense": lambda: m.score_sequences(fd, lib, method="dense")}
            a, d = calls["active"](), calls["dense"]()
            diff = float((a["token_log_probs"] - d["token_log_probs"]).abs().max())
            t = measure(calls, reps)
            rows = a["active_rows"].tolist()
            o, rank = m.order_and_rank(fd["mask"], fd["chain_mask"], fd["randn"])
            E_idx = m.featurize(fd)[2][0]
            var = torch.zeros(L, dtype=torch.bool, device=dev); var[torch.from_numpy(np.nonzero(cx["mask"] * cx["chain_mask"])[0]).to(dev)] = True
            # rows evaluated per sequence: act_l + var (namp_library.h); the counts of one plan
            bw = rank[0][E_idx.long()] < rank[0][:, None]
            prev, evaluated = torch.zeros(L, dtype=torch.bool, device=dev), []
            for _ in range(3):
                prev = (fd["mask"][0] != 0) & (prev | (bw & (var | prev)[E_idx.long()]).any(-1))
                evaluated.append(int((prev | var).sum()))
            chunk = max(1, 3 * m.score_library_tokens // max(1, sum(evaluated)))
            ws = hip.lib().namp_library_workspace_bytes(L, min(K, L), 3, n_var, min(n, chunk), *evaluated)
            (am, alo, ahi), (dm, dlo, dhi) = t["active"], t["dense"]
            print(f"{name} L={L} K={K} n_var={n_var} n={n} {prec}: active {am:.2f} ms [{alo:.2f}, {ahi:.2f}] in {a['chunks']} calls  "
                  f"dense {dm:.2f} ms [{dlo:.2f}, {dhi:.2f}] in {d['chunks']} calls  dense / active {dm / am:.2f}x "
                  f"(dense - active {dm - am:+.2f} ms, larger min-max spread {max(ahi - alo, dhi - dlo):.2f} ms); layer evaluations per sequence: "
                  f"active rows {rows} = {sum(rows)}, evaluated {sum(evaluated)}, dense {3 * L}; workspace of one attached call {ws / 2 ** 20:.0f} MiB; "
                  f"max|d token_log_probs| active vs dense {diff:.2e}; {reps} alternated calls each, from coordinates", flush=True)
