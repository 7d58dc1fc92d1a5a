"""Time ProteinMPNN.conditional_probs() on cuda:0: the cone kernels (namp_decoder_loo) against the dense L-stream form of the same
build, alternated in one process — medians of synchronised calls after warm-up —, beside one score() call on the same complex.

    python tools/conditional_time.py [--reps 5] [--prec x3,fp32] [--sizes 1000x48,1000x32,300x48,3000x48]
    rocprofv3 --kernel-trace --stats -d <dir> -o loo -- python tools/conditional_time.py --profile 1000x48
        (two warm-up calls and ONE traced steady-state cone call; tools/rocpd_summary.py reads the database, and --launches <db>
         lists the launches of the last call in order: the per-phase times)
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
