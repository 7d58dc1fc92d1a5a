"""Time context states — ProteinMPNN.sample() with state_S / state_mask beside state_weights — on cuda:0 against the
plain multi-state call of the SAME build and shape: the same backbones, once with the shared rows, once with per-state tokens on the
fixed third of the residues, once with those residues absent in the last state as well.  All calls start from coordinates; each
context form is alternated with the plain call in one process, synchronised, and reported as medians with their [min, max] spread
after warm-up; the two context forms alternated with each other show the cost of a call on NEW tensors (their check reads back once).

    python tools/context_states_time.py [--reps 7] [--sizes 2x500x48x1,4x250x48x8]        (M x L x K x batch_size)
    --parent DIR    a checkout of the parent commit with its library built: the plain multi-state call and the cfg1 design call (97
                    residues, K = 32, batch_size 1, forced draws) run in child processes, this tree and DIR in turn (two rounds of
                    --reps calls each); per call this build's median - the parent's beside the larger min-max spread of the two, and
                    whether the results are the parent's bits.
"""
import os, subprocess, sys, tempfile, time
import numpy as np, torch


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, arg("--package-root", HERE))          # (a child of --parent imports the parent's package)
from na_mpnn_amd import spec, synth                      # noqa: E402
from na_mpnn_amd.model import ProteinMPNN                # noqa: E402
torch.set_grad_enabled(False)
SHARED = ("S", "mask", "chain_mask", "R_idx", "chain_labels", "protein_mask", "dna_mask", "rna_mask", "R_polymer_type")
reps = int(arg("--reps", "7"))
sizes = arg("--sizes", "2x500x48x1,4x250x48x8").split(",")


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in synth.make_weights(0).items()})
    return m.to("cuda:0").eval()


def states_of(cx, M, seed):
    """Seeded smooth deformations of one complex (tools/tied_states_time.py): states whose neighbour lists differ."""
    rng = np.random.default_rng(seed)
    X = cx["X"].astype(np.float64)
    out, scale = [cx["X"]], max(1.0, float(np.abs(X).max()))
    for _ in range(1, M):
        D = sum(np.sin(X @ (rng.standard_normal(3) * 2.5 / scale) + rng.uniform(0, 6.28))[..., None] * rng.standard_normal(3) * 2.0 for _ in range(3))
        out.append(((X + D + 0.15 * rng.standard_normal(X.shape)) * cx["X_m"][:, :, None]).astype(np.float32))
    return np.stack(out)


def inputs(M, L, bs):
    """-> (the plain multi-state feature_dict, the same with per-state tokens, the same with per-state tokens and presence)."""
    dev = "cuda:0"
    cx = synth.make_complex(seed=3, n=L)
    fixed = np.arange(L - L // 3, L)                                    # the partner: the last third, fixed
    cx["chain_mask"][fixed] = 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    plain = {k: t(cx[k])[None] for k in SHARED}
    gen = torch.Generator().manual_seed(L)
    plain.update(batch_size=bs, temperature=0.1, symmetry_residues=[[]], symmetry_weights=[[]], X=t(states_of(cx, M, 11)),
                 X_m=t(cx["X_m"])[None].repeat(M, 1, 1), bias=torch.zeros(1, L, 33, device=dev),
                 randn=torch.randn(bs, L, generator=gen).to(dev), state_weights=[1.0] + [-0.5 / max(M - 1, 1)] * (M - 1))
    rng = np.random.default_rng(M)
    sS = np.tile(cx["S"], (M, 1))
    sS[1::2, fixed] = (sS[1::2, fixed] + 1 + rng.integers(0, 19, sS[1::2, fixed].shape)) % 20
    sm = np.tile(cx["mask"], (M, 1))
    sm[M - 1, fixed] = 0
    tokens = dict(plain, state_S=t(sS).long())
    both = dict(tokens, state_mask=t(sm), X=plain["X"] * t(sm)[:, :, None, None], X_m=plain["X_m"] * t(sm)[:, :, None])
    return plain, tokens, both


def cfg1_inputs():
    cx = synth.make_complex(seed=3, n=97, n_chains=1, frac_protein=0.0, frac_dna=0.0)
    fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None].to("cuda:0") for k_, v in cx.items()}
    fd.update(batch_size=1, temperature=0.1, bias=torch.zeros(1, 97, 33, device="cuda:0"), symmetry_residues=[[]], symmetry_weights=[[]],
              S_forced=fd["S"].long())                                 # (forced draws: two builds' results can be compared bit for bit)
    return fd


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(calls):
    for f in calls.values():
        f(); f()                                                        # warm-up: weights packed, workspaces allocated
    t = {name: [] for name in calls}
    for _ in range(reps):                                               # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    return t


def fmt(v):
    return f"{float(np.median(v)):.3f} ms [{min(v):.3f}, {max(v):.3f}]"


if "--child" in sys.argv:
    # one build's share of --parent: the plain multi-state call of every size and the cfg1 design call, timed, with their results
    out = {}
    for size in sizes:
        M, L, K, bs = map(int, size.split("x"))
        m, (plain, _, _) = model(K), inputs(M, L, bs)
        u = torch.rand(bs, L, generator=torch.Generator().manual_seed(1)).to("cuda:0")
        res = m._sample(plain, True, uniform=u)
        out["plain multi-state " + size] = (measure({"x": lambda: m.sample(plain)})["x"], {k: res[k].cpu() for k in ("S", "log_probs", "sampling_probs")})
    m, fd1 = model(32), cfg1_inputs()
    res = m.sample(fd1)
    out["cfg1 design call"] = (measure({"x": lambda: m.sample(fd1)})["x"], {k: res[k].cpu() for k in ("S", "log_probs")})
    torch.save(out, arg("--dump", ""))
    sys.exit(0)

if arg("--parent", ""):
    roots = {"this": HERE, "parent": os.path.abspath(arg("--parent", ""))}
    got = {k: {} for k in roots}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(2):
            for who, root in roots.items():                             # (a fresh child each: this process never opens the GPU)
                dump = os.path.join(tmp, f"{who}{rnd}.pt")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--package-root", root, "--dump", dump, "--reps", str(reps),
                                "--sizes", ",".join(sizes)], check=True, cwd=root, timeout=900)
                for name, (ts, res) in torch.load(dump, weights_only=False).items():
                    slot = got[who].setdefault(name, ([], res))
                    slot[0].extend(ts)
                    assert all(torch.equal(slot[1][k], res[k]) for k in res), (who, name, "differs between two processes of one build")
    for name in got["this"]:
        a, b = got["this"][name], got["parent"][name]
        same = all(torch.equal(a[1][k], b[1][k]) for k in a[1])
        spread = max(max(a[0]) - min(a[0]), max(b[0]) - min(b[0]))
        d = float(np.median(a[0]) - np.median(b[0]))
        print(f"parent check: {name} {fmt(a[0])}, parent {fmt(b[0])}: this - parent {d:+.3f} ms (larger min-max spread of the two "
              f"{spread:.3f} ms: {'within' if abs(d) <= spread else 'BEYOND'} it), the parent's bits: {same}; 2 x {reps} calls each in "
              "alternated processes, from coordinates", flush=True)
    sys.exit(0)

for size in sizes:
    M, L, K, bs = map(int, size.split("x"))
    m = model(K)
    plain, tokens, both = inputs(M, L, bs)
    u = torch.rand(bs, L, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    a, b = m._sample(plain, True, uniform=u), m._sample(tokens, True, uniform=u)
    # Each context form alternated with the plain call.  The model keeps the check of the context tensors for the LAST set of tensor
    # objects it saw (as it does for the tokens of S): a resident feature_dict is checked once.  Alternating the two context
    # feature_dicts with each other makes every call check anew — one read-back —: the third measurement, the cost on new tensors.
    forms = {"contexts (tokens)": tokens, "contexts (tokens + presence)": both}
    txt, verdicts = [], []
    for name, fd in forms.items():
        t = measure({"plain multi-state": lambda: m.sample(plain), name: lambda fd=fd: m.sample(fd)})
        base, mine = t["plain multi-state"], t[name]
        d = float(np.median(mine) - np.median(base))
        spread = max(max(mine) - min(mine), max(base) - min(base))
        txt.append(f"plain multi-state {fmt(base)}  {name} {fmt(mine)}")
        verdicts.append(f"{name} - plain {d:+.3f} ms ({'within' if d <= spread else 'BEYOND'} the larger min-max spread {spread:.3f} ms)")
    t = measure({name: (lambda fd=fd: m.sample(fd)) for name, fd in forms.items()})
    txt.append("checked anew on every call: " + "  ".join(f"{name} {fmt(v)}" for name, v in t.items()))
    print(f"M={M} L={L} K={K} batch_size={bs}: {'  |  '.join(txt)}  ({'; '.join(verdicts)}; {int(a['levels'])} levels, {a['work_items']} work items; "
          f"the tokens change the result: {not torch.equal(a['log_probs'], b['log_probs'])}; {reps} calls each, from coordinates)", flush=True)
