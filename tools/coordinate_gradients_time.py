"""Time the coordinate gradients on cuda:0: train.forward_train + the label-smoothed loss + backward, from coordinates,
with and without X.requires_grad, medians [min, max] of alternated synchronised calls in one process after warm-up.

    python tools/coordinate_gradients_time.py [--reps 7] [--shapes b1,cfg5] [--prec x3,fp32]
        b1     (B, N, K) = (1, 1000, 48)
        cfg5   (B, N, K) = (16, 1500, 48), the training benchmark's shape
    --parent PATH   another build of the library (libnamp_hip.so of the parent commit) as a second library of this process: the step
                    without X.requires_grad runs alternated on both builds; this build's median - its median beside the larger min-max
                    spread of the two, and whether log_probs, the loss and every parameter gradient are its bits (K = 48 is a multiple of
                    16: the backward has no fp32 atomics and repeats its own bits).

Beside the extra time of the gradient the line gives the fp32-MFMA lower bound of the new launch: E * 128 * 5184 * 2 FLOP at 157 TFLOP/s,
scaled by the share of live (a, b) blocks per 64-edge tile (the presence words the launch skips dead blocks by).
"""
import ctypes, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


from na_mpnn_amd import hip, shard, spec, synth, train
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
dev = torch.device("cuda:0")
w = synth.make_weights(0)
RTI = spec.restype_to_int()
SHAPES = {"b1": (1, 1000, 48), "cfg5": (16, 1500, 48)}
PEAK_F32_MFMA = 157e12


def model(k, prec):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, dropout=0.0, atom_dict=spec.atom_dict(), restype_to_int=RTI,
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()})
    m = m.to(dev).train()
    m.message_precision = prec
    return m


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(calls, reps):
    for f in calls.values():
        f(); f()                                                        # warm-up: images packed, plans made, allocator filled
    t = {name: [] for name in calls}
    for _ in range(reps):                                               # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}


def batch(B, N):
    fd = shard.pad_batch([synth.make_complex(seed=900 + b, n=N, n_chains=4) for b in range(B)])
    fd["S"] = fd["S"].long()
    return {k_: v.to(dev) for k_, v in fd.items()}


def live_share(m, fd):
    """The share of (a, b) blocks that are live per 64-edge tile: popcount(residue-side atoms) * popcount(neighbour-side atoms) / 324."""
    with torch.no_grad():
        _, E_idx = train.edge_embedding(m, fd)
        _, M18 = train._atom_frames(m, fd["X"].float(), fd)
    B, L, K = E_idx.shape
    j = (E_idx.long() + (torch.arange(B, device=dev) * L)[:, None, None]).view(-1)
    i = torch.arange(B * L, device=dev).repeat_interleave(K)
    Mf = (M18.view(B * L, 18) != 0)
    E = B * L * K
    pad = (-E) % 64
    mi = torch.cat((Mf[i], Mf.new_zeros(pad, 18))).view(-1, 64, 18).any(1).sum(1)
    mj = torch.cat((Mf[j], Mf.new_zeros(pad, 18))).view(-1, 64, 18).any(1).sum(1)
    return float((mi * mj).double().mean() / 324.0)


def step_of(m, fd, randn, with_x, keep=None):
    rm, rn = train.polymer_restype_tables(RTI, 33, dev)
    no_loss = torch.tensor([RTI[t] for t in cpu_ref.NO_LOSS_TOKENS], device=dev)
    S, mfl = train._mask_for_loss(fd, no_loss)
    pm = {"protein": fd["protein_mask"], "dna": fd["dna_mask"], "rna": fd["rna_mask"]}

    def call():
        m.zero_grad(set_to_none=True)
        X = fd["X"].detach().clone().float().requires_grad_(with_x)
        with torch.enable_grad():
            lp, _ = train.forward_train(m, dict(fd, X=X), randn)
            _, loss = train.loss_smoothed(S, lp, mfl, pm, rm, rn, weight=0.1, tokens=2000.0, num_letters=lp.shape[-1])
            loss.backward()
        if keep is not None:
            keep[:] = [lp.detach(), loss.detach()] + [p.grad for p in m.parameters()]
    return call


reps = int(arg("--reps", "7"))
parent_lib = None
if arg("--parent", ""):
    parent_lib = ctypes.CDLL(arg("--parent", ""))
    for name, (res, args) in hip._PROTOTYPES.items():
        if hasattr(parent_lib, name):
            fn = getattr(parent_lib, name)
            fn.restype, fn.argtypes = res, args
    assert parent_lib.namp_abi_version() == hip.NAMP_ABI_VERSION
this_lib = hip.lib()


def on_parent(f):
    def call():
        hip._lib = parent_lib
        try:
            return f()
        finally:
            hip._lib = this_lib
    return call


for name in arg("--shapes", "b1,cfg5").split(","):
    B, N, K = SHAPES[name]
    fd = batch(B, N)
    randn = torch.randn(B, N, generator=torch.Generator().manual_seed(1)).to(dev)
    for prec in arg("--prec", "x3,fp32").split(","):
        m = model(K, prec)
        share = live_share(m, fd)
        E = B * N * K
        bound = E * 128 * 5184 * 2 * share / PEAK_F32_MFMA * 1e3
        k0, k1 = [], []
        calls = {"plain": step_of(m, fd, randn, False, k0), "with dX": step_of(m, fd, randn, True)}
        if parent_lib is not None:
            calls["parent"] = on_parent(step_of(m, fd, randn, False, k1))
        r = measure(calls, reps)
        p, x = r["plain"], r["with dX"]
        line = (f"{name} B={B} N={N} K={K} {prec}: step without X.requires_grad {p[0]:.3f} ms [{p[1]:.3f}, {p[2]:.3f}], with {x[0]:.3f} ms "
                f"[{x[1]:.3f}, {x[2]:.3f}]: extra {x[0] - p[0]:+.3f} ms for {E} edges, live-block share {share:.3f}, fp32-MFMA lower bound of "
                f"the new launch {bound:.3f} ms")
        if parent_lib is not None:
            q = r["parent"]
            same = len(k0) == len(k1) and all(torch.equal(a, b) for a, b in zip(k0, k1))
            line += (f"; parent {q[0]:.3f} ms [{q[1]:.3f}, {q[2]:.3f}]: this - parent {p[0] - q[0]:+.3f} ms (larger min-max spread of the two "
                     f"{max(p[2] - p[1], q[2] - q[1]):.3f} ms), the parent's bits: {same}")
        print(line + f"; {reps} alternated calls each, from coordinates", flush=True)
        del m
        torch.cuda.empty_cache()
