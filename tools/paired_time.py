"""Time base-paired design — ProteinMPNN.sample() with paired_residues: complementary tokens tied across two strands — on cuda:0:
the device plan (namp_pairs_plan + namp_pairs_work_lists) against the host route of the same build (symmetry_visits and
level_work_lists: a Python loop over the L visits and host read-backs per call), and against the same complex designed UNPAIRED by
plain sample() — the floor, and the parent build's code.  Synthetic backbones (synth.make_complex); all calls start from coordinates,
in split-bf16; they are alternated in one process, synchronised, and reported as medians with their [min, max] spread after warm-up.

    python tools/paired_time.py [--reps 7] [--sizes 300x20x32x1,0x150x48x8]     (protein residues x strand length x K x batch_size)

--wobble: the same shapes with an RNA duplex, the paired call (device plan) with paired_wobble on — the class tables of the sampler,
G-U pairs allowed — alternated with the same call with wobble off (the token maps: canonical pairs only).
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
w = synth.make_weights(0)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def model(k):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in w.items()}); return m.to(dev).eval()


def inputs(n_prot, n_strand, bs, rna=False):
    """A protein of n_prot residues (none for 0) with a DNA (rna: RNA) duplex of 2 x n_strand residues, the strands paired antiparallel."""
    L = n_prot + 2 * n_strand
    cx = synth.make_complex(seed=3, n=L, n_chains=1, frac_protein=n_prot / L, frac_dna=0.0 if rna else 2 * n_strand / L)
    cx["chain_labels"] = np.searchsorted([n_prot, n_prot + n_strand] if n_prot else [n_strand], np.arange(L), side="right").astype(np.int32)
    for c in range(int(cx["chain_labels"].max()) + 1):
        sel = cx["chain_labels"] == c
        cx["R_idx"][sel] = np.arange(sel.sum(), dtype=np.int32) + 100 * c
    fd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)[None] for k, v in cx.items()}
    fd.update(batch_size=bs, temperature=0.1, symmetry_residues=[[]], symmetry_weights=[[]], bias=torch.zeros(1, L, 33, device=dev),
              randn=torch.randn(bs, L, device=dev))
    pairs = [(n_prot + k, L - 1 - k) for k in range(n_strand)]
    return fd, dict(fd, paired_residues=pairs), pairs


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def time_wobble(m, n_prot, n_strand, K, bs, reps):
    """Wobble on against wobble off on an RNA duplex: medians of `reps` alternated synchronised calls, with what was drawn."""
    _, paired, pairs = inputs(n_prot, n_strand, bs, rna=True)
    calls = {"wobble on": lambda: m.sample(dict(paired, paired_wobble=True)), "wobble off": lambda: m.sample(paired)}
    torch.manual_seed(1); a = calls["wobble on"]()
    rti = spec.restype_to_int()
    i, j = (torch.tensor(v, device=dev) for v in zip(*pairs))
    comp = torch.tensor(spec.token_map(rti, "same"), device=dev)
    Si, Sj = a["S"][:, i], a["S"][:, j]
    canonical = Sj == comp[Si]
    gu = ((Si == rti["G"]) & (Sj == rti["U"])) | ((Si == rti["U"]) & (Sj == rti["G"]))
    for f in calls.values():
        f(); f()
    t = {name: [] for name in calls}
    for _ in range(reps):
        for name, f in calls.items():
            t[name].append(timed(f))
    med = {name: float(np.median(v)) for name, v in t.items()}
    txt = "  ".join(f"{name} {med[name]:.2f} ms [{min(v):.2f}, {max(v):.2f}]" for name, v in t.items())
    spread = max(max(v) - min(v) for v in t.values())
    print(f"protein={n_prot} RNA duplex=2x{n_strand} K={K} batch_size={bs}: {txt}  (on - off {med['wobble on'] - med['wobble off']:+.2f} ms, "
          f"larger min-max spread of the two {spread:.2f} ms; {int(a['levels'])} levels, {a['work_items']} work items; pairs drawn with "
          f"wobble on: {int(canonical.sum())} canonical, {int(gu.sum())} G-U, {int((~canonical & ~gu).sum())} other; {reps} calls each, "
          f"from coordinates)", flush=True)


reps = int(arg("--reps", "7"))
for size in arg("--sizes", "300x20x32x1,0x150x48x8").split(","):
    n_prot, n_strand, K, bs = map(int, size.split("x"))
    m = model(K)
    if "--wobble" in sys.argv:
        time_wobble(m, n_prot, n_strand, K, bs, reps)
        continue
    plain, paired, pairs = inputs(n_prot, n_strand, bs)

    def route(device_plan):
        m.sample_pairs_device_plan = device_plan
        return m.sample(paired)

    calls = {"device plan": lambda: route(True), "host route": lambda: route(False), "unpaired sample()": lambda: m.sample(plain)}
    torch.manual_seed(1); a = route(True)
    torch.manual_seed(1); b = route(False)
    same = bool(torch.equal(a["S"], b["S"]) and torch.equal(a["log_probs"], b["log_probs"]))
    comp = torch.tensor(spec.token_map(spec.restype_to_int(), "same"), device=dev)
    i, j = (torch.tensor(v, device=dev) for v in zip(*pairs))
    paired_ok = bool(torch.equal(a["S"][:, j], comp[a["S"][:, i]]))
    for f in calls.values():
        f(); f()                                                    # warm-up: weights packed, workspaces allocated
    t = {name: [] for name in calls}
    for _ in range(reps):                                           # alternated: a drift of the clocks hits every form alike
        for name, f in calls.items():
            t[name].append(timed(f))
    med = {name: float(np.median(v)) for name, v in t.items()}
    txt = "  ".join(f"{name} {med[name]:.2f} ms [{min(v):.2f}, {max(v):.2f}]" for name, v in t.items())
    spread = max(max(t[n]) - min(t[n]) for n in ("device plan", "host route"))
    print(f"protein={n_prot} duplex=2x{n_strand} K={K} batch_size={bs}: {txt}  (device - host {med['device plan'] - med['host route']:+.2f} ms, "
          f"larger min-max spread of the two {spread:.2f} ms; {int(a['levels'])} levels, {a['work_items']} work items device / "
          f"{b['work_items']} host; routes bit-identical: {same}; strands complementary: {paired_ok}; {reps} calls each, from coordinates)",
          flush=True)
