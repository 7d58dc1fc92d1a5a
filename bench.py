#!/usr/bin/env python
"""bench.py — residues/s of the NA-MPNN encoder+decoder forward on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg1|cfg2|cfg3|cfg4|cfg5] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W [--full]

A "step" is one pass of the hot path — (V, E, E_idx, S, mask, decoding ranks) -> log_probs, i.e.
W_v/W_e + 3 x EncLayer + decoder context + 3 x DecLayer + W_out + log_softmax — over
one batch of synthetic graphs already resident in HBM.  Default workload = BASELINE.json configs[1]
("cfg2": B=1, N=1000, K=48, H=128, 3+3 layers).  Every rank runs its own independent
complexes (weak scaling, no data-path collective); with --full, one RCCL all-gather of the arg-max
sequences at the end collates results for reporting, outside the timed region.

A plain run does only what the headline needs: it sets up, warms up, times the K steps, writes
--dump-outputs if given and prints the result line (the contract keys: `metric`, `value`, `unit`,
`ms_per_step`, `dtype`, ...).  Everything else below is measured only with `--full`.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment re-executes this file under
`torch.distributed.run` with N ranks (one per GPU, backend nccl = RCCL); under a launcher it uses
the launcher's ranks and refuses a WORLD_SIZE that contradicts --gpus.

The headline of cfg2 (`value`, `dtype` "f32") is the EXACT fp32 evaluation (v_mfma_f32_16x16x4_f32, what
BASELINE configs[1] states).  A --full cfg2 run times the path again with the same K / W: the `x3`
object beside the headline is the split-bf16 evaluation (three bf16 products per fp32 product, fp32-equivalent
to ~2^-16), the model's default.  With --full, rank 0 prints ONE COMPACT JSON line (< 6 KB) with the driver's contract keys plus
  roofline      – dominant kernel: EXECUTED FLOPs / HIP-event-measured duration vs the MFMA peak of its dtype (`frac`); the
                  rate of the reference's dense formulation (the launch executes about half of it) beside it as
                  `algorithmic_*`; `traffic` = HBM bytes per launch from two live rocprofv3 PMC passes of this very workload
  cpu_baseline  – the CPU oracle (oracle/cpu_ref.py, kind "port") timed on this box's host cores
  parity        – max |dlogp|, arg-max equality and sequence recovery vs the CPU oracle on the same inputs
  gather        – the standalone neighbour-gather (cat_neighbors_nodes) HBM figure, cfg3-shaped
  x3            – the split-bf16 evaluation of the same pass (cfg2 only)
  secondary     – short runs of cfg3 (bf16, B=64), cfg5 (training step), cfg1 (design call) and cfg4 (the split), N = 1 only
Everything longer (per-kernel tables, sample descriptions, the full line of every secondary workload) goes to
`--detail-out` (default gpurun_out/bench_detail.json when that directory exists) or to stdout's line with --verbose.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import na_mpnn_amd  # noqa: E402,F401   (first: sets HIP_FORCE_DEV_KERNARG before the HIP runtime initialises)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from na_mpnn_amd import hip, shard, spec, synth   # noqa: E402
from na_mpnn_amd.pack import PackedWeights        # noqa: E402

WORKLOADS = {"cfg1": dict(B=1, N=97, K=32), "cfg2": dict(B=1, N=1000, K=48), "cfg3": dict(B=64, N=1000, K=48), "cfg4": dict(B=1373, N=0, K=48),
             "cfg5": dict(B=16, N=1500, K=48)}
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0    # dense bf16 MFMA peak
PEAK_HBM_GBS = 8000.0             # HBM3E spec peak
# algorithmic FLOP / residue of the dense reference formulation, K=48, H=128
ALGO_FLOP = {"enc_message": 7_864_320, "enc_edge_update": 7_864_320, "dec_message": 9_437_184,
             "enc_edge_message": 15_728_640,       # fused launch: edge update of layer l-1 + message of layer l
             "enc_edge_dec_message": 7_864_320 + 9_437_184,    # last edge update + DecLayer 0 message
             # the persistent launch = the whole pass but the first residue-level launch (W_v + EncLayer 0's tables):
             # W_e + 3 x (EncLayer message + FFN + edge update) + 3 x (DecLayer message + FFN) + W_out
             "encdec_persistent": 78_684_416 - 32_768}
# per-edge 128 x 128 tile GEMMs a launch EXECUTES: the message MLP's third layer is linear and runs behind the K-sum, once per
# residue, so a message stage executes 2 per edge where the reference's formulation (ALGO_FLOP) has 3
EXEC_GEMMS = {"enc_message": 2, "enc_edge_update": 3, "dec_message": 2, "enc_edge_message": 5, "enc_edge_dec_message": 5,
              "encdec_persistent": 22}           # 1 (W_e) + 9 edge-update + 12 message GEMMs per edge
ALGO_FLOP_TOTAL = 78_684_416
# algorithmic HBM bytes per launch at cfg2 (N = 1000): h_E rows 48 x 128 x 4 B per residue and pass (message: one read;
# edge update: read + write), E_idx 192 B, residue rows 512 B each
TRAFFIC_ALGO = {"enc_message": 1000 * (24_576 + 192 + 4 * 512), "dec_message": 1000 * (24_576 + 192 + 8 + 4 * 512),
                "enc_edge_message": 1000 * (2 * 24_576 + 192 + 5 * 512), "enc_edge_dec_message": 1000 * (2 * 24_576 + 192 + 8 + 6 * 512)}
KERNEL_OF = {"encdec_persistent": "encdec_persistent_kernel"}      # launch kind -> kernel name when it is not edge_mlp_kernel
# executed FLOP / residue of the hoisted formulation (three 128x128 GEMMs per edge)
EXEC_FLOP_EDGE = 48 * 3 * 2 * 128 * 128
DUMP_BUDGET_BYTES = 60_000_000   # --dump-outputs: array bytes in all (the .npy files stay under 64 MB)


class Runner:
    """Owns the device tensors of one rank's batch and enqueues one step."""

    def __init__(self, dev, B, N, K, seed, precision="x3"):
        self.L = hip.lib()
        self.dev, self.B, self.N, self.K = dev, B, N, K
        w = synth.make_weights(0)
        self.w_np = w
        self.packed = PackedWeights({k: torch.from_numpy(v).to(dev) for k, v in w.items()}, 3, 3, spec.VOCAB, dev)
        self.packed.set_precision(precision)
        # graphs are generated one at a time to bound host memory at B=64
        parts = [synth.make_graph(seed=seed + b, batch=1, n=N, k=K) for b in range(B)]
        self.g_np = {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}
        d = {k: torch.from_numpy(v).to(dev) for k, v in self.g_np.items()}
        self.d = d
        order = torch.argsort((d["mask"] * d["chain_mask"] + 0.0001) * torch.abs(d["randn"]))
        rank = torch.empty_like(order)
        rank.scatter_(1, order, torch.arange(N, device=dev).expand(B, -1))
        self.rank = rank.to(torch.int32).contiguous()
        self.hV = torch.empty(B, N, 128, device=dev)
        self.hE = torch.empty(B, N, K, 128, device=dev)
        self.logp = torch.empty(B, N, spec.VOCAB, device=dev)
        self.ws = torch.empty(2 * self.L.namp_workspace_bytes(B, B, N, K), dtype=torch.uint8, device=dev)

    def step(self):
        d, L, s = self.d, self.L, hip.current_stream()
        B, N, K = self.B, self.N, self.K
        # one library call for the whole path (namp_encdec_fwd == namp_encoder_fwd + namp_decoder_fwd, fused across the
        # encoder/decoder boundary while the batch takes the fused residue tail)
        hip.check(L.namp_encdec_fwd(self.packed.model(), d["V"].data_ptr(), d["E"].data_ptr(), d["E_idx"].data_ptr(),
                                    d["mask"].data_ptr(), d["S"].data_ptr(), self.rank.data_ptr(), self.hV.data_ptr(),
                                    self.hE.data_ptr(), self.logp.data_ptr(), None, self.ws.data_ptr(), self.ws.numel(),
                                    B, N, K, s), "encdec_fwd")


def gather_microbench(dev, reps=10):
    """cat_neighbors_nodes at the cfg3 shape (B=64,N=1000,K=48,C=128|128): 1,540 B/edge algorithmic."""
    L = hip.lib()
    B, N, K = 64, 1000, 48
    hE = torch.randn(B, N, K, 128, device=dev)
    hV = torch.randn(B, N, 128, device=dev)
    idx = torch.randint(0, N, (B, N, K), device=dev, dtype=torch.int32)
    out = torch.empty(B, N, K, 256, device=dev)
    s = hip.current_stream()
    run = lambda: hip.check(L.namp_cat_neighbors_nodes_f32(hV.data_ptr(), hE.data_ptr(), idx.data_ptr(), out.data_ptr(),
                                                           B, N, K, 128, 128, s))
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nbytes = B * N * K * 1540 + B * N * 128 * 4
    gbs = nbytes / (ms * 1e-3) / 1e9
    # the practical ceiling on this box: a device-to-device copy of the same order of bytes (3.1 GB read + written)
    src, dst = out.view(-1)[: hE.numel()], hE.view(-1)
    for _ in range(2):
        dst.copy_(src)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy_gbs = 2 * src.numel() * 4 / (e0.elapsed_time(e1) / reps * 1e-3) / 1e9
    del hE, hV, idx, out, src, dst
    torch.cuda.empty_cache()
    return {"kernel": "gather_cat_kernel", "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(gbs / PEAK_HBM_GBS, 4), "bytes_per_launch": nbytes, "ms_per_launch": round(ms, 4),
            "shape": "B=64 N=1000 K=48 C=128|128 fp32", "traffic": None,
            "d2d_copy_GBps": round(copy_gbs, 1), "frac_of_d2d_copy": round(gbs / copy_gbs, 3)}


def pmc_child():
    """`bench.py --pmc-child`: the launches whose HBM traffic the parent reads from rocprofv3's PMC passes — three cfg2 passes in
    exact fp32, three in split-bf16, two gather launches at the cfg3 shape.  Prints nothing."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    for prec in ("fp32", "x3"):
        r = Runner(dev, 1, 1000, 48, seed=3, precision=prec)
        for _ in range(3):
            r.step()
        torch.cuda.synchronize()
        del r
    gather_microbench(dev, reps=1)
    torch.cuda.synchronize()
    m = _feat_model(dev)
    fd = _feat_inputs(dev, "cfg4")
    for _ in range(2):
        m._featurize_hip(fd, want_E=False, want_hE=True)
    torch.cuda.synchronize()


# edge_mlp_kernel<MODE, TAIL, PREC, PRE> -> launch kind (PREC 0 = exact fp32, 2 = split-bf16)
PMC_KIND = {(0, 1): "enc_message", (0, 3): "enc_edge_message", (1, 3): "enc_edge_dec_message", (1, 0): "dec_message"}


def live_pmc_traffic(timeout_s=150):
    """HBM-side bytes per launch, measured in THIS run: two rocprofv3 passes (FETCH_SIZE and WRITE_SIZE need separate passes,
    MI355X_MICROARCH.md) over `bench.py --pmc-child`; bytes = 2 x FETCH_SIZE KB (gfx950 counts a wide read's 128-B request as
    64 B) + WRITE_SIZE KB, averaged over the dispatches of a kernel.  Returns ({"fp32": {kind: bytes}, "x3": {...},
    "gather": bytes}, source-description) or (None, reason)."""
    import re
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    from collections import defaultdict
    if os.environ.get("NAMP_BENCH_NO_PMC") == "1" or any(k.startswith("ROCPROFILER_") or k.startswith("ROCP_") for k in os.environ):
        return None, "skipped (NAMP_BENCH_NO_PMC=1 or already under a profiler)"
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    per = {}
    tmp = tempfile.mkdtemp(prefix="namp_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", NAMP_BENCH_NO_PMC="1")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__), "--pmc-child"]
            p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            dbs = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
            if p.returncode != 0 or not dbs:
                return None, f"rocprofv3 --pmc {counter} failed (rc {p.returncode}): {p.stderr[-200:]}"
            rows = sqlite3.connect(dbs[0]).execute("select kernel_name, dispatch_id, counter_name, value from counters_collection").fetchall()
            acc = defaultdict(float)
            for k, disp, c, v in rows:
                if c == counter:
                    acc[(re.sub(r"\(.*", "", k), disp)] += v
            agg = defaultdict(list)
            for (k, _), v in acc.items():
                agg[k].append(v)
            per[counter] = {k: sum(v) / len(v) for k, v in agg.items()}
    except Exception as e:                                       # noqa: BLE001 — a failed profile must not take the line down
        return None, f"{type(e).__name__}: {e}"[:200]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {"fp32": {}, "x3": {}, "gather": None, "features": None}
    for k in set(per["FETCH_SIZE"]) | set(per["WRITE_SIZE"]):
        nbytes = round((2 * per["FETCH_SIZE"].get(k, 0.0) + per["WRITE_SIZE"].get(k, 0.0)) * 1024)
        m = re.search(r"edge_mlp_kernel<(\d+), (\d+), (\d+), (\d+)>", k)
        if m:
            mode, tail, prec, pre = map(int, m.groups())
            kind = PMC_KIND.get((mode, pre))
            if kind and tail:
                out["x3" if prec == 2 else "fp32"][kind] = nbytes
        if "gather_cat_kernel" in k:
            out["gather"] = nbytes
        if "edge_features_kernel" in k:
            out["features"] = nbytes
    return out, "live: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (two passes) over `bench.py --pmc-child` in this run; bytes = 2 x FETCH_SIZE KB + WRITE_SIZE KB"


# featuriser (a11 / f1): algorithmic work per residue at K = 48 — 5200 -> 128 edge-embedding GEMM + positional, and the RBF exps
FEAT_FLOP_ALGO = 63_897_600 + 101_376
FEAT_EXP_ALGO = 248_832


def _feat_model(dev):
    from na_mpnn_amd.model import ProteinMPNN
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=48, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    return m.to(dev).eval()


def _feat_inputs(dev, which):
    """cfg2 from coordinates: one synthetic 1000-residue complex (70 % protein / 15 % DNA / 15 % RNA, 4 chains); cfg4 batch: the middle
    token-bucket batch (<= 32,000 padded tokens) of the design_test-sized split, as split_bench forms it."""
    if which == "cfg2":
        cx = synth.make_complex(seed=77, n=1000, n_chains=4)
        return {k: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k, v in cx.items()}
    lengths = shard.synthetic_lengths()
    bs_ = shard.token_batches(lengths, indices=list(range(len(lengths))), max_tokens=32000)
    b = bs_[len(bs_) // 2]                                   # a middle batch of the length-sorted walk (the first holds ~600 50-residue chains)
    return shard.pad_batch([synth.make_complex(seed=40000 + i, n=int(lengths[i]), n_chains=1 + i % 4) for i in b], device=dev)


def _feat_executed_flop(fd, E_idx, x3_products=3):
    """FLOPs edge_features_kernel EXECUTES on this input (csrc/namp_kernels.h): per 16-neighbour tile of residue i, for every atom a
    present on i and every pair of neighbour atoms (b0, b0 + 1) present on any of the tile's neighbours, one K = 32 step over 8 channel
    tiles (2 x 16 x 32 x 128 FLOP, x the three bf16 products of a split product) — structurally-zero atom pairs are skipped — plus the
    positional tile and the fused W_e product (fp32-equivalent K = 16 + 128)."""
    Xm = fd["X_m"] > 0
    na = (fd["dna_mask"] + fd["rna_mask"]) > 0
    M18 = torch.cat([Xm, (fd["protein_mask"] > 0)[..., None], na[..., None]], -1) & (fd["mask"] > 0)[..., None]     # [B, L, 18]
    B, L, K = E_idx.shape
    bidx = torch.arange(B, device=E_idx.device)[:, None, None]
    Mj = M18[bidx, E_idx.long()]                                                       # [B, L, K, 18]
    pad = (-K) % 16
    if pad:
        Mj = torch.cat([Mj, Mj.new_zeros(B, L, pad, 18)], 2)
    tile_any = Mj.view(B, L, -1, 16, 18).any(3)                                        # [B, L, tiles, 18]
    pairs = (tile_any[..., 0::2] | tile_any[..., 1::2]).sum(-1)                        # live (b0, b0+1) steps per tile
    n_a = M18.sum(-1)[..., None]                                                       # atoms present on residue i
    steps = float((pairs * n_a).sum())
    tiles = float(B * L * tile_any.shape[2])
    return steps * 2 * 16 * 32 * 128 * x3_products + tiles * 2 * 16 * (16 + 128) * 128 * x3_products


def features_bench(dev):
    """The `features` object of the default line: edge_features_kernel — the dominant launch of the fused featuriser
    (model_utils.py:489-593; 27 % of a cfg4 pass) — timed from the device trace of one featurise call at cfg2-from-coordinates and at a
    32,000-token cfg4 batch; `frac` prices the FLOPs it executes against the bf16 dense MFMA peak (its products run as split-bf16),
    `algorithmic_frac` the dense formulation of SURVEY 8(d) (63.9 MFLOP + 248,832 exp per TOKEN: the launch walks every token of the padded batch;
    `algorithmic_frac_unmasked_residues` prices the unmasked residues only)."""
    from torch.profiler import profile, ProfilerActivity
    m = _feat_model(dev)
    res = {"kernel": "edge_features_kernel", "bound": "mfma", "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "basis": "executed FLOPs",
           "traffic": None}
    for which in ("cfg2", "cfg4"):
        fd = _feat_inputs(dev, which)
        for _ in range(2):
            out = m._featurize_hip(fd, want_E=False, want_hE=True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = m._featurize_hip(fd, want_E=False, want_hE=True)
            torch.cuda.synchronize()
        t = {}
        for ev in prof.key_averages():
            us = getattr(ev, "self_device_time_total", None)
            if us is None:
                us = getattr(ev, "self_cuda_time_total", 0.0)
            for name in ("edge_features_kernel", "feat_finish_kernel", "knn_select_kernel", "knn_kernel", "prep_atoms_kernel"):
                if name in ev.key:
                    t[name] = t.get(name, 0.0) + us / 1e3
        # one complex runs its edge-feature launch in parts (round 6): the finishing launch (sum of the partial rows, LayerNorm, W_e) is priced with it
        ef = t.get("edge_features_kernel", 0.0) + t.get("feat_finish_kernel", 0.0)
        residues = int((fd["mask"] > 0).sum())
        tokens = int(fd["mask"].numel())
        ex = _feat_executed_flop(fd, out[3])
        tag = "cfg2_from_X" if which == "cfg2" else "cfg4_batch"
        res[tag] = {"tokens": tokens, "residues": residues, "avg_launch_ms": round(ef, 4),
                    "frac": round(ex / max(ef, 1e-9) / 1e9 / PEAK_BF16_MFMA_TFLOPS, 4),
                    "algorithmic_frac": round(FEAT_FLOP_ALGO * tokens / max(ef, 1e-9) / 1e9 / PEAK_BF16_MFMA_TFLOPS, 4),
                    "algorithmic_frac_unmasked_residues": round(FEAT_FLOP_ALGO * residues / max(ef, 1e-9) / 1e9 / PEAK_BF16_MFMA_TFLOPS, 4),
                    "gexp_per_s": round(FEAT_EXP_ALGO * residues / max(ef, 1e-9) / 1e6, 1),
                    "finish_launch_ms": round(t.get("feat_finish_kernel", 0.0), 4),
                    "knn_select_ms": round(t.get("knn_select_kernel", t.get("knn_kernel", 0.0)), 4),
                    "prep_atoms_ms": round(t.get("prep_atoms_kernel", 0.0), 4)}
        if which == "cfg2":
            # the GPU partner of cpu_baseline.full_forward_from_X ("features timed separately AND as full forward"): score() from
            # coordinates — featuriser + encoder + decoder, the same synthetic complex (synth.make_complex(seed=77, n=1000, n_chains=4)) —
            # 20 calls back to back between two device syncs after 5 warm-up calls, randn fixed
            fd["batch_size"] = 1
            fd["randn"] = torch.randn(1, tokens, generator=torch.Generator().manual_seed(7)).to(dev)
            for _ in range(5):
                sc = m.score(fd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                sc = m.score(fd)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 20
            res["full_forward_from_X"] = {"value": round(residues / dt, 1), "unit": "residues/s", "ms_per_call": round(dt * 1e3, 4),
                                          "dtype": "bf16x3 (the product default: split-bf16 products, fp32-equivalent to 2^-16 — the headline beside it is exact fp32)"
                                                   if getattr(m, "message_precision", "x3") == "x3" else "f32",
                                          "sample": f"ProteinMPNN.score() from coordinates (HIP featuriser + enc + dec), the cpu_baseline complex "
                                                    f"({tokens} residues, K=48), 20 calls after 5 warm-up calls",
                                          "finite": bool(torch.isfinite(sc["log_probs"]).all())}
            del sc
        del fd, out
    big = res["cfg4_batch"]
    res.update({"achieved": round(big["frac"] * PEAK_BF16_MFMA_TFLOPS, 2), "frac": big["frac"], "algorithmic_frac": big["algorithmic_frac"],
                "avg_launch_ms": big["avg_launch_ms"]})
    del m
    torch.cuda.empty_cache()
    return res


def seq_recovery(S_true, S_pred, mask):
    """get_seq_rec of the reference (inference/data_utils.py:18-30): sum(match * mask) / sum(mask) per complex."""
    match = (S_true == S_pred).to(torch.float32)
    m = mask.to(torch.float32)
    return (match * m).sum(-1) / m.sum(-1)


def parity_vs_cpu(logp_gpu, ref_out, S_true, mask):
    """Parity side-metric of BASELINE.json's `metric`: the designed (arg-max) sequence vs the CPU reference path's on
    identical inputs — identical arg-max, and the sequence recovery (vs the native S) of both."""
    lp, rp = logp_gpu.float().cpu(), ref_out["log_probs"]
    seq_g, seq_c = lp.argmax(-1), rp.argmax(-1)
    return {"max_abs_dlogp_vs_cpu": round(float((lp - rp).abs().max()), 7),
            "argmax_equal": bool(torch.equal(seq_g, seq_c)),
            "seq_recovery": {"gpu_vs_cpu_argmax": round(float(seq_recovery(seq_c, seq_g, mask).mean()), 6),
                             "gpu_vs_native": round(float(seq_recovery(S_true, seq_g, mask).mean()), 6),
                             "cpu_vs_native": round(float(seq_recovery(S_true, seq_c, mask).mean()), 6),
                             "definition": "get_seq_rec, inference/data_utils.py:18-30 (random-init weights: recovery vs "
                                           "the native sequence is chance level; the graded number is gpu_vs_cpu_argmax)"}}


def cpu_baseline(runner, budget_s=25.0):
    """The oracle on this box's host cores, same cfg2 inputs (bounded sample): best intra-op thread count, one thread,
    and the full forward from coordinates (features + enc + dec: `cpu_ref.score`) — SURVEY 8(d) / BASELINE.md §3."""
    from oracle import cpu_ref
    w = {k: torch.from_numpy(v) for k, v in runner.w_np.items()}
    g = {k: torch.from_numpy(v[:1]) for k, v in runner.g_np.items()}
    E_idx = g["E_idx"].long()
    f = lambda: cpu_ref.encdec_from_graph(w, g["V"], g["E"], E_idx, g["S"], g["mask"], g["chain_mask"], g["randn"])
    n = g["V"].shape[1]
    K = int(E_idx.shape[-1])
    ncpu = os.cpu_count() or 1
    # eager PyTorch on a many-core host is fastest well below the core count at this problem size:
    # try a few intra-op thread counts inside the time budget and report the best one.
    best, out, tried, t_start = None, None, [], time.perf_counter()
    with torch.no_grad():
        for nt in [t for t in (8, 16, 32, 64) if t <= max(ncpu, 8)]:
            if time.perf_counter() - t_start > budget_s:
                break
            torch.set_num_threads(min(nt, ncpu))
            out = f()                                       # warm-up at this thread count
            times = []
            for _ in range(3):
                t0 = time.perf_counter(); out = f(); times.append(time.perf_counter() - t0)
                if time.perf_counter() - t_start > budget_s:
                    break
            tried.append((min(nt, ncpu), min(times)))
            if best is None or min(times) < best[1]:
                best = (min(nt, ncpu), min(times))
        # one thread (the scalar-port figure)
        torch.set_num_threads(1)
        t0 = time.perf_counter(); f(); t_one = time.perf_counter() - t0
        # full forward from coordinates: features (kNN, 18x18x16 RBFs, 5200 -> 128 embedding) + enc + dec
        torch.set_num_threads(best[0])
        cx = synth.make_complex(seed=77, n=n, n_chains=4)
        fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None] for k, v in cx.items()}
        fd["batch_size"] = 1
        t0 = time.perf_counter(); cpu_ref.score(w, fd, K); t_full = time.perf_counter() - t0
    return out, {"value": round(n / best[1], 1), "unit": "residues/s", "cores": best[0], "kind": "port",
                 "sample": f"oracle/cpu_ref.py enc+dec forward, B=1 N={n} K={K} fp32, eager PyTorch CPU, "
                           f"best of <=3 after 1 warm-up per thread count; tried (threads, s): "
                           + ", ".join(f"({a}, {b:.3f})" for a, b in tried) + f"; host has {ncpu} logical cores",
                 "one_thread": {"value": round(n / t_one, 1), "unit": "residues/s", "cores": 1,
                                "sample": f"same forward, torch.set_num_threads(1), one run ({t_one:.2f} s)"},
                 "full_forward_from_X": {"value": round(n / t_full, 1), "unit": "residues/s", "cores": best[0],
                                         "sample": f"oracle/cpu_ref.py score() from coordinates (features + enc + dec), one "
                                                   f"synthetic {n}-residue complex, one run ({t_full:.2f} s)"}}


# algorithmic FLOP / residue of one training step at K=48 (SURVEY §8(d) figures): forward (enc+dec 78.7 M + features
# 64.0 M) + backward = 2 x forward (data + weight gradients) ; the recompute the reference's checkpointing implies is
# NOT counted (it is overhead, not algorithmic work).
TRAIN_FLOP_FWD = 78_684_416 + 63_897_600 + 101_376
TRAIN_FLOP_STEP = 3 * TRAIN_FLOP_FWD
# dominant kernel of the step: edge_chain_bwd_kernel — per edge 5 GEMMs of 2*128*128 executed (2 recompute + 3 dgrad);
# algorithmic = the 3 data-gradient GEMMs
BWD_FLOP_EDGE_ALGO = 3 * 2 * 128 * 128
BWD_FLOP_EDGE_EXEC = 5 * 2 * 128 * 128


def train_step_profile(m, step, B, N, K):
    """--full, cfg5: one more training step under the device profiler -> the roofline of the per-edge backward launches and the
    per-kernel table of the step."""
    from na_mpnn_amd import train
    # dominant kernel, timed live with HIP events on the launch stream (torch's current stream)
    from na_mpnn_amd import hip as H_
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(); torch.cuda.synchronize()
    kern = {}
    for ev in prof.key_averages():
        t_us = getattr(ev, "self_device_time_total", None)
        if t_us is None:
            t_us = getattr(ev, "self_cuda_time_total", 0.0)
        if t_us > 0:
            kern[ev.key] = (t_us / 1e3, ev.count)
    ours = {k: v for k, v in kern.items() if any(s in k for s in ("edge_chain_bwd", "edge_bwd_dw", "edge_update_bwd_", "reduce_sum_kernel", "pack_multi", "pos_grad", "pos_features", "radj_", "adam_", "loss_smoothed", "wgrad_kernel", "feat_wgrad", "edge_features",
                                                                  "edge_mlp_kernel", "edge_mlp_x3_persistent", "edge_mlp_bf16", "knn_kernel", "knn_select", "pack_image", "pack_feat", "scatter_rows",
                                                                  "prep_atoms", "wgrad_x3", "wgrad_bf16", "tail_train", "tile_presence", "cvt_tables", "ln_rows", "node_update", "node_linear",
                                                                  "embed_ln_bwd", "class_sums", "wcolsum"))}
    total_dev_ms = sum(v[0] for v in kern.values())
    # the per-edge backward launches.  128 x 128 GEMM-equivalents per edge row — (executed, algorithmic = data + weight gradients):
    #   edge_bwd_dw*           message stage owning its weight gradients: 2 recompute + 2 data-gradient + 2 weight-gradient  (6, 4)
    #   edge_chain_bwd<0|1>    message stage of rounds 1-3 (weight gradients in separate launches)                            (4, 2)
    #   edge_chain_bwd<2|3>    three-layer stage / EncLayer edge update: 3 recompute + 3 data-gradient                        (6, 3)
    #   edge_update_bwd_a16    edge update, launch A: 3 recompute + W13^T + the dW13 contraction                                   (5, 2)
    #   edge_update_bwd_b16    edge update, launch B: 1 recompute + W12^T, W11b^T + the dW12, dW11b contractions                   (5, 4)
    def gemms_of(name):
        if "edge_update_bwd_a16" in name:
            return 5, 2
        if "edge_update_bwd_b16" in name:
            return 5, 4
        if "edge_bwd_dw" in name:
            return 6, 4
        return (4, 2) if ("edge_chain_bwd_kernel<0" in name or "edge_chain_bwd_kernel<1" in name) else (6, 3)
    bwd = [(k, v) for k, v in ours.items() if "edge_chain_bwd" in k or "edge_bwd_dw" in k or "edge_update_bwd_" in k]
    bwd_ms = sum(v[0] for _, v in bwd); bwd_n = sum(v[1] for _, v in bwd)
    avg_s = bwd_ms / max(bwd_n, 1) * 1e-3
    edges = B * N * K
    mp = getattr(m, "message_precision", "x3")
    x3 = mp != "fp32"                                       # bf16 pipe; "x3": 3 bf16 MFMAs per algorithmic product, "bf16": 1
    peak = PEAK_BF16_MFMA_TFLOPS if x3 else PEAK_F32_MFMA_TFLOPS
    gemm_flop = 2 * 128 * 128 * edges
    # (split-bf16: the edge update's backward walks the batch in train.EDGE_UPDATE_SLICES slices — a launch covers that fraction of the edges)
    cover = lambda k: 1.0 / min(B, train.EDGE_UPDATE_SLICES) if ("edge_chain_bwd_kernel<3" in k and mp == "x3") else 1.0
    exec_flop = sum(gemms_of(k)[0] * v[1] * cover(k) for k, v in bwd) * gemm_flop * (3 if mp == "x3" else 1)
    algo_flop = sum(gemms_of(k)[1] * v[1] * cover(k) for k, v in bwd) * gemm_flop
    exec_tf = exec_flop / max(bwd_ms, 1e-9) / 1e9
    algo_tf = algo_flop / max(bwd_ms, 1e-9) / 1e9
    dom_b = max(bwd, key=lambda kv: kv[1][0])[0] if bwd else "edge_chain_bwd_kernel"
    roofline = {"kernel": dom_b.replace("void ", "")[:48], "bound": "mfma",
                "achieved": round(exec_tf, 3), "peak": peak, "unit": "TFLOP/s",
                "frac": round(exec_tf / peak, 4), "basis": "executed FLOPs", "executed_frac": round(exec_tf / peak, 4),
                "algorithmic_achieved": round(algo_tf, 3), "algorithmic_frac": round(algo_tf / peak, 4), "traffic": None,
                "avg_launch_ms": round(avg_s * 1e3, 4), "launches_per_step": bwd_n,
                "note": "all per-edge backward launches of the step together; algorithmic = data- and weight-gradient GEMMs per edge, "
                        "executed adds the recomputed forward GEMMs (the reference's checkpoint-recompute policy) and counts the "
                        "three bf16 products of a split product; durations from the device trace of one step"}
    return {"roofline": roofline,
            "per_kernel_ms_per_step": {k: round(v[0], 3) for k, v in sorted(ours.items(), key=lambda kv: -kv[1][0])},
            "device_ms_per_step": round(total_dev_ms, 3), "hip_kernel_share": round(sum(v[0] for v in ours.values()) / total_dev_ms, 3),
            "other_kernels_ms_per_step": {k[:90]: [round(v[0], 3), v[1]] for k, v in sorted(((k, v) for k, v in kern.items() if k not in ours),
                                                                                     key=lambda kv: -kv[1][0])[:16]}}


def train_bench(args, dev, rank, world, dist):
    """BASELINE configs[4] ("cfg5"): one optimisation step of na_run.py:198-238 — featurise, forward, label-smoothed loss,
    backward, gradient clip, Noam/Adam — on B x N synthetic residues per rank, dropout 0.1, coordinate noise 0.1 A."""
    from na_mpnn_amd import train
    from na_mpnn_amd.model import ProteinMPNN
    cfg = WORKLOADS["cfg5"]
    B, N, K = cfg["B"], cfg["N"], cfg["K"]
    rti = spec.restype_to_int()
    torch.manual_seed(1234 + rank)
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=K, dropout=0.1, augment_eps=0.1, atom_dict=spec.atom_dict(),
                    restype_to_int=rti, polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    m.to(dev).train()
    if getattr(args, "precision", None):
        m.message_precision = args.precision          # "bf16" = the mixed-precision mode (na_run.py MIXED_PRECISION)
    cxs = [synth.make_complex(seed=5000 + 100 * rank + b, n=N, n_chains=4) for b in range(B)]
    fd = {k: torch.from_numpy(np.stack([c[k] for c in cxs])).to(dev) for k in cxs[0]}
    fd["S"] = fd["S"].long()
    opt = train.get_std_opt(m.parameters(), 128, 0)
    rm, rn = train.polymer_restype_tables(rti, 33, dev)
    no_loss = torch.tensor([rti[t] for t in ("UNK", "DX", "RX", "MAS", "PAD")], device=dev)
    torch.set_grad_enabled(True)

    def step():
        return train.train_step(m, opt, fd, rm, rn, no_loss, label_smoothing=0.1, loss_tokens=6000.0, gradient_norm=1.0,
                                data_parallel=dist is not None)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    quiet_gc.collect()
    torch.cuda.reset_peak_memory_stats()                 # peak_mem_gib is this workload's own peak (the secondary runs share the process)
    for _ in range(args.warmup):
        step()
    barrier()
    with quiet_gc():
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, _ = step()
        torch.cuda.synchronize()
        barrier()
        elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=coll_device(dev, dist), dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / args.steps * 1e3
    value = world * B * N * args.steps / elapsed
    mp = getattr(m, "message_precision", "x3")
    out = {"metric": "residues/sec trained (featurise + fwd + bwd + clip + Noam/Adam), N=1500 K=48 h=128", "value": round(value, 1),
           "unit": "residues/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": {"x3": "bf16x3 (per-edge GEMMs of forward, backward and weight gradients as split-bf16 products, fp32 accumulate; fp32 elsewhere)",
                     "bf16": "bf16 mixed precision (per-edge GEMMs as plain bf16 products, fp32 accumulate; fp32 master weights, "
                             "residue-level math, loss and optimiser)", "fp32": "f32"}[mp],
           "data": "synthetic",
           "config": {"workload": f"cfg5: B={B} x N={N} residues per rank, K={K}, H=128, 3+3 layers, dropout 0.1, coordinate noise 0.1, "
                                  "label smoothing 0.1, seeded random-init weights; N > 1: data parallel, one RCCL "
                                  "all-reduce of the 9.2 MB gradient bucket per step (the reference trains single-GPU)",
                      "global_batch": B * world, "seq_len": N, "parallelism": f"dp{world}"}}
    if args.full:
        out.update(train_step_profile(m, step, B, N, K))
    out["whole_step"] = {"algorithmic_tflops": round(TRAIN_FLOP_STEP * B * N / (ms_per_step * 1e-3) / 1e12, 2),
                         "final_loss": round(float(loss), 5),
                         "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if rank == 0 and not args.no_cpu_baseline and world == 1 and args.full:
        out["cpu_baseline"] = cpu_train_baseline(cxs[0], K, rti)
    torch.set_grad_enabled(False)
    return out


def split_bench(args, dev, rank, world, dist):
    """BASELINE configs[3] ("cfg4"): the design_test split (1,373 complexes; synthetic coordinates of the split's size
    distribution) sharded over the ranks by LPT as independent complexes; each complex runs the whole
    path FROM COORDINATES (featurise + encode + decode, `ProteinMPNN.score`), and one RCCL all-gather collates the
    arg-max sequences.  A "step" is one pass over the rank's shard (strong scaling: total work fixed)."""
    from na_mpnn_amd.model import ProteinMPNN
    lengths = shard.synthetic_lengths()
    if args.split_limit:
        lengths = lengths[:args.split_limit]
    mine = shard.lpt_assign(lengths, world)[rank]
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=48, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    m.to(dev).eval()
    # token-bucket batches inside the shard (the reference's StructureLoader rule, na_data_utils.py:1405-1426)
    batches = shard.token_batches(lengths, indices=mine, max_tokens=args.batch_tokens)
    fds = []
    for b in batches:
        cxs = [synth.make_complex(seed=40000 + i, n=int(lengths[i]), n_chains=1 + i % 4) for i in b]
        fd = shard.pad_batch(cxs, device=dev)
        fd["batch_size"] = 1
        fd["randn"] = torch.from_numpy(np.random.default_rng(b[0]).standard_normal(tuple(fd["mask"].shape)).astype(np.float32)).to(dev)
        fds.append(fd)
    result = {}

    def step():
        for b, fd in zip(batches, fds):
            seq = m.score(fd)["log_probs"].argmax(-1)
            for row, i in enumerate(b):
                result[i] = seq[row, :int(lengths[i])]

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    quiet_gc.collect()
    for _ in range(max(args.warmup, 1)):
        step()
    # Strong scaling divides one pass by the rank count (~40 ms per pass at N = 8): a timed region of a few passes would be
    # decided by launch latency and the slowest rank's jitter.  The pass count is therefore scaled so that the timed region
    # lasts >= --min-seconds on the SLOWEST rank (every rank uses the same count: MAX all-reduce of one calibration pass).
    barrier()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    t_pass = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([t_pass], device=coll_device(dev, dist), dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t_pass = float(t.item())
    steps_requested = args.steps
    args.steps = max(args.steps, int(np.ceil(args.min_seconds / max(t_pass, 1e-6))))
    barrier()
    with quiet_gc():
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        my_elapsed = time.perf_counter() - t0                 # this rank's own passes, before waiting for the others
        barrier()
        elapsed = time.perf_counter() - t0
    my_res = int(sum(lengths[i] for i in mine))
    if dist is not None:
        t = torch.tensor([elapsed], device=coll_device(dev, dist), dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    total_res = int(lengths.sum())
    out = {"metric": "residues/sec (featurise + enc + dec forward from coordinates), design_test-sized split", "unit": "residues/s",
           "value": round(total_res * args.steps / elapsed, 1), "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "bf16x3 (GEMMs as split-bf16 products, fp32 accumulate: fp32-equivalent to 2^-16; fp32 elsewhere)" if getattr(m, "message_precision", "x3") == "x3" else "f32", "data": "synthetic",
           "config": {"workload": f"cfg4: {len(lengths)} complexes, {total_res} residues (N_i log-uniform 50..3000), K=48, one "
                                  "score() from coordinates per token-bucket batch, LPT shards, no data-path collective",
                      "global_batch": len(lengths), "seq_len": int(np.median(lengths)), "parallelism": f"independent complexes x{world}"}}
    if not args.full:
        return out
    # --full: the shard's per-rank figures and the collation of the designed sequences
    per_rank = [[float(my_res), my_elapsed]]
    if dist is not None:
        mine_t = torch.tensor([float(my_res), my_elapsed], device=coll_device(dev, dist), dtype=torch.float64)
        allr = [torch.empty_like(mine_t) for _ in range(world)]
        dist.all_gather(allr, mine_t)
        per_rank = [[float(a[0]), float(a[1])] for a in allr]
    t1 = time.perf_counter()
    collated = shard.all_gather_ragged(result, len(lengths), device=coll_device(dev, dist))
    torch.cuda.synchronize()
    gather_ms = (time.perf_counter() - t1) * 1e3
    n_coll = sum(int(x.numel()) for x in collated if x is not None)
    rr, rs = [a[0] for a in per_rank], [a[1] for a in per_rank]
    out["shard"] = {"rank0_complexes": len(mine), "rank0_batches": len(batches), "batch_tokens": args.batch_tokens, "rank0_residues": my_res,
                    "ideal_residues_per_rank": total_res // world, "steps_requested": steps_requested, "calibration_pass_s": round(t_pass, 4),
                    "per_rank_residues": {"min": int(min(rr)), "mean": round(sum(rr) / len(rr), 1), "max": int(max(rr))},
                    "per_rank_seconds": {"min": round(min(rs), 4), "mean": round(sum(rs) / len(rs), 4), "max": round(max(rs), 4)},
                    "lpt_imbalance": round(max(rr) / (sum(rr) / len(rr)), 4)}
    out["collation"] = {"collective": "all_reduce(lengths) + all_gather(padded int32 sequences)", "ms": round(gather_ms, 3),
                        "backend": (dist.get_backend() if dist is not None else None),
                        "ranks": (dist.get_world_size() if dist is not None else 1), "residues_collated": n_coll}
    assert n_coll == total_res, (n_coll, total_res)
    return out


def design_bench(args, dev, rank, world, dist, specificity=False):
    """BASELINE configs[0] on the GPU: the design call of inference/run.py (`model.sample(feature_dict)`, run.py:367) on a
    4oqu-sized complex (97 RNA residues, K=32, batch_size 1, T=0.1), from coordinates: featurise + encode + sample.
    specificity=True ("cfg1s"): the reference's second inference mode (run.py:559-583) — batch_size 30, T 0.6 — on a 1am9-sized complex
    (389 residues: 313 protein + 76 DNA in 8 chains)."""
    from na_mpnn_amd.model import ProteinMPNN
    n, K, bs = 97, 32, args.design_batch
    temp = 0.1
    if specificity:
        n, bs, temp = 389, 30, 0.6
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=K, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()})
    m.to(dev).eval()
    if specificity:
        cx = synth.make_complex(seed=40 + rank, n=n, n_chains=8, frac_protein=313 / 389, frac_dna=76 / 389)   # 1am9-shaped
    else:
        cx = synth.make_complex(seed=4 + rank, n=n, n_chains=1, frac_protein=0.0, frac_dna=0.0)          # one RNA chain, like 4oqu
    fd = {k: torch.from_numpy(np.ascontiguousarray(v))[None].to(dev) for k, v in cx.items()}
    fd.update({"batch_size": bs, "temperature": temp, "bias": torch.zeros(1, n, 33, device=dev),
               "symmetry_residues": [[]], "symmetry_weights": [[]]})

    def step():
        fd["randn"] = torch.randn(bs, n, device=dev)
        return m.sample(fd)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    quiet_gc.collect()
    for _ in range(args.warmup):
        step()
    barrier()
    with quiet_gc():
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        torch.cuda.synchronize()
        barrier()
        elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=coll_device(dev, dist), dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # --full: latency of ONE synchronised design call (the timed region above issues the calls back to back: pipelined throughput — the
    # host enqueues call i + 1 while call i runs): median of 20 calls, each bracketed by device syncs
    lat = []
    if args.full:
        with quiet_gc():
            for _ in range(20):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                lat.append(time.perf_counter() - t1)
        lat.sort()
    res = {"metric": "sampled residues/sec (design: featurise + encode + autoregressive sample), " + ("1am9-sized complex, specificity mode" if specificity else "4oqu-sized complex"),
           **({"latency_ms": round(lat[len(lat) // 2] * 1e3, 3), "latency_ms_min": round(lat[0] * 1e3, 3)} if lat else {}),
           "value": round(world * bs * n * args.steps / elapsed, 1), "unit": "residues/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "bf16x3 (GEMMs as split-bf16 products, fp32 accumulate: fp32-equivalent to 2^-16; fp32 elsewhere)" if getattr(m, "message_precision", "x3") == "x3" else "f32", "data": "synthetic",
           "config": {"workload": (f"cfg1s: model.sample() on one {n}-residue protein-DNA complex (8 chains), K={K}, batch_size={bs}, T={temp} "
                                   "(run.py:559-583 specificity mode), from coordinates; level-parallel decoding" if specificity else
                                   f"cfg1: model.sample() on one {n}-residue RNA chain, K={K}, batch_size={bs}, T=0.1, from "
                                   "coordinates; level-parallel decoding"), "global_batch": bs * world, "seq_len": n,
                      "parallelism": f"replicas x{world}"},
           "levels": (int(out["levels"]) if out.get("levels") is not None else None)}
    if rank == 0 and not args.no_cpu_baseline and world == 1 and args.full:
        if True:
            from oracle import cpu_ref
            torch.set_num_threads(min(8, os.cpu_count() or 1))
            w = {k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()}
            fdc = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}
            bs_cpu = bs if specificity else 1
            fdc["batch_size"] = bs_cpu; fdc["randn"] = fdc["randn"][:bs_cpu]
            with torch.no_grad():
                if not specificity:
                    cpu_ref.sample(w, fdc, K)                # warm-up (the specificity call is ~10 s: one timed run)
                t1 = time.perf_counter(); cpu_ref.sample(w, fdc, K); dt = time.perf_counter() - t1
            res["cpu_baseline"] = {"value": round(bs_cpu * n / dt, 1), "unit": "residues/s", "cores": torch.get_num_threads(), "kind": "port",
                                   "sample": f"oracle/cpu_ref.py features + encode + sample(), one {n}-residue complex, batch_size {bs_cpu}, "
                                             f"eager PyTorch CPU ({dt:.2f} s)"}
    return res


def cpu_train_baseline(cx, K, rti, n=300):
    """The oracle's training step (autograd through oracle/cpu_ref.py + Adam) on the host: B=1, first n residues."""
    from oracle import cpu_ref
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    w = {k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()}
    fd = {k: torch.from_numpy(np.ascontiguousarray(v[:n]))[None] for k, v in cx.items()}
    fd["S"] = fd["S"].long()
    randn = torch.randn(1, n)
    params = [torch.nn.Parameter(v.clone()) for v in w.values()]
    adam = torch.optim.Adam(params, lr=1e-4, betas=(0.9, 0.98), eps=1e-9)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        wl = dict(zip(w.keys(), [p.detach() for p in params]))
        _, _, grads = cpu_ref.train_loss_and_grads(wl, fd, K, randn, rti, tokens=6000.0)
        for p, k in zip(params, w.keys()):
            p.grad = grads[k]
        adam.step()
        times.append(time.perf_counter() - t0)
    return {"value": round(n / min(times), 1), "unit": "residues/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle/cpu_ref.py training step (features + fwd + loss + autograd bwd + Adam), B=1 N={n} K={K}, "
                      f"eager PyTorch CPU, best of 3 ({', '.join(f'{t:.2f}s' for t in times)})"}


class quiet_gc:
    """Python's cyclic garbage collector paused over a timed region (collected before the warm-up steps, re-enabled after): a generation-2 pass
    over the process's ~10^6 objects stalls the launching thread for 90-150 ms — one such pass inside a 4-step cfg5 region doubles the
    reported step time (measured: 40 steps, one 100 ms outlier with the collector on, none with it off; profiles/r04e)."""

    @staticmethod
    def collect():
        """Call BEFORE the warm-up steps, never between warm-up and t0: a full collection walks ~10^6 objects and leaves the host's
        caches cold — the first launches behind it enqueue slower than the device executes them, which put ~0.9 ms of device idle
        into a 20-step cfg2 region (0.483 -> 0.528 ms per step, HEAD and the round-3 kernels alike; profiles/r05a_region_probe.md)."""
        import gc
        gc.collect()

    def __enter__(self):
        import gc
        self._was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()


class ClockSampler:
    """Shader clock (MHz) the device reports while a timed region runs: a host thread polls the driver's current-sclk reading
    (torch.cuda.clock_rate -> amdsmi, else the starred level of pp_dpm_sclk in sysfs) every millisecond.  Peaks are quoted at the
    2.4 GHz maximum; DVFS runs loaded kernels lower (MI355X_MICROARCH.md "DVFS give-back"), so `frac` is also given rescaled to the
    measured clock.  Returns None when the box exposes neither interface."""

    def __init__(self, dev):
        import glob
        import threading
        self.samples, self._stop = [], threading.Event()
        self._idx = dev.index or 0
        self._sysfs = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
        self._th = threading.Thread(target=self._run, daemon=True)

    def _read(self):
        try:
            return float(torch.cuda.clock_rate(self._idx))
        except Exception:                                       # noqa: BLE001
            pass
        for f in self._sysfs[self._idx:self._idx + 1] or self._sysfs[:1]:
            try:
                for ln in open(f).read().splitlines():
                    if ln.strip().endswith("*"):
                        return float(ln.split(":")[1].strip().split("M")[0])
            except Exception:                                   # noqa: BLE001
                pass
        return None

    def _run(self):
        while not self._stop.is_set():
            v = self._read()
            if v:
                self.samples.append(v)
            time.sleep(0.001)

    def __enter__(self):
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._th.join(timeout=1.0)

    def mean(self):
        return round(sum(self.samples) / len(self.samples)) if self.samples else None


def capture_outputs(runner):
    """Host float32 copies of what one step hands its caller (log_probs, h_V, h_E), at most DUMP_BUDGET_BYTES in all.  An array
    that does not fit the rest of the budget is replaced by a fixed, seeded sample of its rows (last axis kept whole), stored
    with the flat row indices beside it as `<name>_rows` (float64, exact)."""
    out, left = {}, DUMP_BUDGET_BYTES
    for name, t in (("log_probs", runner.logp), ("h_V", runner.hV), ("h_E", runner.hE)):
        rows = t.reshape(-1, t.shape[-1])
        row_bytes = rows.shape[1] * 4
        if rows.shape[0] * row_bytes <= left:
            out[name] = t.float().cpu().numpy()
            left -= out[name].nbytes
            continue
        n = min(rows.shape[0], left // (row_bytes + 8))
        idx = np.sort(np.random.default_rng(0).choice(rows.shape[0], size=n, replace=False))
        out[name] = rows[torch.from_numpy(idx).to(t.device)].float().cpu().numpy()
        out[name + "_rows"] = idx.astype(np.float64)
        left -= out[name].nbytes + out[name + "_rows"].nbytes
    return out


def write_outputs(outputs, directory):
    os.makedirs(directory, exist_ok=True)
    for name, a in outputs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(directory, f"{name}.npy"), a)


def coll_device(dev, dist):
    """Device of the collectives' buffers: the GPU under RCCL; host memory when the harness is exercised over gloo."""
    return torch.device("cpu") if (dist is not None and dist.get_backend() == "gloo") else dev


def encdec_bench(args, dev, rank, world, dist, workload, precision, steps, warmup, profile_steps=None, capture=False, full=True):
    """Time `steps` passes of the encoder+decoder forward (one namp_encdec_fwd call each) at `precision`.  capture=True keeps
    host copies of the last timed step's outputs in `runner.outputs` (see capture_outputs).  full=False returns the headline keys
    only; full=True adds the polled clock, the collation of the arg-max sequences and the event-instrumented per-kernel pass
    behind `roofline` / `per_kernel`."""
    cfg = WORKLOADS[workload]
    B, N, K = cfg["B"], cfg["N"], cfg["K"]
    cfg_idx = 1 if workload == "cfg2" else 2
    runner = Runner(dev, B, N, K, seed=1 + cfg_idx + 1000 * rank, precision=precision)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # set-up, not measurement: bring the device out of its idle clocks before the W warm-up steps (a 20-step timed region of
    # this path is ~10 ms — one clock ramp inside it shows as +25 %; measured once in profiles/r02i)
    quiet_gc.collect()
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.05:
        runner.step()
        torch.cuda.synchronize()
    for _ in range(warmup):
        runner.step()
    barrier()
    with quiet_gc():
        t0 = time.perf_counter()
        for _ in range(steps):
            runner.step()
        torch.cuda.synchronize()
        barrier()
        elapsed = time.perf_counter() - t0
    if capture:
        runner.outputs = capture_outputs(runner)         # outside the timed region, before any further step
    if dist is not None:
        t = torch.tensor([elapsed], device=coll_device(dev, dist), dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / steps * 1e3
    value = world * B * N * steps / elapsed
    dtype = {"fp32": "f32", "x3": "bf16x3 (per-edge GEMMs as three bf16 products of split fp32 operands, fp32 accumulate: "
                                   "fp32-equivalent to 2^-16; fp32 everywhere else)",
             "bf16": "bf16 (per-edge GEMMs; fp32 accumulate, fp32 elsewhere)"}[precision]
    out = {"metric": "residues/sec (enc+dec fwd), N~1000 K=48 h=128; seq-recovery vs CPU ref", "value": round(value, 1),
           "unit": "residues/s", "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": round(ms_per_step, 4),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": dtype, "data": "synthetic",
           "config": {"workload": f"{workload}: B={B} x N={N} residues per rank, K={K}, H=128, 3 enc + 3 dec layers, "
                                  f"per-edge GEMMs {precision}, seeded random-init weights, independent complexes per rank",
                      "precision": precision, "global_batch": B * world, "seq_len": N, "parallelism": f"replicas x{world}"}}
    if not full:
        return out, runner
    # the clock under this workload (outside the timed region: ~0.2 s of the same steps with a poller thread beside them)
    clock_mhz = None
    if rank == 0:
        with ClockSampler(dev) as cs:
            t_c = time.perf_counter()
            while time.perf_counter() - t_c < 0.2:
                runner.step()
            torch.cuda.synchronize()
        clock_mhz = cs.mean()

    # reporting-only collective: all-gather of the arg-max sequences (north_star: "RCCL all-gather ... only
    # for throughput reporting"); outside the timed region.
    seq = runner.logp.argmax(-1)
    local = {rank * B + b: seq[b] for b in range(B)}              # complex id -> designed sequence
    t1 = time.perf_counter()
    collated = shard.all_gather_ragged(local, world * B, device=coll_device(dev, dist))
    torch.cuda.synchronize()
    gather_ms = (time.perf_counter() - t1) * 1e3
    n_collated = sum(int(x.numel()) for x in collated if x is not None)
    assert n_collated == world * B * N, (n_collated, world, B, N)

    # per-kernel durations: the same steps again with the library's HIP-event hook on the launch stream (a second,
    # event-instrumented pass: its sum sits a few percent above ms_per_step, which has no events between launches)
    psteps = profile_steps or max(steps, 50)
    runner.L.namp_profile_enable(1)
    for _ in range(psteps):
        runner.step()
    prof = hip.profile_collect()
    runner.L.namp_profile_enable(0)
    per_kernel = {k: {"launches_per_step": c // psteps, "avg_ms": round(ms / max(c, 1), 5),
                      "ms_per_step": round(ms / psteps, 5)} for k, (ms, c) in prof.items() if c}
    dom = max((k for k in per_kernel if k in ALGO_FLOP), key=lambda k: per_kernel[k]["ms_per_step"])
    avg_s = per_kernel[dom]["avg_ms"] * 1e-3
    algo = ALGO_FLOP[dom] * B * N
    # fp32: exact fp32 MFMA (peak 157.3).  x3 / bf16: the products run on the bf16 pipe (dense peak 2500); x3 executes three
    # bf16 products per fp32 product.  `achieved` / `frac` price the FLOPs the launch EXECUTES (hoisted first layer, layer 3
    # behind the K-sum: about half of the reference's dense formulation) — the matrix-pipe utilisation; the rate of the dense
    # formulation of SURVEY 8(d) is reported beside it as algorithmic_*.
    peak = PEAK_F32_MFMA_TFLOPS if precision == "fp32" else PEAK_BF16_MFMA_TFLOPS
    mult = 3 if precision == "x3" else 1
    exec_flop = EXEC_FLOP_EDGE * B * N * EXEC_GEMMS[dom] // 3 * mult
    roofline = {"kernel": f"{KERNEL_OF.get(dom, 'edge_mlp_kernel')}<{dom}>", "bound": "mfma", "achieved": round(exec_flop / avg_s / 1e12, 3),
                "peak": peak, "unit": "TFLOP/s", "frac": round(exec_flop / avg_s / 1e12 / peak, 4),
                "basis": "executed FLOPs", "executed_frac": round(exec_flop / avg_s / 1e12 / peak, 4),
                "algorithmic_achieved": round(algo / avg_s / 1e12, 3), "algorithmic_frac": round(algo / avg_s / 1e12 / peak, 4),
                "traffic": None, "flop_per_launch_algorithmic": algo, "flop_per_launch_executed": exec_flop,
                "avg_launch_ms": per_kernel[dom]["avg_ms"], "launch_kind": dom}
    if clock_mhz:
        roofline["clock_mhz"] = clock_mhz
        roofline["frac_at_measured_clock"] = round(roofline["frac"] * 2400.0 / max(float(clock_mhz), 1.0), 4)
    out.update({"roofline": roofline, "per_kernel": per_kernel,
                "per_kernel_note": f"separate event-instrumented pass of {psteps} steps (HIP events around every launch)",
                "whole_path": {"algorithmic_tflops": round(ALGO_FLOP_TOTAL * B * N / (ms_per_step * 1e-3) / 1e12, 3),
                               "ms_per_step_instrumented_pass": round(sum(v["ms_per_step"] for v in per_kernel.values()), 5)},
                "collation": {"collective": "all_reduce(lengths) + all_gather(padded int32 arg-max sequences), outside the timed region",
                              "backend": (dist.get_backend() if dist is not None else None),
                              "ranks": (dist.get_world_size() if dist is not None else 1),
                              "collated_residues": n_collated, "expected_residues": world * B * N, "ms": round(gather_ms, 3)}})
    return out, runner


def secondary_runs(args, dev):
    """Short runs of the other single-GPU workloads, so that their numbers are in the driver's record too (N = 1 only).
    Each entry is a full bench line of that workload (its own metric / roofline / cpu_baseline) or {"error": ...}."""
    import copy
    res = []
    # (step counts: every timed region >= ~0.15 s — at 6 steps of 5 ms cfg3 read 5.35 ms where 30 steps read 5.0: fixed start / drain cost)
    for wl, steps, warm in (("cfg3", 30, 5), ("cfg5", 6, 3), ("cfg1", 40, 5), ("cfg1s", 20, 3), ("cfg4", 1, 1)):
        a = copy.copy(args)
        a.steps, a.warmup, a.workload = steps, warm, ("cfg1" if wl == "cfg1s" else wl)
        t0 = time.perf_counter()
        try:
            if wl == "cfg3":
                o, r = encdec_bench(a, dev, 0, 1, None, "cfg3", "bf16", steps, warm, profile_steps=steps)
                lp = r.logp
                o["checks"] = {"rows_normalised_max_err": round(float((lp.exp().sum(-1) - 1).abs().max()), 7),
                               "finite": bool(torch.isfinite(lp).all())}
                del r
            elif wl == "cfg5":
                a.precision = None
                o = train_bench(a, dev, 0, 1, None)
                a2 = copy.copy(a)
                a2.precision, a2.no_cpu_baseline = "bf16", True
                o2 = train_bench(a2, dev, 0, 1, None)            # the mixed-precision mode of the same step
                o["mixed_precision_bf16"] = {k: o2[k] for k in ("value", "ms_per_step", "dtype", "hip_kernel_share", "roofline")}
                o["mixed_precision_bf16"]["final_loss"] = o2["whole_step"]["final_loss"]
                o["mixed_precision_bf16"]["peak_mem_gib"] = o2["whole_step"]["peak_mem_gib"]
            elif wl == "cfg4":
                a.min_seconds = 0.0                              # one pass over the split (BASELINE configs[3] at N = 1)
                o = split_bench(a, dev, 0, 1, None)
            else:
                o = design_bench(a, dev, 0, 1, None, specificity=(wl == "cfg1s"))
        except Exception as e:          # a failing secondary must not take the headline down with it
            o = {"workload": wl, "error": f"{type(e).__name__}: {e}"[:400]}
        o["wall_s"] = round(time.perf_counter() - t0, 1)
        res.append(o)
        torch.cuda.empty_cache()
    return res


def short_dtype(d):
    return str(d).split(" (")[0]


def compact_roofline(r):
    keep = ("kernel", "bound", "achieved", "peak", "unit", "frac", "basis", "algorithmic_achieved", "algorithmic_frac", "traffic",
            "traffic_algorithmic", "avg_launch_ms", "clock_mhz", "frac_at_measured_clock")
    return {k: r[k] for k in keep if k in r}


def compact_secondary(o):
    """What the driver's record needs of a secondary workload; the full line goes to the detail file."""
    if "error" in o:
        return o
    wl = o.get("config", {}).get("workload", "")
    c = {"workload": wl.split(":")[0], "value": o["value"], "unit": o["unit"], "ms_per_step": o["ms_per_step"], "steps": o["steps"],
         "dtype": short_dtype(o["dtype"])}
    if "latency_ms" in o:                                     # design calls: one synchronised call (ms_per_step is pipelined throughput)
        c["latency_ms"] = o["latency_ms"]
    if "roofline" in o:
        r = o["roofline"]
        c["roofline"] = {"kernel": r["kernel"], "frac": r["frac"], "algorithmic_frac": r.get("algorithmic_frac"),
                         "avg_launch_ms": r.get("avg_launch_ms")}
        if "clock_mhz" in r:
            c["roofline"]["clock_mhz"] = r["clock_mhz"]
            if "frac_at_measured_clock" in r:                     # (the chip runs the bf16 batch at ~1.94 GHz: the peak it is priced on assumes 2.4)
                c["roofline"]["frac_at_measured_clock"] = r["frac_at_measured_clock"]
    if "cpu_baseline" in o:
        c["cpu_baseline"] = o["cpu_baseline"]["value"]
    for k in ("hip_kernel_share", "checks", "levels"):
        if k in o:
            c[k] = o[k]
    if "whole_step" in o:
        c["peak_mem_gib"] = o["whole_step"]["peak_mem_gib"]
        c["final_loss"] = o["whole_step"]["final_loss"]
    if "mixed_precision_bf16" in o:
        m = o["mixed_precision_bf16"]
        c["mixed_precision_bf16"] = {"value": m["value"], "ms_per_step": m["ms_per_step"], "hip_kernel_share": m.get("hip_kernel_share"),
                                     "peak_mem_gib": m.get("peak_mem_gib")}
    if "shard" in o:
        c["batches"] = o["shard"]["rank0_batches"]
        c["residues"] = o["collation"]["residues_collated"]
    c["wall_s"] = o.get("wall_s")
    return c


def compact_line(out):
    """The one JSON line rank 0 prints: contract keys first, then roofline / cpu_baseline / parity / gather / x3, then the
    secondaries — all short; per-kernel tables and sample descriptions stay in the detail file."""
    c = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "latency_ms", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data", "config") if k in out}
    c["dtype"] = short_dtype(c["dtype"])
    if "roofline" in out:
        c["roofline"] = compact_roofline(out["roofline"])
        if "traffic_source" in out["roofline"]:
            c["roofline"]["traffic_source"] = out["roofline"]["traffic_source"][:60]
    if "cpu_baseline" in out:
        cb = out["cpu_baseline"]
        c["cpu_baseline"] = {"value": cb["value"], "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                             "sample": cb["sample"][:110]}
        if "one_thread" in cb:
            c["cpu_baseline"]["one_thread"] = cb["one_thread"]["value"]
            c["cpu_baseline"]["full_forward_from_X"] = cb["full_forward_from_X"]["value"]
            gf = (out.get("features") or {}).get("full_forward_from_X")
            if gf:                                            # its GPU partner: score() from coordinates on the same complex (features_bench)
                c["cpu_baseline"]["gpu_full_forward_from_X"] = gf["value"]
                c["cpu_baseline"]["gpu_full_forward_ms"] = gf["ms_per_call"]
                c["cpu_baseline"]["gpu_full_forward_dtype"] = short_dtype(gf.get("dtype", "bf16x3"))
    if "parity" in out:
        pr = out["parity"]
        c["parity"] = {"max_abs_dlogp_vs_cpu": pr["max_abs_dlogp_vs_cpu"], "argmax_equal": pr["argmax_equal"],
                       "seq_recovery_gpu_vs_cpu_argmax": pr["seq_recovery"]["gpu_vs_cpu_argmax"]}
    if "gather" in out:
        g = out["gather"]
        c["gather"] = {k: g[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "bytes_per_launch", "ms_per_launch",
                                         "traffic", "d2d_copy_GBps")}
    if "features" in out:
        f = out["features"]
        c["features"] = {k: f[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "algorithmic_frac", "avg_launch_ms", "traffic",
                                           "traffic_algorithmic") if k in f}
        for tag in ("cfg2_from_X", "cfg4_batch"):
            if tag in f:
                c["features"][tag] = {k: f[tag][k] for k in ("tokens", "avg_launch_ms", "finish_launch_ms", "frac", "algorithmic_frac", "knn_select_ms") if k in f[tag]}
        if "full_forward_from_X" in f:
            c["features"]["full_forward_from_X"] = {k: f["full_forward_from_X"][k] for k in ("value", "unit", "ms_per_call")}
            c["features"]["full_forward_from_X"]["dtype"] = short_dtype(f["full_forward_from_X"].get("dtype", "bf16x3"))
    if "x3" in out:
        x = out["x3"]
        c["x3"] = {"value": x["value"], "ms_per_step": x["ms_per_step"], "dtype": "bf16x3", "kernel": x["roofline"]["kernel"],
                   "executed_frac": x["roofline"]["frac"], "algorithmic_frac": x["roofline"]["algorithmic_frac"],
                   "avg_launch_ms": x["roofline"]["avg_launch_ms"], "traffic": x["roofline"].get("traffic")}
        if "parity" in x:
            c["x3"]["max_abs_dlogp_vs_cpu"] = x["parity"]["max_abs_dlogp_vs_cpu"]
            c["x3"]["argmax_equal"] = x["parity"]["argmax_equal"]
    if "x3_persistent_launch" in out:
        c["x3_persistent_launch_ms"] = out["x3_persistent_launch"]["ms_per_step"]
    for k in ("hip_kernel_share", "levels"):
        if k in out:
            c[k] = out[k]
    if "whole_step" in out:
        c["whole_step"] = out["whole_step"]
    if "mixed_precision_bf16" in out:
        c["mixed_precision_bf16"] = out["mixed_precision_bf16"]
    if "shard" in out:
        c["shard"] = out["shard"]
    if "collation" in out:
        co = out["collation"]
        c["collation"] = {k: co[k] for k in ("backend", "ranks", "collated_residues", "expected_residues", "residues_collated", "ms") if k in co}
    if "cfg4_strong" in out:
        c["cfg4_strong"] = out["cfg4_strong"]
    if "secondary" in out:
        c["secondary"] = [compact_secondary(o) for o in out["secondary"]]
    return c


def respawn(args):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default per workload; cfg2: 500 = 0.25 s — a 20-50-step region reads 4-10 %% high: ~1 ms of fixed start / drain cost)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default 20 for cfg2, 5 otherwise)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2")
    ap.add_argument("--specificity", action="store_true", help="with --workload cfg1: the specificity-mode call (cfg1s: batch_size 30, T 0.6, 389 residues)")
    ap.add_argument("--precision", choices=["x3", "fp32", "bf16"], default=None,
                    help="per-edge GEMM evaluation of the headline: default fp32 for cfg2 (exact fp32 MFMA, BASELINE configs[1]; with "
                         "--full the x3 evaluation is timed beside it), bf16 for cfg3 (BASELINE configs[2]); x3 = split-bf16 products")
    ap.add_argument("--design-batch", type=int, default=1, help="cfg1: batch_size of the design call")
    ap.add_argument("--split-limit", type=int, default=0, help="cfg4: use only the first n complexes of the split")
    ap.add_argument("--batch-tokens", type=int, default=32000,
                    help="cfg4: padded-token budget per batch inside a shard (32,000 tokens = 0.8 GB of h_E: sized for 288 GB of HBM; "
                         "measured 2.66 / 2.76 / 2.91 / 2.85 M residues/s at 8,000 / 16,000 / 32,000 / 64,000)")
    ap.add_argument("--min-seconds", type=float, default=1.0,
                    help="cfg4: the pass count is raised until the timed region lasts at least this long on the slowest rank")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline: per-kernel / roofline pass, clock, collation, PMC traffic, gather and "
                         "featuriser figures, CPU baselines and parity, the x3 evaluation, design-call latency, the secondary workloads "
                         "(N = 1) or cfg4_strong (N > 1).  Off: set-up, warm-up, the timed steps, --dump-outputs and the result line only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines and the parity against the CPU oracle")
    ap.add_argument("--no-pmc", action="store_true", help="with --full: skip the two live rocprofv3 PMC passes behind roofline.traffic")
    ap.add_argument("--verbose", action="store_true", help="print the full detail (per-kernel tables, every secondary line) instead of the compact line")
    ap.add_argument("--detail-out", default=None, help="file for the full detail (default: gpurun_out/bench_detail.json when gpurun_out/ exists)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-gather", action="store_true", help="with --full: skip the gather and featuriser figures")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the persistent-launch run and the short cfg3 / cfg5 / cfg1 / cfg4 runs (N = 1), cfg4_strong (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="cfg2 / cfg3: write what the headline's last timed step computed (log_probs, h_V, h_E of rank 0; float32, "
                         "< 64 MB in all, a seeded row sample of what does not fit) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.dump_outputs and args.workload not in ("cfg2", "cfg3"):
        raise SystemExit(f"bench.py: --dump-outputs covers the encoder+decoder workloads cfg2 / cfg3, not {args.workload}")
    # default step counts per workload: the timed region is >= ~0.2 s everywhere (cfg5: a training step is ~100x a cfg2 forward)
    if args.steps is None:
        args.steps = {"cfg2": 500, "cfg3": 50, "cfg1": 20, "cfg4": 2, "cfg5": 10}.get(args.workload, 50)
    if args.warmup is None:
        args.warmup = 20 if args.workload == "cfg2" else 5
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.pmc_child:
        return pmc_child()

    launched = "WORLD_SIZE" in os.environ
    if not launched and args.gpus > 1:
        respawn(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} contradicts the launcher's WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    # NAMP_BENCH_ONE_DEVICE=1 / NAMP_BENCH_BACKEND=gloo: validate the N>1 code path on a single-GPU box
    if os.environ.get("NAMP_BENCH_ONE_DEVICE") == "1":
        local = 0
    elif local >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants device {local} but only {torch.cuda.device_count()} are visible "
                         "(NAMP_BENCH_ONE_DEVICE=1 shares device 0 between ranks for harness tests)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("NAMP_BENCH_BACKEND", "nccl")       # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    torch.set_grad_enabled(False)

    if dist is not None:
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
        # one process per GPU over RCCL whenever the node has more than one device; gloo is only for the one-device harness tests
        if torch.cuda.device_count() > 1 and os.environ.get("NAMP_BENCH_ONE_DEVICE") != "1":
            assert dist.get_backend() == "nccl", f"multi-GPU run must collate over RCCL (backend nccl), got {dist.get_backend()}"

    def finish(out):
        if rank == 0:
            assert out["n_gpus"] == world == args.gpus
            detail = args.detail_out or (os.path.join(ROOT, "gpurun_out", f"bench_detail_{args.workload}.json")
                                         if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else None)
            if not (args.full or args.detail_out):
                detail = None                           # a plain run writes no file beside --dump-outputs
            if detail:
                try:
                    with open(detail, "w") as f:
                        json.dump(out, f, indent=1)
                except OSError:
                    detail = None
            line = out if args.verbose else compact_line(out)
            if detail and not args.verbose:
                line["detail_file"] = os.path.relpath(detail, ROOT)
            print(json.dumps(line), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()

    if args.workload == "cfg1":
        return finish(design_bench(args, dev, rank, world, dist, specificity=bool(getattr(args, "specificity", False))))
    if args.workload == "cfg4":
        args.warmup = min(args.warmup, 1)
        return finish(split_bench(args, dev, rank, world, dist))
    if args.workload == "cfg5":
        return finish(train_bench(args, dev, rank, world, dist))

    precision = args.precision or ("bf16" if args.workload == "cfg3" else "fp32")
    out, runner = encdec_bench(args, dev, rank, world, dist, args.workload, precision, args.steps, args.warmup,
                               capture=bool(args.dump_outputs) and rank == 0, full=args.full)
    if args.dump_outputs and rank == 0:
        write_outputs(runner.outputs, args.dump_outputs)
        del runner.outputs
    if not args.full:
        return finish(out)
    ref_out = None
    traffic = None
    if rank == 0 and world == 1:
        if not args.no_gather:
            out["gather"] = gather_microbench(dev)
            if args.workload == "cfg2":
                try:
                    out["features"] = features_bench(dev)
                except Exception as e:                       # noqa: BLE001 — reporting only
                    out["features"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        if args.workload == "cfg2" and not args.no_pmc:
            # HBM bytes per launch of the dominant kernel (and of the gather), measured in this run by two rocprofv3 PMC passes
            traffic, tsrc = live_pmc_traffic()
            out["roofline"]["traffic_source"] = tsrc
            if traffic:
                out["roofline"]["traffic"] = traffic.get(precision if precision in traffic else "fp32", {}).get(out["roofline"]["launch_kind"])
                out["roofline"]["traffic_algorithmic"] = TRAFFIC_ALGO.get(out["roofline"]["launch_kind"])
                if "gather" in out:
                    out["gather"]["traffic"] = traffic.get("gather")
                if "features" in out and "cfg4_batch" in out["features"]:
                    f = out["features"]
                    f["traffic"] = traffic.get("features")
                    # compulsory bytes of the launch: the h_E rows it writes, E_idx, the 18-atom frames of the residues (gathered frames hit in cache)
                    f["traffic_algorithmic"] = f["cfg4_batch"]["tokens"] * (48 * 128 * 4 + 48 * 4 + 54 * 4 + 4 * 4)

        if not args.no_cpu_baseline:
            ref_out, cb = cpu_baseline(runner)
            out["cpu_baseline"] = cb
            g = runner.g_np
            out["parity"] = parity_vs_cpu(runner.logp[:1], ref_out, torch.from_numpy(g["S"][:1]).long(), torch.from_numpy(g["mask"][:1]))
    if args.workload == "cfg2" and args.precision is None:
        # the split-bf16 evaluation (the model's default) on the same inputs, same K / W, every rank
        del runner
        x3, rx = encdec_bench(args, dev, rank, world, dist, "cfg2", "x3", args.steps, args.warmup)
        xo = {k: x3[k] for k in ("value", "unit", "ms_per_step", "dtype", "roofline", "per_kernel", "whole_path")}
        if traffic:
            xo["roofline"]["traffic"] = traffic.get("x3", {}).get(xo["roofline"]["launch_kind"])
        if ref_out is not None:
            g = rx.g_np
            xo["parity"] = parity_vs_cpu(rx.logp[:1], ref_out, torch.from_numpy(g["S"][:1]).long(), torch.from_numpy(g["mask"][:1]))
        out["x3"] = xo
        del rx
        torch.cuda.empty_cache()
        if world == 1 and not args.no_secondary:
            # the opt-in one-launch form of the same pass (encdec_persistent_kernel), for the record: slower than the chain
            Lb = hip.lib()
            prev = Lb.namp_set_persistent(1)
            try:
                pz, rp = encdec_bench(args, dev, rank, world, dist, "cfg2", "x3", args.steps, args.warmup)
                out["x3_persistent_launch"] = {"value": pz["value"], "ms_per_step": pz["ms_per_step"], "per_kernel": pz["per_kernel"],
                                               "note": "namp_set_persistent(1): the whole pass as node_linear + ONE persistent launch "
                                                       "(six stages, five grid barriers); bit-identical outputs; off by default"}
                del rp
            finally:
                Lb.namp_set_persistent(prev)
        if rank == 0 and world == 1 and not args.no_secondary:
            out["secondary"] = secondary_runs(args, dev)
    if world > 1 and args.workload == "cfg2" and not args.no_secondary:
        # N > 1: the same invocation also yields the STRONG-scaling point of BASELINE configs[3] — one >= 1 s region of passes over the
        # 1,373-complex split, LPT-sharded over the ranks (evaluation/rna_design_scripts/design_sequences.sh:41-50 runs independent
        # structures as independent tasks) — so that one SCALE run carries both curves.
        import copy
        a4 = copy.copy(args)
        a4.steps, a4.warmup, a4.workload = 2, 1, "cfg4"
        try:
            o4 = split_bench(a4, dev, rank, world, dist)
            out["cfg4_strong"] = {"value": o4["value"], "unit": o4["unit"], "ms_per_pass": o4["ms_per_step"], "passes": o4["steps"], "scaling": "strong",
                                  "n_gpus": o4["n_gpus"], "per_rank_seconds": o4["shard"]["per_rank_seconds"],
                                  "per_rank_residues": o4["shard"]["per_rank_residues"], "lpt_imbalance": o4["shard"]["lpt_imbalance"],
                                  "backend": o4["collation"]["backend"]}
        except Exception as e:                               # noqa: BLE001 — must not take the weak-scaling value down
            out["cfg4_strong"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    finish(out)


if __name__ == "__main__":
    main()
