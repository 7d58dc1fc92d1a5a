"""GPU tests of the mixed-precision training kernels (train.X3 == 2) on exactly solvable weights (tests/solvable_train.py): every 128 x 128
matrix a signed permutation, so that every forward and data-gradient product has one exact term.  The autograd Functions of train.py must
then equal the fp64 evaluation of a hand-written forward and backward that rounds where the kernels round — edge_bwd_dw16_kernel,
edge_update_bwd_a16_kernel / _b16_kernel, the bf16 row gather, the bf16 W^T images — except at bf16 ties and in the last bits of the fp32
sums: a missing edge row, a dropped ragged round, a W where W^T belongs or one misplaced rounding moves some observable by three bars and
more (tests/test_solvable_train_host.py).

Bars, computed at run time from the restatement's own fp32-against-fp64 figures: row tensors (out, dL/dh_E, the G1-borne dL/dPj) as in
tests/test_gpu_solvable.py (solvable.bars); sums over edge rows (dW*, db*, dL/dPa, d ln weight, d ln bias) 4 x the reference's largest
difference relative to the tensor's largest entry, or one bf16 step of the sum's largest term where that is more (solvable_train.TIE_STEP).
Every test prints the kernel's figures beside the reference's."""
import functools

import pytest
import torch

import solvable_train as st
from na_mpnn_amd import hip, spec, train
from na_mpnn_amd.model import ProteinMPNN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
H = st.H


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def shape_of(name):
    """SHAPES[name]; the middle shape re-derived for the device's compute-unit count if (1, 560, 30) does not give a workgroup two rounds there."""
    return st.ragged_shape(cus()) if name == "ragged" else st.SHAPES[name]


def stage_cases(stages=st.STAGES):
    return [(s, shape, p) for shape in st.SHAPES for s in stages for p in ((0.0, 0.1) if s == "edge_update" else (0.0,))]


@functools.lru_cache(maxsize=2)
def case_and_reference(stage, shape, p, table):
    """The case, its fp64 restatement under `table`, the fp32 evaluation's figures against it and the bars: computed once per case."""
    c = st.make_case(stage, shape_of(shape), p)
    if table == "exact":
        return c, st.restate(c, F64, "exact"), None, None
    return (c,) + st.reference(c, table)


def run_stage(c, monkeypatch, prec, on_chip):
    """One stage through its autograd Function at precision code `prec` -> {observable: CPU tensor}."""
    monkeypatch.setattr(train, "X3", prec)
    monkeypatch.setattr(train, "DW_ONCHIP", on_chip)
    monkeypatch.setattr(train, "DW_ONCHIP_EDGE", on_chip)
    stage, B, N, K = c["stage"], c["B"], c["N"], c["K"]
    dev = lambda k: c[k].to(DEV)
    with torch.enable_grad():
        if stage == "edge_linear":
            x, W, b = (dev(k).requires_grad_(True) for k in ("x", "W", "b"))
            y = train._EdgeLinear.apply(x, W, b)
            (y * dev("R")).sum().backward()
            got = {"out": y.detach(), "d_x": x.grad, "dW": W.grad, "db": b.grad}
        elif stage == "embed_tail":
            y0, lw, lb, W, b = (dev(k).requires_grad_(True) for k in ("y", "ln_w", "ln_b", "W", "b"))
            out = train._EdgeEmbedTail.apply(y0, lw, lb, W, b)
            (out * dev("R")).sum().backward()
            got = {"out": out.detach(), "d_y": y0.grad, "d_lnw": lw.grad, "d_lnb": lb.grad, "dW": W.grad, "db": b.grad}
        else:
            names = ["h_E", "Pa", "Pj0", "Pj1", "W1", "W2", "b2", "W3", "b3", "ln_w", "ln_b"]
            hE, pa, pj0, pj1, w1, w2, b2, w3, b3, lw, lb = leaves = [dev(k).requires_grad_(True) for k in names]
            E32 = dev("E_idx").to(torch.int32).contiguous()
            if stage == "edge_update":
                y = train._EdgeUpdate.apply(hE, pa, pj0, w1, w2, b2, w3, b3, lw, lb, E32, c["p"], c["seed"])
                (y * dev("R")).sum().backward()
            else:
                mode = 0 if stage == "enc_msg" else 1
                y, h_pass = train._EdgeMLP.apply(mode, hE, pa, pj0, pj1 if mode == 1 else None, w1, w2, b2, w3, b3, E32,
                                                 dev("mask").contiguous() if mode == 0 else None, None, dev("rank").contiguous() if mode == 1 else None)
                ((y * dev("R")).sum() + (h_pass * dev("R2")).sum()).backward()
            gr = dict(zip(names, [l.grad for l in leaves]))
            got = {"out": y.detach(), "d_hE": gr["h_E"], "d_Pa": gr["Pa"], "d_Pj0": gr["Pj0"], "dW1": gr["W1"], "dW2": gr["W2"], "db2": gr["b2"],
                   "dW3": gr["W3"], "db3": gr["b3"]}
            if stage == "dec_msg":
                got["d_Pj1"] = gr["Pj1"]
            if stage == "edge_update":
                got["d_lnw"], got["d_lnb"] = gr["ln_w"], gr["ln_b"]
    torch.cuda.synchronize()
    assert set(got) == set(st.observables(c))
    for k, v in got.items():
        assert v is not None and bool(torch.isfinite(v).all()), k
    return {k: v.detach().cpu() for k, v in got.items()}


def check(tag, got, ref64, ref_figs, bar):
    figs = st.measure(got, ref64)
    over = []
    for k in ref64:
        print(st.line(tag, k, figs[k], ref_figs[k], bar[k]))
        if any(f > b for f, b in zip(figs[k], bar[k])):
            over.append((k, figs[k], bar[k]))
    return over


def test_shapes_walk_the_persistent_bookkeeping():
    """On this device: 10 rounds leave most workgroups without a round; the middle shape gives some workgroups two rounds and ends on a ragged
    one; the largest gives every workgroup several."""
    L = hip.lib()
    n = cus()
    B, N, K = shape_of("idle")
    assert L.namp_train_edge_bwd_dw_groups(B, N, K) == 10 < n
    B, N, K = shape_of("ragged")
    rounds, most, last = st.rounds_per_workgroup((B, N, K), n)
    assert L.namp_train_edge_bwd_dw_groups(B, N, K) == n < rounds < 2 * n and most == 2 and 0 < last < st.ROUND_ROWS and K % 16 != 0
    assert L.namp_train_edge_bwd_dw_rows(B, N, K) == rounds * st.ROUND_ROWS > B * N * K
    B, N, K = shape_of("multi")
    assert st.rounds_per_workgroup((B, N, K), n)[1] >= 3 and K % 16 == 0 and B > 1


@pytest.mark.parametrize("stage,shape,p", stage_cases())
def test_mixed_precision_stage_equals_the_restatement(stage, shape, p, monkeypatch):
    """train.X3 = 2 with the weight-gradient-owning launches (DW_ONCHIP, DW_ONCHIP_EDGE): the output and every gradient of the stage against
    restate(..., float64) under the "mixed" table.  Encoder messages: a masked residue, and an unmasked one whose whole neighbourhood is
    masked, give exactly zero dL/dPa rows and hand the pass-through gradient on unchanged."""
    c, ref64, ref_figs, bar = case_and_reference(stage, shape, p, "mixed")
    got = run_stage(c, monkeypatch, 2, True)
    over = check(f"mixed {stage} {shape} p={p}", got, ref64, ref_figs, bar)
    assert not over, over
    if stage == "enc_msg":
        G, K = c["G"], c["K"]
        dead = c["mask"].view(-1) == 0
        dead[torch.arange(c["B"]) * c["N"] + c["lonely"]] = True
        assert float(got["d_Pa"].view(G, H)[dead].abs().max()) == 0.0
        assert torch.equal(got["d_hE"].view(G, K, H)[dead], c["R2"].view(G, K, H)[dead])


@pytest.mark.parametrize("shape", st.FEAT_SHAPES)
def test_feature_weight_gradient_from_bf16_tiles_equals_the_restatement(shape, weights_np, monkeypatch):
    """train.edge_embedding -> _EdgeEmbedTail in mixed mode on a synthetic complex: the tail's backward hands dL/dy to namp_train_feat_wgrad as
    bf16 operand tiles.  The 5200 -> 128 weight gradient, the positional table's gradients and the tail's own outputs against the restatement
    on the DEVICE's y, neighbour lists and atom frames (the forward embedding is dense: its 5200-term sums are an input here, not an
    observable).  640 edges (one chunk, ten tiles), 16,800 edges (five chunks, a partial last tile) and two complexes of 33,600 edges each.
    That the tiles were handed over is asserted on the call itself: the fp32 rows are what the launch falls back to without a sign."""
    B, N, K = st.SHAPES[shape]
    fd = {k_: v.to(DEV) for k_, v in st.feat_complexes(shape).items()}
    L = hip.lib()
    launch, g16_seen = L.namp_train_feat_wgrad, []

    def spy(*args):
        g16_seen.append(args[5])
        return launch(*args)
    monkeypatch.setattr(L, "namp_train_feat_wgrad", spy)
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=K, dropout=0.0, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    m = m.to(DEV)
    m.message_precision = "bf16"
    monkeypatch.setattr(train, "X3", 2)
    fp = m.features
    with torch.enable_grad():
        y, E_idx = train.edge_embedding(m, fd)
        y.retain_grad()
        X18, M18 = train._atom_frames(m, fd["X"].float(), fd)
        t = dict(y=y.detach().cpu(), E_idx=E_idx.cpu().long(), X18=X18.cpu(), M18=M18.cpu(), R_idx=fd["R_idx"].cpu(), chain=fd["chain_labels"].cpu(),
                 pos_w=fp.embeddings.linear.weight.detach().cpu(), pos_b=fp.embeddings.linear.bias.detach().cpu(),
                 Wedge=m.edge_weight18().detach().cpu())
        c = st.feat_case(t)
        lw, lb, W, b = (c[k_].to(DEV).requires_grad_(True) for k_ in ("ln_w", "ln_b", "W", "b"))
        h = train._EdgeEmbedTail.apply(y, lw, lb, W, b)
        (h * c["R"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert len(g16_seen) == 1 and g16_seen[0], g16_seen                  # one launch, on the tail's bf16 tiles
    got = {"out": h.detach(), "d_y": y.grad, "d_lnw": lw.grad, "d_lnb": lb.grad, "dW": W.grad, "db": b.grad, "dWf": fp.edge_embedding.weight.grad,
           "d_posw": fp.embeddings.linear.weight.grad, "d_posb": fp.embeddings.linear.bias.grad}
    assert set(got) == set(st.observables(c)) and all(v is not None and bool(torch.isfinite(v).all()) for v in got.values())
    ref64, ref_figs, bar = st.reference(c, "mixed")
    over = check(f"mixed {st.FEAT_STAGE} {shape} p=0.0", {k_: v.detach().cpu() for k_, v in got.items()}, ref64, ref_figs, bar)
    assert not over, over


@pytest.mark.parametrize("stage,shape,p", stage_cases(("enc_msg", "dec_msg", "edge_update")))
def test_mixed_precision_row_tensor_forms_equal_their_restatement(stage, shape, p, monkeypatch):
    """The same stages through the row-tensor launches (DW_ONCHIP = False, DW_ONCHIP_EDGE = False: edge_chain_bwd_kernel with bf16 row tensors,
    wgrad_bf16_kernel) under the same bar rules, against the "mixed_rows" table: the Abramowitz-Stegun erf GELU in the backward's
    recomputation, gelu' kept in fp32 where that launch keeps it."""
    c, ref64, ref_figs, bar = case_and_reference(stage, shape, p, "mixed_rows")
    got = run_stage(c, monkeypatch, 2, False)
    over = check(f"mixed_rows {stage} {shape} p={p}", got, ref64, ref_figs, bar)
    assert not over, over


# (_EdgeEmbedTail has no exact-fp32 backward: namp_train_embed_ln_bwd takes precision codes 1 and 2)
@pytest.mark.parametrize("stage,shape,p,prec", [cs + (prec,) for cs in stage_cases() for prec in (0, 1) if (cs[0], prec) != ("embed_tail", 0)])
def test_controls_exact_and_split_bf16(stage, shape, p, prec, monkeypatch):
    """Controls on the same inputs: exact fp32 and split-bf16 products against the unrounded restatement at the project's bars for these
    modes — 2e-5 of the largest entry on the output, 5e-5 on every gradient."""
    c, ref64, _, _ = case_and_reference(stage, shape, p, "exact")
    got = run_stage(c, monkeypatch, prec, True)
    worst = {k: st.rel_max(got[k].reshape(ref64[k].shape), ref64[k]) for k in ref64}
    print(f"SOLVABLE control prec {prec} {stage} {shape} p={p}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < (2e-5 if k == "out" else 5e-5), (k, v, worst)
