"""Host-side guard of tests/weight_variants.py: on the fp64 CPU oracle every variant must reach the numeric regime its row claims (GELU
pre-activations, |mean| / std of the rows entering a LayerNorm, |log p|) on the very inputs tests/test_gpu_range.py uses, and the oracle's
own fp32 evaluation must stay finite and within the project's parity bars of the fp64 one there — the bars the HIP parity modes are held
to are reachable by a plain fp32 implementation with a margin.  F.gelu / F.layer_norm are hooked as oracle.cpu_ref sees them."""
import functools

import pytest
import torch
import torch.nn.functional as F

import weight_variants as wv
from na_mpnn_amd import spec
from oracle import cpu_ref

TOL_LOGP = 1e-3
TOL_ACT = 2e-4
GRAPH_VARIANTS = ("base", "gain2", "gain4", "shift", "affine", "head")


class _ProbedF:
    """torch.nn.functional with gelu / layer_norm recording the range of what they are given."""

    def __init__(self):
        self.max_preact = 0.0
        self.max_mean_over_std = 0.0

    def __getattr__(self, name):
        return getattr(F, name)

    def gelu(self, x, *a, **kw):
        self.max_preact = max(self.max_preact, float(x.detach().abs().max()))
        return F.gelu(x, *a, **kw)

    def layer_norm(self, x, *a, **kw):
        xd = x.detach().double()
        std = xd.std(-1, unbiased=False)
        live = std > 0                                  # rows of masked residues are exactly zero
        if live.any():
            self.max_mean_over_std = max(self.max_mean_over_std, float((xd.mean(-1).abs()[live] / std[live]).max()))
        return F.layer_norm(x, *a, **kw)


def _probed(monkeypatch):
    probe = _ProbedF()
    monkeypatch.setattr(cpu_ref, "F", probe)
    return probe


def _check_reach(name, probe, max_abs_logp):
    print(f"{name}: max |GELU pre-activation| = {probe.max_preact:.1f}, max |row mean| / std entering a LayerNorm = "
          f"{probe.max_mean_over_std:.2f}, max |log p| = {max_abs_logp:.1f}")
    if name == "base":
        assert probe.max_preact < 8
    if name == "gain2":
        assert probe.max_preact > 12
    if name == "gain4":
        assert probe.max_preact > 40
    if name == "shift":
        assert probe.max_mean_over_std > 100
    if name == "head":
        assert max_abs_logp > 30


def _check_parity(lp32, lp64, valid):
    assert torch.isfinite(lp32).all()
    err = float((lp32.double() - lp64)[valid].abs().max())
    print(f"    fp32 oracle vs fp64 oracle: max |dlogp| = {err:.2e}")
    assert err < TOL_LOGP / 10                           # a plain fp32 evaluation keeps a 10 x margin under the parity bar
    assert torch.equal(lp32.argmax(-1)[valid], lp64.argmax(-1)[valid])


@pytest.mark.parametrize("name", GRAPH_VARIANTS)
def test_graph_path_reach_and_fp32_parity(weights_np, name, monkeypatch):
    t = wv.graph_case("small")
    valid = t["mask"].bool()
    probe = _probed(monkeypatch)
    r64 = wv.graph_oracle(wv.torch_weights(weights_np, name, torch.float64), t)
    assert r64["log_probs"].dtype == torch.float64 and r64["h_E"].dtype == torch.float64
    _check_reach(name, probe, float(r64["log_probs"][valid].abs().max()))
    r32 = wv.graph_oracle(wv.torch_weights(weights_np, name), t)
    assert r32["log_probs"].dtype == torch.float32
    _check_parity(r32["log_probs"], r64["log_probs"], valid)
    assert torch.isfinite(r32["h_V"]).all() and torch.isfinite(r32["h_E"]).all()
    assert float((r32["h_V"].double() - r64["h_V"]).abs().max()) < TOL_ACT
    assert float((r32["h_E"].double() - r64["h_E"]).abs().max()) < TOL_ACT
    assert torch.equal(r32["decoding_order"], r64["decoding_order"])


@pytest.mark.parametrize("name", wv.NAMES)
def test_from_coordinates_reach_and_fp32_parity(weights_np, name, monkeypatch):
    fd = wv.coords_case()
    valid = fd["mask"].bool()
    probe = _probed(monkeypatch)
    with torch.no_grad():
        r64 = cpu_ref.score(wv.torch_weights(weights_np, name, torch.float64), cpu_ref.to_dtype(fd, torch.float64), wv.COORDS_K)
        assert r64["log_probs"].dtype == torch.float64
        if name != "feat":
            _check_reach(name, probe, float(r64["log_probs"][valid].abs().max()))
        r32 = cpu_ref.score(wv.torch_weights(weights_np, name), fd, wv.COORDS_K)
        u64 = cpu_ref.unconditional_probs(wv.torch_weights(weights_np, name, torch.float64), cpu_ref.to_dtype(fd, torch.float64), wv.COORDS_K)
        u32 = cpu_ref.unconditional_probs(wv.torch_weights(weights_np, name), fd, wv.COORDS_K)
    assert r32["log_probs"].dtype == torch.float32
    _check_parity(r32["log_probs"], r64["log_probs"], valid)
    _check_parity(u32["log_probs"], u64["log_probs"], valid)
    assert torch.equal(r32["decoding_order"], r64["decoding_order"])


def test_feat_variant_puts_large_mean_rows_into_norm_edges(weights_np, monkeypatch):
    """The featuriser's LayerNorm: the rows entering features.norm_edges carry the + 4.0 of the variant (recorded in
    weight_variants.FEAT_SHIFT_VIA), which the base weights' rows do not."""
    fd = cpu_ref.to_dtype(wv.coords_case(), torch.float64)
    seen = {}
    for name in ("base", "feat"):
        w = wv.torch_weights(weights_np, name, torch.float64)
        rows = []
        real_ln = cpu_ref._ln
        monkeypatch.setattr(cpu_ref, "_ln", lambda w_, n_, x: (rows.append(x) if n_ == "features.norm_edges" else None, real_ln(w_, n_, x))[1])
        with torch.no_grad():
            _, E, E_idx = cpu_ref.features(w, fd, wv.COORDS_K)
        monkeypatch.setattr(cpu_ref, "_ln", real_ln)
        assert E.dtype == torch.float64 and len(rows) == 1
        seen[name] = (rows[0].mean(-1), rows[0].std(-1, unbiased=False), E_idx)
    assert torch.equal(seen["base"][2], seen["feat"][2])
    d_mean = seen["feat"][0] - seen["base"][0]
    ratio = {n: float((m.abs() / s).max()) for n, (m, s, _) in seen.items()}
    print(f"norm_edges input rows: mean shift {float(d_mean.min()):.2f} .. {float(d_mean.max()):.2f}; max |mean| / std base {ratio['base']:.2f}, "
          f"feat {ratio['feat']:.2f}")
    assert float((d_mean - wv.FEAT_SHIFT).abs().max()) < 1.0
    assert ratio["feat"] > 2 * ratio["base"]


@functools.lru_cache(maxsize=None)
def _restypes():
    return spec.restype_to_int()


@pytest.mark.parametrize("name", GRAPH_VARIANTS)
def test_training_fp32_parity(weights_np, name):
    """cpu_ref.train_loss_and_grads in fp32 against fp64 with the bars of test_training_gradients_odd_shapes."""
    fd, randn = wv.train_case()
    l64, _, g64 = cpu_ref.train_loss_and_grads(wv.torch_weights(weights_np, name, torch.float64), cpu_ref.to_dtype(fd, torch.float64),
                                               wv.TRAIN_K, randn, _restypes())
    l32, _, g32 = cpu_ref.train_loss_and_grads(wv.torch_weights(weights_np, name), fd, wv.TRAIN_K, randn, _restypes())
    assert all(g.dtype == torch.float64 for g in g64.values())
    assert abs(float(l32) - float(l64)) <= 1e-5 * max(1e-3, abs(float(l64)))
    worst = 0.0
    for key, ref in g64.items():
        assert torch.isfinite(g32[key]).all(), key
        scale = float(ref.abs().max())
        if scale < 1e-12:
            assert float(g32[key].abs().max()) < 1e-9, key
        else:
            worst = max(worst, float((g32[key].double() - ref).abs().max()) / scale)
    print(f"{name}: fp32 oracle loss {abs(float(l32) - float(l64)) / abs(float(l64)):.1e} relative, worst gradient {worst:.1e} of its tensor's max")
    assert worst < 2e-4


def test_variants_touch_what_they_name(weights_np):
    base = wv.variant(weights_np, "base")
    assert all((base[k] == weights_np[k]).all() and base[k] is not weights_np[k] for k in weights_np)
    changed = lambda name: {k for k, v in wv.variant(weights_np, name).items() if not (v == weights_np[k]).all()}
    layer = {k for k in weights_np if k.startswith(("encoder_layers.", "decoder_layers."))}
    assert changed("gain2") == changed("gain4") == {k for k in layer if "norm" not in k}
    assert changed("shift") == {k for k in layer if k.endswith((".W3.bias", ".W13.bias", ".dense.W_out.bias"))} and len(changed("shift")) == 15
    assert changed("affine") == {k for k in weights_np if "norm" in k}
    assert changed("head") == {"W_out.weight", "W_out.bias", "W_s.weight"}
    assert changed("feat") == {"features.edge_embedding.weight", wv.FEAT_SHIFT_VIA}
    with pytest.raises(KeyError):
        wv.variant(weights_np, "nope")


def test_samplers_run_in_fp64(weights_np):
    """cpu_ref.sample / sample_symmetric follow the weights' dtype: teacher-forced with the fp32 draw, the fp64 evaluation returns fp64
    log_probs / sampling_probs within fp32 round-off of the fp32 ones, and the same decoding order."""
    from na_mpnn_amd import synth
    n, k, bs = 24, 8, 2
    cx = synth.make_complex(seed=3, n=n, n_chains=2)
    fd = {key: torch.from_numpy(v)[None] for key, v in cx.items()}
    fd.update({"batch_size": bs, "temperature": 0.5, "bias": torch.zeros(1, n, 33),
               "randn": torch.randn(bs, n, generator=torch.Generator().manual_seed(1))})
    w32, w64 = wv.torch_weights(weights_np, "base"), wv.torch_weights(weights_np, "base", torch.float64)
    with torch.no_grad():
        torch.manual_seed(2)
        r32 = cpu_ref.sample(w32, fd, k)
        r64 = cpu_ref.sample(w64, cpu_ref.to_dtype(fd, torch.float64), k, S_forced=r32["S"])
        fds = dict(fd, symmetry_residues=[[1, 9], [4, 13, 20]], symmetry_weights=[[1.0, 1.0], [0.5, 0.25, 0.25]],
                   randn=fd["randn"][:1])
        torch.manual_seed(2)
        s32 = cpu_ref.sample_symmetric(w32, fds, k)
        s64 = cpu_ref.sample_symmetric(w64, cpu_ref.to_dtype(fds, torch.float64), k, S_forced=s32["S"])
    for a, b in ((r32, r64), (s32, s64)):
        assert a["log_probs"].dtype == torch.float32 and b["log_probs"].dtype == torch.float64 and b["sampling_probs"].dtype == torch.float64
        assert torch.equal(a["decoding_order"], b["decoding_order"]) and torch.equal(a["S"], b["S"])
        assert float((a["log_probs"].double() - b["log_probs"]).abs().max()) < 1e-4
        assert float((a["sampling_probs"].double() - b["sampling_probs"]).abs().max()) < 1e-4
