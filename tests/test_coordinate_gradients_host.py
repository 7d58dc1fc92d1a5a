"""Coordinate gradients without a device: the premises of the reference tests/xgrad_ref.py, the layout of the
carrier's workspace sections and the attach-and-carry state machine of namp_train_feat_xgrad.

Bars, measured here in fp64 (each printed before it is asserted):
  * xgrad_ref's autograd against the autograd of oracle/cpu_ref.py::features, a random cotangent on the LayerNormed rows: two fp64
    evaluations of one formula, 4.7e-16 (rows) and 4.3e-16 (dX) measured -> bar 5e-14 (two orders above);
  * the closed form against autograd: 1.1e-15 measured -> bar 1e-13;
  * central differences, step 1e-5 A on a dozen coordinates: truncation h^2 f''' / 6 ~ 1e-10 relative, rounding eps |L| / h ~ 1e-9 of the
    largest gradient entry; 1.3e-10 measured -> bar 1e-7: a wrong sign (2), a missing factor 2 (0.5) or a dropped 1e-6 under the root (the
    self-pair terms, see the test) are all far above it.
"""
import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, synth
from oracle import cpu_ref
import xgrad_ref
from xgrad_ref import rel

EINVAL = -1


def _case(n=23, k=9, seed=5):
    cx = synth.make_complex(seed=seed, n=n, n_chains=2, missing_atom_frac=0.05, masked_frac=0.04)
    fd = {k_: torch.from_numpy(np.ascontiguousarray(v))[None] for k_, v in cx.items()}
    w = {k_: torch.from_numpy(v) for k_, v in synth.make_weights(0).items()}
    fd64, w64 = cpu_ref.to_dtype(fd, torch.float64), cpu_ref.to_dtype(w, torch.float64)
    return fd64, w64, k


@pytest.fixture(scope="module")
def case():
    return _case()


def test_reference_autograd_equals_the_oracle_features_autograd(case):
    fd, w, k = case
    X = fd["X"].clone().requires_grad_(True)
    with torch.enable_grad():
        _, E, E_idx = cpu_ref.features(w, dict(fd, X=X), k)
        cot = torch.randn(E.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
        (E * cot).sum().backward()
    W = w["features.edge_embedding.weight"]
    X2 = fd["X"].clone().requires_grad_(True)
    with torch.enable_grad():
        X18, M18 = xgrad_ref.atom_frames(X2, fd)
        y = xgrad_ref.rbf_rows(W, X18, M18, E_idx) + xgrad_ref.pos_rows(W, w["features.embeddings.linear.weight"],
                                                                        w["features.embeddings.linear.bias"], fd, E_idx)
        E2 = cpu_ref._ln(w, "features.norm_edges", y + w["features.edge_embedding.bias"]) if "features.edge_embedding.bias" in w else \
            cpu_ref._ln(w, "features.norm_edges", y)
        (E2 * cot).sum().backward()
    ev, eg = rel(E2, E), rel(X2.grad, X.grad)
    print(f"rows {ev:.2e}  dX {eg:.2e}")
    assert float(X.grad.abs().max()) > 0
    assert ev < 5e-14 and eg < 5e-14


def _kernel_level(case):
    fd, w, k = case
    W = w["features.edge_embedding.weight"]
    _, _, E_idx = cpu_ref.features(w, fd, k)
    X18, M18 = xgrad_ref.atom_frames(fd["X"], fd)
    g = torch.randn(*E_idx.shape, 128, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    return W, X18, M18, E_idx, g


def test_closed_form_equals_autograd(case):
    W, X18, M18, E_idx, g = _kernel_level(case)
    auto = xgrad_ref.dX18_autograd(W, X18, M18, E_idx, g)
    closed = xgrad_ref.dX18_closed_form(W, X18, M18, E_idx, g)
    e = rel(closed, auto)
    print(f"closed form vs autograd {e:.2e}")
    assert e < 1e-13
    assert bool((auto[M18 == 0] == 0).all())                     # a masked atom's coordinates give exactly zero
    assert abs(float(auto.sum())) < 1e-9 * float(auto.abs().sum())   # translation invariance


def test_central_differences_agree(case):
    W, X18, M18, E_idx, g = _kernel_level(case)
    auto = xgrad_ref.dX18_autograd(W, X18, M18, E_idx, g)
    f = lambda x: float((xgrad_ref.rbf_rows(W, x, M18, E_idx) * g).sum())
    live = torch.nonzero(M18[0] != 0)
    pick = live[torch.randperm(live.shape[0], generator=torch.Generator().manual_seed(4))[:12]]
    h, worst = 1e-5, 0.0
    for q, (i, a) in enumerate(pick.tolist()):
        c = q % 3
        xp, xm = X18.clone(), X18.clone()
        xp[0, i, a, c] += h
        xm[0, i, a, c] -= h
        fdiff = (f(xp) - f(xm)) / (2 * h)
        worst = max(worst, abs(fdiff - float(auto[0, i, a, c])) / float(auto.abs().max()))
    print(f"central differences vs autograd {worst:.2e}")
    assert worst < 1e-7
    # what the bar has to catch: the sign, the factor 2, and the 1e-6 under the root (an atom pair at distance 0 — a residue that is its own
    # neighbour, a == b — has a finite, zero gradient only because of it: without it the closed form divides 0 by 0)
    assert rel(-auto, auto) > 1e-3 and rel(0.5 * auto, auto) > 1e-3
    assert bool((E_idx[0] == torch.arange(E_idx.shape[1])[:, None]).any()) and bool(torch.isfinite(auto).all())


# ---- sizes and offsets --------------------------------------------------------------------------------------------------
DIMS = [(1, 1, 1), (1, 17, 17), (2, 20, 5), (1, 1000, 48), (3, 333, 30)]


@pytest.mark.parametrize("B,L,K", DIMS)
def test_sections_are_aligned_disjoint_and_ordered(B, L, K):
    Lb = hip.lib()
    E, G = B * L * K, B * L
    total, o_in, o_out = (getattr(Lb, "namp_train_feat_xgrad_" + n)(E, B, L, K) for n in ("ws_ints", "in_offset", "out_offset"))
    pres = Lb.namp_train_feat_wgrad_ws_ints(E)
    for o in (total, o_in, o_out):
        assert o > 0 and (4 * o) % 256 == 0
    assert pres <= o_in                                            # the plain call's presence words come first, [0, pres)
    assert o_in == (4 * pres + 255) // 256 * 64                    # ... and the input section is the next 256-byte granule
    assert o_in + 128 * 5200 <= o_out                              # input section [o_in, o_in + 128 * 5200), then scratch
    scratch = o_out - (o_in + 128 * 5200)
    assert scratch >= 108 * E + 3 * E + 3 * G + 1                  # rows, clamped lists, reverse adjacency and its scratch
    assert o_out + 54 * G <= total < o_out + 54 * G + 64           # output section last


def test_invalid_dims_give_zero():
    Lb = hip.lib()
    for name in ("ws_ints", "in_offset", "out_offset"):
        fn = getattr(Lb, "namp_train_feat_xgrad_" + name)
        assert fn(20, 1, 5, 4) > 0
        for bad in ((21, 1, 5, 4), (0, 0, 5, 4), (0, 1, 0, 4), (0, 1, 5, 0), (30, 1, 5, 6), (-20, -1, 5, 4), (2 ** 31, 1, 2 ** 16, 2 ** 15)):
            assert fn(*bad) == 0, (name, bad)


# ---- the state machine, without a device: every carrier call below fails before any launch -----------------------------
def _carrier(B=1, L=4, K=2):
    Lb = hip.lib()
    rc = Lb.namp_train_feat_wgrad(None, None, None, None, None, None, None, None, 0, B, L, K, None)
    return rc, Lb.namp_last_error()


def test_state_machine_without_a_device():
    Lb = hip.lib()
    need = Lb.namp_train_feat_xgrad_ws_ints(8, 1, 4, 2)
    plain = b"null tile workspace"
    rc, msg = _carrier()
    assert rc == EINVAL and plain in msg                          # nothing attached: the plain call's own first check
    # too few ws_ints: rejected by the carrier, which has taken the record
    assert Lb.namp_train_feat_xgrad(need - 1) == 0
    rc, msg = _carrier()
    assert rc == EINVAL and b"too small" in msg
    rc, msg = _carrier()
    assert rc == EINVAL and plain in msg
    # enough: the call goes on to its pointer checks
    assert Lb.namp_train_feat_xgrad(need) == 0
    rc, msg = _carrier()
    assert rc == EINVAL and plain in msg
    # the record is cleared by a failing carrier call (bad dims here), not kept for the next one
    assert Lb.namp_train_feat_xgrad(1) == 0
    rc, msg = _carrier(K=5)
    assert rc == EINVAL and b"bad dims" in msg
    rc, msg = _carrier()
    assert rc == EINVAL and plain in msg
    # a second attach replaces the first, either way round
    assert Lb.namp_train_feat_xgrad(1) == 0 and Lb.namp_train_feat_xgrad(need) == 0
    assert plain in _carrier()[1]
    assert Lb.namp_train_feat_xgrad(need) == 0 and Lb.namp_train_feat_xgrad(1) == 0
    assert b"too small" in _carrier()[1]
    # a failing attach leaves nothing attached
    assert Lb.namp_train_feat_xgrad(1) == 0
    assert Lb.namp_train_feat_xgrad(0) == EINVAL and b"ws_ints" in Lb.namp_last_error()
    assert plain in _carrier()[1]


def test_the_record_belongs_to_the_calling_thread():
    import threading
    Lb = hip.lib()
    assert Lb.namp_train_feat_xgrad(1) == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(_carrier()[1]))
    t.start()
    t.join()
    assert b"null tile workspace" in seen[0]                      # another thread's call carries nothing
    assert b"too small" in _carrier()[1]                          # ... and this thread's record is still there
