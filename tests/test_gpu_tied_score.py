"""GPU tests of ProteinMPNN.score_tied: the item route (namp_tied_score on namp_decoder_fwd), the stream route and the
sampler route against the CPU oracle's tied stream and against each other, the sensitivity to hidden-backward edges, the call without
ties against score_sequences, and the invariants of the item route (chunks, order, neighbours in the call)."""
import pytest
import torch

from na_mpnn_amd import spec
from na_mpnn_amd.model import ProteinMPNN
import tied_score_ref as tr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
PARITY = 1e-3        # the project's parity bound against the CPU oracle
BETWEEN = 2e-4       # what the project allows between two GPU implementations
_models = {}


def model(weights_np, k, prec):
    if (k, prec) not in _models:
        m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                        polytype_to_int=spec.polytype_to_int())
        m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
        m = m.to(DEV).eval()
        m.message_precision = prec
        _models[(k, prec)] = m
    return _models[(k, prec)]


def to_dev(fd):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def listed_ties(fd):
    sym = fd.get("symmetry_residues")
    return bool(fd.get("paired_residues")) or not (sym is None or len(sym) == 0 or (len(sym) == 1 and len(sym[0]) == 0))


def routes_of(fd):
    return ("items", "sampler") if listed_ties(fd) else ("items", "stream", "sampler")


def max_diff(a, b, on=None):
    """Largest |a - b| over the entries of `on`; the -inf entries must coincide."""
    a, b = a.double().cpu(), b.double().cpu()
    if on is not None:
        a, b = a[..., on], b[..., on]
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    assert torch.equal(fa, fb), "the sequences that break a tie differ"
    return float((a[fa] - b[fa]).abs().max()) if bool(fa.any()) else 0.0


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", tr.GPU_CASES)
def test_every_route_against_the_oracle_and_the_routes_against_each_other(weights_np, name, prec):
    """token_log_probs, member_log_probs and log_likelihood / units of every route within 1e-3 of the oracle's tied stream on every
    entry; items against sampler, and items against stream where the stream route is defined, within 2e-4.
    Measured (MI355X, x3 / fp32, maxima over the cases): items 2.7e-5 / 7.3e-6, stream 9.8e-6 / 2.7e-6, sampler 2.9e-5 / 4.4e-6;
    items against sampler 2.2e-5 / 2.9e-6, items against stream 5.3e-6 / 1.4e-6."""
    c = tr.oracle_case(name)
    fd = to_dev(c["fd"])
    m = model(weights_np, tr.K_OF[name], prec)
    L = c["fd"]["S"].shape[1]
    N = len(c["mask"])
    on, on_L = c["mask"] != 0, c["mask"][:L] != 0
    counted = tr.counted_units(c)
    units = int(counted.sum())
    ref_ll = c["unit"][:, :L][:, counted].sum(-1) / max(units, 1)
    outs = {}
    for route in routes_of(c["fd"]):
        out = outs[route] = m.score_tied(fd, c["S_lib"].to(DEV), method=route)
        assert out["method"] == route and int(out["units"]) == units
        assert torch.equal(out["leader"].cpu(), torch.as_tensor(c["leader"][:L]))
        assert tuple(out["token_log_probs"].shape) == (tr.N_SEQ, L) and tuple(out["member_log_probs"].shape) == (tr.N_SEQ, N // L, L)
        d = (max_diff(out["token_log_probs"], c["unit"][:, :L], on_L), max_diff(out["member_log_probs"].reshape(tr.N_SEQ, N), c["own"], on),
             max_diff(out["log_likelihood"] / max(units, 1), ref_ll))
        print(f"{name} {prec} {route}: units {d[0]:.2e} members {d[1]:.2e} ll/units {d[2]:.2e}")
        assert max(d) < PARITY
        assert torch.equal(out["consistent"].cpu(), torch.isfinite(c["unit"][:, :L][:, counted]).all(-1))
    for other in routes_of(c["fd"])[1:]:
        d = (max_diff(outs["items"]["token_log_probs"], outs[other]["token_log_probs"], on_L),
             max_diff(outs["items"]["member_log_probs"].reshape(tr.N_SEQ, N), outs[other]["member_log_probs"].reshape(tr.N_SEQ, N), on))
        print(f"{name} {prec} items vs {other}: units {d[0]:.2e} members {d[1]:.2e}")
        assert max(d) < BETWEEN


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_hidden_backward_edges_are_read_without_the_token(weights_np, prec):
    """The oracle that reads hidden-backward edges as ordinary backward edges is farther than 1e-3 from the item and sampler routes."""
    name = tr.SENSITIVE
    c, wrong = tr.oracle_case(name), tr.oracle_case(name, hide=False)
    m = model(weights_np, tr.K_OF[name], prec)
    L = c["fd"]["S"].shape[1]
    on_L = c["mask"][:L] != 0
    for route in ("items", "sampler"):
        got = m.score_tied(to_dev(c["fd"]), c["S_lib"].to(DEV), method=route)["token_log_probs"]
        d = max_diff(got, wrong["unit"][:, :L], on_L)
        print(f"{prec} {route}: {d:.2e} from the oracle that does not hide")
        assert d > PARITY


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("name", ["plain_l17", "paired_l40"])
def test_without_ties_it_is_score_sequences(weights_np, name, prec):
    c = tr.oracle_case(name)
    fd = to_dev({k: v for k, v in c["fd"].items() if k not in tr.TIE_KEYS})
    m = model(weights_np, tr.K_OF[name], prec)
    S_lib = c["S_lib"].to(DEV)
    ref = m.score_sequences(fd, S_lib, method="dense")["token_log_probs"]
    on = c["mask"] != 0
    for route in ("auto", "items", "stream", "sampler"):
        out = m.score_tied(fd, S_lib, method=route)
        assert out["method"] == ("stream" if route == "auto" else route)
        d = max_diff(out["token_log_probs"], ref, on)
        print(f"{name} {prec} {route}: {d:.2e}")
        assert d < BETWEEN
        assert torch.equal(out["leader"].cpu(), torch.arange(len(on))) and bool(out["consistent"].all())


@pytest.mark.parametrize("name", ["trimer_l24", "plain_l17", "states_pairs"])
def test_a_sequence_keeps_its_bits_wherever_it_travels(weights_np, name):
    """Item route: three chunks, one sequence alone, a shuffled library and a duplicated sequence are bit-equal per sequence to the
    one-chunk call (trimer_l24: 72 and 24 item rows, plain_l17: 51 and 17 — no multiples of the item tile of 16), and so is a second call."""
    c = tr.oracle_case(name)
    fd = to_dev(c["fd"])
    m = model(weights_np, tr.K_OF[name], "x3")
    S_lib = c["S_lib"].to(DEV)
    N = len(c["mask"])
    keys = ("token_log_probs", "member_log_probs", "log_likelihood")
    one = m.score_tied(fd, S_lib, method="items")
    assert one["chunks"] == 1
    same = lambda a, b: all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32)
                                        if b[k].dtype == torch.float32 else b[k]) for k in keys)
    pick = lambda out, idx: {k: out[k][idx] for k in keys}
    assert same(one, m.score_tied(fd, S_lib, method="items"))
    budget = m.score_library_tokens
    try:
        m.score_library_tokens = N                                     # one sequence per call
        three = m.score_tied(fd, S_lib, method="items")
    finally:
        m.score_library_tokens = budget
    assert three["chunks"] == tr.N_SEQ and same(one, three)
    for k in range(tr.N_SEQ):
        assert same(pick(one, [k]), m.score_tied(fd, S_lib[k:k + 1], method="items"))
    perm = [2, 0, 1, 1]                                                # shuffled, sequence 1 twice
    assert same(pick(one, perm), m.score_tied(fd, S_lib[perm], method="items"))


def test_empty_library_and_the_default_sequence(weights_np):
    name = "trimer_l24"
    c = tr.oracle_case(name)
    fd = to_dev(c["fd"])
    m = model(weights_np, tr.K_OF[name], "x3")
    L = c["fd"]["S"].shape[1]
    for route in ("items", "sampler"):
        out = m.score_tied(fd, torch.zeros(0, L, dtype=torch.long), method=route)
        assert tuple(out["token_log_probs"].shape) == (0, L) and tuple(out["log_likelihood"].shape) == (0,) and out["chunks"] == 0
        assert tuple(out["member_log_probs"].shape) == (0, 1, L) and tuple(out["consistent"].shape) == (0,)
    a = m.score_tied(fd, method="items")
    b = m.score_tied(fd, fd["S"], method="items")
    assert torch.equal(a["S"], fd["S"]) and torch.equal(a["token_log_probs"], b["token_log_probs"]) and a["method"] == "items"
    assert m.score_tied(fd)["method"] == "items"                       # auto: listed ties, three layers, x3


def test_bf16_takes_the_sampler_route(weights_np):
    name = "mixed_l12"
    c = tr.oracle_case(name)
    m = model(weights_np, tr.K_OF[name], "bf16")
    fd = to_dev(c["fd"])
    with pytest.raises(NotImplementedError, match="items"):
        m.score_tied(fd, c["S_lib"].to(DEV), method="items")
    out = m.score_tied(fd, c["S_lib"].to(DEV))
    assert out["method"] == "sampler"
    L = c["fd"]["S"].shape[1]
    N = len(c["mask"])
    on = c["mask"] != 0
    # The bf16 mode's own accuracy class (tests/test_gpu_parity.py::test_bf16_throughput_mode: log-probs within 0.055 of the oracle)
    # holds for the members' own rows.  A group's total is sum_t w_t row_t, off by at most sum_t |w_t| * 0.055 per class, and
    # log_softmax moves by at most twice the largest change of its input: the units within 2 * max over the groups of sum |w| * 0.055.
    BF16 = 0.055
    d_own = max_diff(out["member_log_probs"].reshape(tr.N_SEQ, N), c["own"], on)
    d_unit = max_diff(out["token_log_probs"], c["unit"][:, :L], on[:L])
    bound = 2 * max(sum(abs(w) for w in s[1]) for s in c["specs"]) * BF16
    print(f"bf16 sampler route: members {d_own:.2e} (bound {BF16}), units {d_unit:.2e} (bound {bound:.3f})")
    assert d_own < BF16 and d_unit < bound
