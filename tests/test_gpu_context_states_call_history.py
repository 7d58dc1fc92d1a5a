"""Context states in a call history (tests/call_history.py): sample() and score_tied() with state_S / state_mask interleaved with the
plain multi-state call, score() and plain sample() on ONE long-lived model, every result bit-identical to a fresh model's on cloned
inputs — the cached tie tables (whose key carries the presence), the token checks and the workspaces do not leak from one call into
the next, in either direction."""
import pytest
import torch

import call_history as ch
from context_states_ref import case
from tied_states_ref import state_fd, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CONTEXT_KEYS = ("state_S", "state_mask")


def test_call_history_with_context_states(weights_np):
    m = ch.make_model(weights_np, 48)
    fd_a, fd_b, fd_p = case("LltK")[1], case("unbound")[1], case("tokens_equal_rows")[1]
    ctx_a, ctx_b = to_dev(fd_a, ch.DEV), to_dev(fd_b, ch.DEV)                  # L = 30 < K: absent residues in neighbour lists; L = 60
    fd_p = {k: v for k, v in fd_p.items() if k not in CONTEXT_KEYS}            # the plain multi-state call: no context keys
    plain = to_dev(fd_p, ch.DEV)
    one = to_dev(state_fd(fd_p, 0), ch.DEV)                                    # ... and its state 0 alone: plain sample() / score()
    one_score = dict(one, batch_size=1, randn=one["randn"][:1].clone())
    lib_a = torch.randint(0, 20, (4, fd_a["S"].shape[1]), generator=torch.Generator().manual_seed(2)).to(ch.DEV)
    lib_b = torch.randint(0, 20, (3, fd_b["S"].shape[1]), generator=torch.Generator().manual_seed(3)).to(ch.DEV)

    def sample(mm, fd):
        torch.manual_seed(11)
        return mm.sample(fd)

    def host_plan(mm, fd):
        mm.sample_states_device_plan = False
        try:
            return sample(mm, fd)
        finally:
            del mm.sample_states_device_plan
    history = [
        ("context sample", sample, ctx_a),
        ("plain multi-state sample", sample, plain),
        ("context score_tied items", lambda mm, fd: mm.score_tied(fd, lib_a, method="items"), ctx_a),
        ("score", lambda mm, fd: mm.score(fd), one_score),
        ("plain multi-state score_tied items", lambda mm, fd: mm.score_tied(fd, lib_b, method="items"), plain),
        ("context sample, other shape", sample, ctx_b),
        ("context score_tied stream", lambda mm, fd: mm.score_tied(fd, lib_a, method="stream"), ctx_a),
        ("plain sample", sample, one),
        ("context sample, host plan", host_plan, ctx_a),
        ("context score_tied sampler, other shape", lambda mm, fd: mm.score_tied(fd, lib_b, method="sampler"), ctx_b),
        ("plain multi-state sample again", sample, plain),
        ("context score_tied items again", lambda mm, fd: mm.score_tied(fd, lib_a, method="items"), ctx_a),
        ("context sample again", sample, ctx_a),
    ]
    first = {}
    for what, call, fd in history:
        got = ch.step(m, call, fd, what)
        base = what.replace(" again", "")
        if base in first:
            ch.assert_same(got, first[base], what + " against the first call")
        first.setdefault(base, got)
    # the host plan is the device plan, bit for bit (levels: a device scalar on either)
    for k in ("S", "S_states", "sampling_probs", "log_probs", "decoding_order", "uniform"):
        assert torch.equal(first["context sample"][k], first["context sample, host plan"][k]), k
