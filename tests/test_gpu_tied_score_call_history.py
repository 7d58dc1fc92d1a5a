"""score_tied in a call history (tests/call_history.py): its three routes interleaved with score, score_sequences, score_mutations,
conditional_probs(tied=True) and sample on ONE long-lived model, every result bit-identical to a fresh model's on cloned inputs —
the cached tie tables, the workspaces and the thread's attachments do not leak from one call into the next."""
import pytest
import torch

import call_history as ch
import tied_score_ref as tr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def to_dev(fd):
    return {k: (v.to(ch.DEV) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def test_call_history_with_score_tied(weights_np):
    m = ch.make_model(weights_np, tr.K_OF["trimer_l24"])
    tied, states, plain = (tr.oracle_case(n) for n in ("trimer_l24", "states_m3_l20", "paired_l40"))
    fd_t, fd_s = to_dev(tied["fd"]), to_dev(states["fd"])
    fd_p = to_dev({k: v for k, v in plain["fd"].items() if k not in tr.TIE_KEYS})
    fd_p.update(symmetry_residues=[[]], symmetry_weights=[[]])
    lib_t, lib_s, lib_p = (c["S_lib"].to(ch.DEV) for c in (tied, states, plain))

    def sample(mm, fd):
        torch.manual_seed(11)
        return mm.sample(fd)
    history = [
        ("score_tied items", lambda mm, fd: mm.score_tied(fd, lib_t, method="items"), fd_t),
        ("score", lambda mm, fd: mm.score(fd), fd_p),
        ("score_tied stream (states)", lambda mm, fd: mm.score_tied(fd, lib_s, method="stream"), fd_s),
        ("score_sequences", lambda mm, fd: mm.score_sequences(fd, lib_p), fd_p),
        ("score_tied sampler", lambda mm, fd: mm.score_tied(fd, lib_t, method="sampler"), fd_t),
        # (the scan's `delta` grid holds NaN on the cells no variant fills: the per-variant arrays are compared)
        ("score_mutations", lambda mm, fd: {k: v for k, v in mm.score_mutations(fd).items() if k != "delta"}, fd_p),
        ("score_tied items (states)", lambda mm, fd: mm.score_tied(fd, lib_s, method="items"), fd_s),
        ("conditional_probs tied", lambda mm, fd: mm.conditional_probs(fd, tied=True), fd_t),
        ("score_tied items again", lambda mm, fd: mm.score_tied(fd, lib_t, method="items"), fd_t),
        ("sample", sample, fd_t),
        ("score_tied stream (no ties)", lambda mm, fd: mm.score_tied(fd, lib_p), fd_p),
        ("score_sequences active", lambda mm, fd: mm.score_sequences(fd, lib_p, method="active"), fd_p),
        ("score_tied sampler (states)", lambda mm, fd: mm.score_tied(fd, lib_s, method="sampler"), fd_s),
        ("score_tied items, once more", lambda mm, fd: mm.score_tied(fd, lib_t, method="items"), fd_t),
    ]
    first = None
    for what, call, fd in history:
        got = ch.step(m, call, fd, what)
        if what.startswith("score_tied items") and fd is fd_t:
            first = got if first is None else first
            ch.assert_same(got, first, what + " against the first call")
