"""Call history of library scoring: on ONE long-lived model score_sequences (both routes, and "auto") is interleaved with score,
conditional_probs (plain and paired) and sample; every result equals a fresh model's on cloned inputs bit for bit
(tests/call_history.py).  The library is attached to 'the NEXT namp_decoder_fwd call' of the thread: every plain call that follows
an attached one must be a plain call."""
import numpy as np
import pytest
import torch

import call_history as ch
from call_history import assert_same, make_model, step
from test_gpu_call_history import K_DUPLEX, L_DUPLEX, _duplex, cone, duplex_fd, sampler, score

pytestmark = pytest.mark.gpu


def library(n, seed):
    """Positions: the designed residues of the RNA strand; tokens [n, n_var] in the RNA alphabet."""
    cx = _duplex()[0]
    pos = np.nonzero((cx["mask"] * cx["chain_mask"] * cx["rna_mask"]) != 0)[0]
    tok = np.random.default_rng(seed).integers(26, 30, (n, len(pos)))
    return torch.from_numpy(pos).to(ch.DEV), torch.from_numpy(tok).to(ch.DEV)


def scorer(pos, tok, method):
    return lambda mo, f: mo.score_sequences(f, tok, pos, method=method)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_score_sequences_in_a_call_history(weights_np, prec):
    """active -> score -> dense -> cone -> auto (another library) -> cone with pairs -> active -> sample -> active -> score -> a
    score() batch of two -> active: every step equals a fresh model's, repeated steps equal their first occurrence, and the active
    and dense routes stay within 2e-4 of each other."""
    pairs = _duplex()[1]
    one, two = duplex_fd(bs=1), duplex_fd(bs=2)
    pos, tok = library(9, 1)
    pos_b, tok_b = library(5, 2)
    u = ch.uniforms(two, 8)
    m = make_model(weights_np, K_DUPLEX, precision=prec)
    a0 = step(m, scorer(pos, tok, "active"), one, "active, first")
    assert "active_rows" in a0 and 2 * len(pos) <= L_DUPLEX
    s0 = step(m, score, one, "score after active")
    d0 = step(m, scorer(pos, tok, "dense"), one, "dense")
    assert float((a0["token_log_probs"] - d0["token_log_probs"]).abs().max()) < 2e-4
    c0 = step(m, cone, one, "cone after dense")
    b0 = step(m, scorer(pos_b, tok_b, "auto"), one, "auto, another library")
    assert "active_rows" in b0
    c1 = step(m, cone, dict(one, paired_residues=pairs), "cone with pairs")
    assert not torch.equal(c1["log_probs"], c0["log_probs"])
    assert_same(step(m, scorer(pos, tok, "active"), one, "active after the paired cone"), a0, "active, before and after the cones")
    draw = step(m, sampler(u), two, "sample after active")
    assert_same(step(m, scorer(pos, tok, "active"), one, "active after sample"), a0, "active, before and after sample")
    assert_same(step(m, score, one, "score after active, again"), s0, "score, before and after")
    step(m, score, two, "score with batch_size 2 (streams of the plain decoder) after active")
    assert_same(step(m, scorer(pos, tok, "active"), one, "active, last"), a0, "active, first and last")
    assert_same(step(m, sampler(u), two, "sample, last"), draw, "sample, before and after")
    assert_same(step(m, cone, one, "cone, last"), c0, "cone, first and last")
    print(f"library call history ({prec}): oracle max|dlogp| of score() = {ch.anchor_score(m, one):.3e}")


def test_refused_library_calls_leave_nothing_behind(weights_np):
    """A token id 33 (IndexError) and unsorted positions (ValueError) are refused on the host before anything is attached: the calls
    that follow equal the fresh model's."""
    one = duplex_fd(bs=1)
    pos, tok = library(4, 3)
    m = make_model(weights_np, K_DUPLEX)
    a0 = step(m, scorer(pos, tok, "active"), one, "active, first")
    bad = tok.clone()
    bad[1, 2] = 33
    with pytest.raises(IndexError):
        m.score_sequences(one, bad, pos, method="active")
    with pytest.raises(ValueError):
        m.score_sequences(one, tok, pos.flip(0), method="active")
    s0 = step(m, score, one, "score after the refused calls")
    assert_same(step(m, scorer(pos, tok, "active"), one, "active after the refused calls"), a0, "active, before and after")
    assert_same(step(m, score, one, "score, last"), s0, "score, before and after")
